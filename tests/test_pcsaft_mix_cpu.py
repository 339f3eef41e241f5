"""The fp64 mixture PC-SAFT oracle of tests/pcsaft_mix_ref.py pinned on its own (no GPU): reduction to the pure oracle,
symmetry, the binary interaction parameter, thermodynamic consistency, the mass-action equations, Esper's parameters
against measured binary densities, the recorded random-mixture results, and the bindings of the two new entry points."""
import json
import os

import numpy as np

from tests import pcsaft_mix_cases as C
from tests import pcsaft_mix_ref as MR
from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pure_molecules():
    with open(os.path.join(ROOT, "tests", "golden", "pcsaft_thermoml.json")) as fh:
        return json.load(fh)["molecules"]


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_fixture_is_small_and_covers_the_class_pairs():
    sy = C.systems()
    assert os.path.getsize(C.FIXTURE) < 64 * 1024
    assert [s["pair"] for s in sy] == [p for p in C.PAIRS for _ in range(4)]
    assert any(s["names"] == ["ethanol", "water"] for s in sy if s["pair"] == "AA")
    for s in sy:
        assert len(s["params"]) == 2 and all(len(p) == 9 for p in s["params"]) and len(s["points"]) == 8
        for T, P, x1, x2, rho in s["points"]:
            assert T > 0 and P > 0 and x1 >= 0 and x2 >= 0 and abs(x1 + x2 - 1) < 1e-3 and rho > 0


def test_reduces_to_the_pure_oracle():
    """a_res, Z and density of the pure oracle at 1e-12 relative for nc = 1, for two identical rows at x = (0.3, 0.7),
    and for x = (1, 0) beside a different second component (non-polar, dipolar and associating ones), at three measured
    (T, P) states of each of 6 molecules.  The density is compared at (T, P); a_res and Z at T and the pure oracle's
    liquid density there (eta 0.39 .. 0.45).  At a liquid root Z = 1 + rho da/drho is 2e-3 .. 1e-2, what is left when
    terms of size 10 cancel, so Z is held as Z - 1 at 1e-12 max(1, |Z - 1|), the form of the GPU test.  Largest
    deviations seen: a_res 1.4e-15, Z - 1 scaled 4.8e-14, density 7.4e-16; |dZ| / |Z| itself reaches 7.0e-12 there.
    In addition a_res and Z are compared plainly at 1e-12 relative at one packing fraction per state away from the
    root (0.005, 0.02, 0.45 or 0.5, the first with |Z| > 0.1)."""
    mols = _pure_molecules()
    others = [mols[3]["params"], mols[19]["params"], mols[35]["params"], mols[47]["params"]]
    assert others[2][3] > 0 and others[3][3] > 0 and others[1][5] > 0  # associating, associating, dipolar
    worst = [0.0, 0.0, 0.0, 0.0]
    for m in mols[::8]:
        row = m["params"]
        for k, (T, P, *_) in enumerate(m["rho"][:3]):
            rho_ref = R.density(row, T, P)
            rl = rho_ref * R.TO_A3  # the liquid state itself
            al_ref, zl_ref = R.a_res(row, T, rl), R.compressibility(row, T, rl)
            assert 0.3 < rl * R.eta_per_rho(row, T) < 0.5 and abs(al_ref) > 1.0
            etas = [(0.005, 0.02, 0.45)[(k + i) % 3] for i in range(3)] + [0.5]
            rn = next(e / R.eta_per_rho(row, T) for e in etas if abs(R.compressibility(row, T, e / R.eta_per_rho(row, T))) > 0.1)
            a_ref, z_ref = R.a_res(row, T, rn), R.compressibility(row, T, rn)
            cases = [MR.Mixture([row], [1.0]), MR.Mixture([row, row], [0.3, 0.7])]
            cases += [MR.Mixture([row, o], [1.0, 0.0]) for o in others] + [MR.Mixture([others[2], row], [0.0, 2.0])]
            for mix in cases:
                al, zl, rho = MR.a_res(mix, T, rl), MR.compressibility(mix, T, rl), MR.density(mix, T, P)
                found = (_rel(al, al_ref), abs(zl - zl_ref) / max(1.0, abs(zl_ref - 1.0)), _rel(rho, rho_ref),
                         _rel(zl, zl_ref))
                worst = [max(w, f) for w, f in zip(worst, found)]
                assert max(found[:3]) <= 1e-12, (m["name"], T, found)
                assert _rel(MR.a_res(mix, T, rn), a_ref) <= 1e-12, (m["name"], T)
                assert _rel(MR.compressibility(mix, T, rn), z_ref) <= 1e-12, (m["name"], T, z_ref)
    print("largest deviations at the liquid states (a_res, Z - 1 scaled, density, |dZ| / |Z|):", worst)


def test_absent_component_contributes_exactly_nothing():
    mols = _pure_molecules()
    a, b, c = mols[0]["params"], mols[20]["params"], mols[40]["params"]
    T, rn = 320.0, 0.3 / MR.Mixture([a, c], [0.4, 0.6]).eta_per_rho(320.0)
    two = MR.a_terms(MR.Mixture([a, c], [0.4, 0.6]), T, rn)
    three = MR.a_terms(MR.Mixture([a, b, c], [0.4, 0.0, 0.6]), T, rn)
    for u, v in zip(two, three):
        assert np.isfinite(v) and abs(u - v) <= 1e-14 * max(1.0, abs(u))


def test_component_swap_leaves_the_density_unchanged():
    for s in C.systems()[::3]:
        rows = s["params"]
        kij = [[0.0, 0.03], [0.03, 0.0]]
        for T, P, x1, x2, _ in s["points"][::3]:
            r1 = MR.density(MR.Mixture(rows, [x1, x2], kij=kij), T, P)
            r2 = MR.density(MR.Mixture(rows[::-1], [x2, x1], kij=np.transpose(kij)), T, P)
            assert _rel(r1, r2) <= 1e-12, (s["names"], T, P)


def test_kij_and_eab_are_read_from_the_upper_triangle():
    """The convention of DESIGN.md §4c: entry [min(i, j)][max(i, j)] counts for the pair, whatever the lower triangle
    and the diagonal hold."""
    s = C.systems()[-1]
    assert s["names"] == ["ethanol", "water"]
    T, P, x1, x2, _ = s["points"][3]
    sym = MR.Mixture(s["params"], [x1, x2], kij=[[0.0, 0.03], [0.03, 0.0]], eab=[[np.nan, 2400.0], [2400.0, np.nan]])
    low = MR.Mixture(s["params"], [x1, x2], kij=[[0.7, 0.03], [-0.5, 0.7]], eab=[[1.0, 2400.0], [np.nan, 9e3]])
    plain = MR.Mixture(s["params"], [x1, x2])
    assert MR.density(sym, T, P) == MR.density(low, T, P) != MR.density(plain, T, P)


def test_binary_interaction_parameter_moves_a_res_by_the_dispersion_sums():
    """k_12 = 0.05 on a non-polar pair changes only eps_12 of the two dispersion sums: the change of a_res is
    -2 pi rho I1 dS1 - pi rho mbar C1 I2 dS2 with the sums written out here."""
    s = C.systems()[1]
    assert s["pair"] == "NN"
    r1, r2 = s["params"]
    mixed = [p for p in s["points"] if p[2] > 0 and p[3] > 0]
    assert len(mixed) >= 4
    for T, _, x1, x2, _ in mixed:
        x = np.array([x1, x2]) / (x1 + x2)
        base, moved = MR.Mixture([r1, r2], x), MR.Mixture([r1, r2], x, kij=[[0.0, 0.05], [0.05, 0.0]])
        rn = 0.35 / base.eta_per_rho(T)
        sums = []
        for k12 in (0.0, 0.05):
            s1 = s2 = 0.0
            for i, ri in enumerate((r1, r2)):
                for j, rj in enumerate((r1, r2)):
                    e = np.sqrt(ri[2] * rj[2]) * (1.0 - (k12 if i != j else 0.0)) / T
                    w = x[i] * x[j] * ri[0] * rj[0] * (0.5 * (ri[1] + rj[1])) ** 3
                    s1, s2 = s1 + w * e, s2 + w * e * e
            sums.append((s1, s2))
        mb, eta = x[0] * r1[0] + x[1] * r2[0], 0.35
        i1, i2 = R._poly(R._interp(R.DISP_A, mb), eta), R._poly(R._interp(R.DISP_B, mb), eta)
        c1 = 1.0 / (1.0 + mb * (8 * eta - 2 * eta ** 2) / (1 - eta) ** 4
                    + (1 - mb) * (20 * eta - 27 * eta ** 2 + 12 * eta ** 3 - 2 * eta ** 4) / ((1 - eta) * (2 - eta)) ** 2)
        want = -2 * np.pi * rn * i1 * (sums[1][0] - sums[0][0]) - np.pi * rn * mb * c1 * i2 * (sums[1][1] - sums[0][1])
        got = MR.a_res(moved, T, rn) - MR.a_res(base, T, rn)
        assert want > 0 and abs(got - want) <= 1e-12 * abs(MR.a_res(base, T, rn)), (T, got, want)


# |Z(complex step) - Z(central difference of a_res, step 1e-5 rho)| / max(1, |Z|), largest value over every density
# state of the pure fixture x eta in (1e-3, 0.1, 0.3, 0.45) with tests/pcsaft_ref.py: 4.7e-9 (the mixtures of the
# binary fixture reach 3.9e-9 at the same points)
PURE_CD_ERROR = 4.7e-9


def test_complex_step_pressure_matches_a_central_difference():
    """p from the complex step equals rho k T (1 + rho da/drho) from a central difference of a_res, within 10 x the
    central difference's own error measured on the pure oracle (PURE_CD_ERROR)."""
    params, comp, owner, T, _, x, _ = C.fixture_points()
    worst = 0.0
    for j in range(0, len(owner), 2):
        mix = MR.Mixture(params[comp[owner[j]]], x[j])
        for eta in (1e-3, 0.1, 0.3, 0.45):
            rn = eta / mix.eta_per_rho(T[j])
            h = rn * 1e-5
            z_fd = 1.0 + rn * (MR.a_res(mix, T[j], rn + h) - MR.a_res(mix, T[j], rn - h)) / (2 * h)
            z = MR.compressibility(mix, T[j], rn)
            worst = max(worst, abs(z - z_fd) / max(1.0, abs(z)))
    print("largest |Z_cs - Z_fd| / max(1, |Z|):", worst)
    assert worst <= 10 * PURE_CD_ERROR


def test_site_fractions_satisfy_the_mass_action_equations():
    params, comp, owner, T, _, x, _ = C.fixture_points()
    sy = C.systems()
    seen = 0
    for j in range(len(owner)):
        if sy[owner[j]]["names"] != ["ethanol", "water"]:
            continue
        seen += 1
        mix = MR.Mixture(params[comp[owner[j]]], x[j])
        for eta in (1e-3, 0.1, 0.3, 0.45):
            rn = eta / mix.eta_per_rho(T[j])
            xa, xb, delta = MR.site_fractions(mix, T[j], rn)
            assert np.all((xa > 0) & (xa <= 1) & (xb > 0) & (xb <= 1))
            assert np.all(delta[0] > 0)  # like and unlike pairs bond
            ra = xa[0] * (1.0 + rn * delta[0] @ (mix.x * mix.nb * xb[0])) - 1.0
            rb = xb[0] * (1.0 + rn * delta[0] @ (mix.x * mix.na * xa[0])) - 1.0
            assert np.abs(ra).max() <= 1e-13 and np.abs(rb).max() <= 1e-13, (T[j], eta, ra, rb)
    assert seen == 8


# observed medians of |oracle - measured| / measured per class pair (Esper's parameters, k_ij = 0):
#   NN 0.23 %, DN 0.33 %, DD 0.72 %, AN 0.41 %, AD 1.91 %, AA 0.38 %; bounds = 1.5 x that, rounded up to one digit
MEDIAN_BOUNDS = {"NN": 0.004, "DN": 0.005, "DD": 0.02, "AN": 0.007, "AD": 0.03, "AA": 0.006}


def test_esper_parameters_reproduce_binary_thermoml_densities():
    """Physical sanity net for the mixing rules: with Esper et al.'s parameters and k_ij = 0 the oracle reproduces the
    measured binary densities.  Observed medians per class pair: NN 0.23 %, DN 0.33 %, DD 0.72 %, AN 0.41 %, AD 1.91 %,
    AA 0.38 %.  A broken mixing rule moves densities by percent."""
    _, _, owner, _, _, _, measured = C.fixture_points()
    ref = C.fixture_oracle()
    assert np.all(np.isfinite(ref))
    sy = C.systems()
    for pair in C.PAIRS:
        idx = [j for j in range(len(owner)) if sy[owner[j]]["pair"] == pair]
        med = np.median(np.abs(ref[idx] / measured[idx] - 1.0))
        print(pair, "median |oracle - measured| / measured:", med)
        assert med <= MEDIAN_BOUNDS[pair], (pair, med)


def test_recorded_random_mixture_results_are_the_oracle_s():
    """tests/golden/pcsaft_mix_random.json holds what the oracle gives on the seeded random mixtures: the layout is as
    the GPU test expects (300 mixtures, 100 of them with a -1 slot, 4 states each), the oracle finds a root on most
    points, and a sample of 24 points recomputed here agrees with the record."""
    groups, rho = C.recorded()
    assert sum(len(g["comp"]) for g in groups) == 300 and sorted(g["nc"] for g in groups) == [1, 2, 3, 4]
    assert sum(int((g["comp"] < 0).any(axis=1).sum()) for g in groups) == 100
    assert rho.shape == (1200,) and np.isfinite(rho).mean() >= 0.7
    at = 0
    for g in groups:
        n = len(g["owner"])
        for j in range(0, n, n // 6 + 1):
            live = C.oracle_point(g, j)
            assert (live is None) == bool(np.isnan(rho[at + j]))
            # 1e-12 and not the bits: the result goes through LAPACK and Brent, a stale record is off by far more
            assert live is None or _rel(live, rho[at + j]) <= 1e-12
        at += n


def test_bindings_declare_the_two_entry_points():
    from gnnepcsaft_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_state"][1]) == 17
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_density"][1]) == 15
    assert _lib.KERNEL_GROUPS[_lib.K_PCSAFT_MIX_STATE] == "pcsaft_mix_state"
    assert _lib.KERNEL_GROUPS[_lib.K_PCSAFT_MIX_RHO] == "pcsaft_mix_density"
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    assert "GNX_K_PCSAFT_MIX_RHO = %d," % _lib.K_PCSAFT_MIX_RHO in header and "#define GNX_ABI_VERSION 7" in header
