"""Mixture bubble and dew temperatures on the GPU (csrc/gnx_pcsaft_mix_tvle.hip, gnnepcsaft_amd/pcsaft.py) against the
oracle of tests/pcsaft_mix_tvle_ref.py: the equilibrium equations at the reported state (the primary check: the oracle's
pressure and finite-difference fugacities share no mechanism with the kernel's duals), the known answer of the inverse
problem, the round trip through the bubble- and dew-pressure kernels, the reductions, the independence of the start,
failures and invalid input, the launch edges, determinism and the reference-shaped I/O.

The points are the inverse problems of the 30 bubble points of tests/pcsaft_mix_vle_ref.py (six named systems and the
first point of each of the 24 systems of the binary fixture): P is the oracle's bubble pressure at (T, x), so the bubble
temperature of (P, x) is T with the vapour y and the dew temperature of (P, y) is T with the liquid x."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_tvle_ref as TR
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

pytestmark = pytest.mark.gpu

VP_TOL = 1e-8        # the bound of test_pcsaft_gpu.py on pcsaft.vapor_pressure against pcsaft_ref.vle
SOLVE_TOL = 1e-10    # kVleMixTol: what the kernel's loop ends on
PRESSURE_TOL = 1e-9  # the standing bound of the pressure kernels against their oracles (test_pcsaft_mix_vle_gpu.py)
NC = 4
BLOCK = 256          # the block size of k_pcsaft_mix


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _solve(dev, dew, params, comp, owner, P, z, T0=None, kij=None, eab=None):
    """(T, w, rho_l, rho_v, status) as host arrays"""
    from gnnepcsaft_amd import pcsaft
    fn = pcsaft.mixture_dew_temperature if dew else pcsaft.mixture_bubble_temperature
    p, c, o, pp, zz, t0, k, e = _dev(dev, np.asarray(params, dtype=np.float64).reshape(-1, 9), comp,
                                     np.asarray(owner, dtype=np.int64), np.asarray(P, dtype=np.float64), z,
                                     None if T0 is None else np.asarray(T0, dtype=np.float64), kij, eab)
    return [v.cpu().numpy() for v in fn(p, c, zz, pp, o, k, e, t0)]


def _forward(dev, dew, params, comp, owner, T, z):
    """(P, w, rho_l, rho_v, status) of the pressure kernel of the same kind"""
    from gnnepcsaft_amd import pcsaft
    fn = pcsaft.mixture_dew_pressure if dew else pcsaft.mixture_bubble_pressure
    p, c, o, t, zz = _dev(dev, np.asarray(params, dtype=np.float64).reshape(-1, 9), comp,
                          np.asarray(owner, dtype=np.int64), np.asarray(T, dtype=np.float64), z)
    return [v.cpu().numpy() for v in fn(p, c, zz, t, o)]


@functools.lru_cache(maxsize=None)
def _pooled(dew):
    """the 30 cases as one pool: params [B, 9], comp [30, 4] (-1 = unused), owner [30], P [30], z [30, 4], T [30]"""
    cases = TR.cases()
    params, comp = [], np.full((len(cases), NC), -1, dtype=np.int64)
    z, P, T = np.zeros((len(cases), NC)), [], []
    for i, (_, rows, t, x, fwd, _) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(rows.tolist())
        z[i, :len(rows)] = fwd["y"] if dew else x
        P.append(fwd["P"])
        T.append(t)
    return np.array(params), comp, np.arange(len(cases), dtype=np.int64), np.array(P), z, np.array(T)


@functools.lru_cache(maxsize=None)
def _all_points(dev, dew, factor=None):
    """the kernel on the 30 cases, one launch: computed once, shared, never modified.  ``factor``: T0 = factor x the
    forward T, None = no T0 array at all"""
    params, comp, owner, P, z, T = _pooled(dew)
    return _solve(dev, dew, params, comp, owner, P, z, None if factor is None else factor * T)


def _oracle(dew):
    return TR.dew_solves() if dew else TR.bubble_solves()


def _returning(dew):
    """the cases the CPU test lists as returning the forward answer from the own start"""
    return [j for j, ((name, *_), (sol, _)) in enumerate(zip(TR.cases(), _oracle(dew)))
            if sol is not None and not (dew and name in TR.OTHER_DEW_POINT)]


def _rel(a, b):
    return abs(a / b - 1.0)


@pytest.mark.parametrize("dew", [False, True], ids=["bubble", "dew"])
def test_equations_hold_at_the_reported_state(gpu_device, dew):
    """On every case the oracle solves (28 bubble; 28 dew, "fixture 15" on its other dew point included): status 0,
    sum w = 1 at 1e-12, rho_l > rho_v > 0, NaN in the -1 slots, the oracle's pressure of (x, rho_l) and (y, rho_v) is the
    given P at 1e-9 (the liquid on the scale max(P, 1e-3 rho R T), as at every small Z), and the oracle's ln f_i agree
    between the phases within 2 x the kernel's tolerance + 10 x the disagreement of the oracle's two difference steps
    at that point.  A case the oracle does not solve may report status 1 with the documented outputs; with status 0 it
    passes the same checks.
    On an MI355X, worst of the 28 checked points (the two near-critical cases report status 1, as in the oracle),
    bubble: sum y - 1 2.2e-16, liquid pressure 7.2e-11, vapour pressure 4.4e-16, fugacities 1.1e-10 (0.11 of the bound at
    that point; the two-step disagreement reaches 4.6e-9); dew: sum x - 1 2.2e-16, liquid pressure 5.8e-11, vapour
    pressure 4.4e-16, fugacities 5.3e-10 (0.40 of the bound at that point; the two-step disagreement reaches 2.8e-9)."""
    T, w, rl, rv, st = _all_points(gpu_device, dew)
    _, comp, _, P, z, _ = _pooled(dew)
    worst = {"sum w": 0.0, "p liquid": 0.0, "p vapour": 0.0, "fugacity": 0.0, "fugacity / bound": 0.0, "two-step": 0.0}
    unsolved = []
    assert sum(s is not None for s, _ in _oracle(dew)) >= 28
    for j, (name, rows, _, _, _, _) in enumerate(TR.cases()):
        k = len(rows)
        if _oracle(dew)[j][0] is None and st[j] == 1:
            unsolved.append(name)
            assert T[j] == 0.0 and rl[j] == 0.0 and rv[j] == 0.0 and np.all(np.isnan(w[j]))
            continue
        assert st[j] == 0 and T[j] > 0.0 and rl[j] > rv[j] > 0.0, name
        assert np.all(np.isnan(w[j, k:])) and np.all(w[j, :k] > 0.0)
        liquid, vapour = (w[j, :k], z[j, :k]) if dew else (z[j, :k], w[j, :k])
        r = V.residuals(rows, liquid, vapour, T[j], P[j], rl[j], rv[j])
        bound = 2.0 * SOLVE_TOL + 10.0 * r["own"]
        fig = {"sum w": abs(w[j, :k].sum() - 1.0),
               "p liquid": abs(r["p_l"] - P[j]) / max(P[j], rl[j] * R.RGAS * T[j] * 1e-3),
               "p vapour": _rel(r["p_v"], P[j]), "fugacity": r["fugacity"], "fugacity / bound": r["fugacity"] / bound,
               "two-step": r["own"]}
        for key, v in fig.items():
            worst[key] = max(worst[key], v)
        assert fig["sum w"] <= 1e-12 and fig["p liquid"] <= 1e-9 and fig["p vapour"] <= 1e-9, (name, fig)
        assert r["fugacity"] <= bound, (name, fig)
    print("status 1 where the oracle has no solution either:", unsolved)
    print("worst over the checked points:", worst)


@pytest.mark.parametrize("dew", [False, True], ids=["bubble", "dew"])
def test_against_the_known_answer(gpu_device, dew):
    """The cases that return the forward answer in the oracle (28 bubble, 27 dew): T (relative) and the composition
    (absolute) within max(1e-9, 10 x what the oracle's own answer moves between its tolerances 1e-9 and 1e-11 there).
    On an MI355X: bubble T within 1.7e-11 and y within 3.3e-11; dew T within 1.2e-11 and x within 1.4e-10 (ethanol +
    water, bound 2.6e-8); the other bounds are 1e-9, but for 4.3e-9 (ethanol + water's bubble point) and 4.1e-9 ("fixture
    20", dew)."""
    T, w, rl, rv, st = _all_points(gpu_device, dew)
    worst = [0.0, 0.0]
    idx = _returning(dew)
    assert len(idx) >= (27 if dew else 28)
    for j in idx:
        name, rows, Tf, x, fwd, _ = TR.cases()[j]
        k = len(rows)
        bound = TR.bound(_oracle(dew)[j][1])
        dt, dw = _rel(T[j], Tf), float(np.max(np.abs(w[j, :k] - (x if dew else fwd["y"]))))
        print(name, "T", T[j], "dT", dt, "dw", dw, "bound", bound)
        worst = [max(worst[0], dt), max(worst[1], dw)]
        assert st[j] == 0 and dt <= bound and dw <= bound, name
    print("worst of", len(idx), "cases: T", worst[0], "composition", worst[1])


@pytest.mark.parametrize("dew", [False, True], ids=["bubble", "dew"])
def test_consistent_with_the_pressure_kernels(gpu_device, dew):
    """The same cases: ``mixture_bubble_pressure`` at the reported (T, x), ``mixture_dew_pressure`` at the reported (T, y),
    return the given P.  An error dT / T of the temperature moves that pressure by (d ln P / d ln T) dT / T, so the bound
    is the bound of the test above times the oracle's d ln P / d ln T at the point (a central difference of its bubble
    pressure at T (1 +- 1e-3); 7.8 to 34.4 on these cases, 1.6 to 2.5 on the four with dissolved methane), plus 1e-9, the
    pressure kernels' own standing bound against their oracles: 2.6e-9 to 3.5e-8 (3.5e-7 for ethanol + water's dew
    point).  (The dew cases are those whose dew pressure returns to the bubble point as well: the CPU tests of the dew
    pressure list the same two exceptions.)
    On an MI355X: bubble within 9.1e-11 on the 28 cases, dew within 9.7e-11 on the 27."""
    T, w, rl, rv, st = _all_points(gpu_device, dew)
    params, comp, owner, P, z, _ = _pooled(dew)
    idx = _returning(dew)
    Pf, _, _, _, stf = _forward(gpu_device, dew, params, comp, owner[idx], T[idx], z[idx])
    slopes = TR.pressure_slopes()
    worst = 0.0
    for i, j in enumerate(idx):
        name = TR.cases()[j][0]
        assert np.isfinite(slopes[j]), name
        bound = TR.bound(_oracle(dew)[j][1]) * abs(slopes[j]) + PRESSURE_TOL
        err = _rel(Pf[i], P[j])
        print(name, "P", P[j], "forward kernel", Pf[i], "error", err, "d ln P / d ln T", slopes[j], "bound", bound)
        worst = max(worst, err)
        assert stf[i] == 0 and err <= bound, name
    print("worst of", len(idx), "cases:", worst)


def test_reductions(gpu_device):
    from gnnepcsaft_amd import pcsaft
    rows = np.array([V.HEXANE, V.BUTANE, V.ETHANOL, V.METHANE], dtype=np.float64)
    Tref = np.array([350.0, 330.0, 340.0])
    p, t = _dev(gpu_device, rows[:3], Tref)
    ps, pl, pv, pst = [v.cpu().numpy() for v in pcsaft.vapor_pressure(p, t)]
    assert np.all(pst == 0)

    def psat(T):
        return pcsaft.vapor_pressure(p, _dev(gpu_device, T)[0])[0].cpu().numpy()

    # one component, and a binary at (1, 0): T is where the pure vapour pressure is P; w is 1.0, and 0.0 for the absent
    # component; the bubble and the dew temperature are the same
    comp1 = np.arange(3, dtype=np.int64)[:, None]
    comp2 = np.stack([np.arange(3), (np.arange(3) + 1) % 3], axis=1).astype(np.int64)
    z10 = np.tile([1.0, 0.0], (3, 1))
    got = {}
    for dew in (False, True):
        T1, w1, rl1, rv1, st1 = _solve(gpu_device, dew, rows, comp1, np.arange(3), ps, np.ones((3, 1)))
        worst = max(np.max(np.abs(psat(T1) / ps - 1)), np.max(np.abs(rl1 / pl - 1)), np.max(np.abs(rv1 / pv - 1)))
        print("one component against pcsaft.vapor_pressure:", worst, "T", np.max(np.abs(T1 / Tref - 1)))
        assert np.all(st1 == 0) and worst <= VP_TOL and np.all(w1 == 1.0)
        T2, w2, rl2, rv2, st2 = _solve(gpu_device, dew, rows, comp2, np.arange(3), ps, z10)
        assert np.all(st2 == 0) and np.array_equal(w2, z10)
        assert np.max(np.abs(psat(T2) / ps - 1)) <= VP_TOL and np.max(np.abs(T2 / T1 - 1)) <= 1e-12
        got[dew] = T1
        # the same row twice is that component: w = z and its boiling temperature
        same = np.stack([np.arange(3), np.arange(3)], axis=1).astype(np.int64)
        z37 = np.tile([0.3, 0.7], (3, 1))
        T3, w3, _, _, st3 = _solve(gpu_device, dew, rows, same, np.arange(3), ps, z37)
        print("same row twice: w", np.max(np.abs(w3 - z37)), "T", np.max(np.abs(T3 / T1 - 1)))
        assert np.all(st3 == 0) and np.max(np.abs(w3 - z37)) <= 1e-9 and np.max(np.abs(T3 / T1 - 1)) <= 1e-9
    print("bubble against dew temperature of one component:", np.max(np.abs(got[False] / got[True] - 1)))
    assert np.max(np.abs(got[False] / got[True] - 1)) <= 1e-9
    # a -1 slot and a zero slot: the mixture without them, NaN and 0.0 in w
    p2 = np.array([2e6])
    for dew, zb in ((False, [0.1, 0.9]), (True, [0.97, 0.03])):
        Tb, wb, _, _, stb = _solve(gpu_device, dew, rows, np.array([[3, 0]], dtype=np.int64), [0], p2, np.array([zb]))
        Tz, wz, _, _, stz = _solve(gpu_device, dew, rows, np.array([[3, 1, 0]], dtype=np.int64), [0], p2,
                                   np.array([[zb[0], 0.0, zb[1]]]))
        Tm, wm, _, _, stm = _solve(gpu_device, dew, rows, np.array([[3, -1, 0]], dtype=np.int64), [0], p2,
                                   np.array([[zb[0], 0.5, zb[1]]]))
        assert stb[0] == 0 and stz[0] == 0 and stm[0] == 0
        assert _rel(Tz[0], Tb[0]) <= 1e-12 and _rel(Tm[0], Tb[0]) <= 1e-12
        assert wz[0, 1] == 0.0 and np.isnan(wm[0, 1])
        assert np.max(np.abs(wz[0, [0, 2]] - wb[0])) <= 1e-12 and np.max(np.abs(wm[0, [0, 2]] - wb[0])) <= 1e-12


@pytest.mark.parametrize("dew", [False, True], ids=["bubble", "dew"])
def test_component_swap_and_upper_triangle(gpu_device, dew):
    """the swapped mixture gives the same point at 1e-9; what the lower triangle and the diagonal of k_ij hold changes no
    bit.  With a k_ij the pressures are no longer bubble pressures of these mixtures and some points may have no
    solution this start finds: the statuses must agree, and most points must be there to compare.  The non-associating
    named systems only (five points, the near-critical one among them may fail): the launch takes a fraction of a
    second."""
    params, comp, owner, P, z, _ = _pooled(dew)
    pick = np.array([0, 1, 2, 4, 5])
    comp, owner, P, z = comp[pick], np.arange(len(pick)), P[pick], z[pick]
    rng = np.random.default_rng(3)
    kij = np.zeros((len(pick), NC, NC))
    kij[:, 0, 1] = rng.uniform(-0.02, 0.02, len(pick))
    T, w, rl, rv, st = _solve(gpu_device, dew, params, comp, owner, P, z, kij=kij)
    swap = [1, 0, 2, 3]
    Ts, ws, rls, rvs, sts = _solve(gpu_device, dew, params, comp[:, swap].copy(), owner, P, z[:, swap].copy(), kij=kij)
    ok = st == 0
    used = comp >= 0
    print("status 0 with k_ij:", ok.sum(), "of", len(pick))
    assert ok.sum() >= 4 and np.array_equal(st, sts)
    dw = np.max(np.abs(np.where(used, ws[:, swap] - w, 0.0)[ok]))
    print("swap: T", np.max(np.abs(Ts[ok] / T[ok] - 1)), "w", dw, "rho_l", np.max(np.abs(rls[ok] / rl[ok] - 1)))
    assert np.max(np.abs(Ts[ok] / T[ok] - 1)) <= 1e-9 and dw <= 1e-9
    junk = kij + np.tril(rng.uniform(-9.0, 9.0, kij.shape))
    junk[:, 2, 0] = np.nan
    again = _solve(gpu_device, dew, params, comp, owner, P, z, kij=junk)
    for a, b in zip((T, w, rl, rv, st), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dew", [False, True], ids=["bubble", "dew"])
def test_the_answer_does_not_depend_on_the_start(gpu_device, dew):
    """where all three give status 0, the runs from T0 = 0.9 T, from T0 = 1.05 T and from the kernel's own start agree at
    1e-9 in T and the composition, "fixture 15" of the dew point on whichever of its dew points each start leads to
    excepted; a given start also solves the near-critical cases the own start does not reach.  No T0 array and one of
    NaN give the same bytes.
    On an MI355X: bubble 30 + 30 + 28 solved, agreement 3.8e-11; dew 29 + 30 + 28 solved, agreement 4.9e-11."""
    own, low, high = (_all_points(gpu_device, dew, f) for f in (None, 0.9, 1.05))
    params, comp, owner, P, z, _ = _pooled(dew)
    print("solved from 0.9 T:", int((low[4] == 0).sum()), "from 1.05 T:", int((high[4] == 0).sum()), "own start:",
          int((own[4] == 0).sum()))
    assert (low[4] == 0).sum() >= 29 and (high[4] == 0).sum() >= 29
    ok = (own[4] == 0) & (low[4] == 0) & (high[4] == 0)
    if dew:
        ok &= np.array([name not in TR.OTHER_DEW_POINT for name, *_ in TR.cases()])
    assert ok.sum() >= 27
    worst = 0.0
    for other in (low, high):
        worst = max(worst, np.max(np.abs(other[0][ok] / own[0][ok] - 1)),
                    np.max(np.abs(np.where(comp >= 0, other[1] - own[1], 0.0)[ok])))
    print("worst disagreement between the starts:", worst)
    assert worst <= 1e-9
    nan = _solve(gpu_device, dew, params, comp, owner, P, z, np.full(len(P), np.nan))
    for a, b in zip(own, nan):
        assert a.tobytes() == b.tobytes()


def test_failures_and_invalid_input(gpu_device):
    rows = np.array([V.METHANE, V.BUTANE, V.HEXANE], dtype=np.float64)
    comp = np.array([[0, -1, -1], [1, 2, -1], [0, 1, 2]], dtype=np.int64)
    zs = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.1, 0.3, 0.6]])
    for dew in (False, True):
        # methane alone at 10 MPa is above its critical pressure, butane + hexane at 50 MPa above theirs: status 1;
        # butane + hexane at 1 atm and the ternary at 1 MPa boil
        owner = np.array([0, 1, 1, 2])
        P = np.array([1e7, 5e7, 101325.0, 1e6])
        T, w, rl, rv, st = _solve(gpu_device, dew, rows, comp, owner, P, zs[owner])
        assert st.tolist() == [1, 1, 0, 0], st
        assert np.all(T[:2] == 0.0) and np.all(rl[:2] == 0.0) and np.all(rv[:2] == 0.0) and np.all(np.isnan(w[:2]))
        assert np.all(T[2:] > 0.0) and np.array_equal(np.isnan(w[2:]), comp[owner[2:]] < 0)
        # invalid input: status 3, T = 0, NaN in w; the good rows of the same launch keep their bits
        bad_owner = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 3, -1, 1, 2])
        bad_P = np.array([0.0, -1e5, np.nan, np.inf, 101325.0, 101325.0, 101325.0, 101325.0, 101325.0, 101325.0,
                          101325.0, 101325.0, 1e6])
        bad_T0 = np.full(len(bad_owner), np.nan)
        bad_T0[4:7] = [0.0, -300.0, np.inf]
        bad_z = zs[np.clip(bad_owner, 0, 2)].copy()
        bad_z[7, :2] = 0.0
        bad_z[8, 0] = -0.5
        Tb, wb, rlb, rvb, stb = _solve(gpu_device, dew, rows, comp, bad_owner, bad_P, bad_z, bad_T0)
        assert stb.tolist() == [3] * 11 + [0, 0], stb
        assert np.all(Tb[:11] == 0.0) and np.all(rlb[:11] == 0.0) and np.all(rvb[:11] == 0.0)
        assert np.all(np.isnan(wb[:11]))
        for a, b in zip((T, w, rl, rv), (Tb, wb, rlb, rvb)):
            assert a[2:].tobytes() == b[11:].tobytes()
        # the z of a -1 slot is ignored, whatever it holds
        z_junk = zs[1:2].copy()
        z_junk[0, 2] = np.nan
        Tj, wj, _, _, stj = _solve(gpu_device, dew, rows, comp, np.array([1]), P[2:3], z_junk)
        assert stj[0] == 0 and Tj[0] == T[2] and np.array_equal(wj[0], w[2], equal_nan=True)
        none = _solve(gpu_device, dew, rows, comp, np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros((0, 3)))
        assert [v.shape for v in none] == [(0,), (0, 3), (0,), (0,), (0,)]


@pytest.mark.parametrize("dew", [False, True], ids=["bubble", "dew"])
def test_launch_edges_and_two_calls_give_the_same_bits(gpu_device, dew):
    """n = 1 and n one below, at and one above the block size, the same point (methane + butane + hexane) in every lane:
    every lane has the bits of the 30-point launch; two launches of the 30 points give the same bytes"""
    params, comp, owner, P, z, _ = _pooled(dew)
    first = _all_points(gpu_device, dew)
    j = 4
    assert first[4][j] == 0
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1):
        idx = np.full(n, j)
        got = _solve(gpu_device, dew, params, comp, owner[idx], P[idx], z[idx])
        for a, b in zip(got, first):
            assert a.shape[0] == n and a.tobytes() == b[idx].tobytes(), n
    again = _solve(gpu_device, dew, params, comp, owner, P, z)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def test_reference_shaped_io(gpu_device):
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    tern = [V.METHANE, V.BUTANE, V.HEXANE]
    name, _, Tf, x, fwd, _ = TR.cases()[2]
    assert name == "butane+hexane"
    for dew, one, batch in ((False, pcsaft.mix_bubble_t, pcsaft.mix_bubble_t_batch),
                            (True, pcsaft.mix_dew_t, pcsaft.mix_dew_t_batch)):
        # a named point: the numbers of the tensor form
        z = fwd["y"] if dew else x
        T, w = one(rows, [0.0, fwd["P"], *z])
        ref = _solve(gpu_device, dew, rows, np.array([[0, 1]], dtype=np.int64), [0], [fwd["P"]], np.array([z]))
        assert ref[4][0] == 0 and T == ref[0][0] and np.array_equal(w, ref[1][0])
        pooled = _all_points(gpu_device, dew)
        assert _rel(T, pooled[0][2]) <= 1e-12 and np.max(np.abs(w - pooled[1][2, :2])) <= 1e-12
        Tg, wg = one(rows, [123.0, fwd["P"], *z], t_init=0.9 * Tf)
        assert _rel(Tg, T) <= 1e-9 and np.max(np.abs(wg - w)) <= 1e-9
        # the batch form splits at the table cuts; a failed point is a row of NaN
        states = [np.array([[0.0, fwd["P"], *z], [0.0, 101325.0, 0.2, 0.8]]), np.zeros((0, 5)),
                  np.array([[0.0, 1e6, 0.1, 0.3, 0.6]]), np.array([[0.0, 1e7, 1.0]])]
        out = batch([rows, tern, tern, [V.METHANE]], states)
        assert [o.shape for o in out] == [(2, 3), (1, 4), (1, 2)]
        assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
        assert np.all(np.isnan(out[2]))  # methane alone at 10 MPa
        assert T == out[0][0, 0] and np.array_equal(w, out[0][0, 1:])
        with pytest.raises(RuntimeError):
            one([V.METHANE], [0.0, 1e7, 1.0])
        with pytest.raises(RuntimeError):
            one(rows, [0.0, -1.0, 0.5, 0.5])
        assert batch([rows], [np.zeros((0, 4))]) == []
        # a k_ij changes the answer, and the matrices reach the kernel
        Tk, _ = one(rows, [0.0, fwd["P"], *z], kij_matrix=[[0.0, 0.05], [0.05, 0.0]])
        print("k_ij = 0.05:", Tk, "against", T)
        assert abs(Tk / T - 1.0) > 1e-4


def test_txy_diagram(gpu_device):
    """butane + hexane at 101 325 Pa, 5 points: equally long lists, the end points are the two pure boiling temperatures,
    T falls and y0 >= x0 as the light component is added, and the P-x-y diagram at the temperature of the middle point
    passes through it: P within 1e-9 x d ln P / d ln T + 1e-9 (the bound of
    test_consistent_with_the_pressure_kernels at the floor of the oracle's change), y within the same."""
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    d = pcsaft.mix_vle_txy(rows, 101325.0, points=5)
    assert set(d) == set(pcsaft.mix_vle_pxy(rows, 350.0, points=2))
    assert all(len(v) == 5 for v in d.values()) and d["x0"] == [0.0, 0.25, 0.5, 0.75, 1.0]
    T = np.array(d["temperature"])
    p = _dev(gpu_device, np.array(rows, dtype=np.float64))[0]
    boil = pcsaft.vapor_pressure(p, _dev(gpu_device, np.array([T[-1], T[0]]))[0])[0].cpu().numpy()
    print("T", T, "pure vapour pressures at the end points", boil)
    assert np.max(np.abs(boil / 101325.0 - 1.0)) <= VP_TOL
    assert np.all(np.diff(T) < 0.0) and np.all(np.array(d["y0"]) >= np.array(d["x0"]))
    assert d["pressure"] == [101325.0] * 5 and d["y0"][0] == 0.0 and d["y0"][-1] == 1.0
    assert np.all(np.array(d["density liquid"]) > np.array(d["density vapor"]))
    lo, hi = (V.bubble(rows, [0.5, 0.5], T[2] * f)["P"] for f in (1.0 - 1e-3, 1.0 + 1e-3))
    slope = np.log(hi / lo) / np.log((1.0 + 1e-3) / (1.0 - 1e-3))
    bound = 1e-9 * slope + PRESSURE_TOL
    pxy = pcsaft.mix_vle_pxy(rows, T[2], points=5)
    print("P-x-y at", T[2], "K: P", pxy["pressure"][2], "y0", pxy["y0"][2], "against", d["y0"][2], "bound", bound)
    assert pxy["x0"][2] == 0.5 and _rel(pxy["pressure"][2], 101325.0) <= bound
    assert abs(pxy["y0"][2] - d["y0"][2]) <= bound
    with pytest.raises(ValueError, match="No VLE found"):
        pcsaft.mix_vle_txy(rows, 5e7, points=3)
