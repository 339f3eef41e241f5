"""CPU side of the mixture stability test: the pinned case table against the oracles it was built from,
the oracle of tests/pcsaft_mix_stab_ref.py on every pinned verdict, ``distance`` on its own ground, the binding of the
entry point, and the host checks of the reference-shaped functions of gnnepcsaft_amd/pcsaft.py."""
import os
import re

import numpy as np
import pytest

from tests import pcsaft_mix_flash_ref as F
from tests import pcsaft_mix_stab_ref as S
from tests import pcsaft_mix_vle_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return abs(a / b - 1.0)


def test_pinned_table_is_what_the_oracles_give():
    """The literals of ``S.CASES`` against the functions they were computed with, P at 1e-12 relative and z at 1e-12: 12
    tie-line feeds, 4 single-phase points, x of five named bubble points and y of all six at 0.98 and 1.02 x the bubble
    pressure, five water + n-hexane feeds at 300 K and 1e5 Pa."""
    cases = S.cases()
    assert [c[0] for c in cases] == (["tie line"] * 12 + ["single phase"] * 4 + ["bubble side"] * 10 + ["dew side"] * 12
                                     + ["liquid-liquid"] * 5)
    assert len(set(c[1] for c in cases)) == 43
    expect = [(name, rows, T, P, z, False) for name, rows, T, P, z, _, _, _ in F.tie_line_points()]
    expect += [(name, rows, T, P, z, True) for name, rows, T, P, z in F.single_phase_points()]
    named = list(zip(V.NAMED, V.named_solves()))
    for (name, rows, T, x), (sol, _) in named:
        if name != "ethanol+water":
            expect += [(f"{name} x {f}", rows, T, f * sol["P"], x, f > 1.0) for f in (0.98, 1.02)]
    for (name, rows, T, x), (sol, _) in named:
        upper = name == "methane+hexane 0.4"  # an upper, retrograde dew point: the two-phase side is below it
        expect += [(f"{name} y {f}", rows, T, f * sol["P"], sol["y"], (f < 1.0) != upper) for f in (0.98, 1.02)]
    assert len(expect) == 38
    for (_, name, rows, T, P, z, stable), (ename, erows, eT, eP, ez, estable) in zip(cases, expect):
        assert name == ename and stable == estable and T == eT, (name, ename)
        assert np.array_equal(rows, np.asarray(erows, dtype=np.float64)) and _rel(P, eP) <= 1e-12
        assert np.max(np.abs(z - np.asarray(ez))) <= 1e-12, name
    for (_, _, rows, T, P, z, stable), zw, estable in zip(cases[38:], (0.5, 0.999, 1e-3, 1e-6, 1 - 1e-9),
                                                          (False, False, True, True, True)):
        assert np.array_equal(rows, np.asarray([V.WATER, V.HEXANE])) and (T, P, stable) == (300.0, 1e5, estable)
        assert z[0] == zw and z[1] == 1.0 - zw


def test_oracle_reproduces_every_pinned_verdict():
    """All 43 cases, all nc + 2 trials each, none inconclusive.  Seen: every negative distance comes within 2 steps (D
    from -0.0028 to -3.9); trivial trials take 1 to 53 steps; stationary ones 5 to 13, and 181 on the water-rich trial of
    "ethanol+water y 0.98" (D = +0.0196); "methane+butane+hexane above the bubble point" is stable on a non-trivial
    stationary point with D = +0.347, water + n-hexane at z_water = 1e-3 on one with D = +1.51; the water + n-hexane feed
    0.5, which the flash oracle calls "single", is unstable on all four trials."""
    cases, solves = S.cases(), S.table_solves()
    assert len(cases) == len(solves) == 43
    kinds = {"trivial": 0, "negative": 0, "stationary": 0}
    for (group, name, rows, T, P, z, stable), per in zip(cases, solves):
        assert len(per) == len(z) + 2 and all(p is not None for p in per), (name, per)
        trials = [p[0] for p in per]
        print(group, name, [(t["kind"], t["steps"], t["tpd"]) for t in trials])
        assert S.verdict(trials) is stable, name
        for t, (_, change) in zip(trials, per):
            kinds[t["kind"]] += 1
            assert t["steps"] <= S.MAX_STEPS and abs(t["w"].sum() - 1.0) <= 1e-12
            assert (t["kind"] == "trivial") == (t["tpd"] == 0.0) and (t["kind"] == "negative") == (t["tpd"] < S.NEGATIVE)
            assert (change is not None) == (t["kind"] == "stationary")
    print(kinds)
    assert min(kinds.values()) > 0
    assert F.flash(cases[38][2], cases[38][5], 300.0, 1e5) == "single"


def test_distance_on_its_own_ground():
    """at w = z, D = 0 and both pressures are P; for a tie-line feed against the vapour end of its tie line, D is the sum
    over ``V.ln_fugacity`` written out, and negative: the feed is unstable"""
    _, name, rows, T, P, z, _ = S.cases()[2]
    rho_z, lnf_z = S.state(rows, z, T, P)
    same = S.distance(rows, z, z, T, rho_z, rho_z)
    print(name, same)
    assert same["D"] == 0.0 and same["stationarity"] == 0.0
    assert _rel(same["p_z"], P) <= 1e-9 and same["p_z"] == same["p_w"] and 0.0 <= same["own"] < 1e-8
    tie, (sol, _) = F.tie_line_points()[2], V.named_solves()[2]
    assert tie[0] == name and np.max(np.abs(tie[4] - z)) <= 1e-12
    y, rho_v = sol["y"], sol["rho_v"]
    other = S.distance(rows, z, y, T, rho_z, rho_v)
    direct = float(np.sum(y * (V.ln_fugacity(rows, y, T, rho_v) - V.ln_fugacity(rows, z, T, rho_z))))
    print(other, direct)
    assert abs(other["D"] - direct) <= 1e-14 and direct < -0.01 and _rel(other["p_w"], P) <= 1e-9
    assert other["stationarity"] > 1e-6  # the end of a tie line is no stationary point of this feed


def test_oracle_reductions():
    """one component and the same row twice are stable with every trial trivial"""
    for rows, z in (([V.HEXANE], [1.0]), ([V.HEXANE, V.HEXANE], [0.3, 0.7])):
        stable, trials = S.stability(rows, z, 350.0, 4e5)
        assert stable is True and all(t["kind"] == "trivial" for t in trials)


def test_binding_declares_the_stability_entry_point():
    from gnnepcsaft_amd import _lib, build
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_mix_stability is not None and "gnx_pcsaft_mix_stab.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    decl = re.search(r"int32_t gnx_pcsaft_mix_stability\(([^;]*)\);", header)
    assert decl is not None and "is_stable_feos" in header and "kij.py:30" in header
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_stability"][1]) == len(decl.group(1).split(",")) == 19
    assert "const int64_t* trial" in decl.group(1)
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26 and lib.gnx_abi_version() == 7
    assert "GNX_K_COUNT = 26" in header and "#define GNX_ABI_VERSION 7" in header


def test_host_functions_need_a_device():
    """there is no CPU path: without a HIP device ``pcsaft._device`` raises GnxError, and so does every well-formed call"""
    import torch
    from gnnepcsaft_amd import _lib, pcsaft
    rows = [V.BUTANE, V.HEXANE]
    calls = (pcsaft._device,
             lambda: pcsaft.mix_is_stable(rows, [350.0, 4e5, 0.5, 0.5]),
             lambda: pcsaft.mix_stability_batch([rows], [np.array([[350.0, 4e5, 0.5, 0.5]])]))
    if not torch.cuda.is_available():
        for call in calls:
            with pytest.raises(_lib.GnxError, match="no CPU fallback"):
                call()
    assert callable(pcsaft.mixture_stability) and callable(pcsaft.ops.pcsaft_mix_stability)


def test_reduction_of_the_trials():
    """``pcsaft._reduce_trials`` on host tensors: a negative trial wins over a failed one; a failed trial without one
    makes the point inconclusive, 3 over 1; all trivial gives 0.0 and the feed; else the smallest stationary value"""
    import torch
    from gnnepcsaft_amd import pcsaft
    nan = float("nan")
    tpd = torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.0, -1.0, nan, -2.0], [0.0, 0.5, nan, 0.2], [0.3, 0.0, 0.1, 0.0],
                        [nan, 0.0, nan, 0.0]], dtype=torch.float64)
    status = torch.tensor([[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0], [3, 0, 1, 0]], dtype=torch.int32)
    w = torch.arange(5 * 4 * 2, dtype=torch.float64).view(5, 4, 2)
    w[2, 2] = nan
    stable, d, wp, st = pcsaft._reduce_trials(tpd, w, status)
    assert stable.tolist() == [True, False, False, True, False] and st.tolist() == [0, 0, 1, 0, 3] and st.dtype == torch.int32
    assert d[:2].tolist() == [0.0, -2.0] and d[3].item() == 0.1 and torch.isnan(d[[2, 4]]).all()
    assert wp[0].tolist() == [0.0, 1.0] and wp[1].tolist() == [14.0, 15.0] and wp[3].tolist() == [28.0, 29.0]
    assert torch.isnan(wp[[2, 4]]).all()


def test_reference_shaped_functions_reject_malformed_input():
    """the checks that run on the host before anything is uploaded"""
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    state = [350.0, 4e5, 0.5, 0.5]
    for init in ("liquid", "vapor", ""):
        with pytest.raises(ValueError, match="density_initialization"):
            pcsaft.mix_is_stable(rows, state, density_initialization=init)
    with pytest.raises(ValueError):
        pcsaft.mix_is_stable(rows, state, kij_matrix=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        pcsaft.mix_is_stable(rows, state, epsilon_ab=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        pcsaft.mix_is_stable(rows * 3, [350.0, 4e5] + [1.0 / 6] * 6)
    with pytest.raises(ValueError):
        pcsaft.mix_is_stable(rows, [350.0, 4e5, 0.5, 0.3, 0.2])
    with pytest.raises(ValueError):
        pcsaft.mix_stability_batch([rows], [np.zeros((1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError):
        pcsaft.mix_stability_batch([rows], [np.zeros((1, 5))])
    with pytest.raises(ValueError):
        pcsaft.mix_stability_batch([rows], [np.zeros((1, 4))], kij=[np.zeros((3, 3))])
    assert pcsaft.mix_stability_batch([rows], [np.zeros((0, 4))]) == []
