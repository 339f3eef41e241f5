"""CPU side of the mixture bubble and dew temperatures: the oracle of tests/pcsaft_mix_tvle_ref.py
pinned on its own (the inverse problems of the 30 bubble points from its own start and from a given one, its residuals,
one component), the binding of the two entry points, and the host checks of the reference-shaped functions of
gnnepcsaft_amd/pcsaft.py."""
import os

import numpy as np
import pytest

from tests import pcsaft_mix_tvle_ref as TR
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return abs(a / b - 1.0)


def _check_returns(label, sols, dew, may_fail=(), equations_only=()):
    """every solved case returns the forward (T, composition) within ``TR.bound``; -> (solved, worst T, worst w, steps)"""
    worst_t = worst_w = 0.0
    solved, steps = 0, {}
    for (name, rows, T, x, fwd, _), (sol, change) in zip(TR.cases(), sols):
        if sol is None:
            assert name in may_fail, f"{label}: {name} is not solved"
            continue
        solved += 1
        steps[name] = sol["iterations"]
        if name in equations_only:
            continue
        ref = x if dew else fwd["y"]
        dt, dw = _rel(sol["T"], T), float(np.max(np.abs(sol["w"] - ref)))
        worst_t, worst_w = max(worst_t, dt), max(worst_w, dw)
        assert dt <= TR.bound(change) and dw <= TR.bound(change), (label, name, dt, dw, TR.bound(change))
    print(label, "solved", solved, "of 30; worst T", worst_t, "worst composition", worst_w)
    print(label, "steps", steps)
    return solved, worst_t, worst_w, steps


def test_bubble_from_its_own_start():
    """28 of the 30 cases are solved; "methane+hexane 0.4" (8.45 MPa) and "fixture 0" (5.18 MPa) are near-critical and
    the ideal-vapour start never reaches their P.  Every solved one returns the forward T and y: worst 1.9e-11 in T,
    2.6e-11 in y here; 4 to 13 steps."""
    solved, _, _, steps = _check_returns("bubble, own start", TR.bubble_solves(), False, may_fail=TR.NEAR_CRITICAL)
    assert solved >= 28
    assert 2 * max(steps.values()) <= TR.MAX_ITERATIONS


def test_bubble_from_a_given_start():
    """with T0 = 0.9 T all 30 are solved and return: worst 2.6e-11 in T and 2.3e-11 in y here; 4 to 14 steps"""
    solved, _, _, _ = _check_returns("bubble, T0 = 0.9 T", TR.bubble_solves(0.9), False)
    assert solved == 30


def test_dew_from_its_own_start():
    """at least 27 of the 30 return the forward (T, x): worst 1.2e-11 in T and 1.7e-10 in x (ethanol + water, whose bound
    is 2.6e-8: 167 steps of a slowly converging substitution) here; the other steps 6 to 39.  The two near-critical
    cases may fail, and "fixture 15" ends on another dew point of the same vapour (T off by 4 %): it is held to the
    equations only."""
    sols = TR.dew_solves()
    solved, _, _, steps = _check_returns("dew, own start", sols, True, may_fail=TR.NEAR_CRITICAL,
                                         equations_only=TR.OTHER_DEW_POINT)
    assert solved >= 28 and solved - len(TR.OTHER_DEW_POINT) >= 27
    assert 2 * max(steps.values()) <= TR.MAX_ITERATIONS


def test_the_start_takes_few_estimates():
    """the secant of the start ends within 7 estimates on every case whose pressure it reaches: the kernel's cap is more
    than twice that"""
    most = max(_start_counts())
    print("most estimates of a start:", most)
    assert 2 * most <= TR.START_EVALUATIONS


def _start_counts():
    out = []
    for (name, rows, T, x, fwd, _) in TR.cases():
        for dew in (False, True):
            count = []
            if TR.start(rows, fwd["y"] if dew else x, fwd["P"], dew=dew, count=count) is not None:
                out.append(count[0])
    return out


def test_oracle_residuals_at_every_solution():
    """every solved state meets the equations at the bounds of test_oracle_residuals_on_the_named_points: both pressures
    are P at 1e-9 (the liquid's on the scale max(P, 1e-3 rho R T)), the fugacities agree within 2e-10 + 10 x the
    disagreement of the oracle's two difference steps; sum w = 1, rho_l > rho_v > 0"""
    for dew, sols in ((False, TR.bubble_solves()), (False, TR.bubble_solves(0.9)), (True, TR.dew_solves())):
        for (name, rows, T, x, fwd, _), (sol, change) in zip(TR.cases(), sols):
            if sol is None:
                continue
            z, P = (fwd["y"] if dew else x), fwd["P"]
            liquid, vapour = (sol["w"], z) if dew else (z, sol["w"])
            r = V.residuals(rows, liquid, vapour, sol["T"], P, sol["rho_l"], sol["rho_v"])
            scale = max(P, sol["rho_l"] * R.RGAS * sol["T"] * 1e-3)
            print("dew" if dew else "bubble", name, "T", sol["T"], "pressures", abs(r["p_l"] - P) / scale,
                  _rel(r["p_v"], P), "fugacity", r["fugacity"], "two-step", r["own"], "1e-9 -> 1e-11", change)
            assert abs(r["p_l"] - P) <= 1e-9 * scale and _rel(r["p_v"], P) <= 1e-9, name
            assert r["fugacity"] <= 2e-10 + 10.0 * r["own"], name
            assert abs(sol["w"].sum() - 1.0) <= 1e-12 and sol["rho_l"] > sol["rho_v"] > 0.0, name


def test_oracle_reduces_to_the_pure_boiling_temperature():
    """one component: at P = p_sat(T) of pcsaft_ref.vle the bubble and the dew temperature are T at 1e-9, w == 1.0"""
    for row, T in ((V.HEXANE, 350.0), (V.ETHANOL, 330.0)):
        ref = R.vle(np.asarray(row, dtype=np.float64), T)
        assert ref is not None
        for dew in (False, True):
            one = TR.solve([row], [1.0], ref[0], dew=dew)
            assert one is not None
            worst = max(_rel(one["T"], T), _rel(one["rho_l"], ref[1]), _rel(one["rho_v"], ref[2]))
            print("one component against pcsaft_ref.vle:", worst, "iterations", one["iterations"])
            assert worst <= 1e-9 and one["w"][0] == 1.0
    # 10 MPa is above methane's critical pressure: no temperature at which it boils
    assert TR.solve([V.METHANE], [1.0], 1e7) is None and TR.solve([V.METHANE], [1.0], 1e7, dew=True) is None


def test_binding_declares_the_temperature_entry_points():
    from gnnepcsaft_amd import _lib
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_mix_bubble_t is not None and lib.gnx_pcsaft_mix_dew_t is not None
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_bubble_t"][1]) == 18
    assert _lib.SIGNATURES["gnx_pcsaft_mix_bubble_t"] == _lib.SIGNATURES["gnx_pcsaft_mix_dew_t"]
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26 and lib.gnx_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    assert "int32_t gnx_pcsaft_mix_bubble_t(" in header and "int32_t gnx_pcsaft_mix_dew_t(" in header
    assert "GNX_K_COUNT = 26" in header and "#define GNX_ABI_VERSION 7" in header


@pytest.mark.parametrize("name", ["mix_bubble_t", "mix_dew_t"])
def test_reference_shaped_functions_reject_malformed_input(name):
    """the checks that run on the host before anything is uploaded"""
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    state = [0.0, 101325.0, 0.5, 0.5]
    fn = getattr(pcsaft, name)
    with pytest.raises(ValueError):
        fn(rows, state, kij_matrix=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        fn(rows, state, epsilon_ab=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        fn(rows * 3, [0.0, 101325.0] + [1.0 / 6] * 6)
    with pytest.raises(ValueError):
        fn(rows, [0.0, 101325.0, 0.5, 0.3, 0.2])


def test_diagram_rejects_malformed_input():
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    with pytest.raises(ValueError):
        pcsaft.mix_vle_txy(rows + [V.METHANE], 101325.0)
    with pytest.raises(ValueError):
        pcsaft.mix_vle_txy([V.HEXANE], 101325.0)
    with pytest.raises(ValueError):
        pcsaft.mix_vle_txy(rows, 101325.0, points=1)
    with pytest.raises(ValueError):
        pcsaft.mix_vle_txy(rows, 101325.0, kij_matrix=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        pcsaft.mix_vle_txy(rows, 101325.0, epsilon_ab=np.zeros((2, 3)))


@pytest.mark.parametrize("name", ["mix_bubble_t_batch", "mix_dew_t_batch"])
def test_batch_forms_reject_malformed_input(name):
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    fn = getattr(pcsaft, name)
    with pytest.raises(ValueError):
        fn([rows], [np.zeros((1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError):
        fn([rows], [np.zeros((1, 5))])
    with pytest.raises(ValueError):
        fn([rows], [np.zeros((1, 4))], kij=[np.zeros((3, 3))])
    assert fn([rows], [np.zeros((0, 4))]) == []
