"""CPU side of the mixture dew point: the oracle of tests/pcsaft_mix_dew_ref.py pinned on its own (its
convergence on the vapours of the 30 bubble points, its own residuals, one component, the same row twice, a component
swap), the binding of the entry point, and the host checks of the reference-shaped functions of gnnepcsaft_amd/pcsaft.py."""
import os

import numpy as np
import pytest

from tests import pcsaft_mix_dew_ref as D
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return abs(a / b - 1.0)


def test_oracle_converges_and_returns_to_the_bubble_points():
    """from the Raoult start the substitution ends on all 30 vapours, and 28 of the dew points are the bubble points the
    vapours came from; the other two ("methane+hexane 0.4", retrograde, and "fixture 15", whose y two liquids share)
    are another dew point of the same vapour.  Steps: 5 to 40, and 167 for ethanol + water."""
    cases, sols = D.cases(), D.solves()
    solved = [s is not None for s, _, _ in sols]
    returning = [r for _, _, r in sols]
    steps = {name: s["iterations"] for (name, *_), (s, _, _) in zip(cases, sols) if s is not None}
    print("solved", sum(solved), "of", len(cases), "returning", sum(returning), "not returning:",
          [c[0] for c, s, r in zip(cases, solved, returning) if s and not r])
    print("steps:", steps)
    assert len(cases) == 30 and sum(solved) >= 29 and sum(returning) >= 27
    # the kernel's cap is at least twice what the oracle needs
    assert 2 * max(steps.values()) <= D.MAX_ITERATIONS


def test_oracle_residuals_at_every_solution():
    """the oracle's own solutions meet the bounds the GPU test puts on the kernel's: equal pressures at 1e-9 and equal
    fugacities at 2e-10 + 10 x the disagreement of the oracle's two difference steps; sum x = 1, rho_l > rho_v > 0"""
    for (name, rows, T, y, _), (sol, change, returns) in zip(D.cases(), D.solves()):
        if sol is None:
            continue
        r = V.residuals(rows, sol["x"], y, T, sol["P"], sol["rho_l"], sol["rho_v"])
        scale = max(sol["P"], sol["rho_l"] * R.RGAS * T * 1e-3)
        print(name, "P", sol["P"], "iterations", sol["iterations"], "returns", returns, "pressures",
              abs(r["p_l"] - sol["P"]) / scale, _rel(r["p_v"], sol["P"]), "fugacity", r["fugacity"], "two-step", r["own"],
              "1e-9 -> 1e-11", change)
        assert abs(r["p_l"] - sol["P"]) <= 1e-9 * scale and _rel(r["p_v"], sol["P"]) <= 1e-9, name
        assert r["fugacity"] <= 2e-10 + 10.0 * r["own"], name
        assert abs(sol["x"].sum() - 1.0) <= 1e-12 and sol["rho_l"] > sol["rho_v"] > 0.0, name


def test_oracle_reduces_to_the_pure_vapour_pressure():
    """one component: p_sat, rho_l and rho_v of pcsaft_ref.vle at 1e-9 and x == 1.0; the same row twice at any split:
    x = y and that p_sat"""
    for row, T in ((V.HEXANE, 350.0), (V.ETHANOL, 330.0)):
        ref = R.vle(np.asarray(row, dtype=np.float64), T)
        one = D.dew([row], [1.0], T)
        assert ref is not None and one is not None
        worst = max(_rel(one["P"], ref[0]), _rel(one["rho_l"], ref[1]), _rel(one["rho_v"], ref[2]))
        print("one component against pcsaft_ref.vle:", worst, "iterations", one["iterations"])
        assert worst <= 1e-9 and one["x"][0] == 1.0
    twice = D.dew([V.HEXANE, V.HEXANE], [0.3, 0.7], 350.0)
    ref = R.vle(np.asarray(V.HEXANE, dtype=np.float64), 350.0)
    assert np.max(np.abs(twice["x"] - [0.3, 0.7])) <= 1e-9 and _rel(twice["P"], ref[0]) <= 1e-9
    assert D.dew([V.METHANE], [1.0], 300.0) is None  # above its critical temperature: no start


def test_oracle_component_swap():
    (_, rows, T, y, _) = D.cases()[4]
    a = D.solves()[4][0]
    b = D.dew(rows[::-1], y[::-1], T)
    print("swap: P", _rel(a["P"], b["P"]), "x", np.max(np.abs(a["x"] - b["x"][::-1])))
    assert _rel(a["P"], b["P"]) <= 1e-9 and np.max(np.abs(a["x"] - b["x"][::-1])) <= 1e-9


def test_binding_declares_the_dew_entry_point():
    from gnnepcsaft_amd import _lib
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_mix_dew is not None
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_dew"][1]) == 17
    assert _lib.SIGNATURES["gnx_pcsaft_mix_dew"] == _lib.SIGNATURES["gnx_pcsaft_mix_bubble"]
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26 and lib.gnx_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    assert "int32_t gnx_pcsaft_mix_dew(" in header
    assert "GNX_K_COUNT = 26" in header and "#define GNX_ABI_VERSION 7" in header


@pytest.mark.parametrize("name", ["mix_dew", "mix_vp"])
def test_reference_shaped_functions_reject_malformed_input(name):
    """the checks that run on the host before anything is uploaded"""
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    state = [350.0, 0.0, 0.5, 0.5]
    fn = getattr(pcsaft, name)
    with pytest.raises(ValueError):
        fn(rows, state, kij_matrix=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        fn(rows, state, epsilon_ab=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        fn(rows * 3, [350.0, 0.0] + [1.0 / 6] * 6)
    with pytest.raises(ValueError):
        fn(rows, [350.0, 0.0, 0.5, 0.3, 0.2])


def test_batch_form_rejects_malformed_input():
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    with pytest.raises(ValueError):
        pcsaft.mix_dew_batch([rows], [np.zeros((1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError):
        pcsaft.mix_dew_batch([rows], [np.zeros((1, 5))])
    with pytest.raises(ValueError):
        pcsaft.mix_dew_batch([rows], [np.zeros((1, 4))], kij=[np.zeros((3, 3))])
    assert pcsaft.mix_dew_batch([rows], [np.zeros((0, 4))]) == []
