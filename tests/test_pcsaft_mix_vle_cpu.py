"""CPU side of the mixture bubble point: the oracle of tests/pcsaft_mix_vle_ref.py pinned on its own
(one component, the same row twice, a component swap, its own residuals, its convergence on the fixture), the binding
of the entry point, and the host checks of the reference-shaped functions of gnnepcsaft_amd/pcsaft.py."""
import os

import numpy as np
import pytest

from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return abs(a / b - 1.0)


def test_oracle_reduces_to_the_pure_vapour_pressure():
    """one component: p_sat, rho_l and rho_v of pcsaft_ref.vle at 1e-10 (seen: 6.8e-11 for hexane, 4.6e-11 for ethanol:
    what the loop's own tolerance of 1e-10 leaves); the same row twice at any split: y = x and that p_sat"""
    for row, T in ((V.HEXANE, 350.0), (V.ETHANOL, 330.0)):
        ref = R.vle(np.asarray(row, dtype=np.float64), T)
        one = V.bubble([row], [1.0], T)
        assert ref is not None and one is not None
        worst = max(_rel(one["P"], ref[0]), _rel(one["rho_l"], ref[1]), _rel(one["rho_v"], ref[2]))
        print("one component against pcsaft_ref.vle:", worst)
        assert worst <= 1e-10 and one["y"][0] == 1.0
    twice = V.bubble([V.HEXANE, V.HEXANE], [0.3, 0.7], 350.0)
    ref = R.vle(np.asarray(V.HEXANE, dtype=np.float64), 350.0)
    assert np.max(np.abs(twice["y"] - [0.3, 0.7])) <= 1e-9 and _rel(twice["P"], ref[0]) <= 1e-9


def test_oracle_component_swap():
    (_, rows, T, x) = V.NAMED[4]
    a = V.named_solves()[4][0]
    b = V.bubble(rows[::-1], x[::-1], T)
    print("swap: P", _rel(a["P"], b["P"]), "y", np.max(np.abs(a["y"] - b["y"][::-1])))
    assert _rel(a["P"], b["P"]) <= 1e-9 and np.max(np.abs(a["y"] - b["y"][::-1])) <= 1e-9


def test_oracle_residuals_on_the_named_points():
    """the oracle's own solutions meet the bounds the GPU test puts on the kernel's: equal pressures at 1e-9 and equal
    fugacities at 2e-10 + 10 x the disagreement of the oracle's two difference steps"""
    for (name, rows, T, x), (sol, change) in zip(V.NAMED, V.named_solves()):
        r = V.residuals(rows, x, sol["y"], T, sol["P"], sol["rho_l"], sol["rho_v"])
        scale = max(sol["P"], sol["rho_l"] * R.RGAS * T * 1e-3)
        print(name, "P", sol["P"], "iterations", sol["iterations"], "pressures", abs(r["p_l"] - sol["P"]) / scale,
              _rel(r["p_v"], sol["P"]), "fugacity", r["fugacity"], "two-step", r["own"], "1e-9 -> 1e-11", change)
        assert abs(r["p_l"] - sol["P"]) <= 1e-9 * scale and _rel(r["p_v"], sol["P"]) <= 1e-9
        assert r["fugacity"] <= 2e-10 + 10.0 * r["own"]
        assert abs(sol["y"].sum() - 1.0) <= 1e-12 and sol["rho_l"] > sol["rho_v"] > 0.0


def test_oracle_converges_on_the_fixture():
    sols = V.fixture_solves()
    done = [s for s in sols if s is not None]
    print("converged:", len(done), "of", len(sols), "most iterations:", max(s["iterations"] for s in done),
          "pressures from", min(s["P"] for s in done), "to", max(s["P"] for s in done))
    assert len(sols) == 24 and len(done) >= 23


def test_binding_declares_the_bubble_entry_point():
    from gnnepcsaft_amd import _lib
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_mix_bubble is not None
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_bubble"][1]) == 17
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26 and lib.gnx_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    assert "int32_t gnx_pcsaft_mix_bubble(" in header
    assert "GNX_K_COUNT = 26" in header and "#define GNX_ABI_VERSION 7" in header


@pytest.mark.parametrize("name", ["mix_bubble", "mix_vle_pxy"])
def test_reference_shaped_functions_reject_malformed_input(name):
    """the checks that run on the host before anything is uploaded"""
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    second = [350.0, 0.0, 0.5, 0.5] if name == "mix_bubble" else 350.0
    fn = getattr(pcsaft, name)
    with pytest.raises(ValueError):
        fn(rows, second, kij_matrix=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        fn(rows, second, epsilon_ab=np.zeros((2, 3)))
    if name == "mix_bubble":
        with pytest.raises(ValueError):
            fn(rows * 3, [350.0, 0.0] + [1.0 / 6] * 6)
        with pytest.raises(ValueError):
            fn(rows, [350.0, 0.0, 0.5, 0.3, 0.2])
    else:
        with pytest.raises(ValueError):
            fn([V.HEXANE], 350.0)
        with pytest.raises(ValueError):
            fn([V.METHANE, V.BUTANE, V.HEXANE], 350.0)
        with pytest.raises(ValueError):
            fn(rows, 350.0, points=1)


def test_batch_form_rejects_malformed_input():
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    with pytest.raises(ValueError):
        pcsaft.mix_bubble_batch([rows], [np.zeros((1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError):
        pcsaft.mix_bubble_batch([rows], [np.zeros((1, 5))])
    with pytest.raises(ValueError):
        pcsaft.mix_bubble_batch([rows], [np.zeros((1, 4))], kij=[np.zeros((3, 3))])
    assert pcsaft.mix_bubble_batch([rows], [np.zeros((0, 4))]) == []
