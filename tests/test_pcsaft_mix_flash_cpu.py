"""CPU side of the mixture (T, P) flash: the oracle of tests/pcsaft_mix_flash_ref.py pinned on its own
(tie-line feeds split into their ends, the single-phase points, one component, the same row twice, a component swap), the
binding of the entry point, and the host checks of the reference-shaped functions of gnnepcsaft_amd/pcsaft.py."""
import os
import re

import numpy as np
import pytest

from tests import pcsaft_mix_flash_ref as F
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return abs(a / b - 1.0)


def test_oracle_splits_every_tie_line_feed_into_its_ends():
    """The 12 tie-line points (the six named bubble points at beta = 0.3, all of them: "methane+hexane 0.4" is solved, in
    17 steps, and stays; the fixture cases 0 to 5 at beta = 0.5): the oracle's flash solves every one within its 200
    steps and returns the x and y of the bubble point within max(1e-9, 10 x its own change between the tolerances 1e-9
    and 1e-11), beta within that bound over max_i |y_i - x_i| (the lever rule), the material balance at 1e-12, and its
    state meets the bounds the GPU test puts on the kernel's.  Fixture case 0 (5.2 MPa, near-critical) has no liquid of
    its feed at zero pressure: the start falls back to the highest root of z at P.  Seen: 5 to 17 steps, 169 on ethanol +
    water (a factor 0.89 per step); x within 4.0e-10, y within 9.1e-11, beta within 1.2e-9."""
    points, solves = F.tie_line_points(), F.tie_line_solves()
    assert len(points) == 12 and [p[0] for p in points[:6]] == [c[0] for c in V.NAMED]
    for (name, rows, T, P, z, x, y, beta), (sol, change) in zip(points, solves):
        assert isinstance(sol, dict), (name, sol)
        bound = max(1e-9, 10.0 * change)
        dx, dy = float(np.max(np.abs(sol["x"] - x))), float(np.max(np.abs(sol["y"] - y)))
        db = abs(sol["beta"] - beta)
        r = V.residuals(rows, sol["x"], sol["y"], T, P, sol["rho_l"], sol["rho_v"])
        scale = max(P, sol["rho_l"] * R.RGAS * T * 1e-3)
        print(name, "P", P, "steps", sol["iterations"], "dx", dx, "dy", dy, "dbeta", db, "bound", bound, "balance",
              F.balance(z, sol["x"], sol["y"], sol["beta"]), "fugacity", r["fugacity"], "two-step", r["own"])
        assert sol["iterations"] <= 200 and dx <= bound and dy <= bound and db <= bound / np.max(np.abs(y - x))
        assert F.balance(z, sol["x"], sol["y"], sol["beta"]) <= 1e-12
        assert abs(sol["x"].sum() - 1.0) <= 1e-12 and abs(sol["y"].sum() - 1.0) <= 1e-12
        assert 0.0 < sol["beta"] < 1.0 and sol["rho_l"] > sol["rho_v"] > 0.0
        assert abs(r["p_l"] - P) <= 1e-9 * scale and _rel(r["p_v"], P) <= 1e-9
        assert r["fugacity"] <= 2e-10 + 10.0 * r["own"]


def test_oracle_single_phase():
    """above the bubble pressure of the feed and below every vapour pressure there is no split; neither for one
    component, nor for the same row twice, at any pressure away from the vapour pressure"""
    for name, rows, T, P, z in F.single_phase_points():
        assert F.flash(rows, z, T, P) == "single", name
    psat = R.vle(np.asarray(V.HEXANE, dtype=np.float64), 350.0)[0]
    for factor in (0.5, 0.99, 1.01, 2.0):
        assert F.flash([V.HEXANE], [1.0], 350.0, factor * psat) == "single"
        assert F.flash([V.HEXANE, V.HEXANE], [0.3, 0.7], 350.0, factor * psat) == "single"
    assert F.flash([V.METHANE], [1.0], 300.0, 1e6) == "single"


def test_oracle_component_swap():
    name, rows, T, P, z, x, y, beta = F.tie_line_points()[4]
    a = F.tie_line_solves()[4][0]
    b = F.flash(rows[::-1], z[::-1], T, P)
    worst = max(abs(a["beta"] - b["beta"]), np.max(np.abs(a["x"] - b["x"][::-1])), np.max(np.abs(a["y"] - b["y"][::-1])))
    print("swap:", worst)
    assert worst <= 1e-9


def test_rachford_rice():
    """the root is inside the negative-flash window whether beta is inside [0, 1] or not; no root without a K on each
    side of 1"""
    z = np.array([0.2, 0.3, 0.5])
    for K in ([5.0, 1.2, 0.1], [1.5, 0.9, 0.2], [40.0, 2.0, 0.7]):
        K = np.array(K)
        beta = F.rachford_rice(z, K)
        x = z / (1.0 + beta * (K - 1.0))
        assert 1.0 / (1.0 - K.max()) < beta < 1.0 / (1.0 - K.min()) and np.all(x > 0.0)
        assert abs(x.sum() - 1.0) <= 1e-14 and abs((K * x).sum() - 1.0) <= 1e-14
    assert F.rachford_rice(z, np.array([3.0, 2.0, 1.1])) is None
    assert F.rachford_rice(z, np.array([0.9, 0.5, 0.1])) is None


def test_binding_declares_the_flash_entry_point():
    from gnnepcsaft_amd import _lib
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_mix_flash is not None
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    decl = re.search(r"int32_t gnx_pcsaft_mix_flash\(([^;]*)\);", header)
    assert decl is not None
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_flash"][1]) == len(decl.group(1).split(",")) == 19
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26 and lib.gnx_abi_version() == 7
    assert "GNX_K_COUNT = 26" in header and "#define GNX_ABI_VERSION 7" in header


def test_status_and_reason():
    from gnnepcsaft_amd import pcsaft
    assert pcsaft.STATUS_SINGLE_PHASE == 4 and "single phase" in pcsaft._REASON[pcsaft.STATUS_SINGLE_PHASE]
    assert (pcsaft.STATUS_OK, pcsaft.STATUS_NO_CONVERGENCE, pcsaft.STATUS_SUPERCRITICAL, pcsaft.STATUS_BAD_INPUT) == (0, 1, 2, 3)


def test_host_functions_need_a_device():
    """there is no CPU path: without a HIP device a well-formed call raises GnxError, as every function of the module"""
    import torch
    from gnnepcsaft_amd import _lib, pcsaft
    rows = [V.BUTANE, V.HEXANE]
    calls = (lambda: pcsaft.mix_tp_flash(rows, [350.0, 4e5, 0.5, 0.5]),
             lambda: pcsaft.mix_tp_flash_batch([rows], [np.array([[350.0, 4e5, 0.5, 0.5]])]),
             lambda: pcsaft.mix_flash_x1(rows, [[350.0, 4e5]], [0.3, 0.6]))
    if not torch.cuda.is_available():
        for call in calls:
            with pytest.raises(_lib.GnxError):
                call()
    assert callable(pcsaft.mixture_tp_flash)


def test_reference_shaped_functions_reject_malformed_input():
    """the checks that run on the host before anything is uploaded"""
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    state = [350.0, 4e5, 0.5, 0.5]
    with pytest.raises(ValueError):
        pcsaft.mix_tp_flash(rows, state, kij_matrix=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        pcsaft.mix_tp_flash(rows, state, epsilon_ab=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        pcsaft.mix_tp_flash(rows * 3, [350.0, 4e5] + [1.0 / 6] * 6)
    with pytest.raises(ValueError):
        pcsaft.mix_tp_flash(rows, [350.0, 4e5, 0.5, 0.3, 0.2])
    with pytest.raises(ValueError):
        pcsaft.mix_tp_flash_batch([rows], [np.zeros((1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError):
        pcsaft.mix_tp_flash_batch([rows], [np.zeros((1, 5))])
    with pytest.raises(ValueError):
        pcsaft.mix_tp_flash_batch([rows], [np.zeros((1, 4))], kij=[np.zeros((3, 3))])
    assert pcsaft.mix_tp_flash_batch([rows], [np.zeros((0, 4))]) == []
    with pytest.raises(ValueError):
        pcsaft.mix_flash_x1([V.HEXANE], [[350.0, 4e5]], [0.5])
    with pytest.raises(ValueError):
        pcsaft.mix_flash_x1([V.METHANE, V.BUTANE, V.HEXANE], [[350.0, 4e5]], [0.5])
    with pytest.raises(ValueError):
        pcsaft.mix_flash_x1(rows, [350.0, 4e5], [0.5])
    with pytest.raises(ValueError):
        pcsaft.mix_flash_x1(rows, [[350.0, 4e5, 0.5]], [0.5])
    with pytest.raises(ValueError):
        pcsaft.mix_flash_x1(rows, [[350.0, 4e5]], [[0.5, 0.6]])
    with pytest.raises(ValueError):
        pcsaft.mix_flash_x1(rows, [[350.0, 4e5]], [])
    with pytest.raises(ValueError):
        pcsaft.mix_flash_x1(rows, [[350.0, 4e5]], [0.5], kij_matrix=np.zeros((3, 3)))
    assert pcsaft.mix_flash_x1(rows, np.zeros((0, 2)), [0.5]).shape == (0,)
