"""CPU side of the mixture fugacity coefficients: the finite-difference oracle of
tests/pcsaft_mix_phi_ref.py pinned on its own, the bindings of the two entry points, and the host logic of the
reference-shaped functions of gnnepcsaft_amd/pcsaft.py."""
import os

import numpy as np
import pytest

from tests import pcsaft_mix_cases as C
from tests import pcsaft_mix_phi_ref as PR
from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a handful of fixture points of different class pairs (the whole sample runs against the kernel in the GPU test)
POINTS = PR.sample()[::6]


def _point(j):
    params, comp, owner, T, _, x, _ = C.fixture_points()
    return params[comp[owner[j]]], x[j], T[j], C.fixture_oracle()[j] * R.TO_A3


def test_oracle_sum_identity_and_two_step_agreement():
    """sum_i x_i ln phi_i = a_res + Z - 1 - ln Z (Euler's theorem on the extensive F; seen: 8.5e-12 at an absolute step
    of 3e-4 on the whole sample) and the two relative steps agree (seen: 2.4e-10 on the whole sample).  The bounds are
    10 x those figures: a rounding floor is no bound on the error."""
    worst_sum = worst_step = 0.0
    for j in POINTS:
        rows, x, T, rho = _point(j)
        (fixed,) = PR.ln_phi(rows, x, T, rho, steps=(3e-4,), relative=False)
        want = PR.sum_identity(rows, x, T, rho)
        worst_sum = max(worst_sum, float(PR.scaled(np.dot(x / x.sum(), fixed), want)))
        coarse, fine = PR.ln_phi(rows, x, T, rho)
        worst_step = max(worst_step, float(PR.scaled(coarse, fine).max()))
    print("sum identity:", worst_sum, "two-step disagreement:", worst_step)
    assert len(POINTS) >= 8 and worst_sum <= 8.5e-11 and worst_step <= 2.4e-9


def test_oracle_reduces_to_one_component():
    rows, x, T, rho = _point(POINTS[0])
    for row in rows:
        (one,) = PR.ln_phi([row], [1.0], T, rho, steps=(1e-3,))
        assert abs(one[0] - PR.ln_phi_one(row, T, rho)) <= 1e-9 * max(1.0, abs(one[0]))
    # the same row twice is that component, whatever the split
    (twice,) = PR.ln_phi([rows[0], rows[0]], [0.3, 0.7], T, rho, steps=(1e-3,))
    assert abs(twice[0] - twice[1]) <= 1e-9 and abs(twice[0] - PR.ln_phi_one(rows[0], T, rho)) <= 1e-9 * max(
        1.0, abs(twice[0]))


def test_bindings_declare_the_fugacity_entry_points():
    from gnnepcsaft_amd import _lib
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_mix_lnphi_state is not None and lib.gnx_pcsaft_mix_lnphi is not None
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_lnphi_state"][1]) == 16
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_lnphi"][1]) == 17
    assert _lib.KERNEL_GROUPS[_lib.K_PCSAFT_MIX_LNPHI_STATE] == "pcsaft_mix_lnphi_state"
    assert _lib.KERNEL_GROUPS[_lib.K_PCSAFT_MIX_LNPHI] == "pcsaft_mix_lnphi"
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    assert "GNX_K_PCSAFT_MIX_LNPHI_STATE = %d," % _lib.K_PCSAFT_MIX_LNPHI_STATE in header
    assert "GNX_K_PCSAFT_MIX_LNPHI = %d," % _lib.K_PCSAFT_MIX_LNPHI in header
    assert "GNX_K_COUNT = 26" in header and "#define GNX_ABI_VERSION 7" in header
    assert "int32_t gnx_pcsaft_mix_lnphi_state(" in header and "int32_t gnx_pcsaft_mix_lnphi(" in header


@pytest.mark.parametrize("name", ["mix_ln_fugacity_coefficient", "mix_ln_fugacity_coefficient_pure",
                                  "mix_ln_activity_coefficient", "mix_e_gibbs_energy", "mix_r_gibbs_energy",
                                  "mix_gibbs_energy"])
def test_reference_shaped_functions_reject_malformed_input(name):
    """the checks that run on the host before anything is uploaded"""
    from gnnepcsaft_amd import pcsaft
    fn = getattr(pcsaft, name)
    rows = [list(r) for r in C.fixture_points()[0][:2]]
    with pytest.raises(ValueError):
        fn(rows, [300.0, 1e5, 0.5, 0.5], kij_matrix=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        fn(rows, [300.0, 1e5, 0.5, 0.5], epsilon_ab=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        fn(rows * 3, [300.0, 1e5] + [1.0 / 6] * 6)
    with pytest.raises(ValueError):
        fn(rows, [300.0, 1e5, 0.5, 0.3, 0.2])


def test_batch_form_rejects_malformed_input():
    from gnnepcsaft_amd import pcsaft
    rows = [list(r) for r in C.fixture_points()[0][:2]]
    with pytest.raises(ValueError):
        pcsaft.mix_ln_phi_batch([rows], [np.zeros((1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError):
        pcsaft.mix_ln_phi_batch([rows], [np.zeros((1, 5))])
    assert pcsaft.mix_ln_phi_batch([rows], [np.zeros((0, 4))]) == []
