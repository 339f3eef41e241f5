"""The fp64 PC-SAFT oracle of tests/pcsaft_ref.py pinned on its own (no GPU): constant tables against the kernel's
header, limits and identities of the model, the phase equilibria it finds on the ThermoML fixture, and a physical
sanity net (Esper's parameters against measured data) that a self-consistent oracle cannot provide."""
import json
import os
import re

import numpy as np
import pytest

from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pcsaft_thermoml.json")
HEADER = os.path.join(ROOT, "gnnepcsaft_amd", "csrc", "gnx_pcsaft_consts.hpp")


def _molecules():
    with open(FIXTURE) as fh:
        return json.load(fh)["molecules"]


def _header_table(name):
    text = open(HEADER).read()
    body = re.search(name + r"\[3\]\[\d\] = \{(.*?)\};", text, re.S).group(1)
    return np.array([[float(v) for v in row.split(",") if v.strip()] for row in re.findall(r"\{([^{}]*)\}", body)])


def _header_scalar(name):
    return float(re.search(name + r" = ([0-9.e+-]+);", open(HEADER).read()).group(1))


def test_constant_tables_match_the_kernel_header():
    for name, table in [("kDispA", R.DISP_A), ("kDispB", R.DISP_B), ("kDipA", R.DIP_A), ("kDipB", R.DIP_B),
                        ("kDipC", R.DIP_C)]:
        np.testing.assert_array_equal(_header_table(name), table, err_msg=name)
    assert _header_scalar("kAvogadro") == R.NA and _header_scalar("kBoltzmann") == R.KB
    assert _header_scalar("kDipoleFactor") == R.DIPOLE_FACTOR and _header_scalar("kEtaMax") == R.ETA_MAX


def test_fixture_is_small_and_covers_the_classes():
    mols = _molecules()
    assert os.path.getsize(FIXTURE) < 100_000
    classes = [m["class"] for m in mols]
    assert {c: classes.count(c) for c in set(classes)} == {"nonpolar": 16, "dipolar": 16, "associating": 16}
    for m in mols:
        assert len(m["params"]) == 9 and 4 <= len(m["rho"]) <= 8 and 4 <= len(m["vp"]) <= 8
        assert all(len(s) == 5 and s[3] == 1.0 for s in m["rho"]) and all(len(s) == 5 and s[3] == 3.0 for s in m["vp"])


def test_low_density_limit_is_linear_in_eta():
    """Z - 1 = B2 rho + O(rho^2): its values at eta = 1e-8 and 1e-9 differ by a factor 10 (non-associating rows)."""
    rows = [m["params"] for m in _molecules() if m["class"] != "associating"]
    for row in rows:
        for T in (150.0, 300.0, 600.0):
            c = R.eta_per_rho(row, T)
            z8 = R.compressibility(row, T, 1e-8 / c) - 1.0
            z9 = R.compressibility(row, T, 1e-9 / c) - 1.0
            assert abs(z8 / z9 - 10.0) <= 1e-3, (row, T, z8, z9)


def test_complex_step_pressure_matches_a_finite_difference():
    """P from the complex step vs P from a central difference of a_res (step 1e-5 rho), relative to max(|P|, rho R T)
    (at liquid densities P is a small difference of terms of size rho R T)."""
    mols = _molecules()
    for m in mols[::4]:
        row = m["params"]
        for T in (0.8 * row[2], 1.5 * row[2], 3.0 * row[2]):
            for eta in (1e-4, 1e-2, 0.1, 0.3, 0.45):
                rho = eta / R.eta_per_rho(row, T)
                h = rho * 1e-5
                da = (R.a_res(row, T, rho + h) - R.a_res(row, T, rho - h)) / (2 * h)
                p_fd = rho / R.TO_A3 * R.RGAS * T * (1.0 + rho * da)
                p_cs = R.pressure_eta(row, T, eta)
                scale = max(abs(p_cs), rho / R.TO_A3 * R.RGAS * T)
                assert abs(p_cs - p_fd) <= 1e-7 * scale, (m["name"], T, eta, p_cs, p_fd)


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3)])
def test_closed_form_site_fractions_equal_the_iteration(na, nb):
    for x in (1e-6, 1e-3, 0.1, 1.0, 10.0, 300.0):
        xa, xb = R.assoc_fractions(na, nb, x)
        ia, ib = R.assoc_fractions_iterated(na, nb, x)
        assert abs(xa - ia) <= 1e-13 and abs(xb - ib) <= 1e-13, (x, xa, ia, xb, ib)
        assert abs(xa * (1 + nb * x * xb) - 1) <= 1e-13 and abs(xb * (1 + na * x * xa) - 1) <= 1e-13
    for x in (1e8, 1e14, 1e20):  # strong association at low T: the branch of the quadratic must not cancel
        xa, xb = R.assoc_fractions(na, nb, x)
        assert 0 < xa <= 1 and 0 < xb <= 1
        assert abs(xa * (1 + nb * x * xb) - 1) <= 1e-12 and abs(xb * (1 + na * x * xa) - 1) <= 1e-12, (x, xa, xb)


def test_switched_off_terms_are_exactly_zero():
    row = [2.5, 3.5, 250.0, 0.02, 2000.0, 0.0, 0.0, 1.0, 60.0]
    for rho in (1e-6, 1e-3, 4e-3):
        _, _, a_assoc, a_dip = R.a_terms(row, 300.0, rho)
        assert a_assoc == 0.0 and a_dip == 0.0
    on = [2.5, 3.5, 250.0, 0.02, 2000.0, 1.5, 1.0, 1.0, 60.0]
    _, _, a_assoc, a_dip = R.a_terms(on, 300.0, 4e-3)
    assert a_assoc < 0.0 and a_dip < 0.0


def test_phase_equilibrium_at_every_fixture_vapor_pressure():
    """P_L = P_V and mu_L = mu_V to 1e-10.  P_L is a difference of terms of size rho_L R T (Z_L ~ 1e-4), so the pressure
    residual is taken relative to rho_L R T; the chemical potential mu/kT relative to max(1, |mu/kT|)."""
    for m in _molecules():
        row = m["params"]
        for T, *_ in m["vp"]:
            out = R.vle(row, T)
            assert out is not None, (m["name"], T)
            ps, rl, rv = out
            assert ps > 0 and rl > rv > 0
            c = R.eta_per_rho(row, T) * R.TO_A3
            dp = abs(R.pressure(row, T, rl) - R.pressure(row, T, rv)) / (rl * R.RGAS * T)
            gl, gv = R.chem_pot(row, T, rl * c), R.chem_pot(row, T, rv * c)
            assert dp <= 1e-10 and abs(gl - gv) <= 1e-10 * max(1.0, abs(gv)), (m["name"], T, dp, gl, gv)
            assert abs(R.pressure(row, T, rv) - ps) <= 1e-12 * ps
            # ln phi equal as well (same statement at equal pressure)
            assert abs(R.ln_phi(row, T, rl) - R.ln_phi(row, T, rv)) <= 1e-8


# observed median absolute relative deviations of Esper's parameters against the fixture (rho / p_sat):
#   nonpolar 0.41 % / 1.31 %, dipolar 0.23 % / 2.36 %, associating 0.43 % / 1.15 %
MEDIAN_BOUNDS = {"nonpolar": (0.008, 0.026), "dipolar": (0.005, 0.047), "associating": (0.009, 0.023)}


def test_esper_parameters_reproduce_thermoml_data():
    """Physical sanity net: with Esper et al.'s own parameters the oracle reproduces the measured liquid densities and
    vapour pressures of the fixture.  Observed medians of |pred - exp| / exp per class (density / vapour pressure):
    nonpolar 0.41 % / 1.31 %, dipolar 0.23 % / 2.36 %, associating 0.43 % / 1.15 %.  Bounds at about twice that:
    nonpolar 0.8 % / 2.6 %, dipolar 0.5 % / 4.7 %, associating 0.9 % / 2.3 %.  A wrong unit or a wrong dipole factor
    moves these by tens of percent."""
    dev = {}
    for m in _molecules():
        row, cls = m["params"], m["class"]
        for T, P, _, _, exp in m["rho"]:
            r = R.density(row, T, P)
            dev.setdefault((cls, 0), []).append(np.inf if r is None else abs(r - exp) / exp)
        for T, _, _, _, exp in m["vp"]:
            out = R.vle(row, T)
            dev.setdefault((cls, 1), []).append(np.inf if out is None else abs(out[0] - exp) / exp)
    for (cls, kind), d in dev.items():
        assert np.median(d) <= MEDIAN_BOUNDS[cls][kind], (cls, "rho" if kind == 0 else "vp", np.median(d))
