"""Test-only fp64 NumPy oracle of the pure-component saturation properties and critical points of csrc/gnx_pcsaft.hip
(DESIGN.md §4b), built on tests/pcsaft_ref.py.

It shares no mechanism with the kernel.  The temperature derivative of ``a_res`` is a complex step in T (the kernel
evaluates ``a_res`` on a forward dual seeded in T); the densities are those of ``pcsaft_ref.vle``; the critical point is
``scipy.optimize.root`` on (p_rho rho / p, p_rhorho rho² / p) with 5-point central stencils of ``pressure_eta`` in eta
(the kernel uses a third-order dual in rho and nested secants).  Only the bracket in T is found the same way, from above,
because a bracket from a low temperature is not safe: on the scan of ``pcsaft_ref.spinodals`` two fixture molecules show
no loop at 0.2 eps/k.

Definitions.  a(T, rho): reduced residual Helmholtz energy per molecule; Z = 1 + rho a_rho; R = N_A k_B.
  h = R T (-T a_T + Z - 1)   residual molar enthalpy, J/mol
  s = -R (a + T a_T)         residual molar entropy at the same T and V, J/mol/K
At saturation s_V - s_L = (h_V - h_L) / T - R ln(rho_L / rho_V).
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np
from scipy import optimize

from tests import pcsaft_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcsaft_thermoml.json")
METHANE = [1.0, 3.7039, 150.03, 0.0, 0.0, 0.0, 0.0, 0.0, 16.043]
HEXANE = [3.0576, 3.7983, 236.77, 0.0, 0.0, 0.0, 0.0, 0.0, 86.177]
# relative uncertainty of the oracle's (Tc, Pc, rho_c): ten times the measured difference between the stencil steps
# h = 1e-3 and h = 3e-3 (tests/test_pcsaft_sat_cpu.py pins the measured values)
CRIT_TOL_FIXTURE = (1.9e-10, 1.4e-9, 3.1e-8)
CRIT_TOL_RANDOM = (1.1e-9, 1.8e-8, 3.7e-8)


def molecules():
    with open(FIXTURE) as fh:
        return json.load(fh)["molecules"]


def random_rows(rng, n):
    """the generator of tests/test_pcsaft_gpu.py (a copy: test modules with GPU marks are not imported)"""
    m = rng.uniform(1.0, 25.0, n)
    sigma = rng.uniform(1.9, 4.5, n)
    eps = rng.uniform(50.0, 550.0, n)
    kab = rng.uniform(1e-4, 0.9, n)
    eab = rng.uniform(200.0, 5000.0, n)
    mu = rng.uniform(0.0, 4.0, n)
    na, nb = rng.integers(0, 3, n).astype(np.float64), rng.integers(0, 3, n).astype(np.float64)
    return np.stack([m, sigma, eps, kab, eab, mu, na, nb, np.full(n, 100.0)], axis=1)


def a_T(row, T, rho):
    """d a_res / d T at constant rho [1/Å^3] by complex step"""
    h = T * 1e-20
    return float(np.imag(R.a_res(row, T + 1j * h, rho)) / h)


def h_s(row, T, rho_mol):
    """(residual molar enthalpy J/mol, residual molar entropy at the same T and V J/mol/K) at rho_mol [mol/m³]"""
    rho = rho_mol * R.TO_A3
    a, at, z = float(np.real(R.a_res(row, T, rho))), a_T(row, T, rho), float(R.compressibility(row, T, rho))
    return R.RGAS * T * (-T * at + z - 1.0), -R.RGAS * (a + T * at)


def saturation(row, T):
    """(p_sat Pa, rho_L, rho_V mol/m³, h_L, h_V J/mol, s_L, s_V J/mol/K) at T, or None where ``pcsaft_ref.vle`` is"""
    eq = R.vle(row, T)
    if eq is None:
        return None
    p, rl, rv = eq
    (hl, sl), (hv, sv) = h_s(row, T, rl), h_s(row, T, rv)
    return p, rl, rv, hl, hv, sl, sv


@functools.lru_cache(maxsize=None)
def _saturation_cached(row, T):
    return saturation(list(row), T)


def fixture_saturation():
    """[(molecule index, T, saturation(row, T))] over every vapour-pressure point of the fixture the oracle solves, and
    the parameter rows [48, 9]; computed once per process"""
    mols = molecules()
    rows = np.array([m["params"] for m in mols], dtype=np.float64)
    pts = []
    for i, m in enumerate(mols):
        for s in m["vp"]:
            ref = _saturation_cached(tuple(rows[i].tolist()), float(s[0]))
            if ref is not None:
                pts.append((i, float(s[0]), ref))
    return rows, pts


def critical_bracket(row, start=20.0, step=0.8, steps=20, rel=1e-5):
    """(t_lo, t_hi) around the highest T at which ``pcsaft_ref.spinodals`` finds a loop, looked for from above: from
    ``start`` eps/k down by ``step`` until there is one, then bisection to a relative width ``rel``; None if ``start``
    already has a loop or none is found"""
    t_hi = start * row[2]
    if R.spinodals(row, t_hi) is not None:
        return None
    for _ in range(steps):
        t_lo = t_hi * step
        if R.spinodals(row, t_lo) is not None:
            break
        t_hi = t_lo
    else:
        return None
    while t_hi - t_lo > rel * t_lo:
        mid = 0.5 * (t_lo + t_hi)
        if R.spinodals(row, mid) is None:
            t_hi = mid
        else:
            t_lo = mid
    return t_lo, t_hi


@functools.lru_cache(maxsize=None)
def _bracket_cached(row):
    br = critical_bracket(list(row))
    if br is None:
        return None
    evs, els = R.spinodals(list(row), br[0])
    return br[0], br[1], 0.5 * (evs + els)


def critical_point(row, h=1e-3):
    """(Tc K, Pc Pa, rho_c mol/m³) with (dp/drho)_T = (d²p/drho²)_T = 0 on the loop that vanishes last as T rises, or
    None.  ``h``: relative step in eta of the 5-point stencils."""
    row = [float(v) for v in row]
    br = _bracket_cached(tuple(row))
    if br is None:
        return None
    t_lo, _, eta0 = br

    def eqs(x):
        T, eta = x[0] * t_lo, x[1] * eta0
        d = h * eta
        pm2, pm1, p0, pp1, pp2 = (R.pressure_eta(row, T, eta + k * d) for k in (-2, -1, 0, 1, 2))
        p1 = (pm2 - 8.0 * pm1 + 8.0 * pp1 - pp2) / (12.0 * d)
        p2 = (-pm2 + 16.0 * pm1 - 30.0 * p0 + 16.0 * pp1 - pp2) / (12.0 * d * d)
        return [p1 * eta / p0, p2 * eta * eta / p0]

    sol = optimize.root(eqs, [1.0, 1.0], method="hybr", options={"xtol": 1e-15})
    T, eta = sol.x[0] * t_lo, sol.x[1] * eta0
    res = eqs(sol.x)
    if not (np.all(np.isfinite(sol.x)) and 0.0 < eta < R.ETA_MAX and abs(T / t_lo - 1.0) < 1e-2
            and abs(res[0]) < 1e-9 and abs(res[1]) < 1e-7):
        return None
    return T, float(R.pressure_eta(row, T, eta)), eta / R.eta_per_rho(row, T) / R.TO_A3


@functools.lru_cache(maxsize=None)
def critical_point_cached(row, h=1e-3):
    return critical_point(list(row), h)
