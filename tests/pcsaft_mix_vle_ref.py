"""Test-only oracle of the mixture bubble point of csrc/gnx_pcsaft_mix_vle.hip, on top of the mixture
oracles of tests/pcsaft_mix_ref.py and tests/pcsaft_mix_phi_ref.py, which are used as they are.

Equilibrium in the form without ln Z: ln f_i = mu_i^res/kT + ln(rho x_i), rho the number density (1/Å^3), is equal in
both phases for every component, and both phases have the pressure P.

``residuals`` evaluates these equations at a given state.  It shares no mechanism with the kernel: the pressure is a
complex step on a_res, mu^res a five-point central difference in the mole numbers (the kernel: second-order duals in
rho, first-order duals in x, implicit differentiation of the site fractions).  ``bubble`` solves them by the kernel's
outer loop (successive substitution from an ideal-vapour start) on those evaluations, with Brent roots from dense
scans.  Every x_i given here must be > 0.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import pcsaft_mix_phi_ref as PR
from tests import pcsaft_mix_ref as MR
from tests.pcsaft_ref import RGAS, TO_A3

MAX_ITERATIONS = 300
DAMPINGS = 20
# literature rows for the named systems (Gross & Sadowski 2001 Table 2; 2002 for the 2B associating components)
METHANE = [1.0, 3.7039, 150.03, 0, 0, 0, 0, 0, 16.043]
PROPANE = [2.0020, 3.6184, 208.11, 0, 0, 0, 0, 0, 44.096]
BUTANE = [2.3316, 3.7086, 222.88, 0, 0, 0, 0, 0, 58.123]
HEXANE = [3.0576, 3.7983, 236.77, 0, 0, 0, 0, 0, 86.177]
ETHANOL = [2.3827, 3.1771, 198.24, 0.032384, 2653.4, 0, 1, 1, 46.069]
WATER = [1.0656, 3.0007, 366.51, 0.034868, 2500.7, 0, 1, 1, 18.015]
# (name, rows, T, x)
NAMED = (("methane+hexane 0.1", [METHANE, HEXANE], 300.0, [0.1, 0.9]),
         ("methane+hexane 0.4", [METHANE, HEXANE], 300.0, [0.4, 0.6]),
         ("butane+hexane", [BUTANE, HEXANE], 350.0, [0.5, 0.5]),
         ("ethanol+water", [ETHANOL, WATER], 350.0, [0.3, 0.7]),
         ("methane+butane+hexane", [METHANE, BUTANE, HEXANE], 320.0, [0.1, 0.3, 0.6]),
         ("methane+propane+butane+hexane", [METHANE, PROPANE, BUTANE, HEXANE], 320.0, [0.1, 0.2, 0.3, 0.4]))


def vapour_density(mix, T, P):
    """lowest root of P(rho) = P with dP/drho > 0, mol/m³: upward scan of the grid to the first point at or above P,
    then Brent; None if the pressure turns over before it gets there"""
    with np.errstate(all="ignore"):
        p = MR.pressure_eta(mix, T, MR._GRID)
        above = np.nonzero(p >= P)[0]
        if above.size == 0:
            return None
        k = above[0]
        if not np.all(np.isfinite(p[:k + 1])) or np.any(np.diff(p[:k + 1]) <= 0):
            return None
        ideal = P / (RGAS * T) * TO_A3 * mix.eta_per_rho(T)
        lo = MR._GRID[k - 1] if k > 0 else 0.5 * min(ideal, MR._GRID[0])
        try:
            eta = MR._brent(lambda e: MR.pressure_eta(mix, T, e) - P, lo, MR._GRID[k])
        except ValueError:
            return None
        rho = eta / mix.eta_per_rho(T) / TO_A3
        if not MR.dpdrho(mix, T, rho) > 0:
            return None
    return rho


def mu_res(rows, x, T, rho0, kij=None, eab=None, step=PR.STEPS[1]):
    """mu_i^res/kT = dF/dN_i by the five-point difference of ``pcsaft_mix_phi_ref.mu_res`` on its ``_F``, with the
    absolute step ``step`` in N_i, x_i / 3 where that is smaller (the stencil reaches x_i - 2 h and must stay
    positive).  The rounding of F enters as 1e-16 / h: with that module's default, a step relative to x_i, a trace
    component of the vapour (y_i of 1e-4 .. 1e-2) gets h of 1e-8 .. 1e-6, its ln f carries 1e-9, and the substitution
    ends in a cycle of that size instead of converging (fixture systems 13 and 22)."""
    x = np.asarray(x, dtype=np.float64)
    x = x / x.sum()
    out = np.empty(len(x))
    for i in range(len(x)):
        h = min(step, x[i] / 3.0)
        f = []
        for k in (-2, -1, 1, 2):
            N = x.copy()
            N[i] += k * h
            f.append(PR._F(rows, N, T, rho0, kij, eab))
        out[i] = (f[0] - 8.0 * f[1] + 8.0 * f[2] - f[3]) / (12.0 * h)
    return out


def ln_fugacity(rows, x, T, rho_mol, kij=None, eab=None, step=PR.STEPS[1]):
    """ln f_i = mu_i^res/kT + ln(rho x_i) at the molar density rho_mol, rho in 1/Å^3: [nc]"""
    x = np.asarray(x, dtype=np.float64)
    x = x / x.sum()
    rho0 = rho_mol * TO_A3
    return mu_res(rows, x, T, rho0, kij, eab, step) + np.log(rho0 * x)


def residuals(rows, x, y, T, P, rho_l, rho_v, kij=None, eab=None):
    """The equilibrium equations at a given state: dict with p_l, p_v (Pa, the oracle's pressures of (x, rho_l) and
    (y, rho_v)), fugacity = max_i |ln f_i^L - ln f_i^V| at the finer step, and own = the oracle's own error, the largest
    disagreement of mu^res between its two steps in either phase"""
    p_l = MR.pressure(MR.Mixture(rows, x, kij=kij, eab=eab), T, rho_l)
    p_v = MR.pressure(MR.Mixture(rows, y, kij=kij, eab=eab), T, rho_v)
    fl = [ln_fugacity(rows, x, T, rho_l, kij, eab, s) for s in PR.STEPS]
    fv = [ln_fugacity(rows, y, T, rho_v, kij, eab, s) for s in PR.STEPS]
    return {"p_l": p_l, "p_v": p_v, "fugacity": float(np.max(np.abs(fl[1] - fv[1]))),
            "own": float(max(np.max(np.abs(fl[0] - fl[1])), np.max(np.abs(fv[0] - fv[1]))))}


def bubble(rows, x, T, kij=None, eab=None, tol=1e-10, max_iterations=MAX_ITERATIONS, trace=None):
    """Bubble point at (T, x): dict with P (Pa), y [nc], rho_l, rho_v (mol/m³) and iterations, the state at which the
    fugacities were last evaluated; None where there is no liquid at zero pressure, no vapour root within the dampings,
    no convergence within ``max_iterations`` or only the trivial solution.  ``trace``: a list that receives (residual,
    P, y) of every step, from which the solve at a looser tolerance can be read off."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    x = np.asarray(x, dtype=np.float64)
    x = x / x.sum()
    liquid = MR.Mixture(rows, x, kij=kij, eab=eab)
    rho_l = MR.density(liquid, T, 0.0)
    if rho_l is None:
        return None
    f = np.exp(ln_fugacity(rows, x, T, rho_l, kij, eab))  # 1/Å^3: f kT is a pressure
    P = float(f.sum()) / TO_A3 * RGAS * T
    y = f / f.sum()
    previous, damp = 0.0, 0
    for it in range(1, max_iterations + 1):
        rho_l = MR.density(liquid, T, P)
        if rho_l is None:
            return None
        rho_v = vapour_density(MR.Mixture(rows, y, kij=kij, eab=eab), T, P)
        if rho_v is None:
            damp += 1
            if damp > DAMPINGS:
                return None
            P = 0.5 * (P + previous)
            continue
        damp = 0
        d = ln_fugacity(rows, x, T, rho_l, kij, eab) - ln_fugacity(rows, y, T, rho_v, kij, eab)
        if not np.all(np.isfinite(d)):
            return None
        xk = y * np.exp(d)
        s = float(xk.sum())
        res = max(abs(np.log(s)), float(np.max(np.abs(d - np.log(s)))))
        if trace is not None:
            trace.append((res, P, y))
        if res < tol:
            if not rho_l - rho_v > 1e-3 * rho_l:
                return None
            return {"P": P, "y": y, "rho_l": rho_l, "rho_v": rho_v, "iterations": it}
        y, previous, P = xk / s, P, P * s
    return None


@functools.lru_cache(maxsize=None)
def named_solves():
    """per named point (the solve at 1e-10, the change of the solve between the tolerances 1e-9 and 1e-11: relative in P,
    absolute in y); one run to 1e-11 each, computed once and shared"""
    out = []
    for _, rows, T, x in NAMED:
        trace = []
        tight = bubble(rows, x, T, tol=1e-11, trace=trace)
        assert tight is not None
        loose = next(t for t in trace if t[0] < 1e-9)
        change = max(abs(loose[1] / tight["P"] - 1.0), float(np.max(np.abs(loose[2] - tight["y"]))))
        out.append((bubble(rows, x, T), change))
    return out


@functools.lru_cache(maxsize=None)
def fixture_solves():
    """the oracle's solve of every fixture case within 100 steps, None where it does not get there; computed once"""
    return [bubble(rows, x, T, max_iterations=100) for _, rows, T, x in fixture_cases()]


def fixture_cases():
    """(name, rows [2, 9], T, x [2]) of the first point of each system of the binary fixture, x clipped to [0.05, 0.95]"""
    from tests import pcsaft_mix_cases as C
    out = []
    for k, s in enumerate(C.systems()):
        p = s["points"][0]
        x1 = float(np.clip(p[2], 0.05, 0.95))
        out.append((f"fixture {k}", np.asarray(s["params"], dtype=np.float64), float(p[0]), [x1, 1.0 - x1]))
    return out
