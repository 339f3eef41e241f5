"""Test-only oracle of the mixture dew point of csrc/gnx_pcsaft_mix_dew.hip, on the evaluations of
tests/pcsaft_mix_vle_ref.py (``ln_fugacity``, ``vapour_density``, ``residuals``) and tests/pcsaft_mix_ref.py
(``density``), which are imported and used as they are.

The equations are the bubble point's, equal ln f_i = mu_i^res/kT + ln(rho x_i) and equal pressure, with the vapour y
given and the liquid x unknown.  ``dew`` solves them by the kernel's outer loop: a start from Raoult's law on each
component's own liquid at zero pressure, then successive substitution x <- x f^V / f^L, P <- P / sum.  A dew point need
not be unique (a retrograde vapour has two, and two liquids can share one y); this finds the one that start leads to.
Every y_i given here must be > 0.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import pcsaft_mix_ref as MR
from tests import pcsaft_mix_vle_ref as V
from tests.pcsaft_ref import RGAS, TO_A3

MAX_ITERATIONS = 400  # the kernel's kDewMixIters
NO_LIQUID = 100.0     # Raoult pressure of a component without a liquid of its own, in units of the largest one found
RETURNS = 1e-9        # a case "returns": its dew point is the bubble point its vapour came from, within this


def raoult_start(rows, y, T):
    """(P0 [Pa], x0 [nc]) from k_i = kT f_i of component i alone at its liquid root at zero pressure, 100 x the largest
    k for a component that has no such root: P0 = 1 / sum_i y_i / k_i, x0_i = y_i / k_i normalised.  None if no
    component has a liquid at zero pressure."""
    k = np.zeros(len(rows))
    for i, row in enumerate(rows):
        rho = MR.density(MR.Mixture([row], [1.0]), T, 0.0)
        if rho is not None:
            k[i] = float(np.exp(V.ln_fugacity([row], [1.0], T, rho)[0])) / TO_A3 * RGAS * T
    if not np.any(k > 0.0):
        return None
    k = np.where(k > 0.0, k, NO_LIQUID * k.max())
    s = float(np.sum(y / k))
    return 1.0 / s, y / k / s


def dew(rows, y, T, kij=None, eab=None, tol=1e-10, max_iterations=MAX_ITERATIONS, trace=None):
    """Dew point at (T, y): dict with P (Pa), x [nc], rho_l, rho_v (mol/m³) and iterations, the state at which the
    fugacities were last evaluated; None where no component has a liquid at zero pressure, there is no liquid root or no
    vapour root within the dampings, no convergence within ``max_iterations`` or only the trivial solution.  ``trace``: a
    list that receives (residual, P, x, rho_l, rho_v, step) of every evaluated step, from which the solve at a looser
    tolerance can be read off."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    y = np.asarray(y, dtype=np.float64)
    y = y / y.sum()
    start = raoult_start(rows, y, T)
    if start is None:
        return None
    P, x = start
    vapour = MR.Mixture(rows, y, kij=kij, eab=eab)
    previous, damp = 0.0, 0
    for it in range(1, max_iterations + 1):
        rho_l = MR.density(MR.Mixture(rows, x, kij=kij, eab=eab), T, P)
        if rho_l is None:
            return None
        rho_v = V.vapour_density(vapour, T, P)
        if rho_v is None:
            damp += 1
            if damp > V.DAMPINGS:
                return None
            P = 0.5 * (P + previous)
            continue
        damp = 0
        d = V.ln_fugacity(rows, y, T, rho_v, kij, eab) - V.ln_fugacity(rows, x, T, rho_l, kij, eab)
        if not np.all(np.isfinite(d)):
            return None
        xk = x * np.exp(d)
        s = float(xk.sum())
        res = max(abs(np.log(s)), float(np.max(np.abs(d - np.log(s)))))
        if trace is not None:
            trace.append((res, P, x, rho_l, rho_v, it))
        if res < tol:
            if not rho_l - rho_v > 1e-3 * rho_l:
                return None
            return {"P": P, "x": x, "rho_l": rho_l, "rho_v": rho_v, "iterations": it}
        x, previous, P = xk / s, P, P / s
        if not (np.all(x > 0.0) and np.isfinite(P) and P > 0.0):
            return None
    return None


@functools.lru_cache(maxsize=None)
def cases():
    """the 30 tuples (name, rows, T, y, bubble solution): the vapours of the oracle's bubble points of the 6 named and
    the 24 fixture points of tests/pcsaft_mix_vle_ref.py.  Where the bubble oracle has no solution the liquid itself
    stands in for y and the solution is None: such a case cannot return."""
    named = [sol for sol, _ in V.named_solves()]
    out = []
    for (name, rows, T, x), sol in zip(list(V.NAMED) + V.fixture_cases(), named + V.fixture_solves()):
        y = np.asarray(x, dtype=np.float64) if sol is None else sol["y"]
        out.append((name, rows, T, y, sol))
    return out


def _read(entry):
    res, P, x, rho_l, rho_v, it = entry
    return {"P": P, "x": x, "rho_l": rho_l, "rho_v": rho_v, "iterations": it}


@functools.lru_cache(maxsize=None)
def solves():
    """per case (the solve at 1e-10 or None; the change of the solve between the tolerances 1e-9 and 1e-11, relative in P
    and absolute in x; does it return to its bubble point).  One run to 1e-11 each, the looser solves read from its
    trace: what a run to that tolerance ends on.  Where the run does not reach 1e-11 within the steps, the step with the
    smallest residual stands in for it.  Computed once and shared."""
    out = []
    for name, rows, T, y, bub in cases():
        trace = []
        dew(rows, y, T, tol=1e-11, trace=trace)
        sol = next((_read(t) for t in trace if t[0] < 1e-10), None)
        if sol is None or not sol["rho_l"] - sol["rho_v"] > 1e-3 * sol["rho_l"]:
            out.append((None, 0.0, False))
            continue
        loose = next(t for t in trace if t[0] < 1e-9)
        tight = min(trace, key=lambda t: t[0])
        change = max(abs(loose[1] / tight[1] - 1.0), float(np.max(np.abs(loose[2] - tight[2]))))
        returns = bub is not None and abs(sol["P"] / bub["P"] - 1.0) <= RETURNS and \
            float(np.max(np.abs(sol["x"] - liquid(name)))) <= RETURNS
        out.append((sol, change, returns))
    return out


@functools.lru_cache(maxsize=None)
def _liquids():
    return {name: np.asarray(x, dtype=np.float64) / np.sum(x) for name, _, _, x in list(V.NAMED) + V.fixture_cases()}


def liquid(name):
    """the liquid x that the bubble point of case ``name`` was solved for"""
    return _liquids()[name]
