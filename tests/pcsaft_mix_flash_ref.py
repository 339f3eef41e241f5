"""Test-only oracle of the isothermal two-phase (T, P) flash of csrc/gnx_pcsaft_mix_flash.hip, on top
of the bubble-point oracle of tests/pcsaft_mix_vle_ref.py, which is used as it is (``ln_fugacity``, ``vapour_density``,
``residuals``, ``MR.density``).

At (T, P) the feed z splits into a liquid x and a vapour y, the vapour holding the mole fraction beta of the feed:
ln f_i^L(T, rho_l, x) = ln f_i^V(T, rho_v, y) for every component, both phases at the pressure P, and z_i = (1 - beta)
x_i + beta y_i.  ``flash`` solves this by the kernel's outer loop (K from the liquid z at zero pressure under an ideal
vapour, from the highest root of z at P where there is none, then Rachford-Rice and successive substitution on ln K; every
root from a full scan, never from the previous step's) on the oracle's own evaluations: complex-step pressure,
five-point differences in the mole numbers, Brent roots.  ``V.residuals`` stays the solve-independent check of the
equilibrium equations; ``balance`` adds the material balance.  Every z_i given here must be > 0.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import pcsaft_mix_ref as MR
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R
from tests.pcsaft_ref import RGAS, TO_A3

DAMPINGS = 20
TRIVIAL = 1e-3  # rho_l - rho_v <= this * rho_l: both phases are the same fluid


def rachford_rice(z, K):
    """root beta of sum_i z_i (K_i - 1) / (1 + beta (K_i - 1)) = 0 on the negative-flash window (1 / (1 - K_max),
    1 / (1 - K_min)), where the sum falls from +inf to -inf; None if the window is empty (no K above 1, or none below):
    Newton from 0.5 safeguarded by bisection"""
    if not (K.max() > 1.0 > K.min()):
        return None
    lo, hi = 1.0 / (1.0 - K.max()), 1.0 / (1.0 - K.min())
    beta = 0.5
    for _ in range(100):
        r = (K - 1.0) / (1.0 + beta * (K - 1.0))
        g = float(np.sum(z * r))
        if g == 0.0:
            break
        if g > 0.0:
            lo = beta
        else:
            hi = beta
        new = beta + g / float(np.sum(z * r * r))
        if not lo < new < hi:
            new = 0.5 * (lo + hi)
        if not lo < new < hi:  # the bracket has closed on beta
            break
        done = abs(new - beta) <= 1e-16 * max(1.0, abs(beta))
        beta = new
        if done:
            break
    return beta


def balance(z, x, y, beta):
    """max_i |z_i - (1 - beta) x_i - beta y_i| with z normalised by its sum"""
    z = np.asarray(z, dtype=np.float64)
    return float(np.max(np.abs(z / z.sum() - (1.0 - beta) * np.asarray(x) - beta * np.asarray(y))))


def flash(rows, z, T, P, kij=None, eab=None, tol=1e-10, max_iterations=200, trace=None):
    """Flash of the feed z at (T, P): dict with beta, x, y [nc], rho_l, rho_v (mol/m³) and iterations, the state at which
    the fugacities were last evaluated; "single" where there is no vapour-liquid split (one component, an empty
    Rachford-Rice window, convergence with beta outside [0, 1] or onto the trivial solution); None where it does not
    converge (no root of z to start from, no root of a phase within the dampings, ``max_iterations``).  ``trace``: a
    list that receives (residual, beta, x, y, rho_l, rho_v) of every step, from which the solve at a looser tolerance
    can be read off."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    z = np.asarray(z, dtype=np.float64)
    z = z / z.sum()
    if len(z) == 1:
        return "single"
    feed = MR.Mixture(rows, z, kij=kij, eab=eab)
    rho0 = MR.density(feed, T, 0.0)
    if rho0 is None:  # no liquid of z at zero pressure: its highest root at P instead
        rho0 = MR.density(feed, T, P)
    if rho0 is None:
        return None
    pt = P / (RGAS * T) * TO_A3  # p / kT, 1/Å^3
    lnk = V.ln_fugacity(rows, z, T, rho0, kij, eab) - np.log(z * pt)
    previous, damp = lnk, 0
    for it in range(1, max_iterations + 1):
        K = np.exp(lnk)
        beta = rachford_rice(z, K)
        if beta is None:
            return "single"
        x = z / (1.0 + beta * (K - 1.0))
        y = K * x
        if not (np.all(np.isfinite(y)) and np.all(x > 0.0) and np.all(y > 0.0)):
            return None
        rho_l = MR.density(MR.Mixture(rows, x, kij=kij, eab=eab), T, P)
        rho_v = V.vapour_density(MR.Mixture(rows, y, kij=kij, eab=eab), T, P)
        if rho_l is None or rho_v is None:
            damp += 1
            if damp > DAMPINGS:
                return None
            lnk = 0.5 * (lnk + previous)
            continue
        damp = 0
        d = V.ln_fugacity(rows, x, T, rho_l, kij, eab) - V.ln_fugacity(rows, y, T, rho_v, kij, eab)
        if not np.all(np.isfinite(d)):
            return None
        res = float(np.max(np.abs(d)))
        if trace is not None:
            trace.append((res, beta, x, y, rho_l, rho_v))
        if res < tol:
            if not rho_l - rho_v > TRIVIAL * rho_l or not 0.0 <= beta <= 1.0:
                return "single"
            return {"beta": beta, "x": x, "y": y, "rho_l": rho_l, "rho_v": rho_v, "iterations": it}
        previous, lnk = lnk, lnk + d
    return None


@functools.lru_cache(maxsize=None)
def tie_line_points():
    """(name, rows, T, P, z, x, y, beta) of the tie-line feeds: z = (1 - beta) x + beta y on the bubble point (T, x) ->
    (P, y) of the oracle, beta = 0.3 on the six named points and 0.5 on the first six fixture cases that
    ``V.fixture_solves`` solves.  A feed on a tie line splits into its ends."""
    out = []
    for (name, rows, T, x), (sol, _) in zip(V.NAMED, V.named_solves()):
        x = np.asarray(x, dtype=np.float64)
        out.append((name, rows, T, sol["P"], 0.7 * x + 0.3 * sol["y"], x, sol["y"], 0.3))
    solved = [(c, s) for c, s in zip(V.fixture_cases(), V.fixture_solves()) if s is not None][:6]
    for (name, rows, T, x), sol in solved:
        x = np.asarray(x, dtype=np.float64)
        out.append((name, rows, T, sol["P"], 0.5 * x + 0.5 * sol["y"], x, sol["y"], 0.5))
    return out


@functools.lru_cache(maxsize=None)
def tie_line_solves():
    """per tie-line point (the oracle's flash at 1e-10, the change of its answer between the tolerances 1e-9 and 1e-11:
    the largest absolute change of x and y); one run to 1e-11 each, computed once and shared.  That run may take 300 steps:
    ethanol + water loses a factor 0.89 per step and passes 1e-10 at step 179, 1e-11 beyond 200."""
    out = []
    for name, rows, T, P, z, x, y, beta in tie_line_points():
        trace = []
        tight = flash(rows, z, T, P, tol=1e-11, max_iterations=300, trace=trace)
        if not isinstance(tight, dict):
            out.append((tight, None))
            continue
        loose = next(t for t in trace if t[0] < 1e-9)
        change = max(float(np.max(np.abs(loose[2] - tight["x"]))), float(np.max(np.abs(loose[3] - tight["y"]))))
        it, at = next((k + 1, t) for k, t in enumerate(trace) if t[0] < 1e-10)
        if it > 200:  # the solve at the default tolerance and cap does not get there
            out.append((None, None))
            continue
        sol = {"beta": at[1], "x": at[2], "y": at[3], "rho_l": at[4], "rho_v": at[5], "iterations": it}
        out.append((sol, change))
    return out


@functools.lru_cache(maxsize=None)
def single_phase_points():
    """(name, rows, T, P, z) of the four single-phase points: butane + hexane at 350 K, z = (0.5, 0.5), and methane +
    butane + hexane at 320 K, z = (0.1, 0.3, 0.6), each at 1.5 x the oracle's bubble pressure of z (a compressed liquid)
    and at 0.5 x the lowest vapour pressure of its components that are subcritical at that T (a superheated vapour)"""
    out = []
    for k in (2, 4):
        (name, rows, T, z), (sol, _) = V.NAMED[k], V.named_solves()[k]
        sat = [R.vle(np.asarray(row, dtype=np.float64), T) for row in rows]
        lowest = min(s[0] for s in sat if s is not None)
        out.append((name + " above the bubble point", rows, T, 1.5 * sol["P"], z))
        out.append((name + " below every vapour pressure", rows, T, 0.5 * lowest, z))
    return out
