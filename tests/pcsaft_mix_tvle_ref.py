"""Test-only oracle of the mixture bubble and dew temperatures of csrc/gnx_pcsaft_mix_tvle.hip, on the
evaluations of tests/pcsaft_mix_vle_ref.py (``ln_fugacity``, ``vapour_density``, ``residuals``), tests/pcsaft_mix_ref.py
(``density``) and tests/pcsaft_mix_dew_ref.py (``raoult_start``), which are imported and used as they are.

The equations are those of the bubble and dew pressures, equal ln f_i = mu_i^res/kT + ln(rho x_i) and both phases at P,
with P given and T unknown.  ``solve`` is the kernel's loop: a start temperature from a secant in 1/T on the pressure
kernels' own first estimate of P, then successive substitution on the unknown composition with one secant step in 1/T on
ln(sum) per step.  z is the given composition (the liquid x of a bubble point, the vapour y of a dew point), w the one
looked for.  Every z_i given here must be > 0.

The cases are the inverse problems of the 30 bubble points of tests/pcsaft_mix_vle_ref.py: P is the oracle's forward
bubble pressure at (T, x), so the bubble temperature of (P, x) is T with the vapour y, and the dew temperature of
(P, y) is T with the liquid x, known without a new solve.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import pcsaft_mix_dew_ref as D
from tests import pcsaft_mix_ref as MR
from tests import pcsaft_mix_vle_ref as V
from tests.pcsaft_ref import RGAS, TO_A3

START_EVALUATIONS = 40          # kTvleStartEvals
START_TOLERANCE = 1e-2          # kTvleStartTol
MAX_ITERATIONS = 400            # kTvleIters
TROUTON = 10.0                  # kTvleTrouton
SLOPE_MIN, SLOPE_MAX = 0.25, 40.0
# the cases the forward bubble solve of which lies too close to a critical point for the ideal-vapour start to reach
# its pressure: 8.45 MPa and 5.18 MPa
NEAR_CRITICAL = ("methane+hexane 0.4", "fixture 0")
# its vapour has a second dew point at the same P, and the Raoult start leads there
OTHER_DEW_POINT = ("fixture 15",)


def _slope_ok(sec, sign, T):
    r = sign * sec / T
    return bool(np.isfinite(r) and SLOPE_MIN <= r <= SLOPE_MAX)


def estimate(rows, z, T, kij=None, eab=None, dew=False):
    """(P_est [Pa], first w [nc]) at T: the start of the bubble-pressure kernel (the liquid z at zero pressure under an
    ideal vapour) or of the dew-pressure kernel (Raoult's law on each component's own liquid at zero pressure); None
    where there is no such liquid"""
    if dew:
        return D.raoult_start(rows, z, T)
    rho_l = MR.density(MR.Mixture(rows, z, kij=kij, eab=eab), T, 0.0)
    if rho_l is None:
        return None
    f = np.exp(V.ln_fugacity(rows, z, T, rho_l, kij, eab))
    return float(f.sum()) / TO_A3 * RGAS * T, f / f.sum()


def first_guess(rows, z):
    return 0.7 * float(np.sum(z * rows[:, 2] * (0.85 + 0.42 * rows[:, 0])))


def start(rows, z, P, T0=None, kij=None, eab=None, dew=False, count=None):
    """(T, first w) or None: the kernel's start.  ``count``: a list that receives the number of estimates taken."""
    given = T0 is not None and T0 == T0
    T = float(T0) if given else first_guess(rows, z)
    Te, slope, prev = T, 0.0, None
    for ev in range(1, START_EVALUATIONS + 1):
        if count is not None:
            count[:] = [ev]
        est = estimate(rows, z, Te, kij, eab, dew)
        if est is None:
            Te, prev = 0.85 * Te, None
            continue
        if given:
            return T, est[1]
        g = float(np.log(est[0] / P))
        if not g == g:
            return None
        if abs(g) < START_TOLERANCE:
            return Te, est[1]
        u = 1.0 / Te
        if prev is None:
            slope = -TROUTON * Te
        else:
            with np.errstate(all="ignore"):
                sec = (g - prev[1]) / (u - prev[0])
            if _slope_ok(sec, -1.0, Te):
                slope = sec
        un = min(max(u - g / slope, 0.8 * u), 1.25 * u)
        prev, Te = (u, g), 1.0 / un
    return None


def solve(rows, z, P, T0=None, kij=None, eab=None, dew=False, tol=1e-10, max_iterations=MAX_ITERATIONS, trace=None):
    """Bubble (``dew`` False: z = x, w = y) or dew (z = y, w = x) temperature at (P, z): dict with T (K), w [nc], rho_l,
    rho_v (mol/m³), iterations and start (the estimates the start took), the state at which the fugacities were last
    evaluated; None where the start finds no T, a root is lost, the steps run out or only the trivial solution is
    found.  ``trace``: a list that receives (residual, T, w, rho_l, rho_v, step) of every evaluated step."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    z = np.asarray(z, dtype=np.float64)
    z = z / z.sum()
    count = []
    first = start(rows, z, P, T0, kij, eab, dew, count)
    if first is None:
        return None
    T, w = first
    sign = 1.0 if dew else -1.0
    u, prev, slope, damp = 1.0 / T, None, 0.0, 0
    for it in range(1, max_iterations + 1):
        T = 1.0 / u
        x, y = (w, z) if dew else (z, w)
        rho_l = MR.density(MR.Mixture(rows, x, kij=kij, eab=eab), T, P)
        if rho_l is None:
            return None
        rho_v = V.vapour_density(MR.Mixture(rows, y, kij=kij, eab=eab), T, P)
        if rho_v is None:
            damp += 1
            if prev is None or damp > V.DAMPINGS:
                return None
            u = 0.5 * (u + prev[0])
            continue
        damp = 0
        d = V.ln_fugacity(rows, x, T, rho_l, kij, eab) - V.ln_fugacity(rows, y, T, rho_v, kij, eab)
        d = -d if dew else d
        if not np.all(np.isfinite(d)):
            return None
        wk = w * np.exp(d)
        s = float(wk.sum())
        ls = float(np.log(s))
        res = max(abs(ls), float(np.max(np.abs(d - ls))))
        if trace is not None:
            trace.append((res, T, w, rho_l, rho_v, it))
        if not res == res:
            return None
        if res < tol:
            if not rho_l - rho_v > 1e-3 * rho_l:
                return None
            return {"T": T, "w": w, "rho_l": rho_l, "rho_v": rho_v, "iterations": it, "start": count[0]}
        if prev is None:
            slope = sign * TROUTON * T
        else:
            with np.errstate(all="ignore"):
                sec = (ls - prev[1]) / (u - prev[0])
            if _slope_ok(sec, sign, T):
                slope = sec
        w, prev = wk / s, (u, ls)
        u = min(max(u - ls / slope, 0.9 * u), 1.1 * u)
        if not (np.all(w > 0.0) and np.isfinite(u) and u > 0.0):
            return None
    return None


def bubble_temperature(rows, x, P, T0=None, kij=None, eab=None, **kw):
    """``solve`` for the bubble temperature: w is the vapour y"""
    return solve(rows, x, P, T0, kij, eab, dew=False, **kw)


def dew_temperature(rows, y, P, T0=None, kij=None, eab=None, **kw):
    """``solve`` for the dew temperature: w is the liquid x"""
    return solve(rows, y, P, T0, kij, eab, dew=True, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    """the 30 tuples (name, rows [nc, 9], T, x, forward bubble solution with P and y, the forward oracle's own change
    between its tolerances 1e-9 and 1e-11 or None for a fixture case, which it does not run that far)"""
    named = V.named_solves()
    out = []
    for (name, rows, T, x), (sol, change) in zip(list(V.NAMED) + V.fixture_cases(),
                                                 list(named) + [(s, None) for s in V.fixture_solves()]):
        assert sol is not None, name
        x = np.asarray(x, dtype=np.float64)
        out.append((name, np.asarray(rows, dtype=np.float64), float(T), x / x.sum(), sol, change))
    return out


def _read(entry):
    res, T, w, rho_l, rho_v, it = entry
    return {"T": T, "w": w, "rho_l": rho_l, "rho_v": rho_v, "iterations": it}


def _solves(dew, factor):
    """per case (the solve at 1e-10 or None; the change of the solve between the tolerances 1e-9 and 1e-11, relative in T
    and absolute in w): one run to 1e-11 each, the looser solves read from its trace, the step with the smallest
    residual standing in where the run does not reach 1e-11.  ``factor``: T0 = factor x the forward T, None = own start."""
    out = []
    for name, rows, T, x, fwd, _ in cases():
        trace = []
        z = fwd["y"] if dew else x
        solve(rows, z, fwd["P"], None if factor is None else factor * T, dew=dew, tol=1e-11, trace=trace)
        sol = next((_read(t) for t in trace if t[0] < 1e-10), None)
        if sol is None or not sol["rho_l"] - sol["rho_v"] > 1e-3 * sol["rho_l"]:
            out.append((None, 0.0))
            continue
        loose = next(t for t in trace if t[0] < 1e-9)
        tight = min(trace, key=lambda t: t[0])
        change = max(abs(loose[1] / tight[1] - 1.0), float(np.max(np.abs(loose[2] - tight[2]))))
        out.append((sol, change))
    return out


@functools.lru_cache(maxsize=None)
def bubble_solves(factor=None):
    return _solves(False, factor)


@functools.lru_cache(maxsize=None)
def dew_solves(factor=None):
    return _solves(True, factor)


def bound(change):
    """the standing rule of tests/test_pcsaft_mix_vle_gpu.py: 1e-9, or 10 x the oracle's own change between the
    tolerances 1e-9 and 1e-11 where that is more"""
    return max(1e-9, 10.0 * change)


@functools.lru_cache(maxsize=None)
def pressure_slopes():
    """d ln P / d ln T of the forward bubble pressure of every case at its (T, x): the central difference of
    ``V.bubble`` at T (1 +- 1e-3); NaN where one of the two solves fails"""
    out = []
    for name, rows, T, x, fwd, _ in cases():
        lo, hi = V.bubble(rows, x, T * (1.0 - 1e-3)), V.bubble(rows, x, T * (1.0 + 1e-3))
        out.append(float("nan") if lo is None or hi is None else
                   float(np.log(hi["P"] / lo["P"]) / np.log((1.0 + 1e-3) / (1.0 - 1e-3))))
    return out
