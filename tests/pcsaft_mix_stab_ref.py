"""Test-only oracle of the tangent-plane stability test of csrc/gnx_pcsaft_mix_stab.hip, on top of the
mixture oracles, which are used as they are: ``MR.density`` (liquid root), ``V.vapour_density`` (lowest vapour root),
``V.ln_fugacity`` (ln f_i = mu_i^res/kT + ln(rho x_i) from five-point differences in the mole numbers, here with the
step ``STEP``).

``trial`` runs one trial phase by the kernel's loop on those evaluations, ``stability`` all nc + 2 of a feed and the
verdict.  ``distance`` is the solve-independent check: the tangent-plane distance D = sum_i w_i (ln f_i(w) - ln f_i(z)) of
a given (w, rho_w) against a given (z, rho_z), how far it is from stationary, the oracle's pressures of both states and
the oracle's own error.  Every z_i and w_i given here must be > 0.

``CASES`` is the table of the GPU test, pinned as literals: pressures and feeds were computed once with the bubble and
flash oracles (``F.tie_line_points``, ``F.single_phase_points``, ``V.named_solves``) and are checked against them in
tests/test_pcsaft_mix_stab_cpu.py.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import pcsaft_mix_phi_ref as PR
from tests import pcsaft_mix_ref as MR
from tests import pcsaft_mix_vle_ref as V
from tests.pcsaft_ref import RGAS, TO_A3

MAX_STEPS = 400
TOL = 1e-8        # max_i |r_i| of a stationary trial
NEGATIVE = -1e-8  # D below this: unstable
TRIVIAL = 1e-4    # ln(w_i / z_i) and rho_w / rho_z - 1 within this: the trial is the feed
RICH = 0.9
# The difference step of the solve's ln f.  The truncation error of the five-point stencil goes with h^4, and on an
# associating component at trace level it is not small at ``V.ln_fugacity``'s default h = 3e-4: water at z = 1e-3 in
# n-hexane (300 K, 1e5 Pa) gets ln f wrong by 4.7e-7 there (5.8e-9 at 1e-4, 3e-11 at 3e-5, 2e-10 at 1e-5, 1e-8 at 1e-6,
# where the rounding of F, 1e-16 / h, takes over), which is the whole difference to the kernel's tangent-plane distance
# at that point and above the 1e-7 to which the solves are compared.  ``distance`` keeps both steps of ``V.residuals``
# and reports their disagreement.
STEP = 3e-5


def state(rows, x, T, P, kij=None, eab=None):
    """(rho mol/m³, ln f [nc]) of x at (T, P): of the liquid root and the lowest vapour root the one with the lower g =
    sum_i x_i ln f_i, the liquid root on a tie; None where there is no root"""
    mix = MR.Mixture(rows, x, kij=kij, eab=eab)
    best = None
    for rho in (MR.density(mix, T, P), V.vapour_density(mix, T, P)):
        if rho is None:
            continue
        lnf = V.ln_fugacity(rows, x, T, rho, kij, eab, STEP)
        g = float(np.sum(x * lnf))
        if np.all(np.isfinite(lnf)) and (best is None or g < best[0]):
            best = (g, rho, lnf)
    return None if best is None else best[1:]


def start(z, lnf_z, T, P, t):
    """the mole numbers W that trial t of the feed z starts from"""
    lnk = lnf_z - np.log(z * (P / (RGAS * T) * TO_A3))
    if t == 0:
        return z * np.exp(lnk)
    if t == 1:
        return z * np.exp(-lnk)
    W = (1.0 - RICH) * z
    W[t - 2] += RICH
    return W


def trial(rows, z, T, P, t, kij=None, eab=None, tol=TOL, max_steps=MAX_STEPS, trace=None):
    """Trial t (0 vapour-like, 1 liquid-like, 2 + s rich in component s) of the feed z at (T, P): dict with kind
    ("trivial", "negative" or "stationary"), tpd, w [nc], rho_w, rho_z (mol/m³) and steps; None where the feed or a w has
    no root, a value is not finite or ``max_steps`` run out.  ``trace``: a list that receives (residual, D, w, rho_w) of
    every step that ends nothing, from which the answer at a looser ``tol`` can be read off."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    z = np.asarray(z, dtype=np.float64)
    z = z / z.sum()
    feed = state(rows, z, T, P, kij, eab)
    if feed is None:
        return None
    rho_z, d = feed
    if len(z) == 1:
        return {"kind": "trivial", "tpd": 0.0, "w": z, "rho_w": rho_z, "rho_z": rho_z, "steps": 0}
    W = start(z, d, T, P, t)
    for it in range(1, max_steps + 1):
        S = float(W.sum())
        w = W / S
        if not (np.isfinite(S) and S > 0.0 and np.all(np.isfinite(w)) and np.all(w > 0.0)):
            return None
        at = state(rows, w, T, P, kij, eab)
        if at is None:
            return None
        rho_w, lnf = at
        dl = lnf - d
        if not np.all(np.isfinite(dl)):
            return None
        if max(float(np.max(np.abs(np.log(w / z)))), abs(rho_w / rho_z - 1.0)) < TRIVIAL:
            return {"kind": "trivial", "tpd": 0.0, "w": z, "rho_w": rho_z, "rho_z": rho_z, "steps": it}
        D, res = float(np.sum(w * dl)), float(np.max(np.abs(np.log(S) + dl)))
        out = {"tpd": D, "w": w, "rho_w": rho_w, "rho_z": rho_z, "steps": it}
        if D < NEGATIVE:
            return dict(out, kind="negative")
        if trace is not None:
            trace.append((res, D, w, rho_w))
        if res < tol:
            return dict(out, kind="stationary")
        W = w * np.exp(-dl)
    return None


def verdict(trials):
    """True (stable), False (unstable) or None (inconclusive) from the trials of one feed, as ``pcsaft._reduce_trials``"""
    if any(t is not None and t["tpd"] < 0.0 for t in trials):
        return False
    return None if any(t is None for t in trials) else True


def stability(rows, z, T, P, kij=None, eab=None, **kw):
    """(verdict, the nc + 2 trials) of the feed z at (T, P)"""
    trials = [trial(rows, z, T, P, t, kij, eab, **kw) for t in range(len(z) + 2)]
    return verdict(trials), trials


def distance(rows, z, w, T, rho_z, rho_w, kij=None, eab=None):
    """The tangent-plane equations at given states: dict with D = sum_i w_i (ln f_i(w) - ln f_i(z)); stationarity = max_i
    |ln f_i(w) - ln f_i(z) - (-ln S)| with -ln S = D, which it is at a stationary point of normalised w; p_z, p_w (Pa, the
    oracle's pressures of (z, rho_z) and (w, rho_w)); and own = the oracle's own error, the largest disagreement of
    mu^res between its two difference steps in either state, as ``V.residuals`` reports it"""
    z = np.asarray(z, dtype=np.float64)
    z = z / z.sum()
    w = np.asarray(w, dtype=np.float64)
    w = w / w.sum()
    fz = [V.ln_fugacity(rows, z, T, rho_z, kij, eab, s) for s in PR.STEPS]
    fw = [V.ln_fugacity(rows, w, T, rho_w, kij, eab, s) for s in PR.STEPS]
    dl = fw[1] - fz[1]
    D = float(np.sum(w * dl))
    return {"D": D, "stationarity": float(np.max(np.abs(dl - D))),
            "p_z": MR.pressure(MR.Mixture(rows, z, kij=kij, eab=eab), T, rho_z),
            "p_w": MR.pressure(MR.Mixture(rows, w, kij=kij, eab=eab), T, rho_w),
            "own": float(max(np.max(np.abs(fz[0] - fz[1])), np.max(np.abs(fw[0] - fw[1]))))}


NAMES = {"methane": V.METHANE, "propane": V.PROPANE, "butane": V.BUTANE, "hexane": V.HEXANE, "ethanol": V.ETHANOL,
         "water": V.WATER}


def rows_of(key):
    """the component rows of a case: a tuple of names of ``NAMES``, or ("fixture", k) for system k of the binary fixture"""
    if key[0] == "fixture":
        return np.asarray(V.fixture_cases()[key[1]][1], dtype=np.float64)
    return np.asarray([NAMES[name] for name in key], dtype=np.float64)


# (group, name, rows key, T K, P Pa, z, stable)
CASES = (
    ("tie line", "methane+hexane 0.1", ('methane', 'hexane'), 300.0, 1818388.5183354113, (0.36486323107612356, 0.6351367689238764), False),
    ("tie line", "methane+hexane 0.4", ('methane', 'hexane'), 300.0, 8454441.728529088, (0.5755338677817441, 0.4244661322182558), False),
    ("tie line", "butane+hexane", ('butane', 'hexane'), 350.0, 506699.92680219916, (0.605651418744902, 0.394348581255098), False),
    ("tie line", "ethanol+water", ('ethanol', 'water'), 350.0, 89679.34214037994, (0.37674626869373884, 0.6232537313062612), False),
    ("tie line", "methane+butane+hexane", ('methane', 'butane', 'hexane'), 320.0, 2129773.579104033, (0.33856006475525746, 0.2346075658779136, 0.42683236936682895), False),
    ("tie line", "methane+propane+butane+hexane", ('methane', 'propane', 'butane', 'hexane'), 320.0, 2420527.919130938, (0.29894744439926957, 0.18263525749092663, 0.233751850334795, 0.28466544777500874), False),
    ("tie line", "fixture 0", ('fixture', 0), 273.15, 5176824.9760308415, (0.14673821545450327, 0.8532617845454966), False),
    ("tie line", "fixture 1", ('fixture', 1), 293.15, 125.01671706579023, (0.03491045745092488, 0.9650895425490751), False),
    ("tie line", "fixture 2", ('fixture', 2), 293.15, 13.552582082551274, (0.10891193527307419, 0.8910880647269258), False),
    ("tie line", "fixture 3", ('fixture', 3), 293.15, 2.155240489885293, (0.49875896985406654, 0.5012410301459335), False),
    ("tie line", "fixture 4", ('fixture', 4), 303.15, 38137.9879634271, (0.025102842626384445, 0.9748971573736156), False),
    ("tie line", "fixture 5", ('fixture', 5), 303.15, 13504.205682184136, (0.02531913053642145, 0.9746808694635786), False),
    ("single phase", "butane+hexane above the bubble point", ('butane', 'hexane'), 350.0, 760049.8902032988, (0.5, 0.5), True),
    ("single phase", "butane+hexane below every vapour pressure", ('butane', 'hexane'), 350.0, 64741.88063279786, (0.5, 0.5), True),
    ("single phase", "methane+butane+hexane above the bubble point", ('methane', 'butane', 'hexane'), 320.0, 3194660.3686560495, (0.1, 0.3, 0.6), True),
    ("single phase", "methane+butane+hexane below every vapour pressure", ('methane', 'butane', 'hexane'), 320.0, 24094.44914669688, (0.1, 0.3, 0.6), True),
    ("bubble side", "methane+hexane 0.1 x 0.98", ('methane', 'hexane'), 300.0, 1782020.747968703, (0.1, 0.9), False),
    ("bubble side", "methane+hexane 0.1 x 1.02", ('methane', 'hexane'), 300.0, 1854756.2887021196, (0.1, 0.9), True),
    ("bubble side", "methane+hexane 0.4 x 0.98", ('methane', 'hexane'), 300.0, 8285352.893958506, (0.4, 0.6), False),
    ("bubble side", "methane+hexane 0.4 x 1.02", ('methane', 'hexane'), 300.0, 8623530.56309967, (0.4, 0.6), True),
    ("bubble side", "butane+hexane x 0.98", ('butane', 'hexane'), 350.0, 496565.9282661552, (0.5, 0.5), False),
    ("bubble side", "butane+hexane x 1.02", ('butane', 'hexane'), 350.0, 516833.92533824313, (0.5, 0.5), True),
    ("bubble side", "methane+butane+hexane x 0.98", ('methane', 'butane', 'hexane'), 320.0, 2087178.1075219521, (0.1, 0.3, 0.6), False),
    ("bubble side", "methane+butane+hexane x 1.02", ('methane', 'butane', 'hexane'), 320.0, 2172369.0506861135, (0.1, 0.3, 0.6), True),
    ("bubble side", "methane+propane+butane+hexane x 0.98", ('methane', 'propane', 'butane', 'hexane'), 320.0, 2372117.3607483194, (0.1, 0.2, 0.3, 0.4), False),
    ("bubble side", "methane+propane+butane+hexane x 1.02", ('methane', 'propane', 'butane', 'hexane'), 320.0, 2468938.477513557, (0.1, 0.2, 0.3, 0.4), True),
    ("dew side", "methane+hexane 0.1 y 0.98", ('methane', 'hexane'), 300.0, 1782020.747968703, (0.982877436920412, 0.01712256307958795), True),
    ("dew side", "methane+hexane 0.1 y 1.02", ('methane', 'hexane'), 300.0, 1854756.2887021196, (0.982877436920412, 0.01712256307958795), False),
    ("dew side", "methane+hexane 0.4 y 0.98", ('methane', 'hexane'), 300.0, 8285352.893958506, (0.9851128926058138, 0.014887107394186111), False),
    ("dew side", "methane+hexane 0.4 y 1.02", ('methane', 'hexane'), 300.0, 8623530.56309967, (0.9851128926058138, 0.014887107394186111), True),
    ("dew side", "butane+hexane y 0.98", ('butane', 'hexane'), 350.0, 496565.9282661552, (0.85217139581634, 0.14782860418366), True),
    ("dew side", "butane+hexane y 1.02", ('butane', 'hexane'), 350.0, 516833.92533824313, (0.85217139581634, 0.14782860418366), False),
    ("dew side", "ethanol+water y 0.98", ('ethanol', 'water'), 350.0, 87885.75529757234, (0.5558208956457962, 0.4441791043542039), True),
    ("dew side", "ethanol+water y 1.02", ('ethanol', 'water'), 350.0, 91472.92898318755, (0.5558208956457962, 0.4441791043542039), False),
    ("dew side", "methane+butane+hexane y 0.98", ('methane', 'butane', 'hexane'), 320.0, 2087178.1075219521, (0.8952002158508583, 0.08202521959304529, 0.022774564556096468), True),
    ("dew side", "methane+butane+hexane y 1.02", ('methane', 'butane', 'hexane'), 320.0, 2172369.0506861135, (0.8952002158508583, 0.08202521959304529, 0.022774564556096468), False),
    ("dew side", "methane+propane+butane+hexane y 0.98", ('methane', 'propane', 'butane', 'hexane'), 320.0, 2372117.3607483194, (0.7631581479975652, 0.14211752496975547, 0.07917283444931675, 0.015551492583362645), True),
    ("dew side", "methane+propane+butane+hexane y 1.02", ('methane', 'propane', 'butane', 'hexane'), 320.0, 2468938.477513557, (0.7631581479975652, 0.14211752496975547, 0.07917283444931675, 0.015551492583362645), False),
    ("liquid-liquid", "water+hexane z_water 0.5", ('water', 'hexane'), 300.0, 100000.0, (0.5, 0.5), False),
    ("liquid-liquid", "water+hexane z_water 0.999", ('water', 'hexane'), 300.0, 100000.0, (0.999, 0.0010000000000000009), False),
    ("liquid-liquid", "water+hexane z_water 0.001", ('water', 'hexane'), 300.0, 100000.0, (0.001, 0.999), True),
    ("liquid-liquid", "water+hexane z_water 1e-06", ('water', 'hexane'), 300.0, 100000.0, (1e-06, 0.999999), True),
    ("liquid-liquid", "water+hexane z_water 0.999999999", ('water', 'hexane'), 300.0, 100000.0, (0.999999999, 9.999999717180685e-10), True),
)


def cases():
    """(group, name, rows [k, 9], T, P, z [k], stable) of every pinned case"""
    return [(g, name, rows_of(key), T, P, np.asarray(z, dtype=np.float64), stable)
            for g, name, key, T, P, z, stable in CASES]


@functools.lru_cache(maxsize=None)
def table_solves():
    """per case the oracle's nc + 2 trials, stationary ones run on to a residual of 1e-9 (at most 600 steps): each entry
    None or (the trial as ``trial`` ends it at the kernel's 1e-8, the change of its (tpd, w) between the residuals 1e-7 and
    1e-9: None unless stationary).  Computed once, shared, never modified."""
    out = []
    for _, _, rows, T, P, z, _ in cases():
        per = []
        for t in range(len(z) + 2):
            trace = []
            tight = trial(rows, z, T, P, t, tol=1e-9, max_steps=600, trace=trace)
            if tight is None or tight["kind"] != "stationary":
                per.append(None if tight is None or tight["steps"] > MAX_STEPS else (tight, None))
                continue
            step, at = next((k, e) for k, e in enumerate(trace) if e[0] < TOL)
            if tight["steps"] - (len(trace) - 1 - step) > MAX_STEPS:
                per.append(None)
                continue
            loose = next(e for e in trace if e[0] < 1e-7)
            change = max(abs(loose[1] - tight["tpd"]), float(np.max(np.abs(loose[2] - tight["w"]))))
            sol = {"kind": "stationary", "tpd": at[1], "w": at[2], "rho_w": at[3], "rho_z": tight["rho_z"],
                   "steps": tight["steps"] - (len(trace) - 1 - step)}
            per.append((sol, change))
        out.append(per)
    return out
