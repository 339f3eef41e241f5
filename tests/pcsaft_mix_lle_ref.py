"""Test-only oracle of the liquid-liquid flash of csrc/gnx_pcsaft_mix_lle.hip, on top of the stability
oracle of tests/pcsaft_mix_stab_ref.py, which is used as it is: ``S.state`` (of the liquid root and the lowest vapour root
of a composition at (T, P) the one with the lower g = sum_i x_i ln f_i; ln f from five-point differences at ``S.STEP`` =
3e-5) and ``F.rachford_rice``.

At (T, P) the feed z splits into two phases x and y, y holding the mole fraction beta of the feed: ln f_i(T, rho_x, x) =
ln f_i(T, rho_y, y) for every component, both phases at the pressure P, z = (1 - beta) x + beta y.  ``lle`` solves this by
the kernel's loop: successive substitution on ln K from ln K_i = ln(w0_i / z_i), w0 the composition the second phase
starts from (in practice the w of the stability test), every root from a full scan.  On output x is the phase of higher
molar density.  ``residuals`` is the solve-independent check, ``V.residuals`` at difference steps that mean something at
trace compositions.  Every z_i and w0_i given here must be > 0.

The five-point-difference fugacities have a noise floor: on the four-component feeds of ``POINTS`` the residual stalls
between 2e-10 and 4e-9 and never reaches the kernel's 1e-10.  So ``lle`` ends at ``TOL`` = 1e-8, and its looser answer
is read at 1e-7 from the trace (``solve_at``).

``POINTS`` is the table of the GPU test, pinned as literals: each start w0 of an unstable feed is the w of the trial of
``S.stability`` with the most negative tangent-plane distance.  ``SOLVES`` and ``DIAGRAM`` pin what the oracle's loop
gives on them.  All three are checked against the functions they were computed with in
tests/test_pcsaft_mix_lle_cpu.py.
"""
from __future__ import annotations

import numpy as np

from tests import pcsaft_mix_flash_ref as F
from tests import pcsaft_mix_ref as MR
from tests import pcsaft_mix_stab_ref as S
from tests import pcsaft_mix_vle_ref as V

MAX_STEPS = 200
TOL = 1e-8      # max_i |ln f_i(x) - ln f_i(y)| at which the oracle's loop ends; the kernel's is 1e-10
LOOSE = 1e-7    # the residual at which the looser answer is read from the trace
SAME = 1e-4     # max_i |ln(y_i / x_i)| and |rho_y / rho_x - 1| below this: both phases are the same fluid
DAMPINGS = 20
# The two difference steps of ``residuals``.  Water at z = 1e-3 in n-hexane (300 K, 1e5 Pa) gets ln f wrong by 5.8e-9 at
# h = 1e-4, 3e-11 at 3e-5 and 2e-10 at 1e-5 (tests/pcsaft_mix_stab_ref.py): the disagreement of these two is the size of
# the error of either, where that of ``V.residuals``' defaults (1e-3, 3e-4) is 4.5e-6 on that pair.
STEPS = (1e-5, S.STEP)


def lle(rows, z, w0, T, P, kij=None, eab=None, tol=TOL, max_steps=MAX_STEPS, trace=None):
    """Split of the feed z at (T, P) started from ln K = ln(w0 / z): dict with beta (the mole fraction of y), x, y [nc],
    rho_x, rho_y (mol/m³; x the denser phase) and steps; "single" where there is no split (one component, an empty
    Rachford-Rice window, convergence with beta outside [0, 1] or onto equal phases); None where it does not converge
    (a phase without a root within the dampings, a non-finite value, ``max_steps``).  ``trace``: a list that receives
    (residual, beta, x, y, rho_x, rho_y), labelled like the result, of every step, from which the answer at a looser
    ``tol`` can be read off."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    z = np.asarray(z, dtype=np.float64)
    z = z / z.sum()
    if len(z) == 1:
        return "single"
    w0 = np.asarray(w0, dtype=np.float64)
    lnk = np.log(w0 / w0.sum() / z)
    previous, damp = lnk, 0
    for it in range(1, max_steps + 1):
        K = np.exp(lnk)
        beta = F.rachford_rice(z, K)
        if beta is None:
            return "single"
        x = z / (1.0 + beta * (K - 1.0))
        y = K * x
        if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(x > 0.0) and np.all(y > 0.0)):
            return None
        sx, sy = S.state(rows, x, T, P, kij, eab), S.state(rows, y, T, P, kij, eab)
        if sx is None or sy is None:
            damp += 1
            if damp > DAMPINGS:
                return None
            lnk = 0.5 * (lnk + previous)
            continue
        damp = 0
        (rho_x, lnf_x), (rho_y, lnf_y) = sx, sy
        d = lnf_x - lnf_y
        if not np.all(np.isfinite(d)):
            return None
        res = float(np.max(np.abs(d)))
        swap = rho_y > rho_x
        out = ((1.0 - beta, y, x, rho_y, rho_x) if swap else (beta, x, y, rho_x, rho_y))
        if trace is not None:
            trace.append((res, *out))
        if res < tol:
            same = max(float(np.max(np.abs(np.log(y / x)))), abs(rho_y / rho_x - 1.0)) < SAME
            if same or not 0.0 <= beta <= 1.0:
                return "single"
            return {"beta": out[0], "x": out[1], "y": out[2], "rho_x": out[3], "rho_y": out[4], "steps": it}
        previous, lnk = lnk, lnk + d
    return None


def residuals(rows, x, y, T, rho_x, rho_y, kij=None, eab=None, steps=STEPS):
    """The equilibrium equations at a given state, ``V.residuals`` at the difference steps ``steps``: dict with p_x, p_y
    (Pa, the oracle's pressures of (x, rho_x) and (y, rho_y)), fugacity = max_i |ln f_i(x) - ln f_i(y)| at steps[1], and
    own = the oracle's own error, the largest disagreement of ln f between its two steps in either phase"""
    p_x = MR.pressure(MR.Mixture(rows, x, kij=kij, eab=eab), T, rho_x)
    p_y = MR.pressure(MR.Mixture(rows, y, kij=kij, eab=eab), T, rho_y)
    fx = [V.ln_fugacity(rows, x, T, rho_x, kij, eab, s) for s in steps]
    fy = [V.ln_fugacity(rows, y, T, rho_y, kij, eab, s) for s in steps]
    return {"p_x": p_x, "p_y": p_y, "fugacity": float(np.max(np.abs(fx[1] - fy[1]))),
            "own": float(max(np.max(np.abs(fx[0] - fx[1])), np.max(np.abs(fy[0] - fy[1]))))}


def start(rows, z, T, P, kij=None, eab=None, **kw):
    """what ``pcsaft.mixture_lle_flash`` starts from without a w0: the w of the trial of ``S.stability`` with the most
    negative tangent-plane distance; z itself where the feed is stable; None where the test is inconclusive.  ``kw`` goes
    to ``S.trial``: with max_steps=3 an unstable feed keeps its answer wherever every negative distance comes within
    three steps (a trial cut short counts as inconclusive, and a negative one wins over it)."""
    z = np.asarray(z, dtype=np.float64)
    verdict, trials = S.stability(rows, z, T, P, kij, eab, **kw)
    if verdict is None:
        return None
    if verdict:
        return z / z.sum()
    return min((t for t in trials if t is not None and t["tpd"] < 0.0), key=lambda t: t["tpd"])["w"]


# (group, name, rows key of ``S.NAMES``, T K, P Pa, z, w0)
POINTS = (
    ('liquid-liquid', 'water+hexane 300 K z_water 0.5', ('water', 'hexane'), 300.0, 100000.0, (0.5, 0.5), (0.95, 0.04999999999999999)),
    ('liquid-liquid', 'water+hexane 300 K z_water 0.999', ('water', 'hexane'), 300.0, 100000.0, (0.999, 0.001), (0.003375872929985102, 0.9966241270700148)),
    ('liquid-liquid', 'water+hexane 350 K', ('water', 'hexane'), 350.0, 1000000.0, (0.5, 0.5), (0.95, 0.04999999999999999)),
    ('liquid-liquid', 'water+butane', ('water', 'butane'), 300.0, 1000000.0, (0.3, 0.7), (0.93, 0.06999999999999998)),
    ('liquid-liquid', 'water+ethanol+hexane 0.4 0.2 0.4', ('water', 'ethanol', 'hexane'), 300.0, 100000.0, (0.4, 0.2, 0.4), (0.9400000000000001, 0.019999999999999997, 0.039999999999999994)),
    ('liquid-liquid', 'water+ethanol+hexane 0.3 0.4 0.3', ('water', 'ethanol', 'hexane'), 300.0, 100000.0, (0.3, 0.4, 0.3), (0.93, 0.039999999999999994, 0.029999999999999992)),
    ('liquid-liquid', 'water+ethanol+butane+hexane', ('water', 'ethanol', 'butane', 'hexane'), 300.0, 1000000.0, (0.4, 0.2, 0.2, 0.2), (0.9400000000000001, 0.019999999999999997, 0.019999999999999997, 0.019999999999999997)),
    ('liquid-liquid', 'water+propane+butane+hexane', ('water', 'propane', 'butane', 'hexane'), 300.0, 2000000.0, (0.5, 0.1, 0.2, 0.2), (0.95, 0.009999999999999998, 0.019999999999999997, 0.019999999999999997)),
    ('vapour-liquid', 'butane+hexane', ('butane', 'hexane'), 350.0, 506699.92680219916, (0.605651418744902, 0.394348581255098), (0.9060874368231321, 0.09391256317686784)),
    ('vapour-liquid', 'methane+butane+hexane', ('methane', 'butane', 'hexane'), 320.0, 2129773.579104033, (0.33856006475525746, 0.2346075658779136, 0.42683236936682895), (0.9771766827428544, 0.0185951901549699, 0.004228127102175717)),
    ('vapour-liquid', 'methane+propane+butane+hexane', ('methane', 'propane', 'butane', 'hexane'), 320.0, 2420527.919130938, (0.29894744439926957, 0.18263525749092663, 0.233751850334795, 0.28466544777500874), (0.9280974017334319, 0.047579873294382534, 0.021054741031719275, 0.0032679839404661554)),
    ('stable', 'water+hexane z_water 0.001', ('water', 'hexane'), 300.0, 100000.0, (0.001, 0.999), (0.001, 0.999)),
    ('stable', 'water+hexane z_water 1e-06', ('water', 'hexane'), 300.0, 100000.0, (1e-06, 0.999999), (1e-06, 0.999999)),
    ('stable', 'water+hexane z_water 0.999999999', ('water', 'hexane'), 300.0, 100000.0, (0.999999999, 9.999999717180685e-10), (0.999999999, 9.999999717180685e-10)),
    ('single phase', 'butane+hexane above the bubble point', ('butane', 'hexane'), 350.0, 760049.8902032988, (0.5, 0.5), (0.5, 0.5)),
    ('single phase', 'butane+hexane below every vapour pressure', ('butane', 'hexane'), 350.0, 64741.88063279786, (0.5, 0.5), (0.5, 0.5)),
    ('single phase', 'methane+butane+hexane above the bubble point', ('methane', 'butane', 'hexane'), 320.0, 3194660.3686560495, (0.1, 0.3, 0.6), (0.1, 0.3, 0.6)),
    ('single phase', 'methane+butane+hexane below every vapour pressure', ('methane', 'butane', 'hexane'), 320.0, 24094.44914669688, (0.1, 0.3, 0.6), (0.1, 0.3, 0.6)),
)


# per point of ``POINTS`` what ``solve_at`` gives: (beta, x, y, rho_x, rho_y, steps, change) or "single"
SOLVES = (
    (0.5034063107100837, (0.9999819609313947, 1.803906860519787e-05), (0.006784318601203679, 0.9932156813987965), 51114.85609703988, 7561.9917194204145, 23, 7.695593310693817e-08),
    (0.000988686329274883, (0.999981960931366, 1.8039068634009552e-05), (0.006784318473646698, 0.9932156815263534), 51114.85609703237, 7561.991718607798, 19, 1.308937133305164e-07),
    (0.5181974252109096, (0.9998954942030329, 0.00010450579696714603), (0.03521394643275558, 0.9647860535672445), 49500.539210287585, 7214.897872784047, 25, 1.4331012770996133e-07),
    (0.7034560289881536, (0.9998019445258044, 0.00019805547419549983), (0.004996419108110827, 0.995003580891889), 51096.40185821674, 9851.715163489149, 22, 1.4137677073309126e-07),
    (0.6789946709562535, (0.9793672623441525, 0.020593465653331776, 3.9272002515815457e-05), (0.12609508345030654, 0.2848172394482031, 0.5890876771014903), 49220.15124438134, 10308.002604462912, 22, 1.4215338661825667e-07),
    (0.8913842259517795, (0.975308910312917, 0.0246491078954827, 4.198179160017797e-05), (0.21771315008746214, 0.4457367614308981, 0.3365500884816398), 48862.72779723042, 13438.36064375666, 25, 1.3758957270658063e-07),
    (0.6786812131542291, (0.9794038279410341, 0.020406492854623218, 0.00016989537771709364, 1.9783826625743306e-05), (0.12568367669623232, 0.28502779614766793, 0.29460872873447874, 0.29467979842162106), 49225.45363745146, 11472.324799867178, 23, 1.1535677123866491e-07),
    (0.5027075797206715, (0.9997960039269557, 0.00011697529133550274, 7.9660238436632e-05, 7.360543271978408e-06), (0.005587792058205976, 0.19880708607932943, 0.3977668004893331, 0.39783832137313174), 51112.36404055456, 9079.530708487142, 23, 5.262583630287496e-08),
    (0.29999999985657055, (0.5000000000410628, 0.4999999999589372), (0.8521713958888992, 0.14782860411110074), 7812.752051435588, 193.7731619211463, 5, 8.250462054171878e-08),
    (0.2999999998426464, (0.10000000007554075, 0.30000000002202837, 0.5999999999024309), (0.8952002160916885, 0.08202521942731548, 0.02277456448099593), 8361.18524746954, 848.8164764912029, 8, 5.28654987104731e-08),
    (0.2999999996963044, (0.10000000006086239, 0.20000000006861188, 0.30000000000155913, 0.39999999986896656), (0.7631581485268801, 0.14211752475106557, 0.07917283422213132, 0.015551492499922829), 9024.856374097822, 1001.3585486708122, 9, 5.821410190145103e-08),
    'single',
    'single',
    'single',
    'single',
    'single',
    'single',
    'single',
)

# water + n-hexane, z = (0.5, 0.5), at 1e6 Pa and T = linspace(300, 350, 6): (T, ``start(..., max_steps=3)``, ``solve_at``)
DIAGRAM = (
    (300.0, (0.95, 0.04999999999999999), (0.5034022833684817, (0.999981878086518, 1.8121913482022275e-05), (0.006776454501778412, 0.9932235454982216), 51126.12786474123, 7576.027987504614, 23, 7.975610009674418e-08)),
    (310.0, (0.95, 0.04999999999999999), (0.5049643433603275, (0.9999732465547561, 2.6753445243941274e-05), (0.009857304451513038, 0.990142695548487), 50803.57139102799, 7492.794094822044, 24, 1.3255580998040083e-07)),
    (320.0, (0.95, 0.04999999999999999), (0.5070779394374715, (0.99996134445958, 3.8655540419947353e-05), (0.013995863464264555, 0.9860041365357355), 50480.76001560501, 7414.138808689882, 24, 6.494508453296675e-08)),
    (330.0, (0.95, 0.04999999999999999), (0.5098802800169968, (0.9999452217180119, 5.477828198821193e-05), (0.019430302213091378, 0.9805696977869085), 50156.699227149904, 7340.962975818199, 24, 8.73400846807241e-08)),
    (340.0, (0.95, 0.04999999999999999), (0.5135279582608212, (0.9999237294084837, 7.627059151637564e-05), (0.02641542987677227, 0.9735845701232277), 49830.33336963827, 7274.225882720078, 25, 1.2209937825904087e-07)),
    (350.0, (0.95, 0.04999999999999999), (0.5181974252109096, (0.9998954942030329, 0.00010450579696714603), (0.03521394643275558, 0.9647860535672445), 49500.539210287585, 7214.897872784047, 25, 1.4331012770996133e-07)),
)


def points():
    """(group, name, rows [k, 9], T, P, z [k], w0 [k]) of every pinned point"""
    return [(g, name, S.rows_of(key), T, P, np.asarray(z, dtype=np.float64), np.asarray(w0, dtype=np.float64))
            for g, name, key, T, P, z, w0 in POINTS]


def solve_at(rows, z, w0, T, P, kij=None, eab=None):
    """(the oracle's answer at ``TOL``, the change of its answer between the residuals ``LOOSE`` and ``TOL``: the largest
    of |d ln x_i|, |d ln y_i|; None unless it splits)"""
    trace = []
    sol = lle(rows, z, w0, T, P, kij, eab, trace=trace)
    if not isinstance(sol, dict):
        return sol, None
    loose = next(t for t in trace if t[0] < LOOSE)
    change = max(float(np.max(np.abs(np.log(loose[2] / sol["x"])))), float(np.max(np.abs(np.log(loose[3] / sol["y"])))))
    return sol, change


def _pinned(entry):
    if not isinstance(entry, tuple):
        return entry, None
    beta, x, y, rho_x, rho_y, steps, change = entry
    return {"beta": beta, "x": np.asarray(x), "y": np.asarray(y), "rho_x": rho_x, "rho_y": rho_y, "steps": steps}, change


def solves():
    """(answer, change) of every pinned point from the literals of ``SOLVES``, in the form of ``solve_at``: what the GPU
    test compares against without running the oracle's loop again (some 4 s of host time per point)"""
    return [_pinned(e) for e in SOLVES]


def diagram():
    """(T, w0 [2], answer, change) of the six pinned diagram points, from the literals of ``DIAGRAM``"""
    return [(T, np.asarray(w0), *_pinned(e)) for T, w0, e in DIAGRAM]


DIAGRAM_ROWS, DIAGRAM_P, DIAGRAM_Z = ("water", "hexane"), 1e6, (0.5, 0.5)


def agree(sol, pinned):
    """how far an answer of ``solve_at`` is from a pinned one: the largest of |d beta|, |d ln x_i|, |d ln y_i| and the
    relative differences of both densities"""
    return max(abs(sol["beta"] - pinned["beta"]), float(np.max(np.abs(np.log(sol["x"] / pinned["x"])))),
               float(np.max(np.abs(np.log(sol["y"] / pinned["y"])))), abs(sol["rho_x"] / pinned["rho_x"] - 1.0),
               abs(sol["rho_y"] / pinned["rho_y"] - 1.0))
