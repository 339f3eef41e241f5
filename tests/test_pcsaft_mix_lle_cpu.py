"""CPU side of the liquid-liquid flash: the pinned tables of tests/pcsaft_mix_lle_ref.py against the
oracles they were computed with, the oracle on its own ground (one tie line from two feeds, the equations at its own
answers, the endings without a split), the binding of the entry point, and the host checks of the reference-shaped
functions of gnnepcsaft_amd/pcsaft.py."""
import os
import re

import numpy as np
import pytest

from tests import pcsaft_mix_lle_ref as L
from tests import pcsaft_mix_stab_ref as S
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SPLIT = 11  # the points of ``L.POINTS`` that split: 8 liquid-liquid, 3 vapour-liquid


def test_pinned_points_are_what_the_oracles_give():
    """``L.POINTS``: 8 liquid-liquid feeds, the three vapour-liquid tie-line feeds, the three stable water + n-hexane feeds
    and the four single-phase points of ``S.CASES`` (the literals of that table, which its own test checks against the
    flash oracle).  The start w0 of every feed that splits is ``L.start`` at 1e-12, run with max_steps=3: every negative
    distance of these feeds comes within 2 steps, and the trivial trials of the second ternary feed take 147 to 194.
    A feed that does not split starts from itself."""
    pts = L.points()
    assert [p[0] for p in pts] == ["liquid-liquid"] * 8 + ["vapour-liquid"] * 3 + ["stable"] * 3 + ["single phase"] * 4
    assert len(set(p[1] for p in pts)) == 18 and len(L.SOLVES) == 18
    for lit, k in zip(L.POINTS[8:], (2, 4, 5, 40, 41, 42, 12, 13, 14, 15)):
        group, name, key, T, P, z, stable = S.CASES[k]
        assert lit[1:6] == (name, key, T, P, z) and stable == (lit[0] != "vapour-liquid"), name
    for _, name, rows, T, P, z, w0 in pts[:N_SPLIT]:
        first = L.start(rows, z, T, P, max_steps=3)
        print(name, first, w0)
        assert first is not None and np.max(np.abs(first - w0)) <= 1e-12 and abs(w0.sum() - 1.0) <= 1e-12, name
        assert np.max(np.abs(np.log(w0 / z))) > 0.1, name
    for _, name, rows, T, P, z, w0 in pts[N_SPLIT:]:
        assert np.array_equal(w0, z), name
    # the verdict of the stable feeds is the stability oracle's (tests/test_pcsaft_mix_stab_cpu.py runs all of them); one
    # here, in full: a stable feed starts from itself and ends at once
    _, name, rows, T, P, z, _ = pts[15]
    assert name == "butane+hexane below every vapour pressure"
    assert np.array_equal(L.start(rows, z, T, P), z / z.sum())


def test_pinned_solves_are_what_the_oracle_gives():
    """``L.SOLVES`` and ``L.DIAGRAM`` against ``L.solve_at`` (about a minute of host time): every feed that splits ends
    below 1e-8 within 30 steps (seen: 19 to 25 on the liquid-liquid feeds, 5 to 9 on the vapour-liquid ones) with the
    pinned answer.  Bound 1e-8 on beta, ln x, ln y and the relative densities: the five-point differences carry noise of
    1e-10 to 1e-9 in ln f, so two builds of numpy may end a step apart, and what a step moves there is below the residual
    it ends on.  The change between the residuals 1e-7 and 1e-8 is pinned within a factor 2 for the same reason.  The
    other seven points end as "single" without a step."""
    jobs = [(name, rows, z, w0, T, P, pin) for (_, name, rows, T, P, z, w0), pin in zip(L.points(), L.solves())]
    rows = S.rows_of(L.DIAGRAM_ROWS)
    jobs += [(f"diagram {T}", rows, np.asarray(L.DIAGRAM_Z), w0, T, L.DIAGRAM_P, (pin, change))
             for T, w0, pin, change in L.diagram()]
    assert len(jobs) == 24
    for j, (name, rows, z, w0, T, P, (pin, pinned_change)) in enumerate(jobs):
        sol, change = L.solve_at(rows, z, w0, T, P)
        if N_SPLIT <= j < 18:
            assert sol == "single" and pin == "single" and change is None and pinned_change is None, name
            continue
        assert isinstance(sol, dict) and isinstance(pin, dict), (name, sol)
        print(name, "steps", sol["steps"], "change", change, "from the literals", L.agree(sol, pin))
        assert sol["steps"] <= 30 and abs(sol["steps"] - pin["steps"]) <= 1, (name, sol["steps"], pin["steps"])
        assert L.agree(sol, pin) <= 1e-8, (name, sol, pin)
        assert 0.5 * pinned_change <= change <= 2.0 * pinned_change and change < 1e-6, (name, change, pinned_change)
        assert 0.0 < sol["beta"] < 1.0 and sol["rho_x"] > sol["rho_y"] > 0.0, name
    for T, w0, _, _ in L.diagram():
        first = L.start(rows, L.DIAGRAM_Z, T, L.DIAGRAM_P, max_steps=3)
        assert np.max(np.abs(first - w0)) <= 1e-12, T
    assert [d[0] for d in L.diagram()] == np.linspace(300.0, 350.0, 6).tolist()
    assert L.DIAGRAM[5][2] == L.SOLVES[2]  # water + n-hexane at 350 K and 1e6 Pa is in both tables


def test_two_feeds_of_one_tie_line_give_one_tie_line():
    """water + n-hexane at 300 K and 1e5 Pa from z_water = 0.5 and from 0.999: the same x and y within 10 x the larger
    change of the two solves between their residuals 1e-7 and 1e-8 (ln x, ln y), each beta what the lever rule makes of its
    feed, and the numbers of the issue: water fraction 0.00678 in the hexane-rich phase, 0.999982 in the water-rich one"""
    (a, ca), (b, cb) = L.solves()[:2]
    bound = max(1e-7, 10.0 * max(ca, cb))
    fig = max(float(np.max(np.abs(np.log(a["x"] / b["x"])))), float(np.max(np.abs(np.log(a["y"] / b["y"])))))
    print("tie line:", fig, "bound", bound, a["beta"], b["beta"])
    assert fig <= bound
    assert abs(a["y"][0] - 0.00678) < 5e-6 and abs(a["x"][0] - 0.999982) < 5e-7
    for sol, zw in ((a, 0.5), (b, 0.999)):
        lever = (sol["x"][0] - zw) / (sol["x"][0] - sol["y"][0])
        assert abs(sol["beta"] - lever) <= 1e-12
    assert abs(a["beta"] - 0.5034) < 1e-4 and abs(b["beta"] - 9.9e-4) < 1e-5
    assert abs(L.solves()[2][0]["y"][0] - 0.0352) < 5e-5  # 350 K, 1e6 Pa


def test_residuals_of_the_oracles_own_answers():
    """``L.residuals`` at every pinned answer that splits, diagram points included: both pressures are P at 1e-9 on the
    scale max(P, 1e-3 rho R T); the fugacity residual, evaluated at the step the loop runs on, is below the 1e-8 the loop
    ended at plus the 1e-8 the literals may be off by; the two difference steps disagree by less than 1e-8 (seen: 1.9e-10
    to 1.1e-9), which is what makes the GPU test's bound of 2e-10 + 10 x that disagreement a bound"""
    jobs = [(p[1], p[2], p[3], p[4], pin) for p, (pin, _) in zip(L.points()[:N_SPLIT], L.solves())]
    jobs += [(f"diagram {T}", S.rows_of(L.DIAGRAM_ROWS), T, L.DIAGRAM_P, pin) for T, _, pin, _ in L.diagram()]
    for name, rows, T, P, sol in jobs:
        r = L.residuals(rows, sol["x"], sol["y"], T, sol["rho_x"], sol["rho_y"])
        fig = {"p x": abs(r["p_x"] - P) / max(P, sol["rho_x"] * R.RGAS * T * 1e-3),
               "p y": abs(r["p_y"] - P) / max(P, sol["rho_y"] * R.RGAS * T * 1e-3), "fugacity": r["fugacity"], "own": r["own"]}
        print(name, fig)
        assert fig["p x"] <= 1e-9 and fig["p y"] <= 1e-9 and fig["fugacity"] < 2e-8 and fig["own"] < 1e-8, (name, fig)


def test_oracle_endings_without_a_split():
    """one component, w0 = z and the same row twice end as "single", the last after steps that bring every K to 1"""
    assert L.lle([V.HEXANE], [1.0], [1.0], 350.0, 4e5) == "single"
    assert L.lle([V.BUTANE, V.HEXANE], [0.5, 0.5], [0.5, 0.5], 350.0, 4e5) == "single"
    trace = []
    assert L.lle([V.HEXANE, V.HEXANE], [0.3, 0.7], [0.6, 0.4], 350.0, 4e5, trace=trace) == "single" and len(trace) >= 1


def test_binding_declares_the_lle_entry_point():
    from gnnepcsaft_amd import _lib, build
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_mix_lle is not None and "gnx_pcsaft_mix_lle.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    decl = re.search(r"int32_t gnx_pcsaft_mix_lle\(([^;]*)\);", header)
    assert decl is not None and "mix_lle_feos" in header and "kij.py:37" in header
    assert len(_lib.SIGNATURES["gnx_pcsaft_mix_lle"][1]) == len(decl.group(1).split(",")) == 20
    assert "const double* w0" in decl.group(1)
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26 and lib.gnx_abi_version() == 7
    assert "GNX_K_COUNT = 26" in header and "#define GNX_ABI_VERSION 7" in header


def test_host_functions_need_a_device():
    """there is no CPU path: without a HIP device ``pcsaft._device`` raises GnxError, and so does every well-formed call"""
    import torch
    from gnnepcsaft_amd import _lib, pcsaft
    rows = [V.WATER, V.HEXANE]
    state = [300.0, 1e5, 0.5, 0.5]
    calls = (lambda: pcsaft.mix_lle(rows, state),
             lambda: pcsaft.mix_lle_diagram(rows, state, points=3),
             lambda: pcsaft.mix_lle_batch([rows], [np.array([state])]))
    if not torch.cuda.is_available():
        for call in calls:
            with pytest.raises(_lib.GnxError, match="no CPU fallback"):
                call()
    assert callable(pcsaft.mixture_lle_flash) and callable(pcsaft.ops.pcsaft_mix_lle)
    assert callable(pcsaft.ops._pcsaft_mix_lle)


def test_reference_shaped_functions_reject_malformed_input():
    """the checks that run on the host before anything is uploaded"""
    from gnnepcsaft_amd import pcsaft
    rows = [V.WATER, V.HEXANE]
    state = [300.0, 1e5, 0.5, 0.5]
    for call in (pcsaft.mix_lle, pcsaft.mix_lle_diagram):
        with pytest.raises(ValueError):
            call(rows, state, kij_matrix=np.zeros((3, 3)))
        with pytest.raises(ValueError):
            call(rows, state, epsilon_ab=np.zeros((2, 3)))
        with pytest.raises(ValueError):
            call(rows * 3, [300.0, 1e5] + [1.0 / 6] * 6)
        with pytest.raises(ValueError):
            call(rows, [300.0, 1e5, 0.5, 0.3, 0.2])
    with pytest.raises(ValueError, match="at least 1 point"):
        pcsaft.mix_lle_diagram(rows, state, points=0)
    with pytest.raises(ValueError):
        pcsaft.mix_lle_batch([rows], [np.zeros((1, 4)), np.zeros((1, 4))])
    with pytest.raises(ValueError):
        pcsaft.mix_lle_batch([rows], [np.zeros((1, 5))])
    with pytest.raises(ValueError):
        pcsaft.mix_lle_batch([rows], [np.zeros((1, 4))], kij=[np.zeros((3, 3))])
    assert pcsaft.mix_lle_batch([rows], [np.zeros((0, 4))]) == []
