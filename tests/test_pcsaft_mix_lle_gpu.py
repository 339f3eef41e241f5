"""Liquid-liquid flash on the GPU (csrc/gnx_pcsaft_mix_lle.hip, gnnepcsaft_amd/pcsaft.py) against the oracle of
tests/pcsaft_mix_lle_ref.py: the equilibrium equations at the state every splitting point reports (the primary check:
the oracle's pressure and finite-difference fugacities share no mechanism with the kernel's duals), the oracle's own
solve, tie-line invariance, the vapour-liquid flash on the feeds both can split, the gap this entry closes, statuses,
reductions, lanes and repeatability, explicit starts, and the reference-shaped I/O.

The table is the 18 points of ``L.POINTS`` and one single component (1 to 4 used slots of 4): one launch of
``pcsaft.mixture_lle_flash`` with the stability start, which every test shares."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_flash_ref as F
from tests import pcsaft_mix_lle_ref as L
from tests import pcsaft_mix_stab_ref as S
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

pytestmark = pytest.mark.gpu

NC = 4
N_SPLIT = 11      # the first points of the table split: 8 liquid-liquid, 3 vapour-liquid
SOLVE_TOL = 1e-10  # kVleMixTol: the residual the kernel's loop ends on


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _lle(dev, params, comp, owner, T, P, z, w0=None, kij=None, eab=None):
    """(beta, x, y, rho_x, rho_y, status) of ``pcsaft.mixture_lle_flash`` as host arrays; w0 None: the stability start"""
    from gnnepcsaft_amd import pcsaft
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
    p, c, o, t, pp, zz, ww, k, e = _dev(dev, f64(params).reshape(-1, 9), comp, np.asarray(owner, dtype=np.int64), f64(T),
                                        f64(P), f64(z), f64(w0), kij, eab)
    return [v.cpu().numpy() for v in pcsaft.mixture_lle_flash(p, c, zz, t, pp, o, k, e, w0=ww)]


def _flash(dev, params, comp, owner, T, P, z):
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, pp, zz = _dev(dev, np.asarray(params, dtype=np.float64).reshape(-1, 9), comp,
                              np.asarray(owner, dtype=np.int64), np.asarray(T, dtype=np.float64),
                              np.asarray(P, dtype=np.float64), np.asarray(z, dtype=np.float64))
    return [v.cpu().numpy() for v in pcsaft.mixture_tp_flash(p, c, zz, t, pp, o)]


def _cases():
    """(name, rows, T, P, z, w0) of the table: ``L.points()`` and n-hexane alone at 350 K and 4e5 Pa"""
    one = np.asarray([V.HEXANE], dtype=np.float64)
    return [p[1:] for p in L.points()] + [("hexane alone", one, 350.0, 4e5, np.array([1.0]), np.array([1.0]))]


@functools.lru_cache(maxsize=None)
def _table():
    """the table as one pool: params [B, 9], comp [M, 4] (-1 = unused), owner [M], T [M], P [M], z [M, 4], w0 [M, 4]"""
    cases = _cases()
    params, comp = [], np.full((len(cases), NC), -1, dtype=np.int64)
    z, w0 = np.zeros((len(cases), NC)), np.zeros((len(cases), NC))
    for i, (_, rows, _, _, zi, wi) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        z[i, :len(rows)], w0[i, :len(rows)] = zi, wi
    return (np.array(params), comp, np.arange(len(cases), dtype=np.int64), np.array([c[2] for c in cases], dtype=np.float64),
            np.array([c[3] for c in cases], dtype=np.float64), z, w0)


@functools.lru_cache(maxsize=None)
def _table_points(dev):
    """``mixture_lle_flash`` with the stability start on the 19 points, one launch: computed once, shared, never modified"""
    return _lle(dev, *_table()[:6])


def _rel(a, b):
    return abs(a / b - 1.0)


def _same_bytes(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def _assert_failed(out, j, status):
    beta, x, y, rx, ry, st = out
    assert st[j] == status, (j, st[j], status)
    assert beta[j] == 0.0 and rx[j] == 0.0 and ry[j] == 0.0 and np.all(np.isnan(x[j])) and np.all(np.isnan(y[j]))


def _ln_gap(x, y, sol):
    """the largest of |ln x_i - ln x_i(sol)| and |ln y_i - ln y_i(sol)|"""
    return max(float(np.max(np.abs(np.log(x / sol["x"])))), float(np.max(np.abs(np.log(y / sol["y"])))))


def test_the_equations_at_the_reported_state(gpu_device):
    """Every point that splits: status 0, 0 < beta < 1, rho_x > rho_y > 0, -1 slots NaN, sum x = sum y = 1 and the material
    balance at 1e-12; the oracle's pressure of both phases is P within 1e-9 on the scale max(P, 1e-3 rho R T); the oracle's
    max_i |ln f_i(x) - ln f_i(y)| at the reported state is at most 2 x the kernel's 1e-10 + 10 x the oracle's two-step
    disagreement there (difference steps 1e-5 and 3e-5, ``L.STEPS``).  The flash test's bounds for the same equations.
    On an MI355X (one run), worst of the 11 points: sum x - 1 and sum y - 1 2.2e-16, balance 1.1e-16, pressure of x 2.1e-10
    (the second ternary feed), of y 4.1e-12; the oracle's fugacity residual 3.4e-11 to 2.2e-9, at most 0.26 of the bound
    (water + n-hexane at 300 K from z_water = 0.999, where the two steps disagree by 8.1e-10; they disagree by 8.3e-11 to
    9.5e-10 over the points)."""
    cases = _cases()
    beta, x, y, rx, ry, st = _table_points(gpu_device)
    assert x.shape == y.shape == (19, NC) and st.dtype == np.int32
    worst = {"sum x": 0.0, "sum y": 0.0, "balance": 0.0, "p x": 0.0, "p y": 0.0, "fugacity": 0.0, "two-step": 0.0,
             "of bound": 0.0}
    for j, (name, rows, T, P, z, _) in enumerate(cases[:N_SPLIT]):
        k = len(rows)
        assert st[j] == 0 and 0.0 < beta[j] < 1.0 and rx[j] > ry[j] > 0.0, (name, st[j], beta[j], rx[j], ry[j])
        assert np.all(np.isnan(x[j, k:])) and np.all(np.isnan(y[j, k:])) and np.all(x[j, :k] > 0.0) and np.all(y[j, :k] > 0.0)
        r = L.residuals(rows, x[j, :k], y[j, :k], T, rx[j], ry[j])
        bound = 2.0 * SOLVE_TOL + 10.0 * r["own"]
        fig = {"sum x": abs(x[j, :k].sum() - 1.0), "sum y": abs(y[j, :k].sum() - 1.0),
               "balance": F.balance(z, x[j, :k], y[j, :k], beta[j]),
               "p x": abs(r["p_x"] - P) / max(P, rx[j] * R.RGAS * T * 1e-3),
               "p y": abs(r["p_y"] - P) / max(P, ry[j] * R.RGAS * T * 1e-3), "fugacity": r["fugacity"],
               "two-step": r["own"], "of bound": r["fugacity"] / bound}
        print(name, "beta", beta[j], "x", x[j, :k], "y", y[j, :k], fig)
        for key, v in fig.items():
            worst[key] = max(worst[key], v)
        assert fig["sum x"] <= 1e-12 and fig["sum y"] <= 1e-12 and fig["balance"] <= 1e-12, (name, fig)
        assert fig["p x"] <= 1e-9 and fig["p y"] <= 1e-9, (name, fig)
        assert r["fugacity"] <= bound, (name, fig, bound)
    print("worst over", N_SPLIT, "points:", worst)


def test_against_the_oracles_own_solve(gpu_device):
    """Every point that splits, against the pinned answer of the oracle's loop (``L.SOLVES``; x the denser phase in both):
    ln x_i and ln y_i, compared relatively because the compositions reach 1e-5, within max(1e-7, 10 x the change of the
    oracle's answer between its residuals 1e-7 and 1e-8); beta within that bound over max_i |y_i - x_i| (beta is the
    compositions' error seen through the lever rule).  Every other point of ``L.POINTS`` is "single" for the oracle and 4
    here.  On an MI355X (one run): ln x and ln y within 1.2e-8, beta within 3.0e-10, densities within 3.4e-10, at most
    0.015 of the bound; the oracle's own change is 5.3e-8 to 1.4e-7, its step counts 19 to 25 and 5 to 9."""
    beta, x, y, rx, ry, st = _table_points(gpu_device)
    worst = {"ln x, ln y": 0.0, "beta": 0.0, "of bound": 0.0, "change": 0.0}
    for j, ((name, rows, T, P, z, _), (sol, change)) in enumerate(zip(_cases(), L.solves())):
        k = len(rows)
        if j >= N_SPLIT:
            assert sol == "single" and st[j] == 4, (name, sol, st[j])
            continue
        bound = max(1e-7, 10.0 * change)
        lever = bound / float(np.max(np.abs(sol["y"] - sol["x"])))
        fig = {"ln x, ln y": _ln_gap(x[j, :k], y[j, :k], sol), "beta": abs(beta[j] - sol["beta"]), "change": change}
        fig["of bound"] = max(fig["ln x, ln y"] / bound, fig["beta"] / lever)
        print(name, "oracle steps", sol["steps"], fig, "rho_x", _rel(rx[j], sol["rho_x"]), "rho_y", _rel(ry[j], sol["rho_y"]))
        for key, v in fig.items():
            worst[key] = max(worst[key], v)
        assert fig["of bound"] <= 1.0, (name, fig, bound)
    print("worst:", worst)


def test_tie_line_invariance(gpu_device):
    """water + n-hexane at 350 K and the first ternary point: the feeds (1 - b) x + b y, b = 0.2 and 0.8, built from the
    reported x and y, give x and y back within the bound of the oracle comparison (ln x, ln y) and beta = b within that
    bound over max_i |y_i - x_i|; each through its own stability test and start.  On an MI355X (one run): ln x and ln y
    within 2.4e-10, beta within 4.6e-12, densities within 1.4e-11."""
    params, comp, owner, T, P, z, _ = _table()
    beta, x, y, rx, ry, st = _table_points(gpu_device)
    pick, bs = np.array([2, 2, 4, 4]), np.array([0.2, 0.8, 0.2, 0.8])
    assert _cases()[2][0] == "water+hexane 350 K" and _cases()[4][0] == "water+ethanol+hexane 0.4 0.2 0.4"
    feeds = np.nan_to_num((1.0 - bs)[:, None] * x[pick] + bs[:, None] * y[pick])
    out = _lle(gpu_device, params, comp, owner[pick], T[pick], P[pick], feeds)
    for i, (j, b) in enumerate(zip(pick, bs)):
        k = int((comp[j] >= 0).sum())
        bound = max(1e-7, 10.0 * L.solves()[j][1])
        here = {"x": x[j, :k], "y": y[j, :k]}
        fig = {"ln x, ln y": _ln_gap(out[1][i, :k], out[2][i, :k], here), "beta": abs(out[0][i] - b),
               "rho": max(_rel(out[3][i], rx[j]), _rel(out[4][i], ry[j]))}
        print(_cases()[j][0], "b", b, fig, "bound", bound)
        assert out[5][i] == 0 and fig["ln x, ln y"] <= bound, (j, b, fig)
        assert fig["beta"] <= bound / float(np.max(np.abs(y[j, :k] - x[j, :k]))), (j, b, fig)


def test_agrees_with_the_vapour_liquid_flash(gpu_device):
    """The three vapour-liquid tie-line feeds: ``mixture_lle_flash`` from the stability start returns the x, y, beta and
    densities of ``mixture_tp_flash``, within max(1e-9, 10 x the change of the oracle's flash between its tolerances 1e-9
    and 1e-11), the bound of ``F.tie_line_solves``, computed here for these three feeds alone; beta within that bound over
    max_i |y_i - x_i|.  The two solves share no start: an ideal vapour over the liquid feed there, the w of the stability
    test here.  On an MI355X (one run): x within 1.1e-12, y 5.0e-12, beta 2.3e-12, densities 1.7e-12; the bound is 1e-9 on
    all three."""
    params, comp, owner, T, P, z, _ = _table()
    mine = _table_points(gpu_device)
    sub = np.arange(8, N_SPLIT)
    flash = _flash(gpu_device, params, comp, owner[sub], T[sub], P[sub], z[sub])
    for i, j in enumerate(sub):
        name, rows, Tj, Pj, zj, _ = _cases()[j]
        k = len(rows)
        trace = []
        tight = F.flash(rows, zj, Tj, Pj, tol=1e-11, max_iterations=300, trace=trace)
        loose = next(t for t in trace if t[0] < 1e-9)
        change = max(float(np.max(np.abs(loose[2] - tight["x"]))), float(np.max(np.abs(loose[3] - tight["y"]))))
        bound = max(1e-9, 10.0 * change)
        assert flash[5][i] == 0 and mine[5][j] == 0, name
        fig = {"x": float(np.max(np.abs(mine[1][j, :k] - flash[1][i, :k]))),
               "y": float(np.max(np.abs(mine[2][j, :k] - flash[2][i, :k]))), "beta": abs(mine[0][j] - flash[0][i]),
               "rho_x": _rel(mine[3][j], flash[3][i]), "rho_y": _rel(mine[4][j], flash[4][i])}
        print(name, fig, "bound", bound)
        assert max(fig["x"], fig["y"], fig["rho_x"], fig["rho_y"]) <= bound, (name, fig, bound)
        assert fig["beta"] <= bound / float(np.max(np.abs(flash[2][i, :k] - flash[1][i, :k]))), (name, fig, bound)


def test_the_gap_this_closes(gpu_device):
    """water + n-hexane at 300 K, 1e5 Pa and z_water = 0.5: ``mixture_tp_flash`` reports 4, ``mixture_lle_flash`` 0, with
    the two liquids of the issue: water fraction 0.999982 in the denser phase and 0.00678 in the other"""
    params, comp, owner, T, P, z, _ = _table()
    assert _cases()[0][0] == "water+hexane 300 K z_water 0.5"
    flash = _flash(gpu_device, params, comp, owner[:1], T[:1], P[:1], z[:1])
    beta, x, y, rx, ry, st = _table_points(gpu_device)
    _assert_failed(flash, 0, 4)
    assert st[0] == 0 and abs(x[0, 0] - 0.999982) < 5e-7 and abs(y[0, 0] - 0.00678) < 5e-6 and abs(beta[0] - 0.5034) < 1e-4
    assert rx[0] > 5 * ry[0] > 2.5e4  # two liquids: no vapour density at 1e5 Pa is near 5000 mol/m³


def test_statuses(gpu_device):
    params, comp, owner, T, P, z, w0 = _table()
    out = _table_points(gpu_device)
    # stable feeds, the single-phase points, one component: status 4, zeros and NaN; so is w0 = z on a feed that splits
    assert out[5].tolist() == [0] * N_SPLIT + [4] * 8
    for j in range(N_SPLIT, 19):
        _assert_failed(out, j, 4)
    # from the pinned starts: seven points with 1 to 3 used slots, splitting and not.  Point 2 is water + n-hexane at 350 K
    sub = np.array([0, 2, 4, 8, 9, 11, 18])
    pinned = _lle(gpu_device, params, comp, owner[sub], T[sub], P[sub], z[sub], w0=w0[sub])
    assert pinned[5].tolist() == out[5][sub].tolist() == [0, 0, 0, 0, 0, 4, 4]
    same = _lle(gpu_device, params, comp, owner[:N_SPLIT], T[:N_SPLIT], P[:N_SPLIT], z[:N_SPLIT], w0=z[:N_SPLIT])
    for j in range(N_SPLIT):
        _assert_failed(same, j, 4)
    # n = 1 and n = 0, with and without a start
    one = _lle(gpu_device, params, comp, [2], T[2:3], P[2:3], z[2:3])
    assert one[5].tolist() == [0] and _same_bytes(one, [v[2:3] for v in out])
    one = _lle(gpu_device, params, comp, [2], T[2:3], P[2:3], z[2:3], w0=w0[2:3])
    assert _same_bytes(one, [v[1:2] for v in pinned])
    for start in (None, np.zeros((0, NC))):
        none = _lle(gpu_device, params, comp, np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0), np.zeros((0, NC)), w0=start)
        assert [v.shape for v in none] == [(0,), (0, NC), (0, NC), (0,), (0,), (0,)]
    # invalid input: status 3 with the same pattern: the flash test's 13, and a w0 that is no positive number in a
    # present slot
    n_bad = 16
    bad_owner = np.full(n_bad, 2)
    bad_T, bad_P = np.full(n_bad, T[2]), np.full(n_bad, P[2])
    bad_z, bad_w = np.tile(z[2], (n_bad, 1)), np.tile(w0[2], (n_bad, 1))
    bad_owner[0], bad_owner[1] = len(owner), -1
    bad_T[2], bad_T[3], bad_T[4], bad_T[5] = np.nan, np.inf, -1.0, 0.0
    bad_P[6], bad_P[7], bad_P[8], bad_P[9] = np.nan, np.inf, 0.0, -1e5
    bad_z[10, 0] = -0.5
    bad_z[11, :2] = 0.0
    bad_z[12, 1] = np.nan
    bad_w[13, 0], bad_w[14, 1], bad_w[15, 0] = np.nan, 0.0, -0.25
    bad = _lle(gpu_device, params, comp, bad_owner, bad_T, bad_P, bad_z, w0=bad_w)
    for j in range(n_bad):
        _assert_failed(bad, j, 3)
    bad = _lle(gpu_device, params, comp, bad_owner[:13], bad_T[:13], bad_P[:13], bad_z[:13])  # through the stability test
    for j in range(13):
        _assert_failed(bad, j, 3)
    # the z and the w0 of a -1 slot are ignored, whatever they hold
    junk_z, junk_w, unused = z[sub].copy(), w0[sub].copy(), comp[sub] < 0
    assert unused.sum() == 2 * 4 + 1 * 2 + 3
    junk_z[unused] = np.tile([np.nan, -3.0, np.inf, 7.0], 4)[:int(unused.sum())]
    junk_w[unused] = np.tile([-1.0, np.inf, 0.0, np.nan], 4)[:int(unused.sum())]
    assert _same_bytes(_lle(gpu_device, params, comp, owner[sub], T[sub], P[sub], junk_z, w0=junk_w), pinned)
    assert _same_bytes(_lle(gpu_device, params, comp, owner[sub], T[sub], P[sub], junk_z), [v[sub] for v in out])


def test_reductions(gpu_device):
    """a used slot with z = 0 and a -1 slot give the binary's answer at 1e-12 with 0.0 / NaN in that column; the swapped
    mixture gives the same labelled split at 1e-9 (every point loses at least a factor 0.5 per step, so the loop's 1e-10
    bounds what two roundings of the same iteration can differ by well below that); what the lower triangle and the
    diagonal of k_ij hold changes no bit, and a k_12 of 0.02 changes the answer"""
    rows = np.array([V.WATER, V.BUTANE, V.HEXANE], dtype=np.float64)
    # water + n-hexane at 350 K and 1e6 Pa: the binary is point 2 of the table; both reductions in one launch
    b = [v[2:3, :2] if v.ndim == 2 else v[2:3] for v in _table_points(gpu_device)]
    both = _lle(gpu_device, rows, np.array([[0, 1, 2], [0, -1, 2]], dtype=np.int64), [0, 1], [350.0] * 2, [1e6] * 2,
                [[0.5, 0.0, 0.5], [0.5, 0.5, 0.5]])
    zero, gone = [v[:1] for v in both], [v[1:] for v in both]
    assert b[5][0] == 0 and zero[5][0] == 0 and gone[5][0] == 0 and 0.0 < b[0][0] < 1.0
    for other in (zero, gone):
        assert abs(other[0][0] - b[0][0]) <= 1e-12 and _rel(other[3][0], b[3][0]) <= 1e-12
        assert _rel(other[4][0], b[4][0]) <= 1e-12
        assert np.max(np.abs(other[1][0, [0, 2]] - b[1][0])) <= 1e-12 and np.max(np.abs(other[2][0, [0, 2]] - b[2][0])) <= 1e-12
    assert zero[1][0, 1] == 0.0 and zero[2][0, 1] == 0.0 and np.isnan(gone[1][0, 1]) and np.isnan(gone[2][0, 1])
    # component swap on every point of the shared launch
    params, comp, owner, T, P, z, _ = _table()
    beta, x, y, rx, ry, st = _table_points(gpu_device)
    swap = [1, 0, 2, 3]
    bs, xs, ys, rxs, rys, sts = _lle(gpu_device, params, comp[:, swap].copy(), owner, T, P, z[:, swap].copy())
    ok = st == 0
    used = (comp >= 0)[ok]
    assert np.array_equal(st, sts) and ok.sum() == N_SPLIT
    fig = {"beta": np.max(np.abs(bs[ok] - beta[ok])), "x": np.max(np.abs(np.where(used, xs[:, swap][ok] - x[ok], 0.0))),
           "y": np.max(np.abs(np.where(used, ys[:, swap][ok] - y[ok], 0.0))), "rho_x": np.max(np.abs(rxs[ok] / rx[ok] - 1)),
           "rho_y": np.max(np.abs(rys[ok] / ry[ok] - 1))}
    print("swap:", fig)
    assert max(fig.values()) <= 1e-9
    # k_ij: only the upper triangle is read.  A binary, a ternary and a vapour-liquid point (2, 4 and 8 of the table)
    sub = np.array([2, 4, 8])
    rng = np.random.default_rng(3)
    kij = np.zeros((len(owner), NC, NC))
    kij[:, 0, 1] = 0.02
    with_kij = _lle(gpu_device, params, comp, owner[sub], T[sub], P[sub], z[sub], kij=kij)
    assert np.all(with_kij[5] == 0) and abs(np.log(with_kij[2][0, 0] / y[2, 0])) > 1e-3  # water in n-hexane at 350 K
    assert not _same_bytes(with_kij, [v[sub] for v in (beta, x, y, rx, ry, st)])
    junk = kij + np.tril(rng.uniform(-9.0, 9.0, kij.shape))
    junk[:, 2, 0] = np.nan
    assert _same_bytes(_lle(gpu_device, params, comp, owner[sub], T[sub], P[sub], z[sub], kij=junk), with_kij)


def test_lanes_and_repeatability(gpu_device):
    """257 points (one past the 256-thread block) with owners shuffled over eight mixtures of the table with 1 to 4 used
    slots, splitting and not: every lane returns the bytes of its point from the shared launch, and two calls give the
    same bytes"""
    params, comp, owner, T, P, z, _ = _table()
    pool = np.array([0, 4, 8, 9, 10, 11, 14, 18])  # liquid-liquid, vapour-liquid, stable, single phase, one component
    assert sorted((comp[pool] >= 0).sum(axis=1).tolist()) == [1, 2, 2, 2, 2, 3, 3, 4]
    idx = pool[np.random.default_rng(5).integers(0, len(pool), 257)]
    first = _table_points(gpu_device)
    a = _lle(gpu_device, params, comp, owner[idx], T[idx], P[idx], z[idx])
    b = _lle(gpu_device, params, comp, owner[idx], T[idx], P[idx], z[idx])
    assert _same_bytes(a, b) and _same_bytes(a, [v[idx] for v in first])
    assert set(a[5].tolist()) == {0, 4} and set(idx.tolist()) == set(pool.tolist())


def test_explicit_start(gpu_device):
    """water + n-hexane at 300 K and 1e5 Pa from w0 = (0.9, 0.1) and from the swapped-role w0 = (0.1, 0.9): the loop's
    phases come out the other way round, the labelled result (x the denser phase, beta the share of the other) is the same
    at 1e-9, and it is the one the stability start leads to"""
    params, comp, owner, T, P, z, _ = _table()
    start = np.zeros((2, NC))
    start[:, :2] = [[0.9, 0.1], [0.1, 0.9]]
    out = _lle(gpu_device, params, comp, [0, 0], T[[0, 0]], P[[0, 0]], z[[0, 0]], w0=start)
    first = [v[0] for v in _table_points(gpu_device)]
    assert out[5].tolist() == [0, 0] and out[3][0] > out[4][0] and out[3][1] > out[4][1]
    for other in ([v[1] for v in out], first):
        fig = [abs(out[0][0] - other[0]), float(np.max(np.abs(out[1][0, :2] - other[1][:2]))),
               float(np.max(np.abs(out[2][0, :2] - other[2][:2]))), _rel(out[3][0], other[3]), _rel(out[4][0], other[4])]
        print("explicit start:", fig)
        assert max(fig) <= 1e-9


def test_reference_shaped_io(gpu_device):
    from gnnepcsaft_amd import pcsaft
    cases = _cases()
    beta, x, y, rx, ry, st = _table_points(gpu_device)
    (_, rows, T, P, z, _), (_, tern, T3, P3, z3, _), (_, _, Ts, Ps, zs, _) = cases[2], cases[4], cases[11]
    assert cases[11][0] == "water+hexane z_water 0.001"
    one = pcsaft.mix_lle(rows, [T, P, *z])
    assert list(one) == ["temperature", "pressure", "density liquid", "density vapor", "x0", "x1", "y0", "y1", "beta"]
    assert all(isinstance(v, list) and len(v) == 1 for v in one.values())
    assert one["temperature"] == [T] and one["pressure"] == [P] and one["beta"] == [beta[2]]
    assert one["density liquid"] == [rx[2]] and one["density vapor"] == [ry[2]]
    assert [one["x0"][0], one["x1"][0]] == x[2, :2].tolist() and [one["y0"][0], one["y1"][0]] == y[2, :2].tolist()
    three = pcsaft.mix_lle(tern, [T3, P3, *z3])
    assert list(three)[4:] == ["x0", "x1", "x2", "y0", "y1", "y2", "beta"]
    assert [three[f"x{i}"][0] for i in range(3)] == x[4, :3].tolist() and three["beta"] == [beta[4]]
    with pytest.raises(ValueError, match="No LLE found at the given conditions."):
        pcsaft.mix_lle(rows, [Ts, Ps, *zs])
    with pytest.raises(ValueError, match="No LLE found at the given conditions."):
        pcsaft.mix_lle([V.METHANE], [300.0, 1e6, 1.0])
    with pytest.raises(ValueError, match="No LLE found at the given conditions."):
        pcsaft.mix_lle(rows, [T, -1.0, *z])
    # the batch form: empty tables skipped, NaN rows where there is no split
    states = [np.array([[T, P, *z], [Ts, Ps, *zs]]), np.zeros((0, 5)), np.array([[T3, P3, *z3]]), np.array([[300.0, 1e6, 1.0]])]
    out = pcsaft.mix_lle_batch([rows, tern, tern, [V.METHANE]], states)
    assert [o.shape for o in out] == [(2, 5), (1, 7), (1, 3)]
    assert np.all(np.isnan(out[0][1])) and np.all(np.isnan(out[2]))
    for j, row in ((2, out[0][0]), (4, out[1][0])):
        k = len(cases[j][1])
        assert row[0] == beta[j] and np.array_equal(row[1:1 + k], x[j, :k]) and np.array_equal(row[1 + k:], y[j, :k])
    assert pcsaft.mix_lle_batch([rows], [np.zeros((0, 4))]) == []
    # a k_ij changes the answer: the matrices reach the kernel
    kij = [[0.0, 0.02], [0.02, 0.0]]
    with_kij = pcsaft.mix_lle(rows, [T, P, *z], kij_matrix=kij)
    assert abs(np.log(with_kij["y0"][0] / one["y0"][0])) > 1e-3
    assert pcsaft.mix_lle_batch([rows], [states[0][:1]], kij=[kij])[0][0, 3] == with_kij["y0"][0]


def test_diagram(gpu_device):
    """``mix_lle_diagram`` of water + n-hexane, z = (0.5, 0.5), at 1e6 Pa from 300 K, 6 points: all six temperatures are
    kept, ``temperature`` is linspace(300, 350, 6), and each point agrees with the oracle's pinned solve at its temperature
    (``L.DIAGRAM``) within the bound of the oracle comparison.  1e6 Pa and not 1e5: there the three-phase temperature of
    this pair lies inside 300 to 350 K, and above it the split is vapour-liquid."""
    from gnnepcsaft_amd import pcsaft
    rows = S.rows_of(L.DIAGRAM_ROWS)
    d = pcsaft.mix_lle_diagram(rows, [300.0, L.DIAGRAM_P, *L.DIAGRAM_Z], points=6)
    assert list(d) == ["temperature", "pressure", "density liquid", "density vapor", "x0", "x1", "y0", "y1", "beta"]
    assert all(len(v) == 6 for v in d.values())
    assert d["temperature"] == np.linspace(300.0, 350.0, 6).tolist() and d["pressure"] == [L.DIAGRAM_P] * 6
    for i, (T, _, sol, change) in enumerate(L.diagram()):
        bound = max(1e-7, 10.0 * change)
        xi, yi = np.array([d["x0"][i], d["x1"][i]]), np.array([d["y0"][i], d["y1"][i]])
        fig = {"ln x, ln y": _ln_gap(xi, yi, sol), "beta": abs(d["beta"][i] - sol["beta"]),
               "rho": max(_rel(d["density liquid"][i], sol["rho_x"]), _rel(d["density vapor"][i], sol["rho_y"]))}
        print(T, fig, "bound", bound)
        assert fig["ln x, ln y"] <= bound and fig["beta"] <= bound / float(np.max(np.abs(sol["y"] - sol["x"]))), (T, fig)
    assert d["beta"][5] == _table_points(gpu_device)[0][2]  # 350 K is point 2 of the table: the same bytes
    # points without a split are dropped: the butane + n-hexane tie-line feed splits at its 350 K and is one stable
    # phase (the oracle's verdict) at 400 K
    _, bh, Tb, Pb, zb, _ = _cases()[8]
    assert _cases()[8][0] == "butane+hexane" and Tb == 350.0
    two = pcsaft.mix_lle_diagram(bh, [Tb, Pb, *zb], points=2)
    assert two["temperature"] == [350.0] and two["beta"] == [_table_points(gpu_device)[0][8]]
