"""Mixture stability tests on the GPU (csrc/gnx_pcsaft_mix_stab.hip, gnnepcsaft_amd/pcsaft.py) against the oracle of
tests/pcsaft_mix_stab_ref.py: the pinned verdict of all 43 cases of its table, the tangent-plane equations at the state
every trial reports (the primary check: the oracle's pressure and finite-difference fugacities share no mechanism with
the kernel's duals), the oracle's own solve, the flash on what the certificate says, the reductions, invalid input, lanes
and repeatability, and the reference-shaped I/O.

The table is one launch of 43 points x 6 trial rows (1 to 4 used slots of 4) that every test shares, once through
``ops.pcsaft_mix_stability`` row by row and once through ``pcsaft.mixture_stability``."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_stab_ref as S
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

pytestmark = pytest.mark.gpu

NC = 4
NT = NC + 2
SOLVE_TOL = 1e-8  # kStabTol: the residual a stationary trial ends on


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _inputs(dev, params, comp, owner, T, P, z, kij, eab, trial=None):
    cols = [np.asarray(params, dtype=np.float64).reshape(-1, 9), comp, np.asarray(owner, dtype=np.int64),
            np.asarray(T, dtype=np.float64), np.asarray(P, dtype=np.float64), np.asarray(z, dtype=np.float64), kij, eab,
            None if trial is None else np.asarray(trial, dtype=np.int64)]
    return _dev(dev, *cols)


def _points(dev, params, comp, owner, T, P, z, kij=None, eab=None):
    """(stable, tpd, w, status) of ``pcsaft.mixture_stability`` as host arrays"""
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, pp, zz, k, e, _ = _inputs(dev, params, comp, owner, T, P, z, kij, eab)
    return [v.cpu().numpy() for v in pcsaft.mixture_stability(p, c, zz, t, pp, o, k, e)]


def _rows(dev, params, comp, owner, trial, T, P, z, kij=None, eab=None):
    """(tpd, w, rho_w, rho_z, status) of ``ops.pcsaft_mix_stability`` as host arrays"""
    from gnnepcsaft_amd import ops
    p, c, o, t, pp, zz, k, e, tr = _inputs(dev, params, comp, owner, T, P, z, kij, eab, trial)
    return [v.cpu().numpy() for v in ops.pcsaft_mix_stability(p, c, k, e, o, tr, t, pp, zz)]


def _all_trials(owner, T, P, z):
    """every point as its NT rows, point by point: (owner, trial, T, P, z)"""
    rep = lambda a: np.repeat(np.asarray(a), NT, axis=0)
    return rep(owner), np.tile(np.arange(NT, dtype=np.int64), len(owner)), rep(T), rep(P), rep(z)


def _pooled(cases):
    """cases (group, name, rows, T, P, z, stable) of 1 to 4 components as one pool: params [B, 9], comp [M, 4] (-1 =
    unused), owner [M], T [M], P [M], z [M, 4]"""
    params, comp, z = [], np.full((len(cases), NC), -1, dtype=np.int64), np.zeros((len(cases), NC))
    for i, (_, _, rows, _, _, zi, _) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        z[i, :len(rows)] = zi
    return (np.array(params), comp, np.arange(len(cases), dtype=np.int64), np.array([c[3] for c in cases], dtype=np.float64),
            np.array([c[4] for c in cases], dtype=np.float64), z)


@functools.lru_cache(maxsize=None)
def _table():
    return _pooled(S.cases())


@functools.lru_cache(maxsize=None)
def _table_points(dev):
    """``mixture_stability`` on the 43 cases, one launch: computed once, shared, never modified"""
    return _points(dev, *_table())


@functools.lru_cache(maxsize=None)
def _table_rows(dev):
    """``ops.pcsaft_mix_stability`` on the 43 x 6 trial rows, one launch: computed once, shared, never modified"""
    params, comp, owner, T, P, z = _table()
    return _rows(dev, params, comp, *_all_trials(owner, T, P, z))


def _reduce(tpd, w, st):
    """the documented reduction of ``mixture_stability`` written out in numpy on [n, NT] trials"""
    n = tpd.shape[0]
    stable, out_t, out_w, out_s = np.zeros(n, dtype=bool), np.full(n, np.nan), np.full(w[:, 0].shape, np.nan), np.zeros(n, np.int32)
    for i in range(n):
        ok = st[i] == 0
        negative = [t for t in range(NT) if ok[t] and tpd[i, t] < 0.0]
        stationary = [t for t in range(NT) if ok[t] and tpd[i, t] > 0.0]
        if negative:
            pick = min(negative, key=lambda t: tpd[i, t])
        elif not ok.all():
            out_s[i] = st[i].max()
            continue
        else:
            stable[i] = True
            pick = min(stationary, key=lambda t: tpd[i, t]) if stationary else 0
        out_t[i], out_w[i] = tpd[i, pick], w[i, pick]
    return stable, out_t, out_w, out_s


def _rel(a, b):
    return abs(a / b - 1.0)


def _same_bytes(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_every_pinned_verdict_and_the_equations_at_the_reported_state(gpu_device):
    """All 43 cases: status 0 and the pinned verdict.  Every trial row: status 0; -1 slots NaN; and, unless it fell onto the
    feed (tpd = 0.0 exactly, w = z, rho_w = rho_z), sum w = 1 at 1e-12, the oracle's ``distance`` at the reported (w,
    rho_w, rho_z) gives the kernel's tpd within 1e-10 + 10 x the oracle's two-step disagreement there, the oracle's pressures
    of (w, rho_w) and (z, rho_z) are P at 1e-9 on the scale max(P, 1e-3 rho R T), and a stationary row (tpd > 0) is
    stationary for the oracle within 2 x the kernel's tolerance + 10 x that disagreement: |d_i - D| = |r_i - sum w r| <= 2
    max |r|.  The bounds are the bubble and flash tests' for the same quantities.
    On an MI355X: 189 rows trivial, 47 negative, 22 stationary.  Worst of the 69 that are not trivial: sum w - 1 2.2e-16,
    pressure of w 1.3e-11, of z 2.5e-11; tpd 4.7e-7 on water + n-hexane at z_water = 1e-3 (0.19 of the bound there: the
    oracle's two steps disagree by 2.5e-7 on water at trace level, by 1.7e-5 on the 0.999 feed) and 1.5e-9 on the 65 rows
    where they agree within 1e-8 (0.13 of the bound); stationarity at most 0.47 of the bound."""
    cases = S.cases()
    stable, tpd_p, w_p, st_p = _table_points(gpu_device)
    tpd, w, rw, rz, st = _table_rows(gpu_device)
    assert len(cases) == 43 and tpd.shape == (43 * NT,) and w.shape == (43 * NT, NC)
    worst = {"sum w": 0.0, "tpd": 0.0, "tpd / bound": 0.0, "p w": 0.0, "p z": 0.0, "stationarity": 0.0,
             "stationarity / bound": 0.0, "two-step": 0.0}
    kinds = {"trivial": 0, "negative": 0, "stationary": 0}
    for j, (group, name, rows, T, P, z, expected) in enumerate(cases):
        k = len(rows)
        assert st_p[j] == 0 and bool(stable[j]) is expected, (name, st_p[j], stable[j], tpd_p[j])
        assert (tpd_p[j] < 0.0) == (not expected) and np.all(np.isnan(w_p[j, k:])) and abs(w_p[j, :k].sum() - 1.0) <= 1e-12
        for t in range(NT):
            i = j * NT + t
            assert st[i] == 0 and np.all(np.isnan(w[i, k:])) and rz[i] > 0.0 and rw[i] > 0.0, (name, t, st[i])
            if tpd[i] == 0.0:
                kinds["trivial"] += 1
                assert np.array_equal(w[i, :k], z / z.sum()) and rw[i] == rz[i], (name, t)
                continue
            assert t < k + 2, (name, t)  # the trial rich in a -1 slot is trivial
            kinds["negative" if tpd[i] < 0.0 else "stationary"] += 1
            d = S.distance(rows, z, w[i, :k], T, rz[i], rw[i])
            fig = {"sum w": abs(w[i, :k].sum() - 1.0), "tpd": abs(d["D"] - tpd[i]),
                   "tpd / bound": abs(d["D"] - tpd[i]) / (1e-10 + 10.0 * d["own"]),
                   "p w": abs(d["p_w"] - P) / max(P, rw[i] * R.RGAS * T * 1e-3),
                   "p z": abs(d["p_z"] - P) / max(P, rz[i] * R.RGAS * T * 1e-3), "two-step": d["own"]}
            if tpd[i] > 0.0:
                fig["stationarity"] = d["stationarity"]
                fig["stationarity / bound"] = d["stationarity"] / (2.0 * SOLVE_TOL + 10.0 * d["own"])
            print(name, "trial", t, "tpd", tpd[i], fig)
            for key, v in fig.items():
                worst[key] = max(worst[key], v)
            assert tpd[i] < S.NEGATIVE or tpd[i] > 0.0, (name, t, tpd[i])
            assert fig["sum w"] <= 1e-12 and np.all(w[i, :k] > 0.0), (name, t, fig)
            assert fig["tpd / bound"] <= 1.0, (name, t, fig)
            assert fig["p w"] <= 1e-9 and fig["p z"] <= 1e-9, (name, t, fig)
            assert fig.get("stationarity / bound", 0.0) <= 1.0, (name, t, fig)
    print("rows:", kinds, "worst:", worst)
    assert min(kinds.values()) > 0


def test_against_the_oracles_own_solve(gpu_device):
    """Every row the kernel ends as stationary: the oracle's own trial ends as stationary too, and tpd and w agree within
    max(1e-7, 10 x the change of the oracle's answer between its residuals 1e-7 and 1e-9).  Every row agrees with the oracle
    on how it ends.  The oracle's solves are shared with tests/test_pcsaft_mix_stab_cpu.py and cost about a minute of
    host time where that test has not run in the same process: 181 steps on ethanol + water.
    On an MI355X, 22 stationary rows: tpd within 1.4e-10, w within 5.0e-11, at most 0.0014 of the bound; the oracle's own
    change is 2.1e-10 to 2.6e-7."""
    tpd, w, rw, rz, st = _table_rows(gpu_device)
    worst = {"tpd": 0.0, "w": 0.0, "of bound": 0.0, "change": 0.0}
    count = 0
    for j, ((group, name, rows, T, P, z, _), per) in enumerate(zip(S.cases(), S.table_solves())):
        k = len(rows)
        for t in range(k + 2):
            i = j * NT + t
            sol, change = per[t]
            kind = "trivial" if tpd[i] == 0.0 else "negative" if tpd[i] < 0.0 else "stationary"
            assert kind == sol["kind"], (name, t, kind, sol["kind"], tpd[i], sol["tpd"])
            if kind != "stationary":
                continue
            count += 1
            bound = max(1e-7, 10.0 * change)
            fig = {"tpd": abs(tpd[i] - sol["tpd"]), "w": float(np.max(np.abs(w[i, :k] - sol["w"]))), "change": change}
            fig["of bound"] = max(fig["tpd"], fig["w"]) / bound
            print(name, "trial", t, "steps", sol["steps"], fig, "rho_w", _rel(rw[i], sol["rho_w"]))
            for key, v in fig.items():
                worst[key] = max(worst[key], v)
            assert fig["of bound"] <= 1.0, (name, t, fig, bound)
    print("stationary rows:", count, "worst:", worst)
    assert count >= 20


def test_the_certificate_is_usable(gpu_device):
    """the flash of every unstable tie-line feed finds the split (status 0); the flash of water + n-hexane at z_water = 0.5,
    unstable too, does not: that split is liquid-liquid, and the stability test is what says so"""
    from gnnepcsaft_amd import pcsaft
    params, comp, owner, T, P, z = _table()
    stable, tpd, _, st = _table_points(gpu_device)
    pick = np.array(list(range(12)) + [38])
    assert S.cases()[38][1] == "water+hexane z_water 0.5" and not stable[pick].any() and np.all(tpd[pick] < 0.0)
    p, c, o, t, pp, zz = _dev(gpu_device, params, comp, owner[pick], T[pick], P[pick], z[pick])
    status = pcsaft.mixture_tp_flash(p, c, zz, t, pp, o)[5].cpu().numpy()
    print("flash status:", status)
    assert np.all(status[:12] == 0) and status[12] != 0


def test_reductions(gpu_device):
    """one component present, and the same row twice: stable, every trial trivial; a used slot with z = 0 and a -1 slot give
    the binary's answer at 1e-12 with 0.0 / NaN in that column of w; the swapped mixture gives the same verdicts and tpd
    at 1e-9; what the lower triangle and the diagonal of k_ij hold changes no bit"""
    rows = np.array([V.HEXANE, V.BUTANE, V.ETHANOL, V.METHANE], dtype=np.float64)
    comp = np.array([[0, 1, -1], [0, -1, -1], [0, 0, -1]], dtype=np.int64)
    z = np.array([[1.0, 0.0, 5.0], [2.0, 7.0, 7.0], [0.3, 0.7, 0.0]])
    nt = 5
    tpd, w, rw, rz, st = _rows(gpu_device, rows, comp, np.repeat([0, 1, 2], nt), np.tile(np.arange(nt), 3),
                               np.full(3 * nt, 350.0), np.full(3 * nt, 4e5), np.repeat(z, nt, axis=0))
    assert np.all(st == 0) and np.all(tpd == 0.0) and np.all(rw == rz) and np.all(rz > 0.0)
    feed = np.where(comp >= 0, z / np.where(comp >= 0, z, 0.0).sum(axis=1, keepdims=True), np.nan)
    assert np.array_equal(feed[:2], [[1.0, 0.0, np.nan], [1.0, np.nan, np.nan]], equal_nan=True)
    assert np.array_equal(w, np.repeat(feed, nt, axis=0), equal_nan=True)
    stable = _points(gpu_device, rows, comp, [0, 1, 2], [350.0] * 3, [4e5] * 3, z)
    assert stable[0].tolist() == [True] * 3 and stable[1].tolist() == [0.0] * 3 and stable[3].tolist() == [0] * 3
    # methane + hexane at 320 K and 3 MPa, z = (0.3, 0.7): between the dew and the bubble pressure
    t320, p3 = [320.0], [3e6]
    b = _points(gpu_device, rows, np.array([[3, 0]], dtype=np.int64), [0], t320, p3, [[0.3, 0.7]])
    zero = _points(gpu_device, rows, np.array([[3, 1, 0]], dtype=np.int64), [0], t320, p3, [[0.3, 0.0, 0.7]])
    gone = _points(gpu_device, rows, np.array([[3, -1, 0]], dtype=np.int64), [0], t320, p3, [[0.3, 0.5, 0.7]])
    assert not b[0][0] and b[3][0] == 0 and b[1][0] < -1e-3
    for other in (zero, gone):
        assert not other[0][0] and other[3][0] == 0 and abs(other[1][0] - b[1][0]) <= 1e-12
        assert np.max(np.abs(other[2][0, [0, 2]] - b[2][0])) <= 1e-12
    assert zero[2][0, 1] == 0.0 and np.isnan(gone[2][0, 1])
    # component swap on every point of the shared launch
    params, comp, owner, T, P, z = _table()
    first = _table_points(gpu_device)
    swap = [1, 0, 2, 3]
    ss, ts, ws, sts = _points(gpu_device, params, comp[:, swap].copy(), owner, T, P, z[:, swap].copy())
    fig = {"tpd": float(np.max(np.abs(ts - first[1]))), "w": float(np.nanmax(np.abs(ws[:, swap] - first[2])))}
    print("swap:", fig)
    assert np.array_equal(ss, first[0]) and np.all(sts == 0) and fig["tpd"] <= 1e-9
    # k_ij: only the upper triangle is read.  The tie-line, single-phase and liquid-liquid points
    sub = np.array(list(range(16)) + list(range(38, 43)))
    rng = np.random.default_rng(3)
    kij = np.zeros((len(owner), NC, NC))
    kij[:, 0, 1] = rng.uniform(-0.02, 0.02, len(owner))
    with_kij = _points(gpu_device, params, comp, owner[sub], T[sub], P[sub], z[sub], kij=kij)
    assert not _same_bytes(with_kij, [v[sub] for v in first])
    junk = kij + np.tril(rng.uniform(-9.0, 9.0, kij.shape))
    junk[:, 2, 0] = np.nan
    assert _same_bytes(_points(gpu_device, params, comp, owner[sub], T[sub], P[sub], z[sub], kij=junk), with_kij)


def test_reduced_form_is_the_reduction_of_the_rows(gpu_device):
    """``mixture_stability`` equals the documented reduction of the rows of ``ops.pcsaft_mix_stability``, bit for bit"""
    tpd, w, _, _, st = _table_rows(gpu_device)
    reduced = _reduce(tpd.reshape(43, NT), w.reshape(43, NT, NC), st.reshape(43, NT))
    first = _table_points(gpu_device)
    assert [v.dtype for v in first] == [np.bool_, np.float64, np.float64, np.int32]
    assert [v.shape for v in first] == [(43,), (43,), (43, NC), (43,)]
    assert _same_bytes(first, reduced)


def _assert_failed(out, j, status):
    tpd, w, rw, rz, st = out
    assert st[j] == status, (j, st[j], status)
    assert np.isnan(tpd[j]) and rw[j] == 0.0 and rz[j] == 0.0 and np.all(np.isnan(w[j]))


def test_invalid_input(gpu_device):
    params, comp, owner, T, P, z = _table()
    rows = _table_rows(gpu_device)
    # n = 1 and n = 0, rows and points.  Point 2 is butane + hexane at 350 K
    one = _rows(gpu_device, params, comp, [2], [0], T[2:3], P[2:3], z[2:3])
    assert one[4].tolist() == [0] and _same_bytes(one, [v[2 * NT:2 * NT + 1] for v in rows])
    none = _rows(gpu_device, params, comp, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0),
                 np.zeros((0, NC)))
    assert [v.shape for v in none] == [(0,), (0, NC), (0,), (0,), (0,)]
    one = _points(gpu_device, params, comp, [2], T[2:3], P[2:3], z[2:3])
    assert _same_bytes(one, [v[2:3] for v in _table_points(gpu_device)])
    none = _points(gpu_device, params, comp, np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0), np.zeros((0, NC)))
    assert [v.shape for v in none] == [(0,), (0,), (0, NC), (0,)]
    # invalid input: status 3, tpd NaN, densities 0.0, the w row NaN
    n_bad = 17
    bad_owner, bad_trial = np.full(n_bad, 2), np.zeros(n_bad, dtype=np.int64)
    bad_T, bad_P, bad_z = np.full(n_bad, T[2]), np.full(n_bad, P[2]), np.tile(z[2], (n_bad, 1))
    bad_owner[0], bad_owner[1] = len(owner), -1
    bad_T[2], bad_T[3], bad_T[4], bad_T[5] = np.nan, np.inf, -1.0, 0.0
    bad_P[6], bad_P[7], bad_P[8], bad_P[9] = np.nan, np.inf, 0.0, -1e5
    bad_z[10, 0] = -0.5
    bad_z[11, :2] = 0.0
    bad_z[12, 1] = np.nan
    bad_trial[13], bad_trial[14], bad_trial[15], bad_trial[16] = -1, NT, 2 ** 40, -2 ** 40
    bad = _rows(gpu_device, params, comp, bad_owner, bad_trial, bad_T, bad_P, bad_z)
    for j in range(n_bad):
        _assert_failed(bad, j, 3)
    # a point with bad input is inconclusive with status 3
    stable, tpd, w, st = _points(gpu_device, params, comp, bad_owner[:13], bad_T[:13], bad_P[:13], bad_z[:13])
    assert not stable.any() and np.all(st == 3) and np.all(np.isnan(tpd)) and np.all(np.isnan(w))
    # the z of a -1 slot is ignored, whatever it holds
    sub = np.arange(12)
    junk = z[sub].copy()
    junk[comp[sub] < 0] = np.tile([np.nan, -3.0, np.inf, 7.0], 12)[:int((comp[sub] < 0).sum())]
    assert _same_bytes(_points(gpu_device, params, comp, owner[sub], T[sub], P[sub], junk),
                       [v[sub] for v in _table_points(gpu_device)])


def test_lanes_and_repeatability(gpu_device):
    """257 points (x 6 rows: past the block edge) shuffled over mixtures of 2 to 4 used slots, stable and unstable: every
    point has the bytes of its point in the table launch, and two calls give the same bytes"""
    params, comp, owner, T, P, z = _table()
    assert sorted(set((comp >= 0).sum(axis=1).tolist())) == [2, 3, 4]
    idx = np.random.default_rng(5).integers(0, len(owner), 257)
    first = _table_points(gpu_device)
    a = _points(gpu_device, params, comp, owner[idx], T[idx], P[idx], z[idx])
    b = _points(gpu_device, params, comp, owner[idx], T[idx], P[idx], z[idx])
    assert _same_bytes(a, b) and _same_bytes(a, [v[idx] for v in first])
    assert set(a[0].tolist()) == {True, False}


def test_reference_shaped_io(gpu_device):
    from gnnepcsaft_amd import pcsaft
    cases = S.cases()
    (_, _, rows, T, P, z, _), (_, _, tern, T3, P3, z3, _), (_, name, _, Tb, Pb, zb, _) = cases[2], cases[4], cases[21]
    assert name == "butane+hexane x 1.02" and Tb == T
    states = [np.array([[T, P, *z], [Tb, Pb, *zb]]), np.zeros((0, 5)), np.array([[T3, P3, *z3]]), np.array([[300.0, 1e6, 1.0]])]
    out = pcsaft.mix_stability_batch([rows, tern, tern, [V.METHANE]], states)
    assert [o.shape for o in out] == [(2, 3), (1, 4), (1, 2)]
    stable, tpd, w, st = _table_points(gpu_device)
    for j, row in ((2, out[0][0]), (21, out[0][1]), (4, out[1][0])):
        k = len(cases[j][2])
        assert row[0] == tpd[j] and np.array_equal(row[1:], w[j, :k]), (j, row, tpd[j], w[j])
    assert out[0][0, 0] < 0.0 < out[0][1, 0] and out[1][0, 0] < 0.0 and np.array_equal(out[2], [[0.0, 1.0]])
    assert pcsaft.mix_is_stable(rows, [T, P, *z]) is False and pcsaft.mix_is_stable(rows, [Tb, Pb, *zb]) is True
    assert pcsaft.mix_is_stable(tern, [T3, P3, *z3]) is False and pcsaft.mix_is_stable([V.METHANE], [300.0, 1e6, 1.0]) is True
    with pytest.raises(RuntimeError, match="invalid parameters or state"):
        pcsaft.mix_is_stable(rows, [T, -1.0, *z])
    assert np.all(np.isnan(pcsaft.mix_stability_batch([rows], [np.array([[T, -1.0, *z]])])[0]))
    assert pcsaft.mix_stability_batch([rows], [np.zeros((0, 4))]) == []
    # a k_ij that flips the verdict (the oracle: butane + hexane at 1.02 x its bubble pressure is unstable with k_12 =
    # 0.02, whose bubble pressure is higher): the matrices reach the kernel
    kij = [[0.0, 0.02], [0.02, 0.0]]
    assert S.stability(rows, zb, Tb, Pb, kij=kij)[0] is False
    assert pcsaft.mix_is_stable(rows, [Tb, Pb, *zb], kij_matrix=kij) is False
    batch_kij = pcsaft.mix_stability_batch([rows], [states[0][1:]], kij=[kij])
    assert batch_kij[0][0, 0] < 0.0
