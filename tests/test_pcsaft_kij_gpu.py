"""The k_ij fit of binaries on the GPU (csrc/gnx_pcsaft_kij.hip; gnnepcsaft_amd/pcsaft.py ``mix_kij_x1``, ``fit_kij``,
``optimize_kij``): the row kernel against the route it replaces (``mix_flash_x1`` / ``mix_tp_flash_batch``, bit for bit),
the chunks of 64 feeds, the sums kernel against numpy, and the fit on planted, oracle and noisy data.

One system throughout, butane + hexane: the states A inside the P-x-y diagram, the dead state D far above it, the feeds
linspace(1e-5, 0.99, 8).  On the CPU oracle (tests/pcsaft_mix_flash_ref.flash) every state of A splits at some feed for
k_12 in {0.2, 0.1, 0.05, 0, -0.03, -0.05}, D at none for k_12 in {0.2, 0.05, 0, -0.03}, and the feed 1e-5 never splits at
A."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_flash_ref as F
from tests import pcsaft_mix_vle_ref as V

pytestmark = pytest.mark.gpu

ROWS = [V.BUTANE, V.HEXANE]
A = [(350.0, 3e5), (350.0, 4e5), (350.0, 5e5), (330.0, 2.5e5)]
D = (350.0, 5e6)
FEEDS = np.linspace(1e-5, 0.99, 8)
CO2 = [2.0729, 2.7852, 169.21, 0, 0, 0, 0, 0, 44.01]
NOISE = np.array([1.03, 0.98, 1.02, 0.97])
EPS = 2.0 ** -52


def _kmat(k):
    return [[0.0, k], [k, 0.0]]


def _same(a, b):
    """the same bits wherever either is a number, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


@functools.lru_cache(maxsize=None)
def _planted(k, n_states=4):
    """x_1 of the first ``n_states`` states of A at k_12 = k from ``mix_flash_x1``: computed once, never modified"""
    from gnnepcsaft_amd import pcsaft
    x1 = pcsaft.mix_flash_x1(ROWS, A[:n_states], FEEDS, kij_matrix=_kmat(k))
    assert np.all(np.isfinite(x1)), (k, x1)
    x1.setflags(write=False)
    return x1


def _system(x1, states):
    return (ROWS, [s[0] for s in states], [s[1] for s in states], np.asarray(x1))


@functools.lru_cache(maxsize=None)
def _four_systems():
    """A with k* = 0.05, its first three states with k* = -0.03, the first alone with k* = 0, D alone"""
    return (_system(_planted(0.05), A), _system(_planted(-0.03, 3), A[:3]), _system(_planted(0.0, 1), A[:1]),
            _system([0.3], [D]))


@functools.lru_cache(maxsize=None)
def _fit_together():
    from gnnepcsaft_amd import pcsaft
    fit = pcsaft.fit_kij(list(_four_systems()), feed_x1s=FEEDS)
    for v in fit.values():
        v.setflags(write=False)
    return fit


def _host_scores(k, x1_exp):
    """(cost, loss, loss_nonan, mape) of system A at k from ``mix_flash_x1``, as the reference computes them"""
    from gnnepcsaft_amd import pcsaft
    pred = pcsaft.mix_flash_x1(ROWS, A, FEEDS, kij_matrix=_kmat(k))
    assert np.all(np.isfinite(pred))
    r = np.log((pred + 1e-6) / (x1_exp + 1e-6))
    return 0.5 * np.sum(r * r), np.mean(r * r), np.mean(np.abs(r)), np.mean(np.abs((pred - x1_exp) / x1_exp))


@pytest.mark.parametrize("n_feeds", [1, 8, 50, 64])
def test_row_kernel_against_flash_x1(gpu_device, n_feeds):
    """States A + D under k_12 = 0 and 0.05 as two candidates of one launch, n = 1 and n = 5 states: x1 is ``mix_flash_x1``
    under that k_12 bit for bit, feed the first index whose ``mix_tp_flash_batch`` row is not NaN (or -1), D has NaN, -1, the
    penalty 10.0 and a status != 0, and the residual is numpy's log((x1 + 1e-6) / (x1_exp + 1e-6)) within 4 x 2^-52 x max(1,
    |r|): one rounding each for the sum, the quotient and the log (whose two implementations may differ by one more)."""
    from gnnepcsaft_amd import pcsaft
    feeds = np.array([0.5]) if n_feeds == 1 else np.linspace(1e-5, 0.99, n_feeds)
    states = np.array(A + [D])
    ks = [0.0, 0.05]
    xe = np.concatenate([_planted(0.05), [0.3]])
    x1, feed, res, st = pcsaft.mix_kij_x1(ROWS, states, xe, feeds, ks)
    assert x1.shape == feed.shape == res.shape == st.shape == (2, 5)
    assert x1.dtype == res.dtype == np.float64 and feed.dtype == st.dtype == np.int32
    one = pcsaft.mix_kij_x1(ROWS, states[:1], xe[:1], feeds, ks)
    assert all(v.shape == (2, 1) for v in one)
    assert _same(one[0], x1[:, :1]) and np.array_equal(one[1], feed[:, :1]) and _same(one[2], res[:, :1])
    assert np.array_equal(one[3], st[:, :1])
    z1 = np.tile(feeds, 5)
    points = np.concatenate([np.repeat(states, n_feeds, axis=0), z1[:, None], 1.0 - z1[:, None]], axis=1)
    for c, k in enumerate(ks):
        assert _same(x1[c], pcsaft.mix_flash_x1(ROWS, states, feeds, kij_matrix=_kmat(k))), (k, x1[c])
        split = ~np.isnan(pcsaft.mix_tp_flash_batch([ROWS], [points], kij=[_kmat(k)])[0][:, 0]).reshape(5, n_feeds)
        first = np.where(split.any(axis=1), np.argmax(split, axis=1), -1)
        assert np.array_equal(feed[c], first), (k, feed[c], first)
        hit = first >= 0
        assert np.array_equal(st[c] == 0, hit) and np.array_equal(np.isnan(x1[c]), ~hit)
        assert np.all(res[c][~hit] == 10.0)
        want = np.log((x1[c][hit] + 1e-6) / (xe[hit] + 1e-6))
        err = np.abs(res[c][hit] - want)
        print("F", n_feeds, "k", k, "feed", feed[c], "status", st[c], "residual", res[c], "error", err)
        assert np.all(err <= 4.0 * EPS * np.maximum(1.0, np.abs(want)))
        assert np.isnan(x1[c, 4]) and feed[c, 4] == -1 and res[c, 4] == 10.0 and st[c, 4] != 0  # D
    if n_feeds >= 8:
        assert np.all(st[:, :4] == 0) and np.all(feed[:, :4] >= 1)  # every state of A splits, and never at the feed 1e-5
    if n_feeds == 8:
        assert np.all(res[1, :4] == 0.0)  # x1_exp is this launch's own x1 at k = 0.05


def test_split_with_a_residual_that_is_not_finite(gpu_device):
    """a state that splits, measured against an x1_exp that is NaN, infinite or below -1e-6: x1 and feed are the split's,
    the residual is the reference's penalty (it turns the NaN into 10.0 too) and the status 3; the row beside them with a
    good x1_exp is untouched.  The sums count such a row as penalised."""
    from gnnepcsaft_amd import ops, pcsaft
    xe = np.array([np.nan, np.inf, -1.0, float(_planted(0.05)[0])])
    x1, feed, res, st = pcsaft.mix_kij_x1(ROWS, [A[0]] * 4, xe, FEEDS, [0.05])
    assert st[0].tolist() == [3, 3, 3, 0] and res[0].tolist() == [10.0, 10.0, 10.0, 0.0]
    assert feed[0].tolist() == [feed[0, 3]] * 4 and feed[0, 3] >= 1
    assert x1[0].tobytes() == np.repeat(_planted(0.05)[:1], 4).tobytes()
    dev = gpu_device
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    both = [np.concatenate([v, v]) for v in (res[0], x1[0], xe, st[0])]  # the same rows as candidate 0 and 1
    sums = ops.pcsaft_kij_sums(up(both[0], np.float64), up(both[1], np.float64), up(both[2], np.float64),
                               up(both[3], np.int32), up([0, 4], np.int64), 1e-5).cpu().numpy()
    assert sums[0].tolist() == [300.0, 3.0, 0.0, 0.0, 300.0, 0.0, 0.0, 1.0]


def test_chunk_edges(gpu_device):
    """the first hit in the second chunk, in the third, and in the first with a later one behind it; 65 feeds without one"""
    from gnnepcsaft_amd import pcsaft
    state, xe, ks = [A[0]], [0.3], [0.05]
    lone = pcsaft.mix_kij_x1(ROWS, state, xe, [0.5], ks)
    assert lone[3][0, 0] == 0 and lone[1][0, 0] == 0 and np.isfinite(lone[0][0, 0])
    for feeds, index in (([1e-5] * 64 + [0.5], 64), ([1e-5] * 129 + [0.5], 129), ([0.5] + [1e-5] * 64 + [0.4], 0)):
        x1, feed, res, st = pcsaft.mix_kij_x1(ROWS, state, xe, feeds, ks)
        assert feed[0, 0] == index and st[0, 0] == 0, (len(feeds), feed, st)
        assert _same(x1, lone[0]) and _same(res, lone[2])
    x1, feed, res, st = pcsaft.mix_kij_x1(ROWS, state, xe, [1e-5] * 65, ks)
    assert np.isnan(x1[0, 0]) and feed[0, 0] == -1 and res[0, 0] == 10.0 and st[0, 0] != 0


def _numpy_sums(r, x1, xe, st, seg, h):
    """(the eight slots, the sum of |terms| of each) per system from the rows [system][candidate][point], in numpy fp64"""
    out, mag = [], []
    for lo, hi in zip(seg[:-1], seg[1:]):
        n = hi - lo
        a, b = slice(2 * lo, 2 * lo + n), slice(2 * lo + n, 2 * hi)
        p0, p1 = st[a] != 0, st[b] != 0
        good, both = ~p0, ~p0 & ~p1
        J = np.where(both, (r[b] - r[a]) / h, 0.0)
        terms = [r[a] * r[a], p0.astype(np.float64), np.abs(r[a][good]), np.abs((x1[a][good] - xe[a][good]) / xe[a][good]),
                 r[b] * r[b], J * r[a], J * J, both.astype(np.float64)]
        out.append([np.sum(t) for t in terms])
        mag.append([np.sum(np.abs(t)) for t in terms])
    return np.array(out), np.array(mag)


def _check_sums(sums, r, x1, xe, st, seg, h):
    want, mag = _numpy_sums(r, x1, xe, st, seg, h)
    n_s = np.diff(seg)[:, None]
    err = np.abs(sums - want)
    print("sums", sums, "error / bound", err / np.maximum((n_s + 6) * 2.0 ** -53 * mag, 1e-300))
    assert np.all(err <= (n_s + 6) * 2.0 ** -53 * mag)
    assert np.array_equal(sums[:, [1, 7]], want[:, [1, 7]])  # the counts are exact


def test_sums_kernel(gpu_device):
    """Systems of 4, 3, 1 and 70 points (more than one pass of the 64 lanes), D among them, candidates at k and k + 1e-5 in
    one row launch; each slot is numpy's within (n_s + 6) x 2^-53 x sum |terms| (n_s roundings of the additions and the
    term's own) and the counts are exact.  Then rows made up on the host, so that every combination of penalised
    candidates occurs, a row penalised at k + h alone included."""
    from gnnepcsaft_amd import ops
    h = 1e-5
    cycle = A + [D]
    xe_of = np.concatenate([_planted(0.05), [0.3]])
    picks = [[0, 1, 2, 3], [0, 1, 4], [0], [j % 5 for j in range(70)]]
    k_of = [0.0, 0.1, 0.05, 0.02]
    seg = np.concatenate([[0], np.cumsum([len(p) for p in picks])]).astype(np.int64)
    owner, T, P, xe = [], [], [], []
    for s, p in enumerate(picks):
        for c in range(2):
            owner += [2 * s + c] * len(p)
            T += [cycle[j][0] for j in p]
            P += [cycle[j][1] for j in p]
            xe += [xe_of[j] for j in p]
    kij = np.zeros((8, 2, 2))
    kij[:, 0, 1] = kij[:, 1, 0] = np.repeat(k_of, 2) + np.tile([0.0, h], 4)
    dev = gpu_device
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    x1, feed, res, st = ops.pcsaft_kij_x1(up(ROWS, np.float64), up(np.tile([0, 1], (8, 1)), np.int64), up(kij, np.float64),
                                          None, up(owner, np.int64), up(T, np.float64), up(P, np.float64),
                                          up(xe, np.float64), up(FEEDS, np.float64))
    d_xe, d_seg = up(xe, np.float64), up(seg, np.int64)
    sums = ops.pcsaft_kij_sums(res, x1, d_xe, st, d_seg, h)
    again = ops.pcsaft_kij_sums(res, x1, d_xe, st, d_seg, h)
    assert sums.shape == (4, 8) and sums.dtype == torch.float64 and torch.equal(sums, again)
    r, x, s = res.cpu().numpy(), x1.cpu().numpy(), st.cpu().numpy()
    assert s[2 * seg[1] + 2] != 0 and r[2 * seg[1] + 2] == 10.0 and (s != 0).sum() == 2 * (1 + 14)  # D, and only D
    _check_sums(sums.cpu().numpy(), r, x, np.array(xe), s, seg, h)
    assert sums[3, 1].item() == 14 and sums[3, 7].item() == 56 and sums[1, 1].item() == 1 and sums[2, 7].item() == 1
    # made-up rows: 130 and 5 points
    rng = np.random.default_rng(11)
    seg2 = np.array([0, 130, 135], dtype=np.int64)
    n = 2 * 135
    s2 = rng.choice([0, 0, 0, 1, 4], n).astype(np.int32)
    r2 = np.where(s2 != 0, 10.0, rng.normal(0.0, 0.3, n))
    xe2 = rng.uniform(0.05, 0.9, n)
    x2 = np.where(s2 != 0, np.nan, xe2 * np.exp(r2))
    sums2 = ops.pcsaft_kij_sums(up(r2, np.float64), up(x2, np.float64), up(xe2, np.float64), up(s2, np.int32), up(seg2, np.int64), h)
    a, b = s2[:130] != 0, s2[130:260] != 0
    assert (a & ~b).any() and (~a & b).any() and (a & b).any() and (~a & ~b).any()
    _check_sums(sums2.cpu().numpy(), r2, x2, xe2, s2, seg2, h)
    # a range outside the rows: NaN, nothing read
    bad = ops.pcsaft_kij_sums(up(r2, np.float64), up(x2, np.float64), up(xe2, np.float64), up(s2, np.int32),
                              up([0, 136], np.int64), h)
    assert torch.isnan(bad).all()


def test_planted_fit(gpu_device):
    """Data from ``mix_flash_x1`` at k*, fit from 0.2.  The data are the kernel's own bits, so the residual at k* is 0; the
    iteration ends on a step below 1e-8, and with a forward difference over 1e-5 the Gauss-Newton ratio is of order 1e-4:
    |k - k*| <= 1e-6.  D ends where it started, with its one row penalised."""
    fit = _fit_together()
    print({key: v.tolist() for key, v in fit.items()})
    for s, k_star in enumerate((0.05, -0.03, 0.0)):
        assert abs(fit["k_12"][s] - k_star) <= 1e-6, (s, fit["k_12"][s])
        assert fit["n_nan"][s] == 0 and fit["reason"][s] != "max_iter"
    assert fit["k_12"][3] == 0.2 and fit["n_nan"][3] == 1 and fit["loss"][3] == 100.0 and fit["reason"][3] == "flat"
    assert fit["loss_nonan"][3] == 1.0 and fit["mape"][3] == 1.0 and fit["iterations"][3] == 0


def test_fit_on_oracle_data(gpu_device):
    """x_1 of A at k* = 0.05 from the CPU oracle's flash (the first feed that splits, tol 1e-11): |k - k*| <= 1e-6 + 10 x
    max_j |x1_gpu_j(k*) - x1_oracle_j| / min_j |dx1_j/dk|, the derivative a central difference of ``mix_flash_x1`` over
    +-1e-4: what the data's own distance from the kernel's x_1 can move the minimum by, with a factor 10."""
    from gnnepcsaft_amd import pcsaft
    k_star = 0.05
    oracle = []
    for T, P in A:
        sol = None
        for f in FEEDS:
            sol = F.flash(ROWS, [f, 1.0 - f], T, P, kij=np.array(_kmat(k_star)), tol=1e-11)
            if isinstance(sol, dict):
                break
        assert isinstance(sol, dict), (T, P)
        oracle.append(sol["x"][0])
    oracle = np.array(oracle)
    slope = (pcsaft.mix_flash_x1(ROWS, A, FEEDS, kij_matrix=_kmat(k_star + 1e-4))
             - pcsaft.mix_flash_x1(ROWS, A, FEEDS, kij_matrix=_kmat(k_star - 1e-4))) / 2e-4
    apart = np.abs(_planted(k_star) - oracle)
    bound = 1e-6 + 10.0 * apart.max() / np.abs(slope).min()
    fit = pcsaft.fit_kij([_system(oracle, A)], feed_x1s=FEEDS)
    print("oracle x1", oracle, "gpu - oracle", apart, "dx1/dk", slope, "bound", bound, "k", fit["k_12"][0],
          "k - k*", fit["k_12"][0] - k_star, "iterations", fit["iterations"][0], fit["reason"][0])
    assert abs(fit["k_12"][0] - k_star) <= bound and fit["n_nan"][0] == 0 and fit["reason"][0] != "max_iter"


def test_noisy_fit_is_a_local_minimum(gpu_device):
    """the planted data of A times (1.03, 0.98, 1.02, 0.97): the cost recomputed on the host from ``mix_flash_x1`` at the
    returned k -+ 1e-4 is not below the one at k, and loss, loss_nonan and mape are the host's at k within 1e-12 relative"""
    from gnnepcsaft_amd import pcsaft
    data = _planted(0.05) * NOISE
    fit = pcsaft.fit_kij([_system(data, A)], feed_x1s=FEEDS)
    k = float(fit["k_12"][0])
    cost, loss, loss_nonan, mape = _host_scores(k, data)
    below, above = _host_scores(k - 1e-4, data)[0], _host_scores(k + 1e-4, data)[0]
    print("k", k, "cost", cost, "at k - 1e-4", below, "at k + 1e-4", above, "iterations", fit["iterations"][0],
          fit["reason"][0], "loss", fit["loss"][0], loss, "loss_nonan", fit["loss_nonan"][0], loss_nonan, "mape",
          fit["mape"][0], mape)
    assert below >= cost and above >= cost and cost > 0.0
    assert fit["n_nan"][0] == 0 and fit["reason"][0] != "max_iter"
    for got, want in ((fit["loss"][0], loss), (fit["loss_nonan"][0], loss_nonan), (fit["mape"][0], mape)):
        assert abs(got - want) <= 1e-12 * abs(want)


def test_lockstep_and_repeatability(gpu_device):
    """the four systems fitted together give the bits of each fitted alone, and the same bits on a second call"""
    from gnnepcsaft_amd import pcsaft
    together = _fit_together()
    again = pcsaft.fit_kij(list(_four_systems()), feed_x1s=FEEDS)
    keys = ("k_12", "loss", "loss_nonan", "mape", "n_nan", "iterations")
    for key in keys:
        assert together[key].tobytes() == again[key].tobytes(), key
    assert together["reason"].tolist() == again["reason"].tolist()
    assert len(set(together["iterations"].tolist())) > 1  # they leave the launches at different times
    for s, system in enumerate(_four_systems()):
        alone = pcsaft.fit_kij([system], feed_x1s=FEEDS)
        for key in keys:
            assert alone[key][0].tobytes() == together[key][s].tobytes(), (s, key, alone[key][0], together[key][s])
        assert alone["reason"][0] == together["reason"][s]


def test_optimize_kij_end_to_end(gpu_device, monkeypatch):
    """Two pairs, the planted and the noisy rows of A, with a null x1 row, a row at 7000 kPa and 350 K (0.95 of the
    7377.3 kPa that count from 304.2 K on: dropped) and a row at 300 K and 100 kPa (below the CO2 vapour pressure there:
    kept): the rows that reach the fit are those with P_kPa / vp < 0.85, the keys are the reference's, and k_12 is
    ``fit_kij`` on those rows bit for bit."""
    from gnnepcsaft_amd import pcsaft
    T = [s[0] for s in A]
    P_kpa = [s[1] / 1e3 for s in A]
    table = {"inchi1": ["butane"] * 4 + ["butane", "butane", "butane'"] + ["butane'"] * 4 + ["butane"],
             "inchi2": ["hexane"] * 4 + ["hexane", "hexane", "hexane'"] + ["hexane'"] * 4 + ["hexane"],
             "T_K": T + [350.0, 350.0, 300.0] + T + [350.0],
             "P_kPa": P_kpa + [400.0, 7000.0, 100.0] + P_kpa + [7000.0],
             "mole_fraction_c1p2": _planted(0.05).tolist() + [None, 0.5, 0.3] + (_planted(0.05) * NOISE).tolist() + [0.5]}
    params = {"butane": V.BUTANE, "hexane": V.HEXANE, "butane'": V.BUTANE, "hexane'": V.HEXANE, pcsaft.CO2_INCHI: CO2}
    seen = []
    fit_kij = pcsaft.fit_kij
    monkeypatch.setattr(pcsaft, "fit_kij", lambda systems, **kw: seen.append((systems, kw)) or fit_kij(systems, **kw))
    out = pcsaft.optimize_kij(table, params, n=8)
    monkeypatch.undo()
    assert list(out) == ["inchi1", "inchi2", "k_12", "loss", "loss_nonan", "mape", "n_nan"]
    assert out["inchi1"] == ["butane", "butane'"] and out["inchi2"] == ["hexane", "hexane'"]
    assert all(isinstance(v, list) and len(v) == 2 for v in out.values())
    # the test's own filter, with the vapour pressure of CO2 from pure_vp
    rows = [r for r in zip(*(table[c] for c in pcsaft.KIJ_COLUMNS)) if r[4] is not None]
    vp = [pcsaft.pure_vp(CO2, [r[2]]) / 1e3 if r[2] < 304.2 else 7377.3 for r in rows]
    kept = [r for r, v in zip(rows, vp) if r[3] / v < 0.85]
    assert len(rows) == 11 and len(kept) == 9 and not any(r[3] == 7000.0 for r in kept) and any(r[2] == 300.0 for r in kept)
    systems = []
    for pair in (("butane", "hexane"), ("butane'", "hexane'")):
        mine = [r for r in kept if (r[0], r[1]) == pair]
        systems.append(([params[pair[0]], params[pair[1]]], np.array([r[2] for r in mine]),
                        np.array([r[3] for r in mine]) * 1e3, np.array([r[4] for r in mine])))
    (got, kw), = seen
    assert kw == {"n": 8} and len(got) == 2
    for mine, theirs in zip(systems, got):
        assert mine[0] == theirs[0] and all(np.array_equal(u, v) for u, v in zip(mine[1:], theirs[1:]))
    assert len(systems[0][1]) == 4 and len(systems[1][1]) == 5  # the null row and both 7000 kPa rows are gone
    fit = pcsaft.fit_kij(systems, n=8)
    print(out, {key: v.tolist() for key, v in fit.items()})
    for key in ("k_12", "loss", "loss_nonan", "mape"):
        assert np.array(out[key]).tobytes() == fit[key].tobytes(), key
    assert out["n_nan"] == fit["n_nan"].tolist()
    assert abs(out["k_12"][0] - 0.05) <= 1e-6 and out["n_nan"][0] == 0
