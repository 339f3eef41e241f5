"""Mixture (T, P) flashes on the GPU (csrc/gnx_pcsaft_mix_flash.hip, gnnepcsaft_amd/pcsaft.py) against the oracle of
tests/pcsaft_mix_flash_ref.py: the equilibrium equations and the material balance at the reported state (the primary
check: the oracle's pressure and finite-difference fugacities share no mechanism with the kernel's duals), the bubble
points the feeds were built from and the oracle's own flash, single-phase feeds and invalid input, the reductions, lanes
and repeatability, the fugacity kernels and the reference-shaped I/O.

The points are the 12 tie-line feeds of the oracle module (the six named bubble points at beta = 0.3, 0.09 to 8.5 MPa, with
association, three and four components; the fixture cases 0 to 5 at beta = 0.5, 2.2 Pa to 5.2 MPa), its four single-phase
points and methane alone at 300 K, all in one launch that every test shares."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_flash_ref as F
from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

pytestmark = pytest.mark.gpu

SOLVE_TOL = 1e-10  # kVleMixTol: what the kernel's loop ends on
ROOT_TOL = 1e-14
NC = 4


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _flash(dev, params, comp, owner, T, P, z, kij=None, eab=None):
    """(beta, x, y, rho_l, rho_v, status) as host arrays"""
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, pp, zz, k, e = _dev(dev, np.asarray(params, dtype=np.float64).reshape(-1, 9), comp,
                                    np.asarray(owner, dtype=np.int64), np.asarray(T, dtype=np.float64),
                                    np.asarray(P, dtype=np.float64), np.asarray(z, dtype=np.float64), kij, eab)
    return [v.cpu().numpy() for v in pcsaft.mixture_tp_flash(p, c, zz, t, pp, o, k, e)]


def _pooled(cases):
    """cases (name, rows, T, P, z) of 1 to 4 components as one pool: params [B, 9], comp [M, 4] (-1 = unused), owner [M],
    T [M], P [M], z [M, 4]"""
    params, comp, z = [], np.full((len(cases), NC), -1, dtype=np.int64), np.zeros((len(cases), NC))
    for i, (_, rows, _, _, zi) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        z[i, :len(rows)] = zi
    return (np.array(params), comp, np.arange(len(cases), dtype=np.int64), np.array([c[2] for c in cases], dtype=np.float64),
            np.array([c[3] for c in cases], dtype=np.float64), z)


@functools.lru_cache(maxsize=None)
def _cases():
    """the 12 tie-line feeds, the 4 single-phase points, methane alone at 300 K: (name, rows, T, P, z)"""
    tie = [(name, rows, T, P, z) for name, rows, T, P, z, _, _, _ in F.tie_line_points()]
    return tie + list(F.single_phase_points()) + [("methane alone", [V.METHANE], 300.0, 1e6, [1.0])]


N_TIE, N_SINGLE = 12, 5


@functools.lru_cache(maxsize=None)
def _all_points(dev):
    """the kernel on every point of ``_cases``, one launch: computed once, shared, never modified"""
    return _flash(dev, *_pooled(_cases()))


def _rel(a, b):
    return abs(a / b - 1.0)


def _same_bytes(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_equations_hold_at_the_reported_state(gpu_device):
    """On every tie-line point: status 0, 0 < beta < 1, sum x = sum y = 1 and z = (1 - beta) x + beta y at 1e-12, rho_l >
    rho_v > 0, the oracle's pressure of (x, rho_l) and (y, rho_v) is P at 1e-9 (the liquid on the scale max(P, 1e-3 rho R
    T), as at every small Z), and the oracle's ln f_i agree between the phases within 2 x the kernel's tolerance + 10 x the
    disagreement of the oracle's two difference steps at that point: the bubble test's bounds for the same equations.
    On an MI355X, worst of the 12: sum x - 1 and sum y - 1 2.2e-16, balance 1.1e-16, liquid pressure 2.9e-11, vapour
    pressure 4.4e-16, fugacities 9.2e-11 (0.14 of the bound at that point; the two-step disagreement reaches 1.6e-10)."""
    cases = _cases()
    beta, x, y, rl, rv, st = _all_points(gpu_device)
    worst = {"sum x": 0.0, "sum y": 0.0, "balance": 0.0, "p liquid": 0.0, "p vapour": 0.0, "fugacity": 0.0,
             "fugacity / bound": 0.0, "two-step": 0.0}
    assert len(cases) == N_TIE + N_SINGLE
    for j, (name, rows, T, P, z) in enumerate(cases[:N_TIE]):
        k = len(rows)
        assert st[j] == 0 and 0.0 < beta[j] < 1.0 and rl[j] > rv[j] > 0.0, (name, st[j], beta[j])
        assert np.all(np.isnan(x[j, k:])) and np.all(np.isnan(y[j, k:])) and np.all(x[j, :k] > 0.0) and np.all(y[j, :k] > 0.0)
        r = V.residuals(rows, x[j, :k], y[j, :k], T, P, rl[j], rv[j])
        bound = 2.0 * SOLVE_TOL + 10.0 * r["own"]
        fig = {"sum x": abs(x[j, :k].sum() - 1.0), "sum y": abs(y[j, :k].sum() - 1.0),
               "balance": F.balance(z, x[j, :k], y[j, :k], beta[j]),
               "p liquid": abs(r["p_l"] - P) / max(P, rl[j] * R.RGAS * T * 1e-3), "p vapour": _rel(r["p_v"], P),
               "fugacity": r["fugacity"], "fugacity / bound": r["fugacity"] / bound, "two-step": r["own"]}
        print(name, fig)
        for key, v in fig.items():
            worst[key] = max(worst[key], v)
        assert fig["sum x"] <= 1e-12 and fig["sum y"] <= 1e-12 and fig["balance"] <= 1e-12, (name, fig)
        assert fig["p liquid"] <= 1e-9 and fig["p vapour"] <= 1e-9, (name, fig)
        assert r["fugacity"] <= bound, (name, fig)
    print("worst over", N_TIE, "points:", worst)


def test_against_the_bubble_point_and_the_oracles_own_flash(gpu_device):
    """Tie-line points: x and y against the bubble point the feed was built from and against the oracle's flash, within
    max(1e-9, 10 x what the oracle's own flash moves between its tolerances 1e-9 and 1e-11 there); beta against 0.3 / 0.5
    and the oracle's within that bound over max_i |y_i - x_i| (beta is x's error seen through the lever rule).
    On an MI355X: against the bubble points x within 4.1e-10, y within 8.6e-11, beta within 1.2e-9 (ethanol + water, bound
    2.7e-8); against the oracle's flash x within 2.4e-11, y within 1.5e-11, beta within 5.5e-10 (fixture case 1, max |y - x|
    = 0.03); at most 0.068 of the bound.  The oracle's own change is 1.9e-12 to 2.7e-9."""
    beta, x, y, rl, rv, st = _all_points(gpu_device)
    worst = {"x": 0.0, "y": 0.0, "beta": 0.0, "x oracle": 0.0, "y oracle": 0.0, "beta oracle": 0.0, "of bound": 0.0}
    for j, ((name, rows, T, P, z, xb, yb, bb), (sol, change)) in enumerate(zip(F.tie_line_points(), F.tie_line_solves())):
        k = len(rows)
        assert st[j] == 0 and isinstance(sol, dict), name
        bound = max(1e-9, 10.0 * change)
        lever = bound / float(np.max(np.abs(yb - xb)))
        fig = {"x": float(np.max(np.abs(x[j, :k] - xb))), "y": float(np.max(np.abs(y[j, :k] - yb))),
               "beta": abs(beta[j] - bb), "x oracle": float(np.max(np.abs(x[j, :k] - sol["x"]))),
               "y oracle": float(np.max(np.abs(y[j, :k] - sol["y"]))), "beta oracle": abs(beta[j] - sol["beta"])}
        fig["of bound"] = max(fig["x"], fig["y"], fig["x oracle"], fig["y oracle"]) / bound
        fig["of bound"] = max(fig["of bound"], fig["beta"] / lever, fig["beta oracle"] / lever)
        print(name, fig, "bound", bound, "rho_l", _rel(rl[j], sol["rho_l"]), "rho_v", _rel(rv[j], sol["rho_v"]))
        for key, v in fig.items():
            worst[key] = max(worst[key], v)
        assert fig["of bound"] <= 1.0, (name, fig, bound)
    print("worst:", worst)


def _assert_failed(out, j, status):
    beta, x, y, rl, rv, st = out
    assert st[j] == status, (j, st[j], status)
    assert beta[j] == 0.0 and rl[j] == 0.0 and rv[j] == 0.0 and np.all(np.isnan(x[j])) and np.all(np.isnan(y[j]))


def test_single_phase_and_invalid_input(gpu_device):
    cases = _cases()
    out = _all_points(gpu_device)
    # above the bubble pressure, below every vapour pressure, one component: status 4, zeros and NaN
    for j in range(N_TIE, N_TIE + N_SINGLE):
        _assert_failed(out, j, 4)
    assert np.all(out[5][:N_TIE] == 0)
    params, comp, owner, T, P, z = _pooled(cases)
    # n = 1 and n = 0
    one = _flash(gpu_device, params, comp, [2], T[2:3], P[2:3], z[2:3])
    assert one[5].tolist() == [0] and _same_bytes(one, [v[2:3] for v in out])
    none = _flash(gpu_device, params, comp, np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0), np.zeros((0, NC)))
    assert [v.shape for v in none] == [(0,), (0, NC), (0, NC), (0,), (0,), (0,)]
    # invalid input: status 3 with the same pattern.  Point 2 is butane + hexane at 350 K
    n_bad = 13
    bad_owner = np.full(n_bad, 2)
    bad_T, bad_P, bad_z = np.full(n_bad, T[2]), np.full(n_bad, P[2]), np.tile(z[2], (n_bad, 1))
    bad_owner[0], bad_owner[1] = len(cases), -1
    bad_T[2], bad_T[3], bad_T[4], bad_T[5] = np.nan, np.inf, -1.0, 0.0
    bad_P[6], bad_P[7], bad_P[8], bad_P[9] = np.nan, np.inf, 0.0, -1e5
    bad_z[10, 0] = -0.5
    bad_z[11, :2] = 0.0
    bad_z[12, 1] = np.nan
    bad = _flash(gpu_device, params, comp, bad_owner, bad_T, bad_P, bad_z)
    for j in range(n_bad):
        _assert_failed(bad, j, 3)
    # the z of a -1 slot is ignored, whatever it holds
    junk = z.copy()
    junk[comp < 0] = np.tile([np.nan, -3.0, np.inf, 7.0], len(cases))[:int((comp < 0).sum())]
    assert _same_bytes(_flash(gpu_device, params, comp, owner, T, P, junk), out)


def test_reductions(gpu_device):
    """a used slot with z = 0 and a -1 slot give the binary's answer at 1e-12 with 0.0 / NaN in that column; the swapped
    mixture gives the same split at 1e-9 (every tie-line point loses at least a factor 0.9 per step, so the loop's 1e-10
    bounds what two roundings of the same iteration can differ by below that); what the lower triangle and the diagonal of
    k_ij hold changes no bit"""
    rows = np.array([V.HEXANE, V.BUTANE, V.ETHANOL, V.METHANE], dtype=np.float64)
    t320, p3 = [320.0], [3e6]  # methane + hexane, z = (0.3, 0.7): between the dew and the bubble pressure
    b = _flash(gpu_device, rows, np.array([[3, 0]], dtype=np.int64), [0], t320, p3, [[0.3, 0.7]])
    zero = _flash(gpu_device, rows, np.array([[3, 1, 0]], dtype=np.int64), [0], t320, p3, [[0.3, 0.0, 0.7]])
    gone = _flash(gpu_device, rows, np.array([[3, -1, 0]], dtype=np.int64), [0], t320, p3, [[0.3, 0.5, 0.7]])
    assert b[5][0] == 0 and zero[5][0] == 0 and gone[5][0] == 0 and 0.0 < b[0][0] < 1.0
    for other in (zero, gone):
        assert abs(other[0][0] - b[0][0]) <= 1e-12 and _rel(other[3][0], b[3][0]) <= 1e-12
        assert _rel(other[4][0], b[4][0]) <= 1e-12
        assert np.max(np.abs(other[1][0, [0, 2]] - b[1][0])) <= 1e-12 and np.max(np.abs(other[2][0, [0, 2]] - b[2][0])) <= 1e-12
    assert zero[1][0, 1] == 0.0 and zero[2][0, 1] == 0.0 and np.isnan(gone[1][0, 1]) and np.isnan(gone[2][0, 1])
    # component swap on every point of the shared launch
    params, comp, owner, T, P, z = _pooled(_cases())
    beta, x, y, rl, rv, st = _all_points(gpu_device)
    swap = [1, 0, 2, 3]
    bs, xs, ys, rls, rvs, sts = _flash(gpu_device, params, comp[:, swap].copy(), owner, T, P, z[:, swap].copy())
    ok = st == 0
    used = (comp >= 0)[ok]
    assert np.array_equal(st, sts) and ok.sum() == N_TIE
    fig = {"beta": np.max(np.abs(bs[ok] - beta[ok])), "x": np.max(np.abs(np.where(used, xs[:, swap][ok] - x[ok], 0.0))),
           "y": np.max(np.abs(np.where(used, ys[:, swap][ok] - y[ok], 0.0))), "rho_l": np.max(np.abs(rls[ok] / rl[ok] - 1)),
           "rho_v": np.max(np.abs(rvs[ok] / rv[ok] - 1))}
    print("swap:", fig)
    assert max(fig.values()) <= 1e-9
    # k_ij: only the upper triangle is read
    rng = np.random.default_rng(3)
    kij = np.zeros((len(owner), NC, NC))
    kij[:, 0, 1] = rng.uniform(-0.02, 0.02, len(owner))
    with_kij = _flash(gpu_device, params, comp, owner, T, P, z, kij=kij)
    assert not _same_bytes(with_kij, (beta, x, y, rl, rv, st))
    junk = kij + np.tril(rng.uniform(-9.0, 9.0, kij.shape))
    junk[:, 2, 0] = np.nan
    assert _same_bytes(_flash(gpu_device, params, comp, owner, T, P, z, kij=junk), with_kij)


def test_lanes_and_repeatability(gpu_device):
    """257 points (the block edge) with owners shuffled over mixtures of 1 to 4 used slots, two-phase and single-phase:
    every lane returns the bytes of its point from the shared launch, and two calls give the same bytes"""
    params, comp, owner, T, P, z = _pooled(_cases())
    assert sorted(set((comp >= 0).sum(axis=1).tolist())) == [1, 2, 3, 4]
    idx = np.random.default_rng(5).integers(0, len(owner), 257)
    first = _all_points(gpu_device)
    a = _flash(gpu_device, params, comp, owner[idx], T[idx], P[idx], z[idx])
    b = _flash(gpu_device, params, comp, owner[idx], T[idx], P[idx], z[idx])
    assert _same_bytes(a, b) and _same_bytes(a, [v[idx] for v in first])
    assert set(a[5].tolist()) == {0, 4}


def test_consistent_with_the_fugacity_kernels(gpu_device):
    """mixture_ln_phi_state at (x, rho_l) and (y, rho_v): ln(phi_i x_i) agrees between the phases within 2 x the kernel's
    tolerance plus the allowance for -ln Z of test_pcsaft_mix_phi_gpu.py, 2e-14 (dp/drho) / (R T Z), of both phases.  The
    named points only: P >= 0.09 MPa there."""
    from gnnepcsaft_amd import pcsaft
    n = len(V.NAMED)
    params, comp, owner, T, P, z = _pooled(_cases()[:n])
    beta, x, y, rl, rv, st = [v[:n] for v in _all_points(gpu_device)]
    assert np.all(st == 0)
    p, c, o, t = _dev(gpu_device, params, comp, owner, T)
    diff, noise = np.zeros((n, NC)), np.zeros(n)
    for sign, comps, rho in ((1.0, np.nan_to_num(x), rl), (-1.0, np.nan_to_num(y), rv)):
        xx, r = _dev(gpu_device, comps, rho)
        lnphi, _, s1 = [v.cpu().numpy() for v in pcsaft.mixture_ln_phi_state(p, c, xx, t, r, o)]
        _, pr, dp, s2 = [v.cpu().numpy() for v in pcsaft.mixture_state(p, c, xx, t, r, o)]
        assert np.all(s1 == 0) and np.all(s2 == 0)
        diff += sign * (lnphi + np.log(np.where(comp >= 0, comps, 1.0)))
        noise += 2.0 * ROOT_TOL * dp * rho / pr
    worst = np.nanmax(np.abs(diff), axis=1)
    print("ln(phi x)_L - ln(phi y)_V:", worst, "allowance for ln Z:", noise)
    assert np.all(worst <= 2.0 * SOLVE_TOL + noise)


def test_reference_shaped_io(gpu_device):
    from gnnepcsaft_amd import pcsaft
    cases = _cases()
    (_, rows, T, P, z), (_, tern, T3, P3, z3), (_, _, _, Ps, _) = cases[2], cases[4], cases[N_TIE]
    states = [np.array([[T, P, *z], [T, Ps, *z]]), np.zeros((0, 5)), np.array([[T3, P3, *z3]]), np.array([[300.0, 1e6, 1.0]])]
    out = pcsaft.mix_tp_flash_batch([rows, tern, tern, [V.METHANE]], states)
    assert [o.shape for o in out] == [(2, 5), (1, 7), (1, 3)]
    assert np.all(np.isnan(out[0][1])) and np.all(np.isnan(out[2]))  # single phase: a row of NaN
    beta, x, y, rl, rv, st = _all_points(gpu_device)
    for j, row in ((2, out[0][0]), (4, out[1][0])):
        k = len(cases[j][1])
        assert row[0] == beta[j] and np.array_equal(row[1:1 + k], x[j, :k]) and np.array_equal(row[1 + k:], y[j, :k])
    one = pcsaft.mix_tp_flash(rows, [T, P, *z])
    assert list(one) == ["beta", "x", "y", "density liquid", "density vapor"]
    assert one["beta"] == out[0][0, 0] and np.array_equal(one["x"], out[0][0, 1:3]) and np.array_equal(one["y"], out[0][0, 3:])
    assert one["density liquid"] == rl[2] and one["density vapor"] == rv[2]
    three = pcsaft.mix_tp_flash(tern, [T3, P3, *z3])
    assert three["beta"] == out[1][0, 0] and np.array_equal(np.concatenate([three["x"], three["y"]]), out[1][0, 1:])
    with pytest.raises(RuntimeError, match="single phase"):
        pcsaft.mix_tp_flash(rows, [T, Ps, *z])
    with pytest.raises(RuntimeError):
        pcsaft.mix_tp_flash([V.METHANE], [300.0, 1e6, 1.0])
    assert pcsaft.mix_tp_flash_batch([rows], [np.zeros((0, 4))]) == []
    # a k_ij changes the answer: the matrices reach the kernel
    with_kij = pcsaft.mix_tp_flash(rows, [T, P, *z], kij_matrix=[[0.0, 0.02], [0.02, 0.0]])
    assert abs(with_kij["x"][0] - one["x"][0]) > 1e-4
    batch_kij = pcsaft.mix_tp_flash_batch([rows], [states[0][:1]], kij=[[[0.0, 0.02], [0.02, 0.0]]])
    assert batch_kij[0][0, 1] == with_kij["x"][0]


def test_flash_x1_lies_on_the_bubble_curve(gpu_device):
    """mix_flash_x1 on butane + hexane at 350 K, three pressures inside the P-x-y diagram and one above it, feeds
    linspace(1e-5, 0.99, 8): each x_1 returned is the liquid of a split, so mix_bubble at that x gives the pressure back,
    within max(1e-9, 10 x the change of the oracle's flash between 1e-9 and 1e-11 at the first feed it splits); NaN above
    the diagram."""
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    d = pcsaft.mix_vle_pxy(rows, 350.0, points=11)
    lo, hi = min(d["pressure"]), max(d["pressure"])
    pressures = [lo + f * (hi - lo) for f in (0.25, 0.5, 0.75)] + [1.2 * hi]
    feeds = np.linspace(1e-5, 0.99, 8)
    x1 = pcsaft.mix_flash_x1(rows, [[350.0, p] for p in pressures], feeds)
    assert x1.shape == (4,) and x1.dtype == np.float64 and np.isnan(x1[3]) and np.all(np.diff(x1[:3]) > 0)
    for p, xk in zip(pressures[:3], x1[:3]):
        trace, sol = [], None
        for f in feeds:
            trace = []
            sol = F.flash(rows, [f, 1.0 - f], 350.0, p, tol=1e-11, trace=trace)
            if isinstance(sol, dict):
                break
        assert isinstance(sol, dict)
        loose = next(t for t in trace if t[0] < 1e-9)
        bound = max(1e-9, 10.0 * float(np.max(np.abs(loose[2] - sol["x"]))))
        back, _ = pcsaft.mix_bubble(rows, [350.0, 0.0, xk, 1.0 - xk])
        print("P", p, "x1", xk, "oracle", sol["x"][0], "bubble pressure back", _rel(back, p), "bound", bound)
        assert abs(xk - sol["x"][0]) <= bound and _rel(back, p) <= bound
    # one state, one feed, with a k_ij: the same bits as the flash itself
    one = pcsaft.mix_flash_x1(rows, [[350.0, pressures[1]]], [0.65], kij_matrix=[[0.0, 0.02], [0.02, 0.0]])
    ref = pcsaft.mix_tp_flash(rows, [350.0, pressures[1], 0.65, 0.35], kij_matrix=[[0.0, 0.02], [0.02, 0.0]])
    assert one[0] == ref["x"][0]
