"""Mixture bubble points on the GPU (csrc/gnx_pcsaft_mix_vle.hip, gnnepcsaft_amd/pcsaft.py) against the oracle of
tests/pcsaft_mix_vle_ref.py: the equilibrium equations at the reported state (the primary check: the oracle's pressure
and finite-difference fugacities share no mechanism with the kernel's duals), the oracle's own solve, the reductions,
the fugacity kernels, failures and invalid input, determinism and the reference-shaped I/O.

The points are the six named systems of the oracle module (1.8 to 8.5 MPa, 90 kPa with association, three and four
components) and the first point of each of the 24 systems of the binary fixture (0.40 Pa to 5.2 MPa)."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_vle_ref as V
from tests import pcsaft_ref as R

pytestmark = pytest.mark.gpu

VP_TOL = 1e-8  # the bound of test_pcsaft_gpu.py on pcsaft.vapor_pressure against pcsaft_ref.vle
SOLVE_TOL = 1e-10  # kVleMixTol: what the kernel's loop ends on
ROOT_TOL = 1e-14
NC = 4


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _bubble(dev, params, comp, owner, T, x, kij=None, eab=None):
    """(P, y, rho_l, rho_v, status) as host arrays"""
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, xx, k, e = _dev(dev, np.asarray(params, dtype=np.float64).reshape(-1, 9), comp, owner, T, x, kij, eab)
    return [v.cpu().numpy() for v in pcsaft.mixture_bubble_pressure(p, c, xx, t, o, k, e)]


def _pooled(cases):
    """cases (name, rows, T, x) of 1 to 4 components as one pool: params [B, 9], comp [M, 4] (-1 = unused), owner [M],
    T [M], x [M, 4]"""
    params, comp, T, x = [], np.full((len(cases), NC), -1, dtype=np.int64), [], np.zeros((len(cases), NC))
    for i, (_, rows, t, xi) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        x[i, :len(rows)] = xi
        T.append(t)
    return np.array(params), comp, np.arange(len(cases), dtype=np.int64), np.array(T), x


def _cases():
    return list(V.NAMED) + V.fixture_cases()


@functools.lru_cache(maxsize=None)
def _all_points(dev):
    """the kernel on the named and the fixture points, one launch: computed once, shared, never modified"""
    return _bubble(dev, *_pooled(_cases()))


def _rel(a, b):
    return abs(a / b - 1.0)


def test_equations_hold_at_the_reported_state(gpu_device):
    """On the 6 named points and every fixture point the oracle solves within 100 steps (all 24 here): status 0, sum y
    = 1, rho_l > rho_v > 0, the oracle's pressure of (x, rho_l) and (y, rho_v) is P at 1e-9 (the liquid on the scale
    max(P, 1e-3 rho R T), as at every small Z), and the oracle's ln f_i agree between the phases within 2 x the kernel's
    tolerance + 10 x the disagreement of the oracle's two difference steps at that point.
    On an MI355X, worst of the 30: sum y - 1 2.2e-16, liquid pressure 6.6e-10, vapour pressure 3.3e-16, fugacities
    1.29e-10 (0.40 of the bound at that point; the two-step disagreement reaches 4.6e-9)."""
    cases = _cases()
    solved = [True] * len(V.NAMED) + [s is not None for s in V.fixture_solves()]
    P, y, rl, rv, st = _all_points(gpu_device)
    worst = {"sum y": 0.0, "p liquid": 0.0, "p vapour": 0.0, "fugacity": 0.0, "fugacity / bound": 0.0, "two-step": 0.0}
    assert sum(solved) >= 29
    for j, (name, rows, T, x) in enumerate(cases):
        if not solved[j]:
            continue
        k = len(rows)
        assert st[j] == 0 and P[j] > 0.0 and rl[j] > rv[j] > 0.0, name
        assert np.all(np.isnan(y[j, k:])) and np.all(y[j, :k] > 0.0)
        r = V.residuals(rows, x, y[j, :k], T, P[j], rl[j], rv[j])
        bound = 2.0 * SOLVE_TOL + 10.0 * r["own"]
        fig = {"sum y": abs(y[j, :k].sum() - 1.0),
               "p liquid": abs(r["p_l"] - P[j]) / max(P[j], rl[j] * R.RGAS * T * 1e-3),
               "p vapour": _rel(r["p_v"], P[j]), "fugacity": r["fugacity"], "fugacity / bound": r["fugacity"] / bound,
               "two-step": r["own"]}
        for key, v in fig.items():
            worst[key] = max(worst[key], v)
        assert fig["sum y"] <= 1e-12 and fig["p liquid"] <= 1e-9 and fig["p vapour"] <= 1e-9, (name, fig)
        assert r["fugacity"] <= bound, (name, fig)
    print("worst over", sum(solved), "points:", worst)


def test_against_the_oracles_own_solve(gpu_device):
    """Named points: P (relative) and y (absolute) within max(1e-9, 10 x what the oracle's own answer moves between its
    tolerances 1e-9 and 1e-11 there); 1e-9 is the standing kernel-against-oracle bound of test_pcsaft_mix_gpu.py.
    On an MI355X: P within 1.2e-11, y within 2.4e-12; the oracle's own change is 2.8e-11 to 6.5e-10."""
    P, y, rl, rv, st = _all_points(gpu_device)
    for j, ((name, rows, T, x), (sol, change)) in enumerate(zip(V.NAMED, V.named_solves())):
        k = len(rows)
        bound = max(1e-9, 10.0 * change)
        dp, dy = _rel(P[j], sol["P"]), float(np.max(np.abs(y[j, :k] - sol["y"])))
        print(name, "P", P[j], "dP", dp, "dy", dy, "rho_l", _rel(rl[j], sol["rho_l"]), "rho_v", _rel(rv[j], sol["rho_v"]),
              "bound", bound)
        assert st[j] == 0 and dp <= bound and dy <= bound


def test_reductions(gpu_device):
    from gnnepcsaft_amd import pcsaft
    rows = np.array([V.HEXANE, V.BUTANE, V.ETHANOL, V.METHANE], dtype=np.float64)
    T = np.array([350.0, 330.0, 340.0])
    p, t = _dev(gpu_device, rows[:3], T)
    ps, pl, pv, pst = [v.cpu().numpy() for v in pcsaft.vapor_pressure(p, t)]
    assert np.all(pst == 0)
    # one component, and a binary at x = (1, 0): the pure vapour pressure; y is 1.0, and 0.0 for the absent component
    comp1 = np.arange(3, dtype=np.int64)[:, None]
    P, y, rl, rv, st = _bubble(gpu_device, rows, comp1, np.arange(3), T, np.ones((3, 1)))
    worst = max(np.max(np.abs(P / ps - 1)), np.max(np.abs(rl / pl - 1)), np.max(np.abs(rv / pv - 1)))
    print("one component against pcsaft.vapor_pressure:", worst)
    assert np.all(st == 0) and worst <= VP_TOL and np.all(y == 1.0)
    comp2 = np.stack([np.arange(3), (np.arange(3) + 1) % 3], axis=1).astype(np.int64)
    x10 = np.tile([1.0, 0.0], (3, 1))
    P2, y2, rl2, rv2, st2 = _bubble(gpu_device, rows, comp2, np.arange(3), T, x10)
    assert np.all(st2 == 0) and np.array_equal(y2, x10)
    assert max(np.max(np.abs(P2 / ps - 1)), np.max(np.abs(rl2 / pl - 1)), np.max(np.abs(rv2 / pv - 1))) <= VP_TOL
    assert np.max(np.abs(P2 / P - 1)) <= 1e-12
    # the same row twice is that component: y = x and its vapour pressure
    same = np.stack([np.arange(3), np.arange(3)], axis=1).astype(np.int64)
    x37 = np.tile([0.3, 0.7], (3, 1))
    P3, y3, _, _, st3 = _bubble(gpu_device, rows, same, np.arange(3), T, x37)
    print("same row twice: y", np.max(np.abs(y3 - x37)), "P", np.max(np.abs(P3 / ps - 1)))
    assert np.all(st3 == 0) and np.max(np.abs(y3 - x37)) <= 1e-9 and np.max(np.abs(P3 / ps - 1)) <= VP_TOL
    # a -1 slot and an x = 0 slot: the mixture without them, NaN and 0.0 in y
    tern = np.array([[3, 1, 0]], dtype=np.int64)  # methane, butane, hexane
    t320, x3 = np.array([320.0]), np.array([[0.2, 0.0, 0.8]])
    Pb, yb, _, _, stb = _bubble(gpu_device, rows, np.array([[3, 0]], dtype=np.int64), [0], t320, np.array([[0.2, 0.8]]))
    Pz, yz, _, _, stz = _bubble(gpu_device, rows, tern, [0], t320, x3)
    Pm, ym, _, _, stm = _bubble(gpu_device, rows, np.array([[3, -1, 0]], dtype=np.int64), [0], t320,
                                np.array([[0.2, 0.5, 0.8]]))
    assert stb[0] == 0 and stz[0] == 0 and stm[0] == 0
    assert _rel(Pz[0], Pb[0]) <= 1e-12 and _rel(Pm[0], Pb[0]) <= 1e-12
    assert yz[0, 1] == 0.0 and np.isnan(ym[0, 1])
    assert np.max(np.abs(yz[0, [0, 2]] - yb[0])) <= 1e-12 and np.max(np.abs(ym[0, [0, 2]] - yb[0])) <= 1e-12


def test_component_swap_and_upper_triangle(gpu_device):
    """the swapped mixture gives the same point at 1e-9; what the lower triangle and the diagonal of k_ij hold changes no
    bit"""
    cases = _cases()
    params, comp, owner, T, x = _pooled(cases)
    rng = np.random.default_rng(3)
    kij = np.zeros((len(cases), NC, NC))
    kij[:, 0, 1] = rng.uniform(-0.02, 0.02, len(cases))
    P, y, rl, rv, st = _bubble(gpu_device, params, comp, owner, T, x, kij=kij)
    swap = [1, 0, 2, 3]
    Ps, ys, rls, rvs, sts = _bubble(gpu_device, params, comp[:, swap].copy(), owner, T, x[:, swap].copy(), kij=kij)
    ok = st == 0
    used = comp >= 0
    assert ok.sum() >= 29 and np.array_equal(st, sts)
    dy = np.max(np.abs(np.where(used, ys[:, swap] - y, 0.0)[ok]))
    print("swap: P", np.max(np.abs(Ps[ok] / P[ok] - 1)), "y", dy, "rho_l", np.max(np.abs(rls[ok] / rl[ok] - 1)))
    assert np.max(np.abs(Ps[ok] / P[ok] - 1)) <= 1e-9 and dy <= 1e-9
    junk = kij + np.tril(rng.uniform(-9.0, 9.0, kij.shape))
    junk[:, 2, 0] = np.nan
    again = _bubble(gpu_device, params, comp, owner, T, x, kij=junk)
    for a, b in zip((P, y, rl, rv, st), again):
        assert a.tobytes() == b.tobytes()


def test_consistent_with_the_fugacity_kernels(gpu_device):
    """mixture_ln_phi_state at (x, rho_l) and (y, rho_v): ln(phi_i x_i) agrees between the phases within 2 x the kernel's
    tolerance plus the allowance for -ln Z of test_pcsaft_mix_phi_gpu.py, 2e-14 (dp/drho) / (R T Z), of both phases.  The
    named points only: P >= 0.09 MPa there."""
    from gnnepcsaft_amd import pcsaft
    cases = list(V.NAMED)
    params, comp, owner, T, x = _pooled(cases)
    n = len(cases)
    P, y, rl, rv, st = [v[:n] for v in _all_points(gpu_device)]
    assert np.all(st == 0)
    p, c, o, t = _dev(gpu_device, params, comp, owner, T)
    diff, noise = np.zeros((n, NC)), np.zeros(n)
    for sign, comps, rho in ((1.0, x, rl), (-1.0, np.nan_to_num(y), rv)):
        xx, r = _dev(gpu_device, comps, rho)
        lnphi, _, s1 = [v.cpu().numpy() for v in pcsaft.mixture_ln_phi_state(p, c, xx, t, r, o)]
        _, pr, dp, s2 = [v.cpu().numpy() for v in pcsaft.mixture_state(p, c, xx, t, r, o)]
        assert np.all(s1 == 0) and np.all(s2 == 0)
        diff += sign * (lnphi + np.log(np.where(comp >= 0, comps, 1.0)))
        noise += 2.0 * ROOT_TOL * dp * rho / pr
    worst = np.nanmax(np.abs(diff), axis=1)
    print("ln(phi x)_L - ln(phi y)_V:", worst, "allowance for ln Z:", noise)
    assert np.all(worst <= 2.0 * SOLVE_TOL + noise)


def test_no_bubble_point_and_invalid_input(gpu_device):
    rows = np.array([V.METHANE, V.BUTANE, V.HEXANE, V.PROPANE], dtype=np.float64)
    comp = np.array([[0, -1, -1, -1], [1, 2, -1, -1], [0, 1, 2, -1], [0, 3, 1, 2]], dtype=np.int64)
    xs = np.array([[1.0, 0, 0, 0], [0.5, 0.5, 0, 0], [0.1, 0.3, 0.6, 0], [0.1, 0.2, 0.3, 0.4]])
    T = np.array([300.0, 350.0, 320.0, 320.0])
    # methane alone at 300 K is above its critical temperature: no bubble point, status 1
    P, y, rl, rv, st = _bubble(gpu_device, rows, comp, np.arange(4), T, xs)
    assert st.tolist() == [1, 0, 0, 0]
    assert P[0] == 0.0 and rl[0] == 0.0 and rv[0] == 0.0 and np.all(np.isnan(y[0]))
    assert np.array_equal(np.isnan(y[1:]), comp[1:] < 0)
    # mixtures with 1 to 4 used slots in one launch, owner shuffled, 257 points: the block edge, and every lane its own
    owner = np.random.default_rng(5).integers(0, 4, 257)
    Pn, yn, rln, rvn, stn = _bubble(gpu_device, rows, comp, owner, T[owner], xs[owner])
    assert np.array_equal(stn, st[owner]) and Pn.tobytes() == P[owner].tobytes()
    assert yn.tobytes() == y[owner].tobytes() and rln.tobytes() == rl[owner].tobytes()
    assert rvn.tobytes() == rv[owner].tobytes()
    # n = 1 and n = 0
    one = _bubble(gpu_device, rows, comp, np.array([2]), T[2:3], xs[2:3])
    assert one[4].tolist() == [0] and one[0][0] == P[2] and np.array_equal(one[1][0], y[2], equal_nan=True)
    none = _bubble(gpu_device, rows, comp, np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros((0, 4)))
    assert [v.shape for v in none] == [(0,), (0, 4), (0,), (0,), (0,)]
    # invalid input: status 3, P = 0, NaN in y
    bad_owner = np.array([1, 1, 1, 4, -1, 1, 1, 1])
    bad_T = np.array([350.0, 350.0, 350.0, 350.0, 350.0, np.nan, np.inf, -1.0])
    bad_x = np.tile(xs[1], (8, 1))
    bad_x[0, 0] = -0.5
    bad_x[1, :2] = 0.0
    bad_x[2, 1] = np.nan
    Pb, yb, rlb, rvb, stb = _bubble(gpu_device, rows, comp, bad_owner, bad_T, bad_x)
    assert np.all(stb == 3) and np.all(Pb == 0.0) and np.all(rlb == 0.0) and np.all(rvb == 0.0)
    assert np.all(np.isnan(yb))
    # the x of a -1 slot is ignored, whatever it holds
    x_junk = xs[1:2].copy()
    x_junk[0, 2:] = [np.nan, -3.0]
    Pj, yj, _, _, stj = _bubble(gpu_device, rows, comp, np.array([1]), T[1:2], x_junk)
    assert stj[0] == 0 and Pj[0] == P[1] and np.array_equal(yj[0], y[1], equal_nan=True)


def test_two_calls_give_the_same_bits(gpu_device):
    cases = _cases()
    params, comp, owner, T, x = _pooled(cases)
    idx = np.arange(257) % len(cases)
    a = _bubble(gpu_device, params, comp, owner[idx], T[idx], x[idx])
    b = _bubble(gpu_device, params, comp, owner[idx], T[idx], x[idx])
    first = _all_points(gpu_device)
    for u, v, w in zip(a, b, first):
        assert u.tobytes() == v.tobytes() and u.tobytes() == w[idx].tobytes()


def test_reference_shaped_io(gpu_device):
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    tern = [V.METHANE, V.BUTANE, V.HEXANE]
    states = [np.array([[350.0, 0.0, 0.5, 0.5], [350.0, 1e5, 0.2, 0.8]]), np.zeros((0, 5)),
              np.array([[320.0, 0.0, 0.1, 0.3, 0.6]]), np.array([[300.0, 0.0, 1.0]])]
    out = pcsaft.mix_bubble_batch([rows, tern, tern, [V.METHANE]], states)
    assert [o.shape for o in out] == [(2, 3), (1, 4), (1, 2)]
    assert np.all(np.isnan(out[2]))  # methane alone at 300 K: a failed point is a row of NaN
    P, y = pcsaft.mix_bubble(rows, [350.0, 123.0, 0.5, 0.5])
    assert P == out[0][0, 0] and np.array_equal(y, out[0][0, 1:])
    P3, y3 = pcsaft.mix_bubble(tern, [320.0, 0.0, 0.1, 0.3, 0.6])
    assert P3 == out[1][0, 0] and np.array_equal(y3, out[1][0, 1:])
    with pytest.raises(RuntimeError):
        pcsaft.mix_bubble([V.METHANE], [300.0, 0.0, 1.0])
    assert pcsaft.mix_bubble_batch([rows], [np.zeros((0, 4))]) == []
    # a k_ij changes the answer, and the matrices reach the kernel
    Pk, _ = pcsaft.mix_bubble(rows, [350.0, 0.0, 0.5, 0.5], kij_matrix=[[0.0, 0.05], [0.05, 0.0]])
    assert Pk > P * 1.01


def test_pxy_diagram(gpu_device):
    from gnnepcsaft_amd import pcsaft
    rows = [V.BUTANE, V.HEXANE]
    d = pcsaft.mix_vle_pxy(rows, 350.0, points=11)
    keys = ["temperature", "pressure", "density liquid", "density vapor", "x0", "x1", "y0", "y1"]
    assert list(d) == keys and all(len(d[k]) == 11 for k in keys)
    assert np.allclose(d["x0"], np.linspace(0, 1, 11)) and np.allclose(np.add(d["x0"], d["x1"]), 1.0)
    p, t = _dev(gpu_device, np.array([V.HEXANE, V.BUTANE], dtype=np.float64), np.array([350.0, 350.0]))
    ps, pl, pv, st = [v.cpu().numpy() for v in pcsaft.vapor_pressure(p, t)]
    assert np.all(st == 0)
    for end, k in ((0, 0), (-1, 1)):  # x0 = 0 is hexane alone, x0 = 1 butane alone
        assert _rel(d["pressure"][end], ps[k]) <= VP_TOL and _rel(d["density liquid"][end], pl[k]) <= VP_TOL
        assert _rel(d["density vapor"][end], pv[k]) <= VP_TOL
    assert d["y0"][0] == 0.0 and d["y1"][0] == 1.0 and d["y0"][-1] == 1.0 and d["y1"][-1] == 0.0
    for j in range(1, 10):
        P, y = pcsaft.mix_bubble(rows, [350.0, 0.0, d["x0"][j], d["x1"][j]])
        assert P == d["pressure"][j] and y[0] == d["y0"][j] and y[1] == d["y1"][j]
    assert np.all(np.diff(d["pressure"]) > 0)  # butane is the lighter component
    # methane + hexane at 300 K: beyond the critical composition there is no bubble point; the rest comes back aligned
    m = pcsaft.mix_vle_pxy([V.METHANE, V.HEXANE], 300.0, points=11)
    n = len(m["pressure"])
    print("methane + hexane at 300 K: points kept", n, "largest x0", m["x0"][-1], "P", m["pressure"][-1])
    assert 3 <= n < 11 and all(len(m[k]) == n for k in keys)
    assert m["x0"][0] == 0.0 and np.allclose(m["x0"], np.linspace(0, 1, 11)[:n])
    with pytest.raises(ValueError, match="No VLE found"):
        pcsaft.mix_vle_pxy([V.METHANE, V.METHANE], 300.0, points=3)
