"""Mixture PC-SAFT on the GPU (csrc/gnx_pcsaft_mix.hip, gnnepcsaft_amd/pcsaft.py) against the fp64 oracle of
tests/pcsaft_mix_ref.py: every point of the binary ThermoML fixture, seeded random mixtures of 1 to 4 components,
the reductions to the pure kernel, small and invalid inputs, determinism and the reference-shaped I/O."""
import json
import os

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_cases as C
from tests import pcsaft_mix_ref as MR
from tests import pcsaft_ref as R

pytestmark = pytest.mark.gpu

RHO_TOL = 1e-9
# The oracle's dP/drho is a central difference (relative step h = 1e-6) of a complex-step pressure and the weaker side.
# At a liquid root Z is what is left of terms of size 10, so the pressure carries an absolute rounding error of about
# 10 eps rho R T; the difference quotient divides it by h rho, which gives 1e-9 R T against dP/drho = 10 .. 50 R T:
# 1e-10 relative at best, 1e-9 with the scan of rounding over 192 points (truncation, h^2, is 1e-12).  The bound is
# 10 x that.  The kernel's arithmetic restated on the host differed from the oracle by 7.8e-10 at worst on the fixture
# (a host figure, not a GPU measurement; the test prints the GPU's own).
DPDRHO_TOL = 1e-8


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _density(dev, params, comp, owner, T, P, x, kij=None, eab=None):
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, pp, xx, k, e = _dev(dev, params, comp, owner, T, P, x, kij, eab)
    rho, st = pcsaft.mixture_density(p, c, xx, t, pp, o, k, e)
    return rho.cpu().numpy(), st.cpu().numpy()


def test_fixture_density_matches_the_oracle(gpu_device):
    params, comp, owner, T, P, x, _ = C.fixture_points()
    assert len(owner) <= 192
    rho, st = _density(gpu_device, params, comp, owner, T, P, x)
    ref = C.fixture_oracle()
    assert np.all(st == 0) and np.all(np.isfinite(ref))
    rel = np.abs(rho / ref - 1.0)
    print("largest relative density deviation on the fixture:", rel.max())
    assert rel.max() <= RHO_TOL


def test_fixture_state_matches_the_oracle(gpu_device):
    from gnnepcsaft_amd import pcsaft
    params, comp, owner, T, _, x, _ = C.fixture_points()
    ref = C.fixture_oracle()
    p, c, o, t, r, xx = _dev(gpu_device, params, comp, owner, T, ref, x)
    a, pr, dp, st = [v.cpu().numpy() for v in pcsaft.mixture_state(p, c, xx, t, r, o)]
    assert np.all(st == 0)
    worst = [0.0, 0.0, 0.0]
    for j in range(len(owner)):
        mix = MR.Mixture(params[comp[owner[j]]], x[j])
        rn = ref[j] * R.TO_A3
        a_ref, z1_ref = MR.a_res(mix, T[j], rn), MR.compressibility(mix, T[j], rn) - 1.0
        z1 = pr[j] / (ref[j] * R.RGAS * T[j]) - 1.0
        worst[0] = max(worst[0], abs(a[j] - a_ref) / max(1.0, abs(a_ref)))
        worst[1] = max(worst[1], abs(z1 - z1_ref) / max(1.0, abs(z1_ref)))
        worst[2] = max(worst[2], abs(dp[j] / MR.dpdrho(mix, T[j], ref[j]) - 1.0))
    print("largest deviations (a_res, Z - 1, dpdrho):", worst)
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9 and worst[2] <= DPDRHO_TOL


def test_random_mixtures_match_the_recorded_oracle(gpu_device):
    """300 mixtures of random rows (the ranges of the pure suite), 1 to 4 slots, 100 with a -1 slot, k_ij from
    [-0.1, 0.1], 4 states each: where kernel and oracle both report a root they agree at 1e-9; the points where only one
    of them does are counted and stay under 1 % (3 of 1200 when the record was written, kernel logic run on the host)."""
    groups, ref = C.recorded()
    at = disagree = both = 0
    for g in groups:
        n = len(g["owner"])
        rho, st = _density(gpu_device, g["rows"], g["comp"], g["owner"], g["T"], g["P"], g["x"], kij=g["kij"])
        want = ref[at:at + n]
        at += n
        assert set(np.unique(st)) <= {0, 1} and np.all(rho[st != 0] == 0.0)
        ok_k, ok_o = st == 0, np.isfinite(want)
        disagree += int((ok_k != ok_o).sum())
        sel = ok_k & ok_o
        both += int(sel.sum())
        assert np.all(np.abs(rho[sel] / want[sel] - 1.0) <= RHO_TOL), (g["nc"], np.abs(rho[sel] / want[sel] - 1.0).max())
    print("points with a root on both sides:", both, "on one side only:", disagree)
    assert at == 1200 and both >= 800 and disagree <= 12


def test_reductions_to_the_pure_kernel(gpu_device):
    from gnnepcsaft_amd import pcsaft
    with open(os.path.join(C.GOLDEN, "pcsaft_thermoml.json")) as fh:
        mols = json.load(fh)["molecules"][::4]
    rows = np.array([m["params"] for m in mols], dtype=np.float64)
    pts = [(i, s[0], s[1]) for i, m in enumerate(mols) for s in m["rho"][:3]]
    owner = np.array([p[0] for p in pts], dtype=np.int64)
    T, P = np.array([p[1] for p in pts]), np.array([p[2] for p in pts])
    p, o, t, pp = _dev(gpu_device, rows, owner, T, P)
    pure, st = pcsaft.density(p, t, pp, o)
    pure = pure.cpu().numpy()
    assert np.all(st.cpu().numpy() == 0)
    B = len(rows)
    same = np.stack([np.arange(B), np.arange(B)], axis=1)
    beside = np.stack([np.arange(B), (np.arange(B) + 5) % B], axis=1)  # a different (often associating) neighbour
    n = len(pts)
    for comp, x in ((same, np.tile([0.3, 0.7], (n, 1))), (beside, np.tile([1.0, 0.0], (n, 1))),
                    (beside[:, ::-1].copy(), np.tile([0.0, 2.0], (n, 1)))):
        rho, st = _density(gpu_device, rows, comp, owner, T, P, x)
        assert np.all(st == 0) and np.abs(rho / pure - 1.0).max() <= RHO_TOL


def test_component_swap(gpu_device):
    params, comp, owner, T, P, x, _ = C.fixture_points()
    kij = np.zeros((len(comp), 2, 2))
    kij[:, 0, 1] = kij[:, 1, 0] = 0.03
    r1, s1 = _density(gpu_device, params, comp, owner, T, P, x, kij=kij)
    r2, s2 = _density(gpu_device, params, comp[:, ::-1].copy(), owner, T, P, x[:, ::-1].copy(),
                      kij=np.transpose(kij, (0, 2, 1)).copy())
    assert np.all(s1 == 0) and np.all(s2 == 0) and np.abs(r1 / r2 - 1.0).max() <= 1e-12


def test_kij_and_eab_are_read_from_the_upper_triangle(gpu_device):
    """The convention of DESIGN.md §4c: entry [min(i, j)][max(i, j)] counts for the pair; what the lower triangle and the
    diagonal hold (NaN included) changes no bit."""
    params, comp, owner, T, P, x, _ = C.fixture_points()
    M = len(comp)
    kij, eab = np.zeros((M, 2, 2)), np.full((M, 2, 2), np.nan)
    kij[:, 0, 1] = kij[:, 1, 0] = 0.03
    eab[-1, 0, 1] = eab[-1, 1, 0] = 2400.0  # ethanol + water
    r1, s1 = _density(gpu_device, params, comp, owner, T, P, x, kij=kij, eab=eab)
    kij[:, 1, 0], kij[:, 0, 0], kij[:, 1, 1] = -0.5, 0.7, np.nan
    eab[:, 1, 0], eab[:, 0, 0], eab[:, 1, 1] = 9e3, 1.0, np.inf
    r2, s2 = _density(gpu_device, params, comp, owner, T, P, x, kij=kij, eab=eab)
    plain, _ = _density(gpu_device, params, comp, owner, T, P, x)
    assert np.all(s1 == 0) and np.all(s2 == 0) and r1.tobytes() == r2.tobytes()
    mixed = np.all(x > 0, axis=1)
    assert mixed.sum() >= 100 and np.all(r1[mixed] != plain[mixed])


def test_small_and_invalid_inputs(gpu_device):
    from gnnepcsaft_amd import pcsaft
    params, comp, owner, T, P, x, _ = C.fixture_points()
    full, _ = _density(gpu_device, params, comp, owner, T, P, x)
    # n = 1 and M = 1
    r, s = _density(gpu_device, params[:2], comp[:1], owner[:1], T[:1], P[:1], x[:1])
    assert s[0] == 0 and r[0] == full[0]
    # n = 257: the second workgroup is partial
    idx = np.arange(257) % len(owner)
    r, s = _density(gpu_device, params, comp, owner[idx], T[idx], P[idx], x[idx])
    assert np.all(s == 0) and np.array_equal(r, full[idx])
    # n = 0
    r, s = _density(gpu_device, params, comp, owner[:0], T[:0], P[:0], x[:0])
    assert r.shape == (0,) and s.shape == (0,)
    p, c, o, t, rr, xx = _dev(gpu_device, params, comp, owner[:0], T[:0], T[:0], x[:0])
    assert all(v.numel() == 0 for v in pcsaft.mixture_state(p, c, xx, t, rr, o))
    # invalid points beside a valid one
    k = 8
    own, xs = owner[:k].copy(), x[:k].copy()
    own[1], own[2] = -1, len(comp)
    xs[3, 0] = -0.1
    xs[4] = 0.0
    xs[5, 1] = np.nan
    bad_comp = comp.copy()
    bad_comp[owner[6]] = [len(params), 0]
    r, s = _density(gpu_device, params, comp, own, T[:k], P[:k], xs)
    assert s.tolist() == [0, 3, 3, 3, 3, 3, 0, 0] and np.all(r[1:6] == 0.0) and r[0] == full[0] and r[7] == full[7]
    r, s = _density(gpu_device, params, bad_comp, owner[:k], T[:k], P[:k], x[:k])
    assert np.all(s[owner[:k] == owner[6]] == 3) and np.all(r[owner[:k] == owner[6]] == 0.0)
    empty = np.full_like(comp, -1)
    r, s = _density(gpu_device, params, empty, owner[:k], T[:k], P[:k], x[:k])
    assert np.all(s == 3) and np.all(r == 0.0)
    # a NaN in eab is the combining rule; a given cross value is not
    sel = np.nonzero(owner == len(comp) - 1)[0]  # ethanol + water
    nan = np.full((len(comp), 2, 2), np.nan)
    r, s = _density(gpu_device, params, comp, owner[sel], T[sel], P[sel], x[sel], eab=nan)
    assert np.all(s == 0) and np.array_equal(r, full[sel])
    given = nan.copy()
    given[-1, 0, 1] = 2000.0
    r, s = _density(gpu_device, params, comp, owner[sel], T[sel], P[sel], x[sel], eab=given)
    mixed = np.all(x[sel] > 0, axis=1)  # the cross value does not reach a pure end point
    assert np.all(s == 0) and mixed.sum() >= 4 and np.all(r[mixed] != full[sel][mixed])
    assert np.array_equal(r[~mixed], full[sel][~mixed])
    two = np.nonzero(mixed)[0][:2]
    ref = [MR.density(MR.Mixture(params[comp[-1]], x[j], eab=given[-1]), T[j], P[j]) for j in sel[two]]
    assert np.abs(r[two] / np.array(ref) - 1.0).max() <= RHO_TOL
    # a -1 slot beside one component is that component
    one = np.stack([comp[:, 0], np.full(len(comp), -1)], axis=1)
    r, s = _density(gpu_device, params, one, owner[:k], T[:k], P[:k], x[:k])
    pure = [R.density(params[comp[o, 0]], t, p) for o, t, p in zip(owner[:k], T[:k], P[:k])]
    assert np.all(s == 0) and np.abs(r / np.array(pure) - 1.0).max() <= RHO_TOL


def test_two_calls_give_the_same_bits(gpu_device):
    params, comp, owner, T, P, x, _ = C.fixture_points()
    idx = np.arange(10_000) % len(owner)
    a = _density(gpu_device, params, comp, owner[idx], T[idx], P[idx], x[idx])
    b = _density(gpu_device, params, comp, owner[idx], T[idx], P[idx], x[idx])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.all(a[1] == 0)


def test_reference_shaped_io(gpu_device):
    from gnnepcsaft_amd import pcsaft
    sy = C.systems()[::5]
    mixtures = [s["params"] for s in sy] + [[sy[0]["params"][0]]]
    tables = [np.array(s["points"])[:, :4] for s in sy] + [np.array([[300.0, 1e5, 1.0]])]
    tables[1] = np.zeros((0, 4))
    out = pcsaft.mix_rho_batch(mixtures, tables)
    assert [len(o) for o in out] == [len(t) for t in tables if len(t) > 0]
    assert all(isinstance(o, np.ndarray) and o.dtype == np.float64 for o in out)
    kept = [i for i, t in enumerate(tables) if len(t) > 0]
    for o, i in zip(out, kept):
        for r, s in zip(o, tables[i]):
            assert r == pcsaft.mix_den(mixtures[i], s.tolist())
    params, comp, owner, T, P, x, _ = C.fixture_points()
    tensor, _ = _density(gpu_device, params, comp, owner, T, P, x)
    assert np.array_equal(out[0], tensor[owner == 0])
    assert out[-1][0] == pcsaft.pure_den(mixtures[-1][0], [300.0, 1e5]) or \
        abs(out[-1][0] / pcsaft.pure_den(mixtures[-1][0], [300.0, 1e5]) - 1.0) <= RHO_TOL
    kij = [[0.0, 0.05], [0.05, 0.0]]
    with_k = pcsaft.mix_rho_batch(mixtures[:1], tables[:1], kij=[kij])
    assert with_k[0][3] == pcsaft.mix_den(mixtures[0], tables[0][3].tolist(), kij_matrix=kij) != out[0][3]
    assert pcsaft.mix_rho_batch(mixtures, [np.zeros((0, 4))] * len(mixtures)) == []
    with pytest.raises(RuntimeError):  # 1e15 Pa is above the pressure at close packing: no liquid root
        pcsaft.mix_den(mixtures[0], [tables[0][0][0], 1e15, 0.5, 0.5])
