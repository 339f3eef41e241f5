"""Mixture fugacity coefficients on the GPU (csrc/gnx_pcsaft_mix_phi.hip, gnnepcsaft_amd/pcsaft.py) against the
finite-difference oracle of tests/pcsaft_mix_phi_ref.py: the binary ThermoML fixture, the recorded random mixtures of 1
to 4 components, the state form, reductions and symmetry, infinite dilution, activity coefficients, a component without
a liquid root, small and invalid inputs, determinism and the reference-shaped I/O.

The oracle is evaluated at the density the kernel returns: ln phi at a liquid root carries -ln Z with Z of 1e-3 .. 1e-2
left over from terms of size 10, so it moves by 1e4 times a relative change of the density, and only values at the same
density compare."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_cases as C
from tests import pcsaft_mix_phi_ref as PR
from tests import pcsaft_mix_ref as MR
from tests import pcsaft_ref as R

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-9  # the bound of test_pcsaft_mix_gpu.py on a_res and Z - 1 of the same oracle
# Gross & Sadowski 2001, Table 2: methane (critical temperature 190.6 K) and n-hexane
METHANE = [1.0, 3.7039, 150.03, 0.0, 0.0, 0.0, 0.0, 0.0, 16.043]
HEXANE = [3.0576, 3.7983, 236.77, 0.0, 0.0, 0.0, 0.0, 0.0, 86.177]


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _np(values):
    return [None if v is None else v.cpu().numpy() for v in values]


def _density(dev, params, comp, owner, T, P, x, kij=None, eab=None):
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, pp, xx, k, e = _dev(dev, params, comp, owner, T, P, x, kij, eab)
    return _np(pcsaft.mixture_density(p, c, xx, t, pp, o, k, e))


def _phi(dev, params, comp, owner, T, P, x, kij=None, eab=None, pure=False):
    """(rho, lnphi, lnphi_pure or None, status) as host arrays"""
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, pp, xx, k, e = _dev(dev, params, comp, owner, T, P, x, kij, eab)
    return _np(pcsaft.mixture_ln_phi(p, c, xx, t, pp, o, k, e, pure=pure))


def _phi_state(dev, params, comp, owner, T, rho, x, kij=None, eab=None):
    """(lnphi, Z, status) as host arrays"""
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, r, xx, k, e = _dev(dev, params, comp, owner, T, rho, x, kij, eab)
    return _np(pcsaft.mixture_ln_phi_state(p, c, xx, t, r, o, k, e))


@functools.lru_cache(maxsize=None)
def _fixture_phi(dev):
    """the kernel on every fixture point, with the pure values: computed once, shared, never modified"""
    params, comp, owner, T, P, x, _ = C.fixture_points()
    return _phi(dev, params, comp, owner, T, P, x, pure=True)


def _sum_identity_error(rows, x, T, rho_mol, lnphi, kij=None):
    want = PR.sum_identity(rows, x, T, rho_mol * R.TO_A3, kij=kij)
    return float(PR.scaled(np.dot(x / x.sum(), lnphi), want))


def _against_oracle(rows, x, T, rho_mol, lnphi, kij=None, eab=None):
    """(the oracle's two-step disagreement, the kernel's deviation from the finer step), both on max(1, |ln phi|)"""
    coarse, fine = PR.ln_phi(rows, x, T, rho_mol * R.TO_A3, kij=kij, eab=eab)
    return float(PR.scaled(coarse, fine).max()), float(PR.scaled(lnphi, fine).max())


@functools.lru_cache(maxsize=None)
def _fixture_sample(dev):
    """(the oracle's two-step disagreement, the kernel's deviation) on the 49 sample points of the fixture"""
    params, comp, owner, T, _, x, _ = C.fixture_points()
    rho, lnphi, _, st = _fixture_phi(dev)
    idx = PR.sample()
    assert len(idx) == 49 and np.all(st[idx] == 0)
    own = got = 0.0
    for j in idx:
        a, b = _against_oracle(params[comp[owner[j]]], x[j], T[j], rho[j], lnphi[j])
        own, got = max(own, a), max(got, b)
    return own, got


def test_fixture_root_and_sum_identity(gpu_device):
    params, comp, owner, T, P, x, _ = C.fixture_points()
    assert len(owner) <= 192
    rho, lnphi, _, st = _fixture_phi(gpu_device)
    ref, ref_st = _density(gpu_device, params, comp, owner, T, P, x)
    assert np.all(st == 0) and np.all(ref_st == 0) and rho.tobytes() == ref.tobytes()
    assert np.all(np.isfinite(lnphi))
    worst = max(_sum_identity_error(params[comp[owner[j]]], x[j], T[j], rho[j], lnphi[j]) for j in range(len(owner)))
    print("largest |sum x ln phi - (a + Z - 1 - ln Z)| on the fixture:", worst)
    assert worst <= SUM_TOL


def test_fixture_components_match_the_finite_difference_oracle(gpu_device):
    """49 points.  The tolerance is 10 x the disagreement of the oracle's two steps on these points, recomputed here: the
    oracle's rounding floor is not a bound on its error, and it is the only thing being measured.
    On an MI355X: two-step disagreement 3.2e-10, kernel deviation from the finer step 3.4e-10 (bound 3.2e-9); the oracle
    is the weaker side."""
    own, got = _fixture_sample(gpu_device)
    print("oracle two-step disagreement:", own, "kernel deviation:", got)
    assert got <= 10.0 * own


@pytest.mark.parametrize("gi", range(len(C.GROUPS)))
def test_random_mixtures(gpu_device, gi):
    """Recorded random mixtures of 1 to 4 slots with -1 holes and k_ij: the status is the density kernel's point by
    point, NaN stands exactly in the -1 slots and the failed rows, the sum identity holds wherever the recorded oracle
    has a root and the status is 0, and every 20th such point is held to the finite-difference oracle per component.
    On an MI355X (slots: points, sum identity, two-step disagreement, kernel deviation): 1: 120, 6.8e-12, 3.7e-11,
    1.6e-11; 2: 300, 4.1e-12, 7.8e-11, 5.5e-11; 3: 245, 4.2e-12, 8.0e-11, 7.4e-11; 4: 229, 1.1e-12, 7.6e-10, 6.6e-10."""
    groups, ref = C.recorded()
    g = groups[gi]
    at = sum(len(h["owner"]) for h in groups[:gi])
    n, nc = len(g["owner"]), g["nc"]
    rho, lnphi, _, st = _phi(gpu_device, g["rows"], g["comp"], g["owner"], g["T"], g["P"], g["x"], kij=g["kij"])
    ref_rho, ref_st = _density(gpu_device, g["rows"], g["comp"], g["owner"], g["T"], g["P"], g["x"], kij=g["kij"])
    assert set(np.unique(st)) <= {0, 1} and np.array_equal(st, ref_st)
    assert np.array_equal(rho, ref_rho)
    hole = (g["comp"][g["owner"]] < 0) | (st != 0)[:, None]
    assert np.array_equal(np.isnan(lnphi), hole) and np.all(np.isfinite(lnphi[~hole]))
    sel = np.nonzero((st == 0) & np.isfinite(ref[at:at + n]))[0]
    worst = own = got = 0.0
    for k, j in enumerate(sel):
        o = g["owner"][j]
        slots = g["comp"][o] >= 0
        rows, kij = g["rows"][g["comp"][o][slots]], g["kij"][o][np.ix_(slots, slots)]
        worst = max(worst, _sum_identity_error(rows, g["x"][j][slots], g["T"][j], rho[j], lnphi[j][slots], kij=kij))
        if k % 20 == 0:
            a, b = _against_oracle(rows, g["x"][j][slots], g["T"][j], rho[j], lnphi[j][slots], kij=kij)
            own, got = max(own, a), max(got, b)
    print(nc, "slots:", len(sel), "points, sum identity", worst, "oracle two-step disagreement", own,
          "kernel deviation", got)
    assert len(sel) >= 0.6 * n and worst <= SUM_TOL and got <= 10.0 * own


def test_state_form(gpu_device):
    """ln phi at the returned density is the root form's (the root form evaluates at the density it reports), and Z is
    p / (rho R T) of mixture_state"""
    from gnnepcsaft_amd import pcsaft
    params, comp, owner, T, _, x, _ = C.fixture_points()
    rho, lnphi, _, _ = _fixture_phi(gpu_device)
    ln2, Z, st = _phi_state(gpu_device, params, comp, owner, T, rho, x)
    assert np.all(st == 0) and PR.scaled(ln2, lnphi).max() <= 1e-12
    p, c, o, t, r, xx = _dev(gpu_device, params, comp, owner, T, rho, x)
    _, pr, _, st = _np(pcsaft.mixture_state(p, c, xx, t, r, o))
    assert np.all(st == 0) and np.abs(Z / (pr / (rho * R.RGAS * T)) - 1.0).max() <= 1e-12


# ln phi carries -ln Z, and at a liquid root Z = P / (rho R T) is what is left of terms of size 10: 7e-4 for water at 1
# bar.  The density solve ends on a relative step or bracket of 1e-14, so two ways to the same state (a
# swap, the same row twice, one component alone) end on densities up to 2e-14 apart, and ln Z moves by dp/drho / (R T Z)
# times that: 1e4 x 2e-14 = 2e-10 at 1 bar, above the bounds of 1e-12 and 1e-10 that these checks carry.  They therefore
# run on the fixture's temperatures and compositions at 200 MPa, where Z is of order 1 and the amplification below 100,
# and once more at the fixture's own pressures with that allowance added to the bound (_ln_z_noise, from the state
# kernel's dp/drho and p).
P_HIGH = 2e8
ROOT_TOL = 1e-14


def _ln_z_noise(dev, params, comp, owner, T, rho, x, kij=None):
    from gnnepcsaft_amd import pcsaft
    p, c, o, t, r, xx, k = _dev(dev, params, comp, owner, T, rho, x, kij)
    _, pr, dp, st = _np(pcsaft.mixture_state(p, c, xx, t, r, o, k))
    assert np.all(st == 0)
    return 2.0 * ROOT_TOL * dp * rho / pr


def test_reductions(gpu_device):
    """lnphi_pure is ln phi of the one-component call (1e-12); the same row twice is that component: ln phi_1 = ln phi_2
    = the pure value and ln gamma = 0 (1e-10)"""
    params, comp, owner, T, P, _, _ = C.fixture_points()
    n = len(owner)
    for s in range(2):
        one, twice = comp[:, s:s + 1].copy(), np.stack([comp[:, s], comp[:, s]], axis=1)
        for press, extra in ((np.full(n, P_HIGH), False), (P, True)):
            rho, alone, alone_pure, st = _phi(gpu_device, params, one, owner, T, press, np.ones((n, 1)), pure=True)
            _, both, both_pure, st2 = _phi(gpu_device, params, twice, owner, T, press, np.tile([0.3, 0.7], (n, 1)),
                                           pure=True)
            assert np.all(st == 0) and np.all(st2 == 0)
            have = ~np.isnan(alone_pure[:, 0])
            assert have.sum() >= 0.8 * n and np.array_equal(np.isnan(both_pure), np.tile(~have[:, None], (1, 2)))
            noise = _ln_z_noise(gpu_device, params, one, owner, T, rho, np.ones((n, 1))) if extra else np.zeros(n)
            d_pure = PR.scaled(alone_pure[have, 0], alone[have, 0])
            d_twice = PR.scaled(both, alone)
            d_gamma = np.abs(both - both_pure)[have]
            print("slot", s, "P", press[0], "lnphi_pure against the one-component call:", d_pure.max(),
                  "the same row twice against it:", d_twice.max(), "its ln gamma:", d_gamma.max(),
                  "allowance for ln Z:", noise.max())
            assert np.all(d_pure <= 1e-12)
            assert np.all(d_twice <= 1e-10 + noise[:, None]) and np.all(d_gamma <= 1e-10 + noise[have, None])


def test_component_swap(gpu_device):
    """a component swap with the transposed k_ij swaps the columns (1e-12)"""
    params, comp, owner, T, P, x, _ = C.fixture_points()
    n = len(owner)
    kij = np.zeros((len(comp), 2, 2))
    kij[:, 0, 1] = kij[:, 1, 0] = 0.03
    for press, extra in ((np.full(n, P_HIGH), False), (P, True)):
        rho, l1, p1, s1 = _phi(gpu_device, params, comp, owner, T, press, x, kij=kij, pure=True)
        _, l2, p2, s2 = _phi(gpu_device, params, comp[:, ::-1].copy(), owner, T, press, x[:, ::-1].copy(),
                             kij=np.transpose(kij, (0, 2, 1)).copy(), pure=True)
        assert np.all(s1 == 0) and np.all(s2 == 0)
        noise = _ln_z_noise(gpu_device, params, comp, owner, T, rho, x, kij) if extra else np.zeros(n)
        print("component swap at P", press[0], ":", PR.scaled(l2[:, ::-1], l1).max(), "allowance for ln Z:", noise.max())
        assert np.all(PR.scaled(l2[:, ::-1], l1) <= 1e-12 + noise[:, None])
        assert np.array_equal(p2[:, ::-1], p1, equal_nan=True)


def test_infinite_dilution(gpu_device):
    params, comp, owner, T, P, _, _ = C.fixture_points()
    n = len(owner)
    _, end, pure, st = _phi(gpu_device, params, comp, owner, T, P, np.tile([1.0, 0.0], (n, 1)), pure=True)
    _, near, _, st2 = _phi(gpu_device, params, comp, owner, T, P, np.tile([1.0, 1e-8], (n, 1)))
    _, next_, _, st3 = _phi(gpu_device, params, comp, owner, T, P, np.tile([1.0, 2e-8], (n, 1)))
    assert np.all(st == 0) and np.all(st2 == 0) and np.all(st3 == 0) and np.all(np.isfinite(end))
    # A solute that does not associate: d ln phi_2 / d x_2 is O(10), so 1e-7 is expected.  One that does starts to bond
    # to itself as soon as it is there, d ln X_A / d x_2 = -rho Delta_22 is several hundred, and the value at 1e-8 is
    # further away than the bound; there, and everywhere, the value at 0 is held to the line through 1e-8 and 2e-8.
    row2 = params[comp[owner, 1]]
    plain = ~((row2[:, 3] > 0) & (row2[:, 6] + row2[:, 7] > 0))
    step = np.abs(end[:, 1] - near[:, 1])
    line = np.abs(end[:, 1] - (2.0 * near[:, 1] - next_[:, 1]))
    print("ln phi_2 at x_2 = 0 against x_2 = 1e-8:", step[plain].max(), "(solute associates:", step[~plain].max(),
          ") against the line through 1e-8 and 2e-8:", line.max())
    assert plain.sum() >= 90 and (~plain).sum() >= 90 and step[plain].max() <= 1e-6 and line.max() <= 1e-6
    have = ~np.isnan(pure[:, 0])
    assert have.sum() >= 0.9 * n and np.abs(end[have, 0] - pure[have, 0]).max() <= 1e-10


def test_activity_of_ethanol_and_water(gpu_device):
    """with a given cross association energy and k_ij: ln gamma against the oracle (mixture ln phi by finite differences
    at the kernel's density, the pure values from the oracle's own density of each component), at the tolerance of the
    fixture test; the Gibbs energies are their defining sums of the kernel's own output, exactly"""
    from gnnepcsaft_amd import pcsaft
    params, comp, owner, T, P, x, _ = C.fixture_points()
    sel = np.nonzero((owner == len(comp) - 1) & np.all(x > 0.02, axis=1))[0]
    j = sel[np.argmin(T[sel])]  # both components are below their critical temperature
    rows = params[comp[-1]]
    kij, eab = [[0.0, -0.05], [-0.05, 0.0]], [[0.0, 2400.0], [2400.0, 0.0]]
    state = [T[j], P[j], x[j, 0], x[j, 1]]
    args = ([list(r) for r in rows], state, kij, eab)
    ln_gamma = pcsaft.mix_ln_activity_coefficient(*args)
    lnphi = pcsaft.mix_ln_fugacity_coefficient(*args)
    assert isinstance(ln_gamma, np.ndarray) and ln_gamma.shape == (2,) and lnphi.shape == (2,)
    assert np.array_equal(ln_gamma, lnphi - pcsaft.mix_ln_fugacity_coefficient_pure(*args))
    rho = pcsaft.mix_den(*args)
    coarse, fine = PR.ln_phi(rows, x[j], T[j], rho * R.TO_A3, kij=kij, eab=eab)
    alone = np.array([PR.ln_phi_one(r, T[j], MR.density(MR.Mixture([r], [1.0]), T[j], P[j]) * R.TO_A3) for r in rows])
    own, got = _fixture_sample(gpu_device)[0], float(PR.scaled(ln_gamma, fine - alone).max())
    print("ln gamma:", ln_gamma, "two-step disagreement here:", float(PR.scaled(coarse, fine).max()),
          "and on the fixture sample:", own, "kernel deviation:", got)
    assert got <= 10.0 * own
    xn = x[j] / x[j].sum()
    assert pcsaft.mix_e_gibbs_energy(*args) == float(np.sum(ln_gamma * xn))
    assert pcsaft.mix_r_gibbs_energy(*args) == float(np.sum(lnphi * xn))
    assert pcsaft.mix_gibbs_energy(*args) == float(np.sum(ln_gamma * xn) + np.sum(xn * np.log(xn)))
    # a pure end point: 0 ln 0 counts as 0
    end = ([list(r) for r in rows], [T[j], P[j], 1.0, 0.0], kij, eab)
    assert abs(pcsaft.mix_gibbs_energy(*end)) <= 1e-10 and np.isfinite(pcsaft.mix_ln_activity_coefficient(*end)[1])


def test_component_without_a_liquid_root(gpu_device):
    """methane at 300 K is far above its critical temperature: p(rho) has no unstable stretch and so no liquid branch"""
    from gnnepcsaft_amd import pcsaft
    rows = np.array([METHANE, HEXANE])
    comp, owner = np.array([[0, 1]]), np.zeros(1, dtype=np.int64)
    T, P, x = np.array([300.0]), np.array([1e6]), np.array([[0.05, 0.95]])
    _, lnphi, pure, st = _phi(gpu_device, rows, comp, owner, T, P, x, pure=True)
    assert st[0] == 0 and np.all(np.isfinite(lnphi)) and np.isnan(pure[0, 0]) and np.isfinite(pure[0, 1])
    state = [300.0, 1e6, 0.05, 0.95]
    with pytest.raises(RuntimeError):
        pcsaft.mix_ln_activity_coefficient(rows.tolist(), state)
    with pytest.raises(RuntimeError):
        pcsaft.mix_e_gibbs_energy(rows.tolist(), state)
    assert np.array_equal(pcsaft.mix_ln_fugacity_coefficient(rows.tolist(), state), lnphi[0])
    assert np.array_equal(pcsaft.mix_ln_fugacity_coefficient_pure(rows.tolist(), state), pure[0], equal_nan=True)
    with pytest.raises(RuntimeError):  # 1e15 Pa is above the pressure at close packing: no root at all
        pcsaft.mix_ln_fugacity_coefficient(rows.tolist(), [300.0, 1e15, 0.05, 0.95])


def test_small_and_invalid_inputs(gpu_device):
    params, comp, owner, T, P, x, _ = C.fixture_points()
    full = _fixture_phi(gpu_device)
    # n = 0
    r, l, p, s = _phi(gpu_device, params, comp, owner[:0], T[:0], P[:0], x[:0], pure=True)
    assert r.shape == (0,) and l.shape == (0, 2) and p.shape == (0, 2) and s.shape == (0,)
    l, z, s = _phi_state(gpu_device, params, comp, owner[:0], T[:0], T[:0], x[:0])
    assert l.shape == (0, 2) and z.shape == (0,) and s.shape == (0,)
    # n = 1 and M = 1
    r, l, _, s = _phi(gpu_device, params[:2], comp[:1], owner[:1], T[:1], P[:1], x[:1])
    assert s[0] == 0 and r[0] == full[0][0] and np.array_equal(l[0], full[1][0])
    # n = 257: the second workgroup is partial
    idx = np.arange(257) % len(owner)
    r, l, p, s = _phi(gpu_device, params, comp, owner[idx], T[idx], P[idx], x[idx], pure=True)
    assert np.all(s == 0) and np.array_equal(r, full[0][idx]) and np.array_equal(l, full[1][idx])
    assert np.array_equal(p, full[2][idx], equal_nan=True)
    # invalid points beside valid ones
    k = 8
    own, xs = owner[:k].copy(), x[:k].copy()
    own[1], own[2] = -1, len(comp)
    xs[3, 0] = -0.1
    xs[4] = 0.0
    xs[5, 1] = np.nan
    r, l, p, s = _phi(gpu_device, params, comp, own, T[:k], P[:k], xs, pure=True)
    assert s.tolist() == [0, 3, 3, 3, 3, 3, 0, 0] and np.all(r[1:6] == 0.0)
    assert np.all(np.isnan(l[1:6])) and np.all(np.isnan(p[1:6]))
    for j in (0, 6, 7):
        assert r[j] == full[0][j] and np.array_equal(l[j], full[1][j]) and np.array_equal(p[j], full[2][j], equal_nan=True)
    l, z, s = _phi_state(gpu_device, params, comp, own, T[:k], full[0][:k], xs)
    assert s.tolist() == [0, 3, 3, 3, 3, 3, 0, 0] and np.all(np.isnan(l[1:6])) and np.all(z[1:6] == 0.0)
    assert np.all(np.isfinite(l[[0, 6, 7]]))
    bad_comp = comp.copy()
    bad_comp[owner[6]] = [len(params), 0]  # a row index past B
    r, l, _, s = _phi(gpu_device, params, bad_comp, owner[:k], T[:k], P[:k], x[:k])
    hit = owner[:k] == owner[6]
    assert np.all(s[hit] == 3) and np.all(r[hit] == 0.0) and np.all(np.isnan(l[hit]))
    assert np.all(s[~hit] == 0) and np.array_equal(l[~hit], full[1][:k][~hit])
    r, l, _, s = _phi(gpu_device, params, np.full_like(comp, -1), owner[:k], T[:k], P[:k], x[:k])
    assert np.all(s == 3) and np.all(r == 0.0) and np.all(np.isnan(l))
    # a -1 slot beside one component is that component, and reports NaN
    one = np.stack([comp[:, 0], np.full(len(comp), -1)], axis=1)
    r, l, _, s = _phi(gpu_device, params, one, owner[:k], T[:k], P[:k], x[:k])
    _, alone, _, _ = _phi(gpu_device, params, comp[:, :1].copy(), owner[:k], T[:k], P[:k], np.ones((k, 1)))
    assert np.all(s == 0) and np.all(np.isnan(l[:, 1])) and np.array_equal(l[:, 0], alone[:, 0])


def test_two_calls_give_the_same_bits(gpu_device):
    params, comp, owner, T, P, x, _ = C.fixture_points()
    idx = np.arange(10_000) % len(owner)
    a = _phi(gpu_device, params, comp, owner[idx], T[idx], P[idx], x[idx], pure=True)
    b = _phi(gpu_device, params, comp, owner[idx], T[idx], P[idx], x[idx], pure=True)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)) and np.all(a[3] == 0)


def test_batch_io(gpu_device):
    from gnnepcsaft_amd import pcsaft
    sy = C.systems()[::5]
    mixtures = [s["params"] for s in sy] + [[sy[0]["params"][0]]]
    tables = [np.array(s["points"])[:3, :4] for s in sy] + [np.array([[300.0, 1e5, 1.0]])]
    tables[1] = np.zeros((0, 4))
    out = pcsaft.mix_ln_phi_batch(mixtures, tables)
    kept = [i for i, t in enumerate(tables) if len(t) > 0]
    assert [o.shape for o in out] == [(len(tables[i]), len(mixtures[i])) for i in kept]
    assert all(isinstance(o, np.ndarray) and o.dtype == np.float64 for o in out)
    act = pcsaft.mix_ln_phi_batch(mixtures, tables, activity=True)
    for o, a, i in zip(out, act, kept):
        for row, arow, s in zip(o, a, tables[i]):
            assert np.array_equal(row, pcsaft.mix_ln_fugacity_coefficient(mixtures[i], s.tolist()))
            alone = pcsaft.mix_ln_fugacity_coefficient_pure(mixtures[i], s.tolist())
            assert np.array_equal(arow, row - alone, equal_nan=True)
    kij = [[0.0, 0.05], [0.05, 0.0]]
    with_k = pcsaft.mix_ln_phi_batch(mixtures[:1], tables[:1], kij=[kij])
    assert np.array_equal(with_k[0][1], pcsaft.mix_ln_fugacity_coefficient(mixtures[0], tables[0][1].tolist(),
                                                                            kij_matrix=kij))
    assert not np.array_equal(with_k[0][1], out[0][1])
    assert pcsaft.mix_ln_phi_batch(mixtures, [np.zeros((0, 4))] * len(mixtures)) == []
