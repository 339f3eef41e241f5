"""GPU tests of the saturation-line and critical-point kernels of csrc/gnx_pcsaft.hip (k_pcsaft_saturation,
k_pcsaft_critical_point) and of their Python forms, against the NumPy oracle of tests/pcsaft_sat_ref.py."""
import itertools

import numpy as np
import pytest
import torch

from tests import pcsaft_ref as R
from tests import pcsaft_sat_ref as S

pytestmark = pytest.mark.gpu

VP_TOL = 1e-8   # psat, rho_l, rho_v against the oracle: the tolerance of tests/test_pcsaft_gpu.py
# h and s against the oracle: a_T is exact arithmetic on the densities, so they get the densities' tolerance (the
# measured worst deviation is in the docstring of test_fixture_saturation_matches_the_oracle)
HS_TOL = 1e-8


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _saturation(rows, owner, T, dev):
    from gnnepcsaft_amd import pcsaft
    out = pcsaft.saturation(_dev(rows, dev), _dev(T, dev), _dev(owner, dev))
    return [t.cpu().numpy() for t in out]


def _vp(rows, owner, T, dev):
    from gnnepcsaft_amd import pcsaft
    return [t.cpu().numpy() for t in pcsaft.vapor_pressure(_dev(rows, dev), _dev(T, dev), _dev(owner, dev))]


def _critical(rows, dev):
    from gnnepcsaft_amd import pcsaft
    return [t.cpu().numpy() for t in pcsaft.critical_point(_dev(rows, dev))]


def _identity(T, values):
    """relative miss of s_lv = h_lv / T - R ln(rho_L / rho_V)"""
    _, rl, rv, hl, hv, sl, sv = values
    return np.abs((hv - hl) / T - R.RGAS * np.log(rl / rv) - (sv - sl)) / np.abs(sv - sl)


def _fixture_points():
    rows, pts = S.fixture_saturation()
    owner = np.array([p[0] for p in pts], dtype=np.int64)
    T = np.array([p[1] for p in pts], dtype=np.float64)
    ref = np.array([p[2] for p in pts], dtype=np.float64)   # [n, 7]
    return rows, owner, T, ref


def test_fixture_saturation_matches_the_oracle(gpu_device):
    """All 370 vapour-pressure points of the fixture in one launch: status and (psat, rho_l, rho_v) are
    ``vapor_pressure``'s, bit for bit; psat and densities match the oracle at 1e-8, h and s at HS_TOL; the saturation
    identity holds on the kernel's own outputs to 1e-10.  Measured on an MI355X: worst deviation from the oracle
    psat 4.7e-14, rho_l 1.3e-15, rho_v 4.7e-14, h_l 3.1e-15, h_v 5.5e-14, s_l 3.6e-15, s_v 5.9e-14; identity 5.8e-15."""
    rows, owner, T, ref = _fixture_points()
    assert len(T) == 370
    out = _saturation(rows, owner, T, gpu_device)
    vp = _vp(rows, owner, T, gpu_device)
    assert np.array_equal(out[7], vp[3]) and np.all(out[7] == 0)
    for a, b in zip(out[:3], vp[:3]):
        assert np.array_equal(a, b)
    dev = np.abs(np.stack(out[:7], axis=1) / ref - 1.0).max(axis=0)
    ident = _identity(T, out[:7]).max()
    print("worst relative deviation (psat, rho_l, rho_v, h_l, h_v, s_l, s_v)", dev.tolist(), "identity", ident)
    assert np.all(dev[:3] <= VP_TOL), dev
    assert np.all(dev[3:] <= HS_TOL), dev
    assert ident <= 1e-10


def test_clausius_clapeyron_ties_h_lv_to_the_vapor_pressure_kernel(gpu_device):
    """h_v - h_l of ``saturation`` against T (1 / rho_V - 1 / rho_L) dp_sat/dT with dp_sat/dT a central difference of
    ``vapor_pressure`` at T (1 +- 1e-4), to 2e-6 relative: the bound of the oracle's own check (four times the truncation
    error of the difference).  No oracle: this ties the new T-derivative to the kernel that was there before.  Measured on
    an MI355X: worst 5.1e-7."""
    rows, owner, T, _ = _fixture_points()
    out = _saturation(rows, owner, T, gpu_device)
    up, dn = _vp(rows, owner, T * (1.0 + 1e-4), gpu_device), _vp(rows, owner, T * (1.0 - 1e-4), gpu_device)
    assert np.all(out[7] == 0) and np.all(up[3] == 0) and np.all(dn[3] == 0)
    dpdt = (up[0] - dn[0]) / (2e-4 * T)
    h_lv = out[4] - out[3]
    miss = np.abs(T * (1.0 / out[2] - 1.0 / out[1]) * dpdt / h_lv - 1.0)
    print("Clausius-Clapeyron worst", miss.max())
    assert miss.max() <= 2e-6


def test_fixture_critical_points_match_the_oracle(gpu_device):
    """the 48 fixture molecules, methane and n-hexane: status 0 on every row (the two glycol ethers without a loop at
    0.2 eps/k among them), (Tc, Pc, rho_c) within the oracle's uncertainty, and ``vapor_pressure`` solves at Tc (1 - 2e-3)
    and reports supercritical at Tc (1 + 2e-3).  Measured on an MI355X: worst deviation (1.3e-11, 1.1e-10, 3.6e-9)
    against the bounds (1.9e-10, 1.4e-9, 3.1e-8)."""
    rows = np.array([m["params"] for m in S.molecules()] + [S.METHANE, S.HEXANE], dtype=np.float64)
    assert rows.shape == (50, 9)
    tc, pc, rc, st = _critical(rows, gpu_device)
    assert np.all(st == 0), st
    ref = np.array([S.critical_point_cached(tuple(r.tolist())) for r in rows], dtype=np.float64)
    dev = np.abs(np.stack([tc, pc, rc], axis=1) / ref - 1.0)
    print("worst relative deviation (Tc, Pc, rho_c)", dev.max(axis=0).tolist())
    assert np.all(dev <= np.array(S.CRIT_TOL_FIXTURE)), dev.max(axis=0)
    owner = np.arange(50, dtype=np.int64)
    assert np.all(_vp(rows, owner, tc * (1.0 - 2e-3), gpu_device)[3] == 0)
    above = _vp(rows, owner, tc * (1.0 + 2e-3), gpu_device)
    assert np.all(above[3] == 2) and np.all(above[0] == 0.0)


def test_random_rows_are_robust_and_match_the_oracle(gpu_device):
    """2000 rows of the generator of tests/test_pcsaft_gpu.py (seed 7).  Critical points: two calls give the same bits;
    every output is finite and positive with status 0 or exactly 0.0 with status 1; at most 5 % report status 1; a 40-row
    subsample (seed 7) matches the oracle within its uncertainty, a row left out only where the oracle's scan shows more
    than one unstable region at Tc (1 - 2e-3), at most 2 of the 40.  Saturation at 8 temperatures Tc x U(0.5, 0.98) per
    row: same bits twice, finite with status 0 or exactly 0.0, and the saturation identity to 1e-9 on every status-0
    point.  Measured on an MI355X: share of status 1 0.0 (Tc from 1.31 to 15.5 eps/k); subsample within (5.6e-11, 5.2e-10,
    3.5e-9) of the oracle, none left out; all 16000 saturation points status 0, identity worst 1.4e-13."""
    rows = S.random_rows(np.random.default_rng(7), 2000)
    a, b = _critical(rows, gpu_device), _critical(rows, gpu_device)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    tc, pc, rc, st = a
    ok = st == 0
    assert np.all((st == 0) | (st == 1))
    for v in (tc, pc, rc):
        assert np.all(np.isfinite(v[ok]) & (v[ok] > 0.0)) and np.all(v[~ok] == 0.0)
    share = float(np.mean(~ok))
    print("critical point: share of status 1", share, "Tc / (eps/k) from", (tc[ok] / rows[ok, 2]).min(), "to",
          (tc[ok] / rows[ok, 2]).max())
    assert share <= 0.05
    left_out, worst = 0, np.zeros(3)
    for i in np.random.default_rng(7).choice(2000, 40, replace=False):
        ref = S.critical_point_cached(tuple(rows[i].tolist()))
        got = np.array([tc[i], pc[i], rc[i]])
        dev = np.full(3, np.inf) if ref is None or st[i] != 0 else np.abs(got / np.array(ref) - 1.0)
        if np.all(dev <= np.array(S.CRIT_TOL_RANDOM)):
            worst = np.maximum(worst, dev)
            continue
        t_below = (tc[i] if st[i] == 0 else ref[0]) * (1.0 - 2e-3)
        assert R.unstable_regions(rows[i], t_below) > 1, (rows[i].tolist(), got.tolist(), st[i], ref)
        left_out += 1
    print("critical point: worst relative deviation of the subsample", worst.tolist(), "left out", left_out)
    assert left_out <= 2

    idx = np.nonzero(ok)[0]
    owner = np.repeat(idx, 8).astype(np.int64)
    T = tc[owner] * np.random.default_rng(11).uniform(0.5, 0.98, owner.size)
    s1, s2 = _saturation(rows, owner, T, gpu_device), _saturation(rows, owner, T, gpu_device)
    for x, y in zip(s1, s2):
        assert np.array_equal(x, y)
    good = s1[7] == 0
    for k, v in enumerate(s1[:7]):
        assert np.all(np.isfinite(v[good])) and np.all(v[~good] == 0.0)
        if k < 3:
            assert np.all(v[good] > 0.0)
    ident = _identity(T[good], [v[good] for v in s1[:7]])
    print("saturation: points", owner.size, "status counts", np.bincount(s1[7], minlength=4).tolist(), "identity worst",
          ident.max())
    assert ident.max() <= 1e-9


def test_edges(gpu_device):
    from gnnepcsaft_amd import ops, pcsaft
    dev = gpu_device
    rows = np.array([S.HEXANE, S.METHANE, [float("nan")] + S.HEXANE[1:]], dtype=np.float64)
    d_rows = _dev(rows, dev)
    # n = 0 and B = 0
    empty = pcsaft.saturation(d_rows, torch.empty(0, dtype=torch.float64, device=dev))
    assert len(empty) == 8 and all(t.numel() == 0 for t in empty) and empty[7].dtype == torch.int32
    empty = pcsaft.critical_point(torch.empty((0, 9), dtype=torch.float64, device=dev))
    assert len(empty) == 4 and all(t.numel() == 0 for t in empty)
    # owner outside [0, B), a NaN row, T >= Tc, a bad T
    tc = _critical(rows, dev)
    assert tc[3].tolist() == [0, 0, 3] and tc[0][2] == 0.0 and tc[1][2] == 0.0 and tc[2][2] == 0.0
    owner = np.array([-1, 3, 2, 0, 0, 0, 0], dtype=np.int64)
    T = np.array([300.0, 300.0, 300.0, tc[0][0], 600.0, -1.0, 300.0])
    out = _saturation(rows, owner, T, dev)
    assert out[7].tolist() == [3, 3, 3, 2, 2, 3, 0]
    for v in out[:7]:
        assert np.all(v[:6] == 0.0) and v[6] != 0.0 and np.isfinite(v[6])
    # every combination of NULL optional outputs, through the out= form
    owner, T = _dev(np.zeros(3, dtype=np.int64), dev), _dev(np.array([250.0, 400.0, 600.0]), dev)
    full = ops._pcsaft_saturation(d_rows, owner, T)
    for mask in itertools.product((False, True), repeat=7):
        bufs = [torch.full((3,), -7.0, dtype=torch.float64, device=dev) if m else None for m in mask]
        status = torch.full((3,), -7, dtype=torch.int32, device=dev)
        got = ops._pcsaft_saturation(d_rows, owner, T, out=(*bufs, status))
        assert torch.equal(got[7], full[7])
        for m, g, f in zip(mask, got[:7], full[:7]):
            assert (g is None) if not m else torch.equal(g, f)
    assert full[7].tolist() == [0, 0, 2]
    with pytest.raises(Exception):
        ops._pcsaft_saturation(d_rows, owner, T, out=(*full[:7], None))
    # the optional h_c, s_c of the critical-point entry equal the saturation entry's arithmetic at (Tc, rho_c): finite,
    # and the other four outputs do not depend on them
    B = rows.shape[0]
    bufs = [torch.empty(B, dtype=torch.float64, device=dev) for _ in range(5)]
    got = ops._pcsaft_critical_point(d_rows, out=(*bufs, torch.empty(B, dtype=torch.int32, device=dev)))
    for k, j in ((0, 0), (1, 1), (2, 2), (5, 3)):
        assert np.array_equal(got[k].cpu().numpy(), tc[j])
    hc, sc = got[3].cpu().numpy(), got[4].cpu().numpy()
    assert np.all(np.isfinite(hc[:2])) and np.all(hc[:2] < 0.0) and np.all(sc[:2] < 0.0) and hc[2] == 0.0 and sc[2] == 0.0
    h_ref, s_ref = S.h_s(S.HEXANE, tc[0][0], tc[2][0])
    assert abs(hc[0] / h_ref - 1.0) <= HS_TOL and abs(sc[0] / s_ref - 1.0) <= HS_TOL


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_tails(gpu_device, n):
    """n around the block size of 256: every point equals the same point of a one-row launch"""
    rows = np.array([S.HEXANE, S.METHANE], dtype=np.float64)
    owner = (np.arange(n) % 2).astype(np.int64)
    T = np.where(owner == 0, 300.0, 120.0) + (np.arange(n) % 7)
    out = _saturation(rows, owner, T, gpu_device)
    assert np.all(out[7] == 0)
    for j in (0, n - 1):
        one = _saturation(rows, owner[j:j + 1], T[j:j + 1], gpu_device)
        for a, b in zip(out, one):
            assert a[j] == b[0]
    many = np.tile(rows, ((n + 1) // 2, 1))[:n]
    c = _critical(many, gpu_device)
    one = _critical(rows, gpu_device)
    assert np.all(c[3] == 0)
    for a, b in zip(c, one):
        assert np.array_equal(a, np.tile(b, (n + 1) // 2)[:n])


def test_reference_shaped_forms(gpu_device):
    from gnnepcsaft_amd import pcsaft
    rows = np.array([S.HEXANE, S.METHANE], dtype=np.float64)
    tc, pc, rc, st = _critical(rows, gpu_device)
    assert pcsaft.critical_points(S.HEXANE) == [tc[0], pc[0], rc[0]]
    owner = np.array([0, 0, 1], dtype=np.int64)
    T = np.array([300.0, 450.0, 150.0])
    out = _saturation(rows, owner, T, gpu_device)
    assert pcsaft.pure_h_lv(S.HEXANE, [300.0]) == (out[4][0] - out[3][0]) / 1e3
    assert pcsaft.pure_s_lv(S.HEXANE, [300.0]) == out[6][0] - out[5][0]
    with pytest.raises(RuntimeError, match="critical temperature"):
        pcsaft.pure_h_lv(S.HEXANE, [600.0])
    with pytest.raises(RuntimeError):
        pcsaft.pure_s_lv(S.HEXANE, [tc[0]])
    states = [[[300.0, 1e5], [450.0, 1e5]], np.zeros((0, 2)), [[150.0, 1e5], [600.0, 1e5]]]
    h = pcsaft.h_lv_batch([S.HEXANE, S.HEXANE, S.METHANE], states)
    s = pcsaft.s_lv_batch([S.HEXANE, S.HEXANE, S.METHANE], states)
    assert [v.shape for v in h] == [(2,), (2,)] and [v.shape for v in s] == [(2,), (2,)]
    assert h[0].tolist() == ((out[4][:2] - out[3][:2]) / 1e3).tolist()
    assert h[1].tolist() == [(out[4][2] - out[3][2]) / 1e3, 0.0]
    assert s[0].tolist() == (out[6][:2] - out[5][:2]).tolist() and s[1].tolist() == [out[6][2] - out[5][2], 0.0]
    cp = pcsaft.critical_points_batch([S.HEXANE, [float("nan")] + S.HEXANE[1:], S.METHANE])
    assert cp.shape == (3, 3) and cp[0].tolist() == [tc[0], pc[0], rc[0]] and cp[2].tolist() == [tc[1], pc[1], rc[1]]
    assert cp[1].tolist() == [0.0, 0.0, 0.0]


def test_phase_diagram_of_hexane(gpu_device):
    from gnnepcsaft_amd import pcsaft
    d = pcsaft.phase_diagram(S.HEXANE, [300.0], points=20)
    assert tuple(d) == pcsaft.PHASE_DIAGRAM_KEYS and len(d) == 14
    assert all(len(v) == 20 for v in d.values())
    rows = np.array([S.HEXANE], dtype=np.float64)
    tc, pc, rc, st = _critical(rows, gpu_device)
    T = np.array(d["temperature"])
    assert T[0] == 300.0 and T[-1] == tc[0] and np.all(np.diff(T) > 0.0)
    assert np.array_equal(T[:-1], np.linspace(300.0, tc[0], 20)[:-1])
    rl, rv, P = np.array(d["density liquid"]), np.array(d["density vapor"]), np.array(d["pressure"])
    assert np.all(np.diff(rl) < 0.0) and np.all(np.diff(rv) > 0.0) and rl[-1] == rv[-1] == rc[0]
    assert np.all(np.diff(P) > 0.0) and P[-1] == pc[0]
    out = _saturation(rows, np.zeros(19, dtype=np.int64), T[:-1], gpu_device)
    mw = S.HEXANE[8] / 1e3
    assert np.all(out[7] == 0)
    for key, col in (("pressure", out[0]), ("density liquid", out[1]), ("density vapor", out[2]),
                     ("mass density liquid", out[1] * mw), ("mass density vapor", out[2] * mw),
                     ("molar enthalpy liquid", out[3] / 1e3), ("molar enthalpy vapor", out[4] / 1e3),
                     ("molar entropy liquid", out[5] / 1e3), ("molar entropy vapor", out[6] / 1e3),
                     ("specific enthalpy liquid", out[3] / 1e3 / mw), ("specific enthalpy vapor", out[4] / 1e3 / mw),
                     ("specific entropy liquid", out[5] / 1e3 / mw), ("specific entropy vapor", out[6] / 1e3 / mw)):
        assert d[key][:-1] == col.tolist(), key
    # both branches end in the one state (Tc, rho_c); along them h_v > h_l
    for what in ("molar enthalpy", "molar entropy", "specific enthalpy", "specific entropy"):
        assert d[what + " liquid"][-1] == d[what + " vapor"][-1]
    assert np.all(np.array(d["molar enthalpy vapor"][:-1]) > np.array(d["molar enthalpy liquid"][:-1]))
    h_ref, s_ref = S.h_s(S.HEXANE, tc[0], rc[0])
    assert abs(d["molar enthalpy liquid"][-1] * 1e3 / h_ref - 1.0) <= HS_TOL
    assert abs(d["molar entropy liquid"][-1] * 1e3 / s_ref - 1.0) <= HS_TOL
    with pytest.raises(ValueError, match="critical temperature"):
        pcsaft.phase_diagram(S.HEXANE, [600.0])
