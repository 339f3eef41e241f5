"""The oracle of the saturation properties and critical points (tests/pcsaft_sat_ref.py) pinned without a GPU, and the
host side of the Python forms (gnnepcsaft_amd/pcsaft.py ``critical_points``, ``pure_h_lv``, ``pure_s_lv``, ``h_lv_batch``,
``s_lv_batch``, ``critical_points_batch``, ``phase_diagram``) with the kernel calls replaced."""
import os
import re

import numpy as np
import pytest

from tests import pcsaft_ref as R
from tests import pcsaft_sat_ref as S
from tests.conftest import ROOT


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_binding_declares_the_saturation_entry_points():
    from gnnepcsaft_amd import _lib
    lib = _lib.load()  # binds every declared symbol of the built library; fails by name if one is missing
    assert lib.gnx_pcsaft_saturation is not None and lib.gnx_pcsaft_critical_point is not None
    header = open(os.path.join(ROOT, "include", "gnx.h")).read()
    for name, count in (("gnx_pcsaft_saturation", 14), ("gnx_pcsaft_critical_point", 9)):
        decl = re.search(r"int32_t %s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count, name
    assert _lib.ABI_VERSION == 7 and _lib.K_COUNT == 26 and lib.gnx_abi_version() == 7
    from gnnepcsaft_amd import ops, pcsaft
    assert callable(ops.pcsaft_saturation) and callable(ops.pcsaft_critical_point)
    for name in ("saturation", "critical_point", "critical_points", "pure_h_lv", "pure_s_lv", "h_lv_batch", "s_lv_batch",
                 "critical_points_batch", "phase_diagram"):
        assert callable(getattr(pcsaft, name)), name


def test_saturation_identity_and_clausius_clapeyron_on_the_fixture():
    """On every vapour-pressure point of the fixture the oracle solves: s_lv = h_lv / T - R ln(rho_L / rho_V) to 1e-12
    relative (measured: 370 points, worst 6.2e-15), and h_lv = T (1 / rho_V - 1 / rho_L) dp_sat/dT with dp_sat/dT a central
    difference of ``pcsaft_ref.vle`` at T (1 +- 1e-4), to 2e-6 relative (measured worst 5.1e-7, the truncation error of the
    difference; the bound is four times that)."""
    rows, pts = S.fixture_saturation()
    assert len(pts) == 370
    worst_id, worst_cc = 0.0, 0.0
    for i, T, (p, rl, rv, hl, hv, sl, sv) in pts:
        h_lv, s_lv = hv - hl, sv - sl
        worst_id = max(worst_id, abs(h_lv / T - R.RGAS * np.log(rl / rv) - s_lv) / abs(s_lv))
        up, dn = R.vle(rows[i], T * (1.0 + 1e-4)), R.vle(rows[i], T * (1.0 - 1e-4))
        assert up is not None and dn is not None, (rows[i].tolist(), T)
        dpdt = (up[0] - dn[0]) / (2e-4 * T)
        worst_cc = max(worst_cc, _rel(T * (1.0 / rv - 1.0 / rl) * dpdt, h_lv))
    print("points", len(pts), "identity worst", worst_id, "Clausius-Clapeyron worst", worst_cc)
    assert worst_id <= 1e-12 and worst_cc <= 2e-6


def test_methane_and_hexane_critical_points():
    for row, ref in ((S.METHANE, (191.4006, 4.67507e6, 9228.45)), (S.HEXANE, (519.334, 3.54272e6, 2654.14))):
        got = S.critical_point(row)
        assert got is not None
        print(row, got)
        for g, r in zip(got, ref):
            assert _rel(g, r) <= 1e-6, (row, got, ref)


def _stencil_spread(rows):
    worst = np.zeros(3)
    for row in rows:
        a, b = S.critical_point_cached(tuple(float(v) for v in row), 1e-3), S.critical_point(row, 3e-3)
        assert a is not None and b is not None, list(row)
        worst = np.maximum(worst, np.abs(np.array(a) / np.array(b) - 1.0))
    return worst


def test_critical_point_stencil_stability():
    """critical points at the stencil steps h = 1e-3 and h = 3e-3 agree.  The bounds are ten times the relative spread in
    (Tc, Pc, rho_c) first measured for such an oracle: fixture (48 molecules) (1.9e-11, 1.4e-10, 3.1e-9), 40 random rows
    (seed 7) (1.1e-10, 1.8e-9, 3.7e-9); this oracle measures (3.0e-11, 2.2e-10, 3.4e-9) and (1.3e-11, 1.7e-10, 3.9e-9).
    The bounds are also the oracle's uncertainty in the GPU test."""
    fixture = _stencil_spread([m["params"] for m in S.molecules()])
    random = _stencil_spread(S.random_rows(np.random.default_rng(7), 40))
    print("fixture", fixture, "random", random)
    assert np.all(fixture <= np.array(S.CRIT_TOL_FIXTURE)), fixture
    assert np.all(random <= np.array(S.CRIT_TOL_RANDOM)), random
    assert S.CRIT_TOL_FIXTURE == (1.9e-10, 1.4e-9, 3.1e-8) and S.CRIT_TOL_RANDOM == (1.1e-9, 1.8e-8, 3.7e-8)


def test_spinodals_exist_below_and_not_above_the_critical_temperature():
    for m in S.molecules():
        row = [float(v) for v in m["params"]]
        tc = S.critical_point_cached(tuple(row))[0]
        assert R.spinodals(row, tc * (1.0 - 2e-3)) is not None, row
        assert R.spinodals(row, tc * (1.0 + 2e-3)) is None, row


def test_a_bracket_from_below_misses_the_glycol_ethers():
    """the two fixture molecules without a loop on the scan at 0.2 eps/k, whose critical points the bracket from above
    finds (683 K and 824 K)"""
    named = {m["params"][4]: m["params"] for m in S.molecules()}
    for eab, tc in ((5000.0, 683.0), (3431.41122, 824.0)):
        row = [float(v) for v in named[eab]]
        assert R.spinodals(row, 0.2 * row[2]) is None
        assert abs(S.critical_point_cached(tuple(row))[0] - tc) < 1.0


# ---- the Python forms with the kernel calls replaced -----------------------------------------------------------------
HEX_TC, HEX_PC, HEX_DC, HEX_HC, HEX_SC = 519.334, 3.54272e6, 2654.14, -9000.0, -12.0


def _fake_saturation(params, owner, T):
    """a made-up smooth saturation line below 500 K per row scale params[:, 0]; status 2 at and above"""
    k = params[owner, 0]
    ok = T < 500.0
    cols = [k * T, 9000.0 - T, 1.0 + T / 100.0, -30000.0 + 10.0 * T, -100.0 - T, -60.0 + T / 50.0, -0.5 + T / 1e4]
    return [np.where(ok, c, 0.0) for c in cols], np.where(ok, 0, 2).astype(np.int32)


def _fake_critical(params, with_h_s=False):
    B = params.shape[0]
    bad = ~np.isfinite(params).all(axis=1)
    vals = [np.where(bad, 0.0, v * params[:, 0]) for v in (500.0, HEX_PC, HEX_DC)]
    hs = [np.full(B, HEX_HC), np.full(B, HEX_SC)] if with_h_s else [None, None]
    return vals + hs, np.where(bad, 3, 0).astype(np.int32)


@pytest.fixture
def fake(monkeypatch):
    from gnnepcsaft_amd import pcsaft
    calls = []

    def sat(params, owner, T):
        calls.append(("sat", owner.copy(), T.copy()))
        return _fake_saturation(params, owner, T)

    def crit(params, with_h_s=False):
        calls.append(("crit", params.copy(), with_h_s))
        return _fake_critical(params, with_h_s)

    monkeypatch.setattr(pcsaft, "_run_saturation", sat)
    monkeypatch.setattr(pcsaft, "_run_critical", crit)
    return calls


ROW1 = [1.0, 3.7, 150.0, 0.0, 0.0, 0.0, 0.0, 0.0, 50.0]
ROW2 = [2.0, 3.8, 250.0, 0.0, 0.0, 0.0, 0.0, 0.0, 80.0]


def test_single_forms_change_units_and_raise(fake):
    from gnnepcsaft_amd import pcsaft
    assert pcsaft.critical_points(ROW2) == [1000.0, 2.0 * HEX_PC, 2.0 * HEX_DC]
    assert pcsaft.pure_h_lv(ROW1, [300.0]) == ((-100.0 - 300.0) - (-30000.0 + 3000.0)) / 1e3
    assert pcsaft.pure_s_lv(ROW1, [300.0]) == (-0.5 + 0.03) - (-60.0 + 6.0)
    with pytest.raises(RuntimeError, match="critical temperature"):
        pcsaft.pure_h_lv(ROW1, [600.0])
    with pytest.raises(RuntimeError):
        pcsaft.pure_s_lv(ROW1, [500.0])
    with pytest.raises(RuntimeError, match="invalid"):
        pcsaft.critical_points([float("nan")] + ROW1[1:])
    with pytest.raises(ValueError):
        pcsaft.critical_points(ROW1[:8])


def test_batch_forms_split_at_the_table_cuts_in_one_call(fake):
    from gnnepcsaft_amd import pcsaft
    states = [[[300.0, 1e5], [600.0, 1e5]], np.zeros((0, 2)), [[400.0, 1e5]]]
    h = pcsaft.h_lv_batch([ROW1, ROW2, ROW2], states)
    assert len(fake) == 1 and fake[0][1].tolist() == [0, 0, 2] and fake[0][2].tolist() == [300.0, 600.0, 400.0]
    assert [v.tolist() for v in h] == [[(-400.0 + 27000.0) / 1e3, 0.0], [(-500.0 + 26000.0) / 1e3]]
    s = pcsaft.s_lv_batch([ROW1, ROW2, ROW2], states)
    assert len(fake) == 2 and [v.shape for v in s] == [(2,), (1,)] and s[0][1] == 0.0
    assert pcsaft.h_lv_batch([ROW1], [np.zeros((0, 2))]) == [] and len(fake) == 2
    with pytest.raises(ValueError):
        pcsaft.h_lv_batch([ROW1, ROW2], [states[0]])
    cp = pcsaft.critical_points_batch([ROW1, [float("nan")] + ROW1[1:], ROW2])
    assert cp.shape == (3, 3) and cp[1].tolist() == [0.0, 0.0, 0.0] and cp[2].tolist() == [1000.0, 2 * HEX_PC, 2 * HEX_DC]
    assert len(fake) == 3 and fake[2][0] == "crit" and fake[2][2] is False
    assert pcsaft.critical_points_batch([]).shape == (0, 3) and len(fake) == 3


def test_phase_diagram_keys_points_and_errors(fake):
    from gnnepcsaft_amd import pcsaft
    d = pcsaft.phase_diagram(ROW1, [300.0], points=5)
    assert tuple(d) == pcsaft.PHASE_DIAGRAM_KEYS and len(pcsaft.PHASE_DIAGRAM_KEYS) == 14
    assert set(d) == {"temperature", "pressure", "density liquid", "density vapor", "mass density liquid",
                      "mass density vapor", "molar enthalpy liquid", "molar enthalpy vapor", "molar entropy liquid",
                      "molar entropy vapor", "specific enthalpy liquid", "specific enthalpy vapor",
                      "specific entropy liquid", "specific entropy vapor"}
    assert all(len(v) == 5 for v in d.values())
    assert d["temperature"] == [300.0, 350.0, 400.0, 450.0, 500.0]
    assert [c[0] for c in fake] == ["crit", "sat"] and fake[0][2] is True and fake[1][2].tolist() == d["temperature"][:-1]
    # the critical point closes both branches
    assert d["pressure"][-1] == HEX_PC and d["density liquid"][-1] == d["density vapor"][-1] == HEX_DC
    assert d["molar enthalpy liquid"][-1] == d["molar enthalpy vapor"][-1] == HEX_HC / 1e3
    assert d["molar entropy liquid"][-1] == d["molar entropy vapor"][-1] == HEX_SC / 1e3
    # units: mw = 50 g/mol
    assert d["density liquid"][0] == 8700.0 and d["mass density liquid"][0] == 8700.0 * 0.05
    assert d["molar enthalpy vapor"][0] == -0.4 and d["specific enthalpy vapor"][0] == -0.4 / 0.05
    assert d["molar entropy liquid"][0] == -54.0 / 1e3 and d["specific entropy liquid"][0] == -54.0 / 1e3 / 0.05
    with pytest.raises(ValueError, match="critical temperature"):
        pcsaft.phase_diagram(ROW1, [500.0])
    with pytest.raises(ValueError, match="critical temperature"):
        pcsaft.phase_diagram(ROW1, [700.0])
    with pytest.raises(ValueError, match="at least 2 points"):
        pcsaft.phase_diagram(ROW1, [300.0], points=1)
    with pytest.raises(ValueError, match="no critical point"):
        pcsaft.phase_diagram([float("nan")] + ROW1[1:], [300.0])


def test_phase_diagram_drops_failed_points_and_raises_when_none_is_left(monkeypatch, fake):
    from gnnepcsaft_amd import pcsaft

    def sat(params, owner, T):
        values, status = _fake_saturation(params, owner, T)
        status[1] = 1
        return [np.where(status == 0, v, 0.0) for v in values], status

    monkeypatch.setattr(pcsaft, "_run_saturation", sat)
    d = pcsaft.phase_diagram(ROW1, [300.0], points=5)
    assert d["temperature"] == [300.0, 400.0, 450.0, 500.0] and all(len(v) == 4 for v in d.values())
    monkeypatch.setattr(pcsaft, "_run_saturation",
                        lambda p, o, T: ([np.zeros(T.shape[0])] * 7, np.ones(T.shape[0], dtype=np.int32)))
    with pytest.raises(ValueError, match="No VLE"):
        pcsaft.phase_diagram(ROW1, [300.0], points=5)
