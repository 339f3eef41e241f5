"""Times the PC-SAFT kernels of csrc/gnx_pcsaft.hip: 1e3 / 1e5 / 1e6 points per call for the liquid
density and the vapour pressure, kernel time (events around the launch) and end-to-end ``rho_batch`` / ``vp_batch``
time (upload, launch, download), next to the CPU oracle (tests/pcsaft_ref.py) timed on a sample of the same points and
scaled to the call size.  Points: the ThermoML fixture's molecules and states, repeated.

With ``--mixture`` it times the mixture kernels of csrc/gnx_pcsaft_mix.hip and csrc/gnx_pcsaft_mix_phi.hip (DESIGN.md
§4c) instead, on the points of the binary ThermoML fixture, repeated: the density and the state kernel, the fugacity
kernel on the same points (without and with the pure-component values, and its state form), ``mix_rho_batch`` end to
end, and the mixture oracle (tests/pcsaft_mix_ref.py) on a sample.

With ``--bubble`` it times the bubble-point kernel of csrc/gnx_pcsaft_mix_vle.hip on the six named systems of
tests/pcsaft_mix_vle_ref.py and the first point of each system of the binary fixture, repeated, and that module's oracle
solve on a sample.  The launch has no kernel id, so the events around the call are the only timing there is.

With ``--dew`` it times the dew-point kernel of csrc/gnx_pcsaft_mix_dew.hip on the vapours of those bubble points (the y
the bubble kernel reports for them), repeated, the bubble-point kernel on the liquids of the same points in the same run
for the ratio, and the oracle of tests/pcsaft_mix_dew_ref.py on a sample.

With ``--flash`` it times the (T, P) flash kernel of csrc/gnx_pcsaft_mix_flash.hip on the tie-line feeds of
tests/pcsaft_mix_flash_ref.py (the six named bubble points at beta = 0.3, six fixture points at beta = 0.5), repeated, the
bubble-point kernel on the liquids of the same tie lines for the ratio, and that module's oracle flash on a sample.

With ``--stability`` it times the tangent-plane stability test of csrc/gnx_pcsaft_mix_stab.hip through
``pcsaft.mixture_stability`` (nc + 2 = 6 trial rows per point) on the 43 cases of tests/pcsaft_mix_stab_ref.py, repeated,
the flash kernel on the 12 tie-line feeds among them in the same run, and that module's oracle on a sample.

With ``--lle`` it times the liquid-liquid flash of csrc/gnx_pcsaft_mix_lle.hip through ``pcsaft.mixture_lle_flash`` with
the stability start (two launches) on the 11 points of tests/pcsaft_mix_lle_ref.py that split, repeated; in the same run
the kernel alone from the pinned w0, ``mixture_stability`` on the same points, ``mixture_tp_flash`` and
``mixture_lle_flash`` on the three vapour-liquid feeds among them, and that module's oracle loop on a sample.

With ``--bubble-t`` / ``--dew-t`` it times the bubble- / dew-temperature kernel of csrc/gnx_pcsaft_mix_tvle.hip on the
inverse problems of those 30 bubble points (the P and y the bubble kernel reports for them), repeated, from its own start
and from T0 = 0.9 T, the bubble- / dew-pressure kernel on the same points in the same run for the ratio, and the oracle of
tests/pcsaft_mix_tvle_ref.py on a sample.

With ``--kij`` it times the k_ij fit of csrc/gnx_pcsaft_kij.hip on butane + hexane at the four states of
tests/test_pcsaft_kij_gpu.py, replicated to ``--systems`` binaries, with the reference's 50 trial feeds: one iteration of
``pcsaft.fit_kij`` (the row launch, the sums launch and the download, wall time), the route there was before it for the same
work in the same run (2 S calls of ``pcsaft.mix_flash_x1``; at most ``--route-calls`` of them are timed and the rest
scaled, the calls being equal and sequential), and a whole fit of data planted at k_12 = 0.05.

With ``--saturation`` it times the saturation kernel of csrc/gnx_pcsaft.hip (``pcsaft.saturation``: the vapour-pressure
solve, then the residual enthalpy and entropy of both phases) on the vapour-pressure points of the ThermoML fixture,
repeated, the vapour-pressure kernel on the same points in the same run for the ratio, ``h_lv_batch`` end to end, and the
oracle of tests/pcsaft_sat_ref.py on a sample.

With ``--critical`` it times the critical-point kernel (``pcsaft.critical_point``, one lane per parameter row) on the
fixture's rows, repeated to each size, ``critical_points_batch`` end to end, and that oracle on a sample.

Usage: python tools/pcsaft_bench.py [--mixture | --bubble | --dew | --bubble-t | --dew-t | --flash | --stability | --lle | --kij | --saturation | --critical] [--reps 3] [--sizes 1000,100000,1000000] [--oracle-sample 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnnepcsaft_amd import pcsaft  # noqa: E402
from tests import pcsaft_ref as R  # noqa: E402


REPS = 3


def _kernel_ms(fn, reps=None):
    reps = REPS if reps is None else reps
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def _mixture(args, dev):
    from tests import pcsaft_mix_cases as C
    from tests import pcsaft_mix_ref as MR
    params, comp, owner, T, P, x, _ = C.fixture_points()
    t0 = time.perf_counter()
    step = max(1, len(owner) // args.oracle_sample)
    sample = range(0, len(owner), step)
    ref = [MR.density(MR.Mixture(params[comp[owner[j]]], x[j]), T[j], P[j]) for j in sample]
    oracle = (time.perf_counter() - t0) / len(ref)
    d_params, d_comp = torch.from_numpy(params).to(dev), torch.from_numpy(comp).to(dev)
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % len(owner)
        o, t, pp, xx = (torch.from_numpy(np.ascontiguousarray(a[idx])).to(dev) for a in (owner, T, P, x))
        rho, _ = pcsaft.mixture_density(d_params, d_comp, xx, t, pp, o)
        k_rho = _kernel_ms(lambda: pcsaft.mixture_density(d_params, d_comp, xx, t, pp, o))
        k_state = _kernel_ms(lambda: pcsaft.mixture_state(d_params, d_comp, xx, t, rho, o))
        k_phi = _kernel_ms(lambda: pcsaft.mixture_ln_phi(d_params, d_comp, xx, t, pp, o))
        k_phi_pure = _kernel_ms(lambda: pcsaft.mixture_ln_phi(d_params, d_comp, xx, t, pp, o, pure=True))
        k_phi_state = _kernel_ms(lambda: pcsaft.mixture_ln_phi_state(d_params, d_comp, xx, t, rho, o))
        mixtures = [s["params"] for s in C.systems()]
        tables = [np.column_stack([T[idx][owner[idx] == i], P[idx][owner[idx] == i], x[idx][owner[idx] == i]])
                  for i in range(len(mixtures))]
        pcsaft.mix_rho_batch(mixtures, tables)
        t0 = time.perf_counter()
        pcsaft.mix_rho_batch(mixtures, tables)
        rec = dict(points=n, mix_density_kernel_ms=k_rho, mix_state_kernel_ms=k_state, mix_ln_phi_kernel_ms=k_phi,
                   mix_ln_phi_pure_kernel_ms=k_phi_pure, mix_ln_phi_state_kernel_ms=k_phi_state,
                   mix_density_points_per_s=n / k_rho * 1e3, mix_ln_phi_points_per_s=n / k_phi * 1e3,
                   mix_rho_batch_ms=(time.perf_counter() - t0) * 1e3, oracle_density_ms_est=oracle * n * 1e3)
        print(json.dumps(rec))
        res.append(rec)
    return res


def _bubble(args, dev):
    from tests import pcsaft_mix_vle_ref as V
    cases = list(V.NAMED) + V.fixture_cases()
    params, comp, T, x = [], np.full((len(cases), 4), -1, dtype=np.int64), [], np.zeros((len(cases), 4))
    for i, (_, rows, t, xi) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        x[i, :len(rows)] = xi
        T.append(t)
    T = np.array(T)
    step = max(1, len(cases) // args.oracle_sample)
    t0 = time.perf_counter()
    sols = [V.bubble(rows, xi, t, max_iterations=100) for _, rows, t, xi in cases[::step]]
    oracle = (time.perf_counter() - t0) / len(sols)
    d_params, d_comp = torch.from_numpy(np.array(params)).to(dev), torch.from_numpy(comp).to(dev)
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % len(cases)
        o, t, xx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (idx.astype(np.int64), T[idx], x[idx]))
        k = _kernel_ms(lambda: pcsaft.mixture_bubble_pressure(d_params, d_comp, xx, t, o))
        st = pcsaft.mixture_bubble_pressure(d_params, d_comp, xx, t, o)[4]
        rec = dict(points=n, mix_bubble_kernel_ms=k, mix_bubble_points_per_s=n / k * 1e3,
                   failed_points=int((st != 0).sum().item()), oracle_bubble_ms_est=oracle * n * 1e3)
        print(json.dumps(rec))
        res.append(rec)
    return res


def _dew(args, dev):
    from tests import pcsaft_mix_dew_ref as D
    from tests import pcsaft_mix_vle_ref as V
    cases = list(V.NAMED) + V.fixture_cases()
    params, comp, T, x = [], np.full((len(cases), 4), -1, dtype=np.int64), [], np.zeros((len(cases), 4))
    for i, (_, rows, t, xi) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        x[i, :len(rows)] = xi
        T.append(t)
    T = np.array(T)
    d_params, d_comp = torch.from_numpy(np.array(params)).to(dev), torch.from_numpy(comp).to(dev)
    every = torch.arange(len(cases), dtype=torch.int64, device=dev)
    _, y, _, _, st = pcsaft.mixture_bubble_pressure(d_params, d_comp, torch.from_numpy(x).to(dev),
                                                   torch.from_numpy(T).to(dev), every)
    assert int((st != 0).sum().item()) == 0, "a bubble point failed: no vapour to start from"
    y = torch.nan_to_num(y).cpu().numpy()
    step = max(1, len(cases) // args.oracle_sample)
    t0 = time.perf_counter()
    sols = [D.dew(rows, y[j, :len(rows)], t) for j, (_, rows, t, _) in list(enumerate(cases))[::step]]
    oracle = (time.perf_counter() - t0) / len(sols)
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % len(cases)
        o, t, xx, yy = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                        for a in (idx.astype(np.int64), T[idx], x[idx], y[idx]))
        k = _kernel_ms(lambda: pcsaft.mixture_dew_pressure(d_params, d_comp, yy, t, o))
        st = pcsaft.mixture_dew_pressure(d_params, d_comp, yy, t, o)[4]
        kb = _kernel_ms(lambda: pcsaft.mixture_bubble_pressure(d_params, d_comp, xx, t, o))
        rec = dict(points=n, mix_dew_kernel_ms=k, mix_dew_points_per_s=n / k * 1e3,
                   failed_points=int((st != 0).sum().item()), mix_bubble_same_points_kernel_ms=kb, dew_over_bubble=k / kb,
                   oracle_dew_ms_est=oracle * n * 1e3)
        print(json.dumps(rec), flush=True)
        res.append(rec)
    return res


def _tvle(args, dev):
    """--bubble-t / --dew-t: the temperature kernels on the inverse problems of the 30 bubble points (P and y are what the
    bubble-pressure kernel reports for them), beside the pressure kernel of the same kind on the same points"""
    from tests import pcsaft_mix_tvle_ref as TR
    from tests import pcsaft_mix_vle_ref as V
    dew = args.dew_t
    cases = list(V.NAMED) + V.fixture_cases()
    params, comp, T, x = [], np.full((len(cases), 4), -1, dtype=np.int64), [], np.zeros((len(cases), 4))
    for i, (_, rows, t, xi) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        x[i, :len(rows)] = xi
        T.append(t)
    T = np.array(T)
    d_params, d_comp = torch.from_numpy(np.array(params)).to(dev), torch.from_numpy(comp).to(dev)
    every = torch.arange(len(cases), dtype=torch.int64, device=dev)
    P, y, _, _, st = pcsaft.mixture_bubble_pressure(d_params, d_comp, torch.from_numpy(x).to(dev),
                                                   torch.from_numpy(T).to(dev), every)
    assert int((st != 0).sum().item()) == 0, "a bubble point failed: no pressure to start from"
    P, y = P.cpu().numpy(), torch.nan_to_num(y).cpu().numpy()
    z = y if dew else x
    step = max(1, len(cases) // args.oracle_sample)
    t0 = time.perf_counter()
    sols = [TR.solve(rows, z[j, :len(rows)], P[j], dew=dew) for j, (_, rows, _, _) in list(enumerate(cases))[::step]]
    oracle = (time.perf_counter() - t0) / len(sols)
    name = "dew" if dew else "bubble"
    solve = pcsaft.mixture_dew_temperature if dew else pcsaft.mixture_bubble_temperature
    forward = pcsaft.mixture_dew_pressure if dew else pcsaft.mixture_bubble_pressure
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % len(cases)
        o, t, pp, zz = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                        for a in (idx.astype(np.int64), T[idx], P[idx], z[idx]))
        k = _kernel_ms(lambda: solve(d_params, d_comp, zz, pp, o))
        st = solve(d_params, d_comp, zz, pp, o)[4]
        kg = _kernel_ms(lambda: solve(d_params, d_comp, zz, pp, o, T0=0.9 * t))
        stg = solve(d_params, d_comp, zz, pp, o, T0=0.9 * t)[4]
        kf = _kernel_ms(lambda: forward(d_params, d_comp, zz, t, o))
        rec = {"points": n, f"mix_{name}_t_kernel_ms": k, f"mix_{name}_t_points_per_s": n / k * 1e3,
               "failed_points": int((st != 0).sum().item()), f"mix_{name}_t_from_0.9T_kernel_ms": kg,
               "failed_points_from_0.9T": int((stg != 0).sum().item()), f"mix_{name}_pressure_same_points_kernel_ms": kf,
               "temperature_over_pressure": k / kf, f"oracle_{name}_t_ms_est": oracle * n * 1e3}
        print(json.dumps(rec), flush=True)
        res.append(rec)
    return res


def _flash(args, dev):
    from tests import pcsaft_mix_flash_ref as F
    points = F.tie_line_points()
    params, comp = [], np.full((len(points), 4), -1, dtype=np.int64)
    z, x = np.zeros((len(points), 4)), np.zeros((len(points), 4))
    for i, (_, rows, _, _, zi, xi, _, _) in enumerate(points):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        z[i, :len(rows)], x[i, :len(rows)] = zi, xi
    T, P = np.array([p[2] for p in points]), np.array([p[3] for p in points])
    step = max(1, len(points) // args.oracle_sample)
    t0 = time.perf_counter()
    sols = [F.flash(rows, zi, t, p) for _, rows, t, p, zi, _, _, _ in points[::step]]
    oracle = (time.perf_counter() - t0) / len(sols)
    d_params, d_comp = torch.from_numpy(np.array(params)).to(dev), torch.from_numpy(comp).to(dev)
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % len(points)
        o, t, pp, zz, xx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                            for a in (idx.astype(np.int64), T[idx], P[idx], z[idx], x[idx]))
        k = _kernel_ms(lambda: pcsaft.mixture_tp_flash(d_params, d_comp, zz, t, pp, o))
        st = pcsaft.mixture_tp_flash(d_params, d_comp, zz, t, pp, o)[5]
        kb = _kernel_ms(lambda: pcsaft.mixture_bubble_pressure(d_params, d_comp, xx, t, o))
        rec = dict(points=n, mix_flash_kernel_ms=k, mix_flash_points_per_s=n / k * 1e3,
                   failed_points=int((st != 0).sum().item()), mix_bubble_same_tie_lines_kernel_ms=kb,
                   flash_over_bubble=k / kb, oracle_flash_ms_est=oracle * n * 1e3)
        print(json.dumps(rec), flush=True)
        res.append(rec)
    return res


def _stability(args, dev):
    from tests import pcsaft_mix_stab_ref as S
    cases = S.cases()
    params, comp, z = [], np.full((len(cases), 4), -1, dtype=np.int64), np.zeros((len(cases), 4))
    for i, (_, _, rows, _, _, zi, _) in enumerate(cases):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        z[i, :len(rows)] = zi
    T, P = np.array([c[3] for c in cases]), np.array([c[4] for c in cases])
    expected = np.array([c[6] for c in cases])
    tie = [i for i, c in enumerate(cases) if c[0] == "tie line"]
    step = max(1, len(cases) // args.oracle_sample)
    t0 = time.perf_counter()
    sols = [S.stability(rows, zi, t, p) for _, _, rows, t, p, zi, _ in cases[::step]]
    oracle = (time.perf_counter() - t0) / len(sols)
    d_params, d_comp = torch.from_numpy(np.array(params)).to(dev), torch.from_numpy(comp).to(dev)
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % len(cases)
        o, t, pp, zz = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (idx.astype(np.int64), T[idx], P[idx], z[idx]))
        k = _kernel_ms(lambda: pcsaft.mixture_stability(d_params, d_comp, zz, t, pp, o))
        stable, _, _, st = pcsaft.mixture_stability(d_params, d_comp, zz, t, pp, o)
        wrong = int((stable.cpu().numpy() != expected[idx]).sum())
        fidx = np.array(tie)[np.arange(n) % len(tie)]
        fo, ft, fp, fz = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                          for a in (fidx.astype(np.int64), T[fidx], P[fidx], z[fidx]))
        kf = _kernel_ms(lambda: pcsaft.mixture_tp_flash(d_params, d_comp, fz, ft, fp, fo))
        rec = dict(points=n, rows=6 * n, mix_stability_ms=k, mix_stability_points_per_s=n / k * 1e3,
                   inconclusive_points=int((st != 0).sum().item()), wrong_verdicts=wrong,
                   mix_flash_tie_line_feeds_kernel_ms=kf, stability_over_flash=k / kf, oracle_stability_ms_est=oracle * n * 1e3)
        print(json.dumps(rec), flush=True)
        res.append(rec)
    return res


def _lle(args, dev):
    from tests import pcsaft_mix_lle_ref as L
    points = [p for p in L.points() if p[0] in ("liquid-liquid", "vapour-liquid")]
    params, comp = [], np.full((len(points), 4), -1, dtype=np.int64)
    z, w0 = np.zeros((len(points), 4)), np.zeros((len(points), 4))
    for i, (_, _, rows, _, _, zi, wi) in enumerate(points):
        comp[i, :len(rows)] = np.arange(len(params), len(params) + len(rows))
        params.extend(np.asarray(rows, dtype=np.float64).tolist())
        z[i, :len(rows)], w0[i, :len(rows)] = zi, wi
    T, P = np.array([p[3] for p in points]), np.array([p[4] for p in points])
    vle = [i for i, p in enumerate(points) if p[0] == "vapour-liquid"]
    step = max(1, len(points) // args.oracle_sample)
    t0 = time.perf_counter()
    sols = [L.lle(rows, zi, wi, t, p) for _, _, rows, t, p, zi, wi in points[::step]]
    oracle = (time.perf_counter() - t0) / len(sols)
    d_params, d_comp = torch.from_numpy(np.array(params)).to(dev), torch.from_numpy(comp).to(dev)
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = np.arange(n) % len(points)
        o, t, pp, zz, ww = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                            for a in (idx.astype(np.int64), T[idx], P[idx], z[idx], w0[idx]))
        k = _kernel_ms(lambda: pcsaft.mixture_lle_flash(d_params, d_comp, zz, t, pp, o))
        st = pcsaft.mixture_lle_flash(d_params, d_comp, zz, t, pp, o)[5]
        kw = _kernel_ms(lambda: pcsaft.mixture_lle_flash(d_params, d_comp, zz, t, pp, o, w0=ww))
        ks = _kernel_ms(lambda: pcsaft.mixture_stability(d_params, d_comp, zz, t, pp, o))
        fidx = np.array(vle)[np.arange(n) % len(vle)]
        fo, ft, fp, fz = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                          for a in (fidx.astype(np.int64), T[fidx], P[fidx], z[fidx]))
        kf = _kernel_ms(lambda: pcsaft.mixture_tp_flash(d_params, d_comp, fz, ft, fp, fo))
        kl = _kernel_ms(lambda: pcsaft.mixture_lle_flash(d_params, d_comp, fz, ft, fp, fo))
        rec = dict(points=n, mix_lle_ms=k, mix_lle_points_per_s=n / k * 1e3, failed_points=int((st != 0).sum().item()),
                   mix_lle_given_w0_kernel_ms=kw, mix_stability_same_points_ms=ks, lle_over_stability=k / ks,
                   lle_kernel_over_stability=kw / ks, mix_flash_vapour_liquid_feeds_kernel_ms=kf,
                   mix_lle_vapour_liquid_feeds_ms=kl, lle_over_flash_vapour_liquid_feeds=kl / kf,
                   oracle_lle_ms_est=oracle * n * 1e3)
        print(json.dumps(rec), flush=True)
        res.append(rec)
    return res


def _kij(args, dev):
    from tests import pcsaft_mix_vle_ref as V
    rows = [V.BUTANE, V.HEXANE]
    states = np.array([(350.0, 3e5), (350.0, 4e5), (350.0, 5e5), (330.0, 2.5e5)])
    feeds = np.linspace(1e-5, 0.99, 50)
    h, k0, k_star = 1e-5, 0.2, 0.05
    kmat = lambda k: [[0.0, k], [k, 0.0]]  # noqa: E731
    data = pcsaft.mix_flash_x1(rows, states, feeds, kij_matrix=kmat(k_star))
    res = []
    for S in [int(s) for s in args.systems.split(",")]:
        systems = [(rows, states[:, 0], states[:, 1], data)] * S
        evaluate, _ = pcsaft._kij_evaluator(systems, feeds, h)
        index, k = np.arange(S, dtype=np.int64), np.full(S, k0)
        evaluate(index, k)
        torch.cuda.synchronize()
        it_ms = float("inf")
        for _ in range(REPS):
            t0 = time.perf_counter()
            evaluate(index, k)
            it_ms = min(it_ms, (time.perf_counter() - t0) * 1e3)
        calls = min(2 * S, args.route_calls)
        pcsaft.mix_flash_x1(rows, states, feeds, kij_matrix=kmat(k0))
        t0 = time.perf_counter()
        for c in range(calls):
            pcsaft.mix_flash_x1(rows, states, feeds, kij_matrix=kmat(k0 + h * (c % 2)))
        route_ms = (time.perf_counter() - t0) * 1e3 / calls * 2 * S
        t0 = time.perf_counter()
        fit = pcsaft.fit_kij(systems, n=50, k0=k0, diff_step=h)
        fit_ms = (time.perf_counter() - t0) * 1e3
        rec = dict(systems=S, states=len(states), feeds=len(feeds), rows_per_launch=2 * S * len(states),
                   kij_iteration_ms=it_ms, flash_x1_route_ms=route_ms, flash_x1_route_calls_timed=calls,
                   route_over_iteration=route_ms / it_ms, kij_fit_ms=fit_ms, fit_iterations=int(fit["iterations"].max()),
                   fit_worst_k_error=float(np.max(np.abs(fit["k_12"] - k_star))),
                   fit_reasons=sorted(set(fit["reason"].tolist())))
        print(json.dumps(rec), flush=True)
        res.append(rec)
    return res


def _fixture_rows():
    mols = json.load(open(os.path.join(ROOT, "tests", "golden", "pcsaft_thermoml.json")))["molecules"]
    rows = np.array([m["params"] for m in mols], dtype=np.float64)
    vp_pts = np.array([(i, s[0]) for i, m in enumerate(mols) for s in m["vp"]])
    return rows, vp_pts


def _saturation(args, dev):
    from tests import pcsaft_sat_ref as S
    rows, vp_pts = _fixture_rows()
    d_rows = torch.from_numpy(rows).to(dev)
    t0 = time.perf_counter()
    for i, T in vp_pts[:args.oracle_sample]:
        S.saturation(rows[int(i)], T)
    oracle = (time.perf_counter() - t0) / args.oracle_sample
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        pv = vp_pts[np.arange(n) % len(vp_pts)]
        owner = torch.from_numpy(pv[:, 0].astype(np.int64)).to(dev)
        T = torch.from_numpy(pv[:, 1].copy()).to(dev)
        k_sat = _kernel_ms(lambda: pcsaft.saturation(d_rows, T, owner))
        k_vp = _kernel_ms(lambda: pcsaft.vapor_pressure(d_rows, T, owner))
        tabs = [np.column_stack([pv[pv[:, 0] == i][:, 1], np.ones(int(np.sum(pv[:, 0] == i)))]) for i in range(len(rows))]
        pcsaft.h_lv_batch(rows.tolist(), tabs)
        t0 = time.perf_counter()
        pcsaft.h_lv_batch(rows.tolist(), tabs)
        rec = dict(points=n, saturation_kernel_ms=k_sat, vp_kernel_ms=k_vp, ratio=k_sat / k_vp,
                   h_lv_batch_ms=(time.perf_counter() - t0) * 1e3, oracle_ms_est=oracle * n * 1e3)
        print(json.dumps(rec))
        res.append(rec)
    return res


def _critical(args, dev):
    from tests import pcsaft_sat_ref as S
    rows, _ = _fixture_rows()
    t0 = time.perf_counter()
    for row in rows[:args.oracle_sample]:
        S.critical_point(row)
    oracle = (time.perf_counter() - t0) / min(args.oracle_sample, len(rows))
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        many = rows[np.arange(n) % len(rows)]
        d_rows = torch.from_numpy(many).to(dev)
        k_crit = _kernel_ms(lambda: pcsaft.critical_point(d_rows))
        status = pcsaft.critical_point(d_rows)[3]
        pcsaft.critical_points_batch(many)
        t0 = time.perf_counter()
        pcsaft.critical_points_batch(many)
        rec = dict(rows=n, critical_kernel_ms=k_crit, critical_points_batch_ms=(time.perf_counter() - t0) * 1e3,
                   failed=int((status != 0).sum().item()), oracle_ms_est=oracle * n * 1e3)
        print(json.dumps(rec))
        res.append(rec)
    return res


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,100000,1000000")
    ap.add_argument("--oracle-sample", type=int, default=20)
    ap.add_argument("--mixture", action="store_true")
    ap.add_argument("--bubble", action="store_true")
    ap.add_argument("--dew", action="store_true")
    ap.add_argument("--flash", action="store_true")
    ap.add_argument("--stability", action="store_true")
    ap.add_argument("--lle", action="store_true")
    ap.add_argument("--bubble-t", action="store_true")
    ap.add_argument("--dew-t", action="store_true")
    ap.add_argument("--kij", action="store_true")
    ap.add_argument("--saturation", action="store_true")
    ap.add_argument("--critical", action="store_true")
    ap.add_argument("--systems", default="1,64,1024", help="--kij: binaries per fit")
    ap.add_argument("--route-calls", type=int, default=16, help="--kij: mix_flash_x1 calls timed, of the 2 S of the old route")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions per kernel, the best of which counts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    REPS = args.reps
    if args.mixture or args.bubble or args.dew or args.flash or args.stability or args.lle or args.bubble_t or args.dew_t or args.kij or args.saturation or args.critical:
        dev = torch.device("cuda", torch.cuda.current_device())
        res = (_saturation if args.saturation else _critical if args.critical else _kij if args.kij else _tvle if args.bubble_t or args.dew_t else _lle if args.lle else _stability if args.stability else _flash if args.flash else _dew if args.dew else _bubble if args.bubble else _mixture)(args, dev)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(dict(device=torch.cuda.get_device_name(dev), oracle_sample=args.oracle_sample, results=res), fh,
                          indent=1)
        return
    mols = json.load(open(os.path.join(ROOT, "tests", "golden", "pcsaft_thermoml.json")))["molecules"]
    rows = np.array([m["params"] for m in mols])
    rho_pts = np.array([(i, s[0], s[1]) for i, m in enumerate(mols) for s in m["rho"]])
    vp_pts = np.array([(i, s[0]) for i, m in enumerate(mols) for s in m["vp"]])
    dev = torch.device("cuda", torch.cuda.current_device())
    d_rows = torch.from_numpy(rows).to(dev)
    # CPU oracle per point, on a sample
    t0 = time.perf_counter()
    for i, T, P in rho_pts[:args.oracle_sample]:
        R.density(rows[int(i)], T, P)
    oracle_rho = (time.perf_counter() - t0) / args.oracle_sample
    t0 = time.perf_counter()
    for i, T in vp_pts[:args.oracle_sample]:
        R.vle(rows[int(i)], T)
    oracle_vp = (time.perf_counter() - t0) / args.oracle_sample
    res = []
    for n in [int(s) for s in args.sizes.split(",")]:
        pr = rho_pts[np.arange(n) % len(rho_pts)]
        pv = vp_pts[np.arange(n) % len(vp_pts)]
        o_r = torch.from_numpy(pr[:, 0].astype(np.int64)).to(dev)
        T_r, P_r = torch.from_numpy(pr[:, 1].copy()).to(dev), torch.from_numpy(pr[:, 2].copy()).to(dev)
        o_v = torch.from_numpy(pv[:, 0].astype(np.int64)).to(dev)
        T_v = torch.from_numpy(pv[:, 1].copy()).to(dev)
        k_rho = _kernel_ms(lambda: pcsaft.density(d_rows, T_r, P_r, o_r))
        k_vp = _kernel_ms(lambda: pcsaft.vapor_pressure(d_rows, T_v, o_v))
        # end to end through the reference-shaped call: one table per molecule
        params = rows.tolist()
        tab_r = [np.zeros((0, 5))] * len(rows)
        tab_v = [np.zeros((0, 5))] * len(rows)
        for i in range(len(rows)):
            sel = pr[pr[:, 0] == i]
            tab_r[i] = np.column_stack([sel[:, 1], sel[:, 2], np.ones(len(sel)), np.ones(len(sel)), np.ones(len(sel))])
            sel = pv[pv[:, 0] == i]
            tab_v[i] = np.column_stack([sel[:, 1], np.ones(len(sel)), np.ones(len(sel)), 3 * np.ones(len(sel)),
                                        np.ones(len(sel))])
        e2e = {}
        for name, fn, tab in (("rho_batch", pcsaft.rho_batch, tab_r), ("vp_batch", pcsaft.vp_batch, tab_v)):
            fn(params, tab)
            t0 = time.perf_counter()
            fn(params, tab)
            e2e[name] = (time.perf_counter() - t0) * 1e3
        rec = dict(points=n, density_kernel_ms=k_rho, vp_kernel_ms=k_vp, rho_batch_ms=e2e["rho_batch"],
                   vp_batch_ms=e2e["vp_batch"], oracle_density_ms_est=oracle_rho * n * 1e3,
                   oracle_vp_ms_est=oracle_vp * n * 1e3)
        print(json.dumps(rec))
        res.append(rec)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(dev), oracle_sample=args.oracle_sample, results=res), fh,
                      indent=1)


if __name__ == "__main__":
    main()
