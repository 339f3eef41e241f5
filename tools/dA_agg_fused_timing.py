"""The dA product + scatter-aggregate backward of one PNA tower ALONE, as the two launches (k_gemm_as3, k_pna_agg_bwd_rc) and
as the fused one (k_pna_dA_agg_bwd, GNX_OPT_DA_AGG_FUSED), at the layer shapes of bench configs 2 and 5 (F = 128, one tower):
event-timed per launch through the library's own profiler, alternating the two forms.
usage: python tools/dA_agg_fused_timing.py [--reps 20] [--rounds 3]
Both forms split the class weights in front of the product here (no gnx_pna_split_all images): that launch is reported under
"split+product" for the pair and under "split" for the fused form."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gnnepcsaft_amd import _lib, ops
from gnnepcsaft_amd.data import synthetic_batch

F = 128

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for cfg, graphs in ((2, 4096), (5, 8192)):
        b = synthetic_batch(graphs, cfg)
        N, E = b.x.size(0), b.edge_index.size(1)
        g = ops.pack_graph(b.edge_index.to(dev), None, None, N, None)
        dc = g.degree_classes()
        torch.manual_seed(cfg)
        m, gout = torch.randn(E, F, device=dev), torch.randn(N, F, device=dev)
        weffs = [torch.randn(dc.D, F, 4 * F, device=dev) / 8]
        A, dA, dm = torch.empty(N, 4 * F, device=dev), torch.empty(N, 4 * F, device=dev), torch.empty(E, F, device=dev)
        forms = (0, 1)
        res = {v: [] for v in forms}
        for rnd in range(a.rounds + 1):
            for fused in forms:
                ops.set_option(dev, _lib.OPT_DA_AGG_FUSED, fused)
                for _ in range(3):
                    took = ops.pna_dA_aggregate_bwd(gout, weffs, m, A, g, dc, 1, F, dA=dA, dm=dm)[1]
                assert took == bool(fused)
                ops.prof_begin(dev, [_lib.K_GEMM_TILED, _lib.K_PNA_AGG_BWD])
                for _ in range(a.reps):
                    ops.pna_dA_aggregate_bwd(gout, weffs, m, A, g, dc, 1, F, dA=dA, dm=dm)
                tiled, agg = ops.prof_read(dev, _lib.K_GEMM_TILED), ops.prof_read(dev, _lib.K_PNA_AGG_BWD)
                ops.prof_end(dev)
                if rnd > 0:
                    res[fused].append((1e3 * tiled[1] / a.reps, 1e3 * agg[1] / a.reps))
        ops.set_option(dev, _lib.OPT_DA_AGG_FUSED, 1)
        for fused, name, first in [(v, "pair " if v == 0 else "fused", "split+product" if v == 0 else "split") for v in forms]:
            t, s = statistics.median(x[0] for x in res[fused]), statistics.median(x[1] for x in res[fused])
            print(f"cfg-{cfg} N={N} E={E} D={dc.D}  {name}: {first} {t:7.1f} us  aggregate-backward group {s:7.1f} us  "
                  f"sum {t + s:7.1f} us", flush=True)
