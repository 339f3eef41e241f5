"""A/B timing of the weight-gradient kernels: wave-specialised split kernel (default, mode 2), two-barrier split kernel
(mode 1: GNX_OPT_WGRAD_PIPE = 0), fp32 MFMA (mode 0: GNX_OPT_GEMM_SPLIT = 0); then the per-degree-class gradient at the cfg-2
class structure in the same modes, the wave-specialised one at the workgroup budgets of DIAG_GROUPED_WGS (0 = the default)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnepcsaft_amd import _lib, ops
dev = torch.device("cuda:0")
ops.set_wgrad_side_stream(False)
for M, N, K, nprob in ((81920, 128, 128, 1), (81920, 128, 128, 8), (163840, 128, 128, 1), (81920, 128, 512, 1)):
    g = [torch.randn(M, N, device=dev) for _ in range(nprob)]
    x = [torch.randn(M, K, device=dev) for _ in range(nprob)]
    dw = [torch.zeros(N, K, device=dev) for _ in range(nprob)]
    def run():
        for i in range(nprob):
            ops.queue_wgrad(g[i], x[i], dw[i])
        ops.flush_wgrads()
    for mode in os.environ.get("DIAG_MODES", "2,1,0").split(","):
        ops.set_option(torch.device("cuda:0"), _lib.OPT_GEMM_SPLIT, 1 if int(mode) else 0)
        ops.set_option(torch.device("cuda:0"), _lib.OPT_WGRAD_PIPE, 1 if int(mode) == 2 else 0)
        for _ in range(3): run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20): run()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        byts = nprob * M * (N + K) * 4
        print(f"M={M} N={N} K={K} x{nprob} split={mode}: {us:7.1f} us  {byts/us/1e6:5.2f} TB/s  {2*nprob*M*N*K/us/1e6:6.1f} TF/s", flush=True)

# the per-degree-class gradient of post-layer 0 at the cfg-2 class structure (synthetic_batch(4096, 2): 81 920 x 128 x 512),
# beside the ungrouped line of the same shape above: mode 2 = k_gemm_wgrad3p_grouped, 1 = k_gemm_wgrad3<true>, 0 = fp32 MFMA
from gnnepcsaft_amd.data import synthetic_batch
b = synthetic_batch(4096, 2).to(dev)
pack = ops.pack_batch(b.edge_index, b.edge_attr, b.batch, int(b.x.size(0)), 4096, max_degree_hint=None)
dc = pack.degree_classes()
M, N, K = int(b.x.size(0)), 128, 512
g, x = torch.randn(M, N, device=dev), torch.randn(M, K, device=dev)
dw = torch.zeros(dc.D, N, K, device=dev)
for mode in os.environ.get("DIAG_MODES", "2,1,0").split(","):
    ops.set_option(dev, _lib.OPT_GEMM_SPLIT, 1 if int(mode) else 0)
    ops.set_option(dev, _lib.OPT_WGRAD_PIPE, 1 if int(mode) == 2 else 0)
    for wgs in [int(w) for w in os.environ.get("DIAG_GROUPED_WGS", "0,64,128,256").split(",")] if int(mode) == 2 else [0]:
        ops.set_option(dev, _lib.OPT_WGRAD_WGS, wgs)
        name, info = ops.gemm_wgrad_grouped_plan(g, x, dc.max_chunks)
        for _ in range(3): ops.gemm_wgrad_grouped(g, x, dw, dc)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20): ops.gemm_wgrad_grouped(g, x, dw, dc)
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        print(f"M={M} N={N} K={K} grouped D={dc.D} chunks={int(dc.nchunks)}/{dc.max_chunks} split={mode} wgs={wgs} {name} "
              f"grid=({info.grid_x},{info.grid_y},{info.grid_z}) S={info.chunks_per_range}: {us:7.1f} us  "
              f"{M*(N+K)*4/us/1e6:5.2f} TB/s  {2*M*N*K/us/1e6:6.1f} TF/s", flush=True)
    ops.set_option(dev, _lib.OPT_WGRAD_WGS, 0)
