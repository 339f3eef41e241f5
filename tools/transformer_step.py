"""fwd + loss + bwd step time of the two reference TransformerConv configs (configs/transformer_msigmae.py: H=256,
heads=2; transformer_msigmae_2.py: H=512, heads=4; both 6 layers) at 512 and 4096 graphs, attention / model dropout
p = 0 and p = 0.25, and the attention kernels' share of the 8 TB/s HBM peak on their algorithmic bytes (gnx_prof_*
ids GNX_K_ATTN_FWD / GNX_K_ATTN_BWD).  Eager launches, weight gradients in place on the side stream (as bench.py).

Usage: python tools/transformer_step.py [--steps 20] [--warmup 5] [--out profiles/transformer_step.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnepcsaft_amd import _lib, dp, functional as Fn, ops  # noqa: E402
from gnnepcsaft_amd.data import calc_deg, default_config, synthetic_batch  # noqa: E402
from gnnepcsaft_amd.train.models import create_model  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
CONFIGS = {"transformer_msigmae": dict(hidden_dim=256, heads=2), "transformer_msigmae_2": dict(hidden_dim=512, heads=4)}


def launches_per_step(step) -> int:
    """GPU kernels of one step, counted by torch.profiler (-1 if the profiler is unavailable)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:  # pylint: disable=broad-except
        return -1


def run(name, graphs, p, steps, warmup, dev):
    cfg = default_config(2)
    cfg.update(dict(conv="Transformer", propagation_depth=6, dropout=p, **CONFIGS[name]))
    batch = synthetic_batch(graphs, 2)
    deg = calc_deg(batch)
    torch.manual_seed(0)
    model = create_model(cfg, deg).to(dev).train()
    model.model.validate_inputs = False
    flat = dp.FlatGradAllReduce(model)
    Fn.set_grad_in_place(True)
    ops.set_wgrad_side_stream(True)
    b = batch.to(dev)

    def step():
        flat.zero_grad()
        b._gnx_pack = None
        model.training_step(b, 0).backward()
        ops.join_side_stream(dev)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    ops.prof_begin(dev, [_lib.K_ATTN_FWD, _lib.K_ATTN_BWD])
    for _ in range(3):
        step()
    kern = {}
    for kid, key in ((_lib.K_ATTN_FWD, "attn_fwd"), (_lib.K_ATTN_BWD, "attn_bwd")):
        w = ops.prof_read_work(dev, kid)
        n = max(w["launches"], 1)
        sec = w["ms"] * 1e-3
        kern[key] = {"us_per_layer": round(w["ms"] / n * 1e3, 2), "GB_per_layer": round(w["bytes"] / n / 1e9, 4),
                     "hbm_peak_share": round(w["bytes"] / sec / PEAK_BYTES_PER_S, 3) if sec > 0 else None}
    ops.prof_end(dev)
    res = {"config": name, "graphs": graphs, "N": int(b.x.size(0)), "E": int(b.edge_index.size(1)), "p": p,
           "ms_per_step": round(ms, 3), "graphs_per_s": round(graphs / ms * 1e3), "launches_per_step": launches_per_step(step),
           **kern}
    Fn.set_grad_in_place(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    rows = []
    for name in CONFIGS:
        for graphs in (512, 4096):
            for p in (0.0, 0.25):
                r = run(name, graphs, p, args.steps, args.warmup, dev)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
