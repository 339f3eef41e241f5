"""``Trainer.fit`` step time with the host ``DataLoader`` against the ``DeviceDataLoader`` (data/device.py), and the
collate alone for both, on cfg-2 PNA (H=128, 6 layers) and the reference's TransformerConv config (H=256, heads=2,
6 layers) at 97, 512 and 4096 graphs per batch (the reference's ``*_assoc*`` / ``*_msigmae*`` batch sizes and cfg-2).

Step time: HIP events recorded on the training stream each time ``fit`` asks the loader for the next batch, so an
interval holds one whole step -- collate, upload, packing, forward, backward, optimizer -- and any time the device
waits for the host.  The two loaders alternate inside one run (``--rounds`` times each) on the same model config and
dataset.  Collate alone: N batches back to back, one synchronise at the end; the host figure is
``Batch.from_data_list`` + ``.to(device)`` as ``Trainer.fit`` does it, and depends on the host CPU (named in the output).

Usage: python tools/loader_bench.py [--steps 30] [--warmup 10] [--rounds 2] [--out profiles/loader_bench.json]"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnepcsaft_amd.data import Batch, DeviceDataLoader, DeviceDataset, calc_deg, default_config, synthetic_batch  # noqa: E402
from gnnepcsaft_amd.train.models import create_model  # noqa: E402
from gnnepcsaft_amd.train.trainer import DataLoader, Trainer  # noqa: E402

MODELS = {"cfg2_pna_h128": dict(),
          "transformer_h256_heads2": dict(conv="Transformer", propagation_depth=6, hidden_dim=256, heads=2)}
BATCHES = (97, 512, 4096)
DATASET_GRAPHS = 8192  # two epochs' worth of cfg-2 batches; 20 atoms / 40 directed bonds per graph


class Stamped:
    """Passes a loader through and records an event on the current stream at every request for a batch."""

    def __init__(self, loader):
        self.loader, self.events = loader, []

    def __len__(self):
        return len(self.loader)

    def stamp(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append(e)

    def __iter__(self):
        it = iter(self.loader)
        while True:
            self.stamp()
            try:
                batch = next(it)
            except StopIteration:
                self.events.pop()  # the epoch's end: the next epoch's first request stamps again
                return
            yield batch


def fit_ms_per_step(cfg, deg, loader, steps, warmup):
    torch.manual_seed(0)
    model = create_model(dict(cfg), deg)
    stamped = Stamped(loader)
    tr = Trainer(max_steps=warmup + steps, log_every_n_steps=10 ** 9, enable_checkpointing=False)
    tr.fit(model, stamped)
    stamped.stamp()
    torch.cuda.synchronize()
    ev = stamped.events
    assert len(ev) == warmup + steps + 1, len(ev)
    return ev[warmup].elapsed_time(ev[-1]) / steps


def collate_ms(fn, batches):
    fn(batches[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for idx in batches:
        fn(idx)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(batches) * 1e3


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loader_bench.py needs a HIP device: times from a CPU say nothing about the loaders")
    dev = torch.device("cuda", torch.cuda.current_device())
    data = synthetic_batch(DATASET_GRAPHS, 2).to_data_list()
    deg = calc_deg(data)
    ds = DeviceDataset(data, dev)
    rng = np.random.Generator(np.random.PCG64(0))
    rows = []
    for B in BATCHES:
        batches = [rng.integers(0, len(data), size=B) for _ in range(20)]
        host, device = [], []
        for _ in range(args.rounds):
            host.append(collate_ms(lambda i: Batch.from_data_list([data[j] for j in i]).to(dev, non_blocking=True), batches))
            device.append(collate_ms(ds.collate, batches))
        r = {"what": "collate_alone", "graphs_per_batch": B, "host_ms": [round(v, 4) for v in host],
             "device_ms": [round(v, 4) for v in device], "host_over_device": round(min(host) / min(device), 1)}
        print(json.dumps(r), flush=True)
        rows.append(r)
    for name, over in MODELS.items():
        cfg = default_config(2)
        cfg.update(over)
        for B in BATCHES:
            host, device = [], []
            for k in range(args.rounds):
                kw = dict(batch_size=B, shuffle=True, seed=k)
                host.append(fit_ms_per_step(cfg, deg, DataLoader(data, **kw), args.steps, args.warmup))
                device.append(fit_ms_per_step(cfg, deg, DeviceDataLoader(ds, **kw), args.steps, args.warmup))
            r = {"what": "fit_step", "model": name, "graphs_per_batch": B, "host_loader_ms": [round(v, 3) for v in host],
                 "device_loader_ms": [round(v, 3) for v in device], "host_over_device": round(min(host) / min(device), 2)}
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "host_cpu": cpu_name(), "host_threads": torch.get_num_threads(),
                       "dataset_graphs": DATASET_GRAPHS, "steps": args.steps, "warmup": args.warmup, "rows": rows}, f,
                      indent=1)


if __name__ == "__main__":
    main()
