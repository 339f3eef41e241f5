"""TransformerConv on the HIP path (gnx_transformer_attn_*) against the fp64 restatement (tests/transformer_ref.py):
single layer forward and every gradient on identical inputs (1e-5 norm-wise relative; the layer has no ReLU / min / max
events, so no row is excluded), attention dropout replayed from the kernel's own keep mask, bitwise-deterministic
d(q|k|v), the whole model against the swapped fp64 reference model, trainer save / resume, a captured training step,
and the InferenceEngine's refusal.
The attention kernels on their own, entry by entry at every thread and head layout: tests/test_attn_ops_gpu.py."""
import copy
import math
import os

import pytest
import torch

from tests.parity_util import rel_err
from tests.transformer_ref import TransformerConv as RefConv, reference_model

pytestmark = pytest.mark.gpu

TOL = 1e-5
NAMES = ("lin_query.weight", "lin_query.bias", "lin_key.weight", "lin_key.bias", "lin_value.weight", "lin_value.bias",
         "lin_edge.weight", "lin_skip.weight", "lin_skip.bias")


def _batch(kind: str):
    from gnnepcsaft_amd.data import synthetic_batch
    from tests import conv_cases
    if kind == "hubs":
        return conv_cases.hub_batch()
    if kind == "lone":
        return conv_cases.lone_atom_batch()
    return synthetic_batch(64, 3)


def _codes(edge_attr: torch.Tensor) -> torch.Tensor:
    """bond code of every edge in the original order (mixed radix over the vocab sizes 5, 6, 2)."""
    return (edge_attr[:, 0] * 6 + edge_attr[:, 1]) * 2 + edge_attr[:, 2]


def _layer_case(dev, kind, H, heads, p=0.0, seed=0):
    """(native conv on dev, fp64 reference conv with the same weights, batch, pack, x, BE, upstream gradient G)."""
    from gnnepcsaft_amd import nn as gnn
    from gnnepcsaft_amd import ops
    torch.manual_seed(seed)
    batch = _batch(kind)
    native = gnn.TransformerConv(H, H // heads, heads, dropout=p, edge_dim=H).to(dev).train()
    ref = RefConv(H, H // heads, heads, dropout=p, edge_dim=H).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in native.state_dict().items()}, strict=True)
    N = batch.x.size(0)
    x = torch.randn(N, H)
    BE = torch.randn(60, H)
    G = torch.randn(N, H)
    b = batch.to(dev)
    pack = ops.pack_graph(b.edge_index, b.edge_attr, b.batch, N, batch.num_graphs)
    return native, ref, batch, pack, x, BE, G


def _run_native(native, pack, x, BE, G, dev):
    xd = x.to(dev).requires_grad_(True)
    bd = BE.to(dev).requires_grad_(True)
    out = native(xd, pack, bd)
    (out * G.to(dev)).sum().backward()
    grads = {n: p.grad for n, p in native.named_parameters()}
    return out, xd.grad, bd.grad, grads


def _run_ref(ref, batch, x, BE, G, keep=None):
    x64 = x.double().requires_grad_(True)
    b64 = BE.double().requires_grad_(True)
    ref.keep = keep
    out = ref(x64, batch.edge_index, b64.index_select(0, _codes(batch.edge_attr)))
    (out * G.double()).sum().backward()
    return out, x64.grad, b64.grad, {n: p.grad for n, p in ref.named_parameters()}


def _assert_parity(nat, ref, tol=TOL):
    out, dx, dbe, g = nat
    out_r, dx_r, dbe_r, g_r = ref
    errs = {"out": rel_err(out, out_r), "dx": rel_err(dx, dx_r), "dBE": rel_err(dbe, dbe_r)}
    errs.update({n: rel_err(g[n], g_r[n]) for n in NAMES if n != "lin_key.bias"})
    # the key bias adds <q_i, b_k> to every score of row i, which the softmax cancels: its gradient is analytically
    # zero (fp64: ~1e-17), so it is measured against the scale of the query-bias gradient (same sums, no cancellation)
    errs["lin_key.bias"] = rel_err(g["lin_key.bias"], g_r["lin_key.bias"],
                                   floor=float(g_r["lin_query.bias"].abs().max()))
    assert max(errs.values()) <= tol, errs
    return errs


LAYER_CASES = [("random", 32, 1), ("random", 32, 2), ("random", 32, 4), ("random", 64, 1), ("random", 64, 2),
               ("random", 64, 4), ("random", 256, 1), ("random", 256, 2), ("random", 256, 4), ("random", 512, 4),
               ("random", 512, 1),
               ("hubs", 64, 2), ("hubs", 256, 2), ("lone", 64, 2), ("lone", 256, 4)]


@pytest.mark.parametrize("kind,H,heads", LAYER_CASES)
def test_single_layer_matches_fp64(gpu_device, kind, H, heads):
    native, ref, batch, pack, x, BE, G = _layer_case(gpu_device, kind, H, heads)
    errs = _assert_parity(_run_native(native, pack, x, BE, G, gpu_device), _run_ref(ref, batch, x, BE, G))
    print(kind, H, heads, max(errs.values()))


@pytest.mark.parametrize("kind,H,heads", [("random", 64, 2), ("hubs", 256, 2), ("random", 512, 4)])
def test_attention_dropout_replays_in_fp64(gpu_device, kind, H, heads):
    from gnnepcsaft_amd import ops
    p = 0.25
    native, ref, batch, pack, x, BE, G = _layer_case(gpu_device, kind, H, heads, p=p)
    nat = _run_native(native, pack, x, BE, G, gpu_device)
    assert native.calls == 1
    # the kernel's keep mask of that call (it depends on (seed, offset, E, heads) only), CSR order -> original order
    qkvs = torch.zeros(x.size(0), 4 * H, device=gpu_device)
    _, _, keep_csr = ops.transformer_attn_fwd(qkvs, torch.zeros(60, H, device=gpu_device), pack, heads, p,
                                              native.seed, native.calls, want_mask=True)
    keep = torch.empty_like(keep_csr)
    keep[pack.perm.long()] = keep_csr
    keep = keep.cpu()
    n = keep.numel()
    frac = float(keep.double().mean())
    assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (frac, n)
    _assert_parity(nat, _run_ref(ref, batch, x, BE, G, keep=keep))
    # the next call draws another mask
    _, _, keep2 = ops.transformer_attn_fwd(qkvs, torch.zeros(60, H, device=gpu_device), pack, heads, p, native.seed,
                                           native.calls + 1, want_mask=True)
    assert not torch.equal(keep_csr, keep2)


def test_backward_is_bitwise_deterministic(gpu_device):
    from gnnepcsaft_amd import ops
    native, ref, batch, pack, x, BE, G = _layer_case(gpu_device, "hubs", 256, 2)
    H, heads = 256, 2
    qkvs = torch.randn(x.size(0), 4 * H, device=gpu_device)
    Le = torch.randn(60, H, device=gpu_device)
    out, alpha, _ = ops.transformer_attn_fwd(qkvs, Le, pack, heads, 0.25, 7, 3)
    dout = G.to(gpu_device)
    a = ops.transformer_attn_bwd(dout, qkvs, Le, alpha, pack, heads, 0.25, 7, 3)
    b = ops.transformer_attn_bwd(dout, qkvs, Le, alpha, pack, heads, 0.25, 7, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[0]).all() and torch.isfinite(out).all()


def _model_cfg(**kw):
    from gnnepcsaft_amd.data import default_config
    cfg = default_config(2)
    cfg.update(dict(conv="Transformer", hidden_dim=32, heads=2, propagation_depth=3, dropout=0.0), **kw)
    return cfg


def test_whole_model_matches_swapped_fp64_reference(gpu_device):
    from oracle import pyg_restatement as O
    from gnnepcsaft_amd import functional as Fn
    from gnnepcsaft_amd.data import calc_deg, synthetic_batch
    from gnnepcsaft_amd.train.models import GNNePCSAFT
    batch = synthetic_batch(96, 3)
    cfg = _model_cfg(deg=calc_deg(batch))
    torch.manual_seed(0)
    native = GNNePCSAFT(cfg).to(gpu_device).train()
    ref = reference_model(cfg).double().train()
    ref.load_state_dict({k: v.double().cpu() for k, v in native.state_dict().items()}, strict=True)
    b = batch.to(gpu_device)
    pred = native(b.x, b.edge_index, b.edge_attr, b.batch)
    loss, _ = Fn.HuberAPEFn.apply(pred, b.para, 0.01)
    loss.backward()
    pred_r = ref(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
    loss_r = O.ape_huber_loss(pred_r, batch.para.double())
    loss_r.backward()
    assert rel_err(pred, pred_r) <= 1e-4 and rel_err(loss, loss_r) <= 1e-4
    gn = {n: p.grad.double().cpu() for n, p in native.named_parameters()}
    gr = {n: p.grad for n, p in ref.named_parameters()}
    num = sum(float(((gn[n] - gr[n]) ** 2).sum()) for n in gr)
    den = sum(float((gr[n] ** 2).sum()) for n in gr)
    assert (num / den) ** 0.5 <= 1e-3, (num / den) ** 0.5
    # eval forward and pred_with_bounds go through the normal path
    native.eval()
    ref.eval()
    with torch.no_grad():
        assert rel_err(native.pred_with_bounds(b), ref.pred_with_bounds(batch)) <= 1e-4


def test_trainer_resume_restores_attention_dropout(gpu_device, tmp_path):
    from gnnepcsaft_amd.data import calc_deg, synthetic_batch
    from gnnepcsaft_amd.train.models import create_model
    from gnnepcsaft_amd.train.trainer import DataLoader, Trainer, read_checkpoint
    dataset = synthetic_batch(64, 3).to_data_list()
    deg = calc_deg(dataset)
    cfg = _model_cfg(dropout=0.25, propagation_depth=2)

    def new_model():
        torch.manual_seed(0)
        return create_model(copy.deepcopy(cfg), deg)

    mA = new_model()
    trA = Trainer(max_steps=4, log_every_n_steps=1, enable_checkpointing=False)
    trA.fit(mA, DataLoader(dataset, batch_size=32, shuffle=True, seed=3))
    mB = new_model()
    trB = Trainer(max_steps=2, log_every_n_steps=1, default_root_dir=str(tmp_path), enable_checkpointing=True)
    trB.fit(mB, DataLoader(dataset, batch_size=32, shuffle=True, seed=3))
    path = os.path.join(str(tmp_path), "last.ckpt")
    ckpt = read_checkpoint(path)
    assert [d["calls"] for d in ckpt["attn_dropout"]] == [2, 2]
    assert [d["seed"] for d in ckpt["attn_dropout"]] == [c.seed for c in mB.model.convs]
    mC = new_model()
    for c in mC.model.convs:
        c.seed, c.calls = 12345, 99  # must come back from the file
    trC = Trainer(max_steps=4, log_every_n_steps=1, enable_checkpointing=False)
    trC.fit(mC, DataLoader(dataset, batch_size=32, shuffle=True, seed=3), ckpt_path=path)
    assert [c.calls for c in mC.model.convs] == [c.calls for c in mA.model.convs] == [4, 4]
    a = [r["train_huber"] for r in trA.logged[2:]]
    c = [r["train_huber"] for r in trC.logged]
    assert len(a) == len(c) == 2 and max(abs(x - y) / x for x, y in zip(a, c)) <= 5e-5, (a, c)


def test_captured_training_step_matches_eager(gpu_device):
    from gnnepcsaft_amd import dp, functional as Fn
    from gnnepcsaft_amd.data import calc_deg, synthetic_batch
    from gnnepcsaft_amd.train.models import create_model
    batch = synthetic_batch(128, 3)
    deg = calc_deg(batch)
    prev_stream = torch.cuda.current_stream(gpu_device)
    s = torch.cuda.Stream(device=gpu_device)
    torch.cuda.set_stream(s)
    try:
        torch.manual_seed(0)
        model = create_model(_model_cfg(), deg).to(gpu_device).train()
        model.model.validate_inputs = False
        flat = dp.FlatGradAllReduce(model)
        flat.enable_overlap(False)
        Fn.set_grad_in_place(True)
        b = batch.to(gpu_device)

        def body():
            flat.zero_grad()
            b._gnx_pack = None
            loss = model.training_step(b, 0)
            loss.backward()
            return loss

        for _ in range(2):
            loss_e = body()
            flat.all_reduce()
            flat.finish()
        torch.cuda.synchronize()
        loss_e, grad_e = float(loss_e), flat.flat.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            static_loss = body()
        g.replay()
        flat.all_reduce()
        flat.finish()
        torch.cuda.synchronize()
        assert abs(float(static_loss) - loss_e) <= 1e-6 * abs(loss_e)
        assert rel_err(flat.flat, grad_e) <= 1e-4
    finally:
        Fn.set_grad_in_place(False)
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev_stream)


def test_attention_dropout_refuses_hip_graph_capture(gpu_device):
    """p > 0: the mask counter lives on the host, so the layer raises under stream capture (before any launch), as
    Dropout does; p = 0 stays capturable."""
    from gnnepcsaft_amd import nn as gnn
    from gnnepcsaft_amd import ops
    from gnnepcsaft_amd.data import synthetic_batch
    conv = gnn.TransformerConv(32, 16, 2, dropout=0.25, edge_dim=32).to(gpu_device).train()
    b = synthetic_batch(8, 3).to(gpu_device)
    pack = ops.pack_graph(b.edge_index, b.edge_attr, b.batch, b.x.size(0), 8)
    x = torch.randn(b.x.size(0), 32, device=gpu_device)
    BE = torch.randn(60, 32, device=gpu_device)
    s = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="cannot be captured"):
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                conv(x, pack, BE)
    torch.cuda.synchronize()
    assert conv.calls == 0


def test_inference_engine_refuses_transformer(gpu_device):
    from gnnepcsaft_amd.inference import InferenceEngine
    from gnnepcsaft_amd.train.models import create_model
    model = create_model(_model_cfg(), [0, 4, 2]).to(gpu_device)
    with pytest.raises(NotImplementedError, match="Transformer"):
        InferenceEngine(model)
