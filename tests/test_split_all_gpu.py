"""gnx_pna_split_all: every PNA layer's split weight images written once per step by k_split_weights_batched and handed to
the layers (gnx_pna_conv_fwd_images / _bwd_images), against the per-call split (GNX_GEMM_SPLIT_ONLY, k_split_weights in
front of each product).

(a) the images are the same bytes; (b) a two-layer stack computes bit-identical activations and input gradients with the
images and without; (c) a layer handed a record that differs from its own plan splits in place and computes the same;
(d) below 4096 rows nothing is split ahead; (e) a step captured into a HIP graph replays to the eager loss.

Launch counts come from the library's host counters (ops.split_launch_counts).  At the row counts used here (4096 ..
8191) the layer's one-segment F x F products take the tiled split-operand kernel too and keep splitting per call (from
8192 rows on they are weights-stationary and split nothing), so the statement checked is a DIFFERENCE: with images a
layer issues exactly three per-call splits less per tower and pass than without."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRE, POST = 2, 2
ROWS = 4096


def _layer_params(rng, T, F, dev):
    H = T * F
    shapes = [(F, H), (F,), (H, H), (H,)]
    for _ in range(T):
        shapes += [(F, 3 * F), (F,), (F, F), (F,), (F, 13 * F), (F,), (F, F), (F,)]
    return [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev) for s in shapes]


def _segs(items):
    from gnnepcsaft_amd import _lib
    arr = (_lib.GemmSeg * len(items))()
    for s, (a, lda, b, ldb, k) in zip(arr, items):
        s.a, s.lda, s.rowscale, s.b, s.ldb, s.k, s._pad = a, lda, None, b, ldb, k, 0
    return arr


# (L, T, F, D): F = 128: post-layer 0 and dx fragment-major (k_gemm3p), dA fragment-major (k_gemm_as3); F = 64: post-layer 0
# fragment-major, dA and dx tile-major (k_gemm3); F = 32: post-layer 0 and dx tile-major, N pads 32 -> 128, dA has a single
# K-tile and no image.  11 layers x 3 = 33 problems: one more than a launch carries.
@pytest.mark.parametrize("L,T,F,D", [(2, 1, 128, 5), (1, 2, 32, 5), (1, 1, 64, 5), (11, 1, 64, 1), (1, 1, 128, 1)])
def test_batched_images_equal_the_per_call_split(gpu_device, L, T, F, D):
    from gnnepcsaft_amd import _lib, ops
    dev = gpu_device
    lib, h = _lib.load(), _lib.handle(dev)
    rng = np.random.default_rng(1000 * L + 10 * F + D)
    H = T * F
    params = [_layer_params(rng, T, F, dev) for _ in range(L)]
    weff = torch.from_numpy(rng.standard_normal((L, T, D, F, 4 * F)).astype(np.float32)).to(dev)
    vp = C.c_void_p
    np_ = len(params[0])
    p_arr = (vp * (L * np_))(*[p.data_ptr() for ps in params for p in ps])
    w_arr = (vp * (L * T))(*[weff[l, t].data_ptr() for l in range(L) for t in range(T)])
    need = lib.gnx_pna_split_all_bytes(h, L, T, F, PRE, POST, D, ROWS, 128)
    slab = torch.full((need,), 0xAA, dtype=torch.uint8, device=dev)
    images = (_lib.PnaLayerImages * L)()
    before = ops.split_launch_counts(dev)
    ops.check(lib.gnx_pna_split_all(h, L, T, F, PRE, POST, D, ROWS, 128, C.cast(p_arr, C.POINTER(vp)), C.cast(w_arr, C.POINTER(vp)),
                                    slab.data_ptr(), need, images))
    after = ops.split_launch_counts(dev)
    per_layer = 3 if F > 32 else 2
    assert after[0] == before[0] and after[1] - before[1] == -(-(L * T * per_layer) // 32)
    # the per-call split of every product, with the arguments the layers use
    x = torch.zeros(ROWS, T * 4 * F, device=dev)       # stands in for every activation and output: SPLIT_ONLY reads none
    table = torch.zeros(16, dtype=torch.int32, device=dev)
    total = 0
    for l in range(L):
        P = params[l]
        for t in range(T):
            k0 = 4 + t * 2 * (PRE + POST)
            kp = k0 + 2 * PRE
            w = weff[l, t].data_ptr()
            strides = (C.c_int64 * 2)(0, 4 * F * F)
            stride1 = (C.c_int64 * 1)(4 * F * F)
            products = {
                "post0": lambda ws, n: lib.gnx_gemm_grouped_rows(
                    h, 2, _segs([(x.data_ptr(), H, P[kp].data_ptr(), 13 * F, F), (x.data_ptr(), T * 4 * F, w, 4 * F, 4 * F)]), strides, D,
                    ROWS, F, P[kp + 1].data_ptr(), None, 0, x.data_ptr(), H, _lib.GEMM_B_TRANS | _lib.GEMM_RELU | _lib.GEMM_SPLIT_ONLY,
                    table.data_ptr(), table.data_ptr(), table.data_ptr(), 4, ws, n, 128),
                "dA": lambda ws, n: lib.gnx_gemm_grouped(
                    h, 1, _segs([(x.data_ptr(), H, w, 4 * F, F)]), stride1, D, ROWS, 4 * F, None, None, 0, x.data_ptr(), T * 4 * F,
                    _lib.GEMM_SPLIT_ONLY, table.data_ptr(), table.data_ptr(), table.data_ptr(), 4, ws, n),
                "dx": lambda ws, n: lib.gnx_gemm(
                    h, 3, _segs([(x.data_ptr(), H, P[kp].data_ptr(), 13 * F, F), (x.data_ptr(), H, P[k0].data_ptr(), 3 * F, F),
                                 (x.data_ptr(), H, P[k0].data_ptr() + 4 * F, 3 * F, F)]), ROWS, F, None, None, 0, x.data_ptr(), H,
                    _lib.GEMM_SPLIT_ONLY, ws, n),
            }
            for name, call in products.items():
                ptr, rec = getattr(images[l], name)[t], getattr(images[l], name + "_rec")[t]
                if name == "dA" and F == 32:
                    assert not ptr and rec.image_bytes == 0
                    continue
                assert ptr and rec.image_bytes > 0, (l, t, name)
                assert rec.bt == (1 if name == "post0" else 0)
                off = ptr - slab.data_ptr()
                assert off == total, (l, t, name)     # back to back, in the order post0, dA, dx
                ws = torch.full((rec.image_bytes,), 0x55, dtype=torch.uint8, device=dev)
                ops.check(call(ws.data_ptr(), ws.numel()))
                assert torch.equal(slab[off:off + rec.image_bytes], ws), (l, t, name, rec.frag)
                total += rec.image_bytes
    assert total == need
    assert ops.split_launch_counts(dev)[0] - after[0] == L * T * per_layer
    if F == 128:
        assert [images[0].post0_rec[0].frag, images[0].dA_rec[0].frag, images[0].dx_rec[0].frag] == [1, 1, 1]
    elif F == 64:
        assert [images[0].post0_rec[0].frag, images[0].dA_rec[0].frag, images[0].dx_rec[0].frag] == [1, 0, 0]
    else:
        assert [images[0].post0_rec[0].frag, images[0].dx_rec[0].frag] == [0, 0]


def test_entry_launches_nothing_without_rows(gpu_device):
    """N = 0 and N = 4095: no bytes asked, no launch, no image handed out (no slab needed)."""
    from gnnepcsaft_amd import _lib, ops
    dev = gpu_device
    lib, h = _lib.load(), _lib.handle(dev)
    rng = np.random.default_rng(3)
    T, F, D = 1, 128, 5
    P = _layer_params(rng, T, F, dev)
    weff = torch.zeros(T, D, F, 4 * F, device=dev)
    vp = C.c_void_p
    p_arr = (vp * len(P))(*[p.data_ptr() for p in P])
    w_arr = (vp * 1)(weff.data_ptr())
    for rows in (0, 4095):
        assert lib.gnx_pna_split_all_bytes(h, 1, T, F, PRE, POST, D, rows, 128) == 0
        images = (_lib.PnaLayerImages * 1)()
        images[0].post0[0] = 1  # (must be cleared)
        before = ops.split_launch_counts(dev)
        ops.check(lib.gnx_pna_split_all(h, 1, T, F, PRE, POST, D, rows, 128, C.cast(p_arr, C.POINTER(vp)),
                                        C.cast(w_arr, C.POINTER(vp)), None, 0, images))
        assert ops.split_launch_counts(dev) == before
        assert not images[0].post0[0] and not images[0].dA[0] and not images[0].dx[0]
        assert images[0].post0_rec[0].image_bytes == images[0].dA_rec[0].image_bytes == images[0].dx_rec[0].image_bytes == 0
    assert lib.gnx_pna_split_all_bytes(h, 1, T, F, PRE, POST, D, 4096, 128) == 4718592


# ---------------------------------------------------------------------------------------------------------------
# a two-layer PNA model (H = 128, one tower) over n nodes with in-degrees 1..4
# ---------------------------------------------------------------------------------------------------------------
def _graph_batch(n, seed):
    from gnnepcsaft_amd.data import ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 5, size=n)
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, size=dst.size)
    order = rng.permutation(dst.size)
    ei = torch.from_numpy(np.stack([src[order], dst[order]])).long()
    x = torch.from_numpy(np.stack([rng.integers(0, d, size=n) for d in ATOM_FEATURE_DIMS], axis=1)).long()
    ea = torch.from_numpy(np.stack([rng.integers(0, d, size=dst.size) for d in BOND_FEATURE_DIMS], axis=1)).long()
    batch = torch.from_numpy(np.arange(n) // 20).long()
    target = torch.from_numpy(rng.uniform(0.5, 1.5, size=(int(batch[-1]) + 1, 3)).astype(np.float32))
    hist = np.bincount(deg, minlength=5).tolist()
    return x, ei, ea, batch, target, hist


class _Stack:
    def __init__(self, n, dev, seed=7):
        from gnnepcsaft_amd import dp
        from gnnepcsaft_amd.data import default_config
        from gnnepcsaft_amd.train.models import GNNePCSAFT
        x, ei, ea, batch, target, hist = _graph_batch(n, seed)
        cfg = default_config(2)
        cfg.update(hidden_dim=128, propagation_depth=2, deg=hist)
        torch.manual_seed(0)
        self.model = GNNePCSAFT(cfg).to(dev).train()
        self.max_degree = len(hist) - 1
        self.flat = dp.FlatGradAllReduce(self.model)
        self.flat.enable_overlap(False)
        self.inputs = [t.to(dev) for t in (x, ei, ea, batch)]
        self.target = target.to(dev)
        self.num_graphs = int(target.size(0))
        self.dev = dev

    def step(self):
        from gnnepcsaft_amd import functional as Fn
        from gnnepcsaft_amd import ops
        self.flat.zero_grad()
        x, ei, ea, batch = self.inputs
        # the packer is part of the step, and sync-free (graph count and degree bound given): it can be captured
        pack = ops.pack_graph(ei, ea, batch, x.size(0), self.num_graphs, validate=False)
        pack.max_degree_hint = self.max_degree
        pred = self.model(x, ei, ea, batch, pack=pack)
        loss, _ = Fn.HuberAPEFn.apply(pred, self.target, 0.01)
        loss.backward()
        return loss

    def run(self, split_all):
        """One forward + backward; everything the issue wants compared, and the split launches it took."""
        from gnnepcsaft_amd import functional as Fn, ops
        got = {"out": [], "saved": [], "dx": {}}
        hooks = []
        for l, conv in enumerate(self.model.convs):
            def pre(_m, _args, kwargs, l=l):
                kwargs["x"].register_hook(lambda g, l=l: got["dx"].__setitem__(l, g.detach().clone()))

            def post(_m, _args, _kwargs, out):
                n_act = len(out.grad_fn.saved_tensors) - len(list(_m._params()))
                got["out"].append(out.detach().clone())
                got["saved"].append([t.detach().clone() for t in out.grad_fn.saved_tensors[:n_act]])  # x, BE, EE, A, amp, att, hs, zs
            hooks += [conv.register_forward_pre_hook(pre, with_kwargs=True), conv.register_forward_hook(post, with_kwargs=True)]
        Fn.set_split_all(split_all)
        before = ops.split_launch_counts(self.dev)
        try:
            loss = self.step()
            torch.cuda.synchronize()
        finally:
            Fn.set_split_all(True)
            for hk in hooks:
                hk.remove()
        after = ops.split_launch_counts(self.dev)
        got.update(loss=loss.detach().clone(), grads=self.flat.flat.detach().clone(), per_call=after[0] - before[0],
                   batched=after[1] - before[1])
        return got


def _assert_same_bits(a, b):
    assert torch.equal(a["loss"], b["loss"])
    assert len(a["out"]) == len(b["out"]) == 2 and sorted(a["dx"]) == sorted(b["dx"]) == [0, 1]
    for l in range(2):
        assert torch.equal(a["out"][l], b["out"][l]), f"layer {l} output"
        assert len(a["saved"][l]) == len(b["saved"][l]) >= 6 + PRE + 1
        for i, (u, v) in enumerate(zip(a["saved"][l], b["saved"][l])):  # [3] is A
            assert torch.equal(u, v), f"layer {l} saved activation {i}"
        assert torch.equal(a["dx"][l], b["dx"][l]), f"layer {l} dx"


@pytest.fixture()
def training_switches():
    from gnnepcsaft_amd import functional as Fn, ops
    Fn.set_grad_in_place(True)
    ops.set_wgrad_side_stream(True)
    yield
    Fn.set_grad_in_place(False)
    ops.set_wgrad_side_stream(False)
    Fn.set_split_all(True)


def test_layers_with_images_equal_layers_that_split_in_place(gpu_device, training_switches):
    """N = 4096 + 37 (a ragged last tile), degrees 1..4, two layers.  ON vs OFF: outputs, A and every saved activation, dx of
    both layers bit-identical.  Parameter gradients (fp32 atomics): |ON - OFF| <= 2 x |OFF - OFF'| (max norm), both printed.
    Measured on MI355X, two runs: OFF vs OFF' = 9.4e-09 / 1.46e-08, ON vs OFF = 1.08e-08 / 1.40e-08 (bounds 1.87e-08 / 2.92e-08)."""
    st = _Stack(ROWS + 37, gpu_device)
    off, off2, on = st.run(False), st.run(False), st.run(True)
    _assert_same_bits(off2, off)
    _assert_same_bits(on, off)
    spread = float((off2["grads"] - off["grads"]).abs().max())
    diff = float((on["grads"] - off["grads"]).abs().max())
    print(f"parameter gradients, max |difference|: OFF vs OFF {spread:.3e}, ON vs OFF {diff:.3e}, bound {2 * spread:.3e}")
    assert diff <= 2 * spread, (diff, spread)
    # two layers x one tower x (post0, dA, dx) per-call splits left the layers; one batched launch came
    assert (off["batched"], on["batched"]) == (0, 1)
    assert off["per_call"] - on["per_call"] == 6, (off["per_call"], on["per_call"])


def test_mismatched_record_falls_back_to_the_split_in_place(gpu_device, training_switches, monkeypatch):
    """Records that differ from the layer's own plan in ONE field each (layer 0: image_bytes of post-layer 0; layer 1: frag of
    post-layer 0, classes of dA, a k offset of dx): those four products split in place, the other two use their images, and
    every result is what the OFF path computes."""
    from gnnepcsaft_amd import nn as gnn
    st = _Stack(ROWS + 37, gpu_device)
    off = st.run(False)
    original = gnn.PNAConv.prepare_all

    def tampered(convs, edge_index, edge_attr):
        wo = original(convs, edge_index, edge_attr)
        im0, im1 = wo.values[0][5][0], wo.values[1][5][0]
        im0.post0_rec[0].image_bytes += 256
        im1.post0_rec[0].frag ^= 1
        im1.dA_rec[0].classes -= 1
        im1.dx_rec[0].koff[1] += 32
        return wo
    monkeypatch.setattr(gnn.PNAConv, "prepare_all", staticmethod(tampered))
    on = st.run(True)
    _assert_same_bits(on, off)
    assert on["batched"] == 1
    assert off["per_call"] - on["per_call"] == 2, (off["per_call"], on["per_call"])


def test_small_batch_runs_as_before(gpu_device, training_switches):
    """4095 rows: nothing is split ahead and the layers issue what they issued before."""
    st = _Stack(ROWS - 1, gpu_device)
    off, on = st.run(False), st.run(True)
    _assert_same_bits(on, off)
    assert (on["batched"], off["batched"]) == (0, 0) and on["per_call"] == off["per_call"]


def test_captured_step_replays_to_the_eager_loss(gpu_device, training_switches):
    """The step captured into a HIP graph with the images on (what bench.py does), replayed twice: the loss of either replay
    is the eager loss, bit for bit."""
    dev = gpu_device
    prev_stream = torch.cuda.current_stream(dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    try:
        st = _Stack(ROWS + 37, dev)
        for _ in range(2):
            loss_e = st.step()
        torch.cuda.synchronize()
        loss_e = loss_e.detach().clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            static_loss = st.step()
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_loss.detach(), loss_e)
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev_stream)
