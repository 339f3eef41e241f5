"""k_pna_dA_agg_bwd (the dA product and the scatter-aggregate backward of a PNA tower in one launch, dA kept in registers)
against the two launches it replaces, on the same inputs: ops.gemm_grouped (which must have taken k_gemm_as3) followed by
ops.pna_aggregate_bwd.  The message gradient must be equal BIT FOR BIT (int32 views: NaNs count, no tolerance), the rows
behind it and the dA buffer must stay untouched, and a call that was meant to be fused and was not fails.

Shapes: F = 128 (the only width the fused kernel takes), T in {1, 2}, N = 4096 (the split path's threshold), 4097 and
4096 + 193, class tables of 128- and 96-row tiles.  In-degrees from {0, 1, 2, 3, 4, 5, 7, 16}: nodes without messages, the
register path (<= 4), the three-pass path, a degree above the edge-tile bound; class sizes 1, 63, 64, 65, 129 (repeated last
rows of a partial 32-row part, both halves of a tile).  Crafted message rows: duplicated messages (ties in min and max), an
extremum exactly 0 (the extra-tie rule), all messages of a node equal (std masked), a NaN row, +-inf."""
import copy

import numpy as np
import pytest
import torch

from gnnepcsaft_amd import _lib

pytestmark = pytest.mark.gpu
F = 128
CANARY = 12345.0
# in-degree -> class size; the rest of the nodes get degree 1, 2 or 3 at random
CLASS_SIZES = {0: 1, 16: 63, 7: 64, 5: 65, 4: 129}


def _i32(t):
    return t.contiguous().view(torch.int32)


def _build(N, T, rows, dev):
    """Graph, degree classes over ``rows``-row tiles, messages with the crafted rows, gradient rows, class weights."""
    from gnnepcsaft_amd import ops
    rng = np.random.default_rng(N * 8 + T * 2 + rows)
    deg = np.concatenate([np.full(n, d) for d, n in CLASS_SIZES.items()])
    deg = np.concatenate([deg, rng.integers(1, 4, size=N - len(deg))])
    rng.shuffle(deg)
    dst = np.repeat(np.arange(N), deg)
    E = len(dst)
    order = rng.permutation(E)
    ei = torch.from_numpy(np.stack([rng.integers(0, N, size=E), dst[order]])).long()
    ops.set_option(dev, _lib.OPT_GEMM_TILE_ROWS, rows)
    try:
        g = ops.pack_graph(ei.to(dev), None, None, N, None)
        dc = g.degree_classes()
    finally:
        ops.set_option(dev, _lib.OPT_GEMM_TILE_ROWS, 0)
    assert dc is not None and dc.D == 17 and dc.tile_rows_p == rows and (dc.tiles_p is not dc.tiles) == (rows == 96)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    assert np.array_equal(g.rowptr.cpu().numpy(), rowptr)
    H = T * F
    torch.manual_seed(N + T)
    m = torch.randn(E, H)

    def nodes(d, k):
        return [int(n) for n in np.flatnonzero(deg == d)[:k]]
    for d in (2, 3, 4, 5, 7, 16):   # both arithmetic paths
        n_dup, n_zero, n_eq, n_nan, n_inf = nodes(d, 5)
        p = rowptr[n_dup]
        m[p + 1] = m[p]                                               # duplicated message: a tie wherever it is an extremum
        m[p + d - 1, ::2] = m[p:p + d, ::2].max(0).values             # ... and a tied maximum for certain
        p = rowptr[n_zero]
        m[p:p + d] = -m[p:p + d].abs() - 0.5                          # extremum exactly 0: the maximum on even channels,
        m[p:p + d, 1::2] *= -1                                        # the minimum on odd ones (the extra-tie rule)
        m[p + d // 2] = 0.0
        p = rowptr[n_eq]
        m[p:p + d] = m[p]                                             # all messages equal: std masked
        m[rowptr[n_nan] + d - 1] = float("nan")
        p = rowptr[n_inf]
        m[p, ::2], m[p, 1::2] = float("inf"), float("-inf")
    n1 = nodes(1, 3)
    m[rowptr[n1[0]]] = 0.0
    m[rowptr[n1[1]]] = float("nan")
    m[rowptr[n1[2]], ::3] = float("inf")
    gout = torch.randn(N, H)
    weffs = [(torch.randn(dc.D, F, 4 * F) / 8).to(dev) for _ in range(T)]
    return g, dc, m.to(dev), gout.to(dev), weffs


_CASES = {}


def _case(N, T, rows, dev):
    """The inputs and, per setting of GNX_OPT_STD_BWD_CENTERED, the two-launch reference: computed once, never changed."""
    from gnnepcsaft_amd import ops
    key = (N, T, rows)
    if key not in _CASES:
        g, dc, m, gout, weffs = _build(N, T, rows, dev)
        fwd = rows == 96
        A = torch.empty(N, T * 4 * F, device=dev)   # required, never read
        dA = torch.full((N, T * 4 * F), float("nan"), device=dev)
        for t in range(T):
            segs, out = [(gout[:, t * F:(t + 1) * F], None, weffs[t][0], 4 * F * F)], dA[:, t * 4 * F:(t + 1) * 4 * F]
            assert ops.gemm_plan(segs, out, b_trans=False, dc=dc, forward_tiles=fwd)[0] == "k_gemm_as3"
            ops.gemm_grouped(segs, out, dc, b_trans=False, forward_tiles=fwd)
        assert not torch.isnan(dA).any()
        ref = {}
        for centered in (1, 0):
            ops.set_option(dev, _lib.OPT_STD_BWD_CENTERED, centered)
            try:
                ref[centered] = _i32(ops.pna_aggregate_bwd(dA, m, A, g, T, F)).clone()
            finally:
                ops.set_option(dev, _lib.OPT_STD_BWD_CENTERED, 1)
        assert not torch.equal(ref[0], ref[1])   # the option reaches the arithmetic
        _CASES[key] = (g, dc, m, gout, weffs, A, ref)
    return _CASES[key]


@pytest.mark.parametrize("centered", [1, 0], ids=["centered", "forward_std"])
@pytest.mark.parametrize("rows", [128, 96])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("N", [4096, 4097, 4096 + 193])
def test_fused_equals_the_two_launches_bit_for_bit(gpu_device, N, T, rows, centered):
    from gnnepcsaft_amd import ops
    dev = torch.device("cuda:0")
    g, dc, m, gout, weffs, A, ref = _case(N, T, rows, dev)
    E, H = m.shape
    for fused_opt in (1, 0):
        buf = torch.full((E + 3, H), CANARY, device=dev)
        dA = torch.full((N, T * 4 * F), CANARY, device=dev)
        ops.set_option(dev, _lib.OPT_STD_BWD_CENTERED, centered)
        ops.set_option(dev, _lib.OPT_DA_AGG_FUSED, fused_opt)
        try:
            dm, fused = ops.pna_dA_aggregate_bwd(gout, weffs, m, A, g, dc, T, F, dA=dA, dm=buf[:E], forward_tiles=rows == 96)
        finally:
            ops.set_option(dev, _lib.OPT_STD_BWD_CENTERED, 1)
            ops.set_option(dev, _lib.OPT_DA_AGG_FUSED, 1)
        assert fused == bool(fused_opt), "the plan did not take the fused kernel" if fused_opt else "the option did not switch it off"
        assert torch.equal(_i32(dm), ref[centered]), (fused_opt, int((_i32(dm) != ref[centered]).sum()))
        assert bool((buf[E:] == CANARY).all())
        if fused:
            assert bool((dA == CANARY).all())   # dA is neither written nor needed


def test_layer_backward_with_and_without_the_fused_launch(gpu_device, monkeypatch):
    """gnx_pna_conv_bwd on a batch of 5120 atoms (F = 128, one tower), GNX_OPT_DA_AGG_FUSED on against off: dx, dP, dQ and
    the message gradients bit-identical; with the option on the layer's dA buffer is never written."""
    from gnnepcsaft_amd import dp, functional as Fn, ops, pna_native
    from gnnepcsaft_amd.data import calc_deg, default_config, synthetic_batch
    from gnnepcsaft_amd.train.models import create_model
    dev = torch.device("cuda:0")
    cfg = default_config(2)
    cfg.update(hidden_dim=128, propagation_depth=1)
    batch = synthetic_batch(256, 2, molecule_like=True)
    deg = calc_deg(batch)
    b = batch.to("cuda:0")
    seen = []
    inner = pna_native.conv_bwd

    def recording(*args, **kw):
        kw["dA"].fill_(CANARY)
        keep = inner(*args, **kw)
        seen.append({k: _i32(kw[k]).clone() for k in ("dx", "dPQ", "gebuf")})
        seen[-1]["dA_untouched"] = bool((kw["dA"] == CANARY).all())
        return keep
    monkeypatch.setattr(pna_native, "conv_bwd", recording)
    runs = {}
    try:
        Fn.set_grad_in_place(True)   # the native layer backward accumulates straight into the flat gradient buffer
        for fused_opt in (1, 0):
            ops.set_option(dev, _lib.OPT_DA_AGG_FUSED, fused_opt)
            torch.manual_seed(0)
            m = create_model(copy.deepcopy(cfg), deg).to("cuda:0").train()
            m.model.max_degree_hint = len(deg) - 1
            flat = dp.FlatGradAllReduce(m)
            flat.zero_grad()
            b._gnx_pack = None
            seen.clear()
            loss = m.training_step(b, 0)
            loss.backward()
            torch.cuda.synchronize()
            assert len(seen) == 1
            runs[fused_opt] = (float(loss.detach()), dict(seen[0]))
    finally:
        Fn.set_grad_in_place(False)
        ops.set_option(dev, _lib.OPT_DA_AGG_FUSED, 1)
    assert runs[1][0] == runs[0][0]
    assert runs[1][1]["dA_untouched"] and not runs[0][1]["dA_untouched"]
    for k in ("gebuf", "dPQ", "dx"):
        assert torch.equal(runs[1][1][k], runs[0][1][k]), k
