"""The gather / scatter kernels of csrc/gnx_aggregate.hip and csrc/gnx_embed.hip, entry by entry against the fp64
references of tests/graph_sum_ref.py: hubs, nodes without edges, doubled edges, the edges of the 128-entry chunks of the
by-code sums, every width that selects another kernel or thread layout, the more-than-64-codes fallbacks, and NaN / Inf.

Sums are held to ``assert_entrywise`` (|got - ref| <= 1.01 (n + extra) 2^-24 sum|term| per entry, exact zero where every
term is zero), maxima and integer arrays to equality.  The ReLU masks are exact (see ``graph_sum_ref.gine_mask``), so no
entry is excluded anywhere.  tests/test_graph_sum_ref_cpu.py shows that the bound accepts plain fp32 sums in any order
and rejects one-edge mutations that the norm-wise metric of tests/test_ops_gpu.py lets through.
"""
import numpy as np
import pytest
import torch

from gnnepcsaft_amd import _lib
from tests import graph_sum_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
CASE_IDS = [g.name for g in CASES]
_PACKS = {}


def _pack(g, dev):
    from gnnepcsaft_amd import ops
    key = (g.name, g.bond_dims)
    if key not in _PACKS:
        _PACKS[key] = ops.pack_graph(g.edge_index.to(dev), g.edge_attr.to(dev), None, g.N, bond_dims=g.bond_dims)
    return _PACKS[key]


def _entry(got, ref, extra=4, what=""):
    R.assert_entrywise(got.cpu(), ref[0], ref[1], ref[2], extra=extra, what=what)


# ----------------------------------------------------------------------------------------------------------------------
# the inverted index by bond code (gnx_group_by_small_key with keys)
# ----------------------------------------------------------------------------------------------------------------------
def _index_graphs(Rc):
    bd = R.BOND_DIMS[Rc]
    return R.cases(bd) + [R.random(50, E, bd) for E in (0, 1, 255, 256, 257, 3000)]  # around the 256-item blocks


@pytest.mark.parametrize("Rc", [1, 60, 64])
@pytest.mark.parametrize("gi", range(len(_index_graphs(60))), ids=[g.name for g in _index_graphs(60)])
def test_code_index_bit_exact(gpu_device, Rc, gi):
    from gnnepcsaft_amd import ops
    g = _index_graphs(Rc)[gi]
    assert g.R == Rc
    gp = _pack(g, gpu_device)
    code = g.csr()[2].numpy()
    assert np.array_equal(gp.code.cpu().numpy(), code)
    pos = gp.code_index(Rc)
    assert pos is not None and pos.dtype == torch.int32
    assert np.array_equal(pos.cpu().numpy()[:g.E], np.argsort(code, kind="stable"))
    ptr = np.zeros(Rc + 1, dtype=np.int64)
    np.cumsum(np.bincount(code, minlength=Rc), out=ptr[1:])
    assert gp._code_index[0] == Rc and np.array_equal(gp._code_index[2].cpu().numpy(), ptr)
    assert gp.code_index(Rc) is pos  # built once
    ops.check_range(gpu_device)


def test_code_index_none_above_64_codes(gpu_device):
    from gnnepcsaft_amd import ops
    g = R.random(50, 257, R.BOND_DIMS[65])
    gp = _pack(g, gpu_device)
    assert gp.code_index(65) is None and ops.bond_code_index(gp, 65, 64) is None
    ops.check_range(gpu_device)


# ----------------------------------------------------------------------------------------------------------------------
# PNA message assembly and its three sums
# ----------------------------------------------------------------------------------------------------------------------
# 4: one quad per row; 7, 250: k_key_segment_sum<1>; 36: 9 threads per row, 28 row lanes, 5 entries each; 200: 5 lanes;
# 260: 3 lanes; 1024: one lane; 1028: no inverted index (bond_code_index is None), the table scatter runs with 60 codes
WIDTHS = [4, 7, 36, 128, 200, 250, 260, 1024, 1028]


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("g", CASES, ids=CASE_IDS)
def test_edge_combine(gpu_device, g, H):
    from gnnepcsaft_amd import ops
    dev = gpu_device
    gp = _pack(g, dev)
    src, dst, code = g.csr()
    for half in (False, True):
        P, Q, Te = R.values((g.N, H), 1, half), R.values((g.N, H), 2, half), R.values((g.R, H), 3, half)
        for relu in (False, True):
            h1 = ops.edge_combine_fwd(P.to(dev), Q.to(dev), Te.to(dev), gp, relu)
            _entry(h1, R.edge_combine_fwd_ref(P, Q, Te, src, dst, code, relu), extra=2, what=f"h1 relu={relu}")
    assert (ops.bond_code_index(gp, g.R, H) is None) == (H == 1028 or g.E == 0)
    gr = R.values((g.E, H), 4)
    dP, dQ, dTe = ops.edge_combine_bwd(gr.to(dev), gp, g.R)
    rP, rQ, rT = R.edge_combine_bwd_ref(gr, src, dst, code, g.N, g.R)
    _entry(dP, rP, what="dP")
    _entry(dQ, rQ, what="dQ")
    _entry(dTe, rT, what="dTe")
    # the rows of nodes without in- / out-edges are written (as zeros), not left as allocated
    dP2, dQ2 = ops.edge_combine_bwd_pq(gr.to(dev), gp)
    indeg, outdeg = np.bincount(dst.numpy(), minlength=g.N), np.bincount(src.numpy(), minlength=g.N)
    assert bool((dP2.cpu()[torch.from_numpy(indeg == 0)] == 0).all())
    assert bool((dQ2.cpu()[torch.from_numpy(outdeg == 0)] == 0).all())
    assert torch.equal(dP2, dP) and torch.equal(dQ2, dQ)
    ops.check_range(dev)


# ----------------------------------------------------------------------------------------------------------------------
# more than 64 codes: k_table_scatter_add<int32_t, 1> from bond codes.  65 codes: 64-column slabs; 300: 32; 600: 16.
# 200 edges: one row chunk, flushed with atomics; 3000 edges: 12 chunks, private tables folded by k_table_reduce.
# ----------------------------------------------------------------------------------------------------------------------
FALLBACK = R.fallback_cases()


@pytest.mark.parametrize("H", [7, 64, 100])
@pytest.mark.parametrize("g", FALLBACK, ids=[f"R{g.R}-E{g.E}" for g in FALLBACK])
def test_bond_table_grad_scatter_fallback(gpu_device, g, H):
    from gnnepcsaft_amd import ops
    gp = _pack(g, gpu_device)
    lib = _lib.load()
    # the geometry this case is here for, from the library's own workspace formula: chunks x slabs x R x CW floats
    cw = 64 if g.R <= 256 else (32 if g.R <= 512 else 16)
    chunks = lib.gnx_table_scatter_workspace_bytes(g.E, g.R, H) // (4 * g.R * cw * -(-H // cw))
    assert chunks == (1 if g.E == 200 else 12)
    code = g.csr()[2]
    gr = R.values((g.E, H), 5)
    dTe = ops.bond_table_grad(gr.to(gpu_device), gp, g.R, None)
    _entry(dTe, R.sum_by(code, g.R, gr), what="dTe")
    ops.check_range(gpu_device)


OFFSETS = [0, 100, 250, 300]


def _embed_inputs(N, H):
    rng = np.random.default_rng([8, N, H])
    idx = torch.from_numpy(np.stack([rng.integers(0, OFFSETS[k + 1] - OFFSETS[k], N) for k in range(3)], 1)).long()
    return idx, R.values((N, H), 6)


# (200, 64): fewer than 256 rows, so the LDS-atomic kernel and not the matrix-core one; (3000, 7): H % 4 != 0, the same
# kernel with 12 row chunks and the two-stage flush; (3000, 64): the same once the matrix-core kernel is switched off
@pytest.mark.parametrize("N,H,mfma_off", [(200, 64, False), (3000, 7, False), (3000, 64, True)])
def test_embed_sum_bwd_table_kernel(gpu_device, N, H, mfma_off):
    from gnnepcsaft_amd import ops
    dev = gpu_device
    idx, dout = _embed_inputs(N, H)
    init = R.values((OFFSETS[-1], H), 7)
    old = ops.set_option(dev, _lib.OPT_EMBED_BWD_MFMA, 0) if mfma_off else None
    try:
        fresh = ops.embed_sum_bwd(idx.to(dev), OFFSETS, dout.to(dev))
        acc = init.clone().to(dev)
        assert ops.embed_sum_bwd(idx.to(dev), OFFSETS, dout.to(dev), out=acc) is acc
    finally:
        if mfma_off:
            ops.set_option(dev, _lib.OPT_EMBED_BWD_MFMA, old)
    _entry(fresh, R.embed_bwd_ref(idx, OFFSETS, dout), what="dtable")
    _entry(acc, R.embed_bwd_ref(idx, OFFSETS, dout, init), what="dtable accumulated")
    ops.check_range(dev)


def test_table_scatter_rejects_a_table_that_does_not_fit(gpu_device):
    """20000 rows exceed the 64 KiB tile even at 8 columns: a returned status before any launch, the table untouched."""
    from gnnepcsaft_amd import ops
    dev = gpu_device
    N, H, rows = 200, 7, 20000
    idx = torch.from_numpy(np.random.default_rng(9).integers(0, rows, (N, 1))).long()
    init = R.values((rows, H), 8)
    acc = init.clone().to(dev)
    with pytest.raises(_lib.GnxError, match="do not fit the LDS tile"):
        ops.embed_sum_bwd(idx.to(dev), [0, rows], R.values((N, H), 9).to(dev), out=acc)
    assert torch.equal(acc.cpu(), init)
    ops.check_range(dev)


# ----------------------------------------------------------------------------------------------------------------------
# GINE aggregate: forward, dx, and dLe through the inverted index (k_gine_dle_segment_sum) by both entry points
# ----------------------------------------------------------------------------------------------------------------------
EPS = [0.0, 0.25, -1.0]  # at -1 the self term vanishes


def _gine_inputs(g, H, half):
    return R.values((g.N, H), 11, half), R.values((g.R, H), 12, half), R.values((g.N, H), 13)


def _gine_fwd_dx(g, gp, x, Le, dout, dev, eps_list):
    """Forward, dx and the dLe of the same call at every eps; ``want_dle=False`` gives the same dx bits and no dLe."""
    from gnnepcsaft_amd import ops
    src, dst, code = g.csr()
    xd, Ld, dd = x.to(dev), Le.to(dev), dout.to(dev)
    # the fp32 mask is the fp64 mask on these inputs: the share of entries excluded from the comparison is 0
    assert torch.equal((x[src] + Le[code]) > 0, R.gine_mask(x, Le, src, code))
    for eps in eps_list:
        _entry(ops.gine_aggregate_fwd(xd, Ld, gp, eps), R.gine_fwd_ref(x, Le, src, dst, code, eps, g.N), what=f"out eps={eps}")
        dx, dLe = ops.gine_aggregate_bwd(dd, xd, Ld, gp, eps)
        rx, rl = R.gine_bwd_ref(dout, x, Le, src, dst, code, eps, g.N)
        _entry(dx, rx, what=f"dx eps={eps}")
        _entry(dLe, rl, what=f"dLe eps={eps}")
        dx2, none = ops.gine_aggregate_bwd(dd, xd, Ld, gp, eps, want_dle=False)
        assert none is None and torch.equal(dx2, dx)


@pytest.mark.parametrize("H", [4, 36, 128, 260])
@pytest.mark.parametrize("g", CASES, ids=CASE_IDS)
def test_gine_aggregate(gpu_device, g, H):
    from gnnepcsaft_amd import ops
    dev = gpu_device
    gp = _pack(g, dev)
    src, dst, code = g.csr()
    for half in (False, True):
        x, Le, dout = _gine_inputs(g, H, half)
        if half and g.E >= 100:  # x + Le == 0 occurs: the strict mask is on trial, and it is exact, so nothing is excluded
            assert int(((x[src] + Le[code]) == 0).sum()) > 0
        _gine_fwd_dx(g, gp, x, Le, dout, dev, EPS)
        pos = gp.code_index(g.R)
        assert pos is not None
        side = ops.gine_dle(dout.to(dev), x.to(dev), Le.to(dev), gp, pos)  # the side-stream entry, same kernel
        _entry(side, R.gine_bwd_ref(dout, x, Le, src, dst, code, 0.0, g.N)[1], what="gine_dle")
    ops.check_range(dev)


# k_gine_bwd_dle, the LDS-privatised table: no inverted index (pos=None), H % 4 != 0, or more than 64 codes; column slabs
# of 64 (60, 65 codes), 32 (300) and 16 (600), the last slab partial at every one of these widths
@pytest.mark.parametrize("H", [7, 64, 100])
@pytest.mark.parametrize("Rc", [60, 65, 300, 600])
def test_gine_dle_lds_table(gpu_device, Rc, H):
    from gnnepcsaft_amd import ops
    dev = gpu_device
    for g in (R.hub(bond_dims=R.BOND_DIMS[Rc]), R.random(300, 1000, R.BOND_DIMS[Rc])):
        gp = _pack(g, dev)
        src, dst, code = g.csr()
        for half in (False, True):
            x, Le, dout = _gine_inputs(g, H, half)
            ref = R.gine_bwd_ref(dout, x, Le, src, dst, code, 0.25, g.N)[1]
            _entry(ops.gine_dle(dout.to(dev), x.to(dev), Le.to(dev), gp, None), ref, what=f"{g.name} gine_dle pos=None")
            # through gine_aggregate_bwd: the LDS kernel above 64 codes and at H = 7, else the inverted index
            _gine_fwd_dx(g, gp, x, Le, dout, dev, [0.25])
    ops.check_range(dev)


# ----------------------------------------------------------------------------------------------------------------------
# segment pool
# ----------------------------------------------------------------------------------------------------------------------
def _ptr(sizes, dev):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)


@pytest.mark.parametrize("mode", ["add", "mean", "max"])
@pytest.mark.parametrize("H", [3, 64, 260])
@pytest.mark.parametrize("sizes", ["edges", "many"])
def test_segment_pool(gpu_device, sizes, H, mode):
    from gnnepcsaft_amd import ops
    dev = gpu_device
    sz = R.POOL_SIZES[sizes]
    N, B = sum(sz), len(sz)
    ptr = _ptr(sz, dev)
    nonempty = torch.tensor(sz) > 0
    for kind in ("randn", "halves", "negative"):
        x = R.values((N, H), 21, kind == "halves")
        if kind == "negative":
            x = -x.abs() - 0.5
        dout = R.values((B, H), 22)
        out = ops.segment_pool_fwd(x.to(dev), ptr, B, mode)
        ref = R.pool_fwd_ref(x, sz, mode)
        if mode == "max":
            assert torch.equal(out.cpu().double(), ref[0]), kind
            if kind == "negative":
                assert bool((out.cpu()[nonempty] < 0).all()) and bool((out.cpu()[~nonempty] == 0).all())
            if kind == "halves":  # the maximum is attained more than once somewhere: the tie split is on trial
                hits = torch.zeros(B, H).index_add_(0, R.segment_index(sz), (x == out.cpu()[R.segment_index(sz)]).float())
                assert int((hits > 1).sum()) > 0
        else:
            _entry(out, ref, what=f"{mode} {kind}")
        dx = ops.segment_pool_bwd(dout.to(dev), x.to(dev), out, ptr, B, mode)
        _entry(dx, R.pool_bwd_ref(dout, x, sz, mode), what=f"{mode} bwd {kind}")
    ops.check_range(dev)


# ----------------------------------------------------------------------------------------------------------------------
# NaN / Inf: one non-finite input element; the NaN entries and the infinite entries of the result are the reference's
# ----------------------------------------------------------------------------------------------------------------------
BAD = {"nan": float("nan"), "inf": float("inf")}


def _poke(t, row, col, v):
    t = t.clone()
    t[row, col] = v
    return t


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("mode", ["add", "mean", "max"])
def test_pool_nonfinite(gpu_device, mode, kind):
    """A NaN anywhere in a segment is the segment's result in every mode (``scatter_reduce_(amax)`` propagates it; fmaxf
    did not, and max pooling replaced a NaN activation by a finite number).  Backward of max: the oracle's autograd gives
    NaN on every row of that segment and channel (its gradient / #ties is g / 0 times a zero mask), so k_pool_bwd
    returns the NaN maximum there instead of 0."""
    from gnnepcsaft_amd import ops
    dev = gpu_device
    sz = R.POOL_SIZES["edges"]
    N, B = sum(sz), len(sz)
    ptr = _ptr(sz, dev)
    first = np.concatenate([[0], np.cumsum(sz)])
    for H in (3, 64):
        # first, middle and last row of the long segment (in and after the 4-row loop), the only row of a 1-row segment,
        # the remainder row of the 5-row segment
        for row in (int(first[8]), int(first[8]) + 150, int(first[9]) - 1, int(first[1]), int(first[5]) + 4):
            x = _poke(R.values((N, H), 31), row, H - 1, BAD[kind])
            out = ops.segment_pool_fwd(x.to(dev), ptr, B, mode)
            ref = R.pool_fwd_ref(x, sz, mode)[0]
            R.same_nonfinite(out, ref, what=f"{mode} H={H} row={row}")
            assert int((~torch.isfinite(ref)).sum()) == 1
            dout = R.values((B, H), 32)
            dx = ops.segment_pool_bwd(dout.to(dev), x.to(dev), out, ptr, B, mode)
            R.same_nonfinite(dx, R.pool_bwd_ref(dout, x, sz, mode)[0], what=f"{mode} bwd H={H} row={row}")
    ops.check_range(dev)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_gine_fwd_nonfinite(gpu_device, kind):
    """relu(NaN) is NaN in the reference: a NaN in x reaches every neighbour's sum, one in Le every edge of that code."""
    from gnnepcsaft_amd import ops
    dev = gpu_device
    g = R.hub()
    gp = _pack(g, dev)
    src, dst, code = g.csr()
    for H in (7, 36):
        x, Le, _ = _gine_inputs(g, H, False)
        for eps in (0.25, -1.0):
            for xs, Ls in ((_poke(x, 1, H - 1, BAD[kind]), Le), (_poke(x, 5, 0, BAD[kind]), Le),
                           (x, _poke(Le, int(code[0]), 2, BAD[kind]))):
                out = ops.gine_aggregate_fwd(xs.to(dev), Ls.to(dev), gp, eps)
                ref = R.gine_fwd_ref(xs, Ls, src, dst, code, eps, g.N)[0]
                assert int((~torch.isfinite(ref)).sum()) > 1
                R.same_nonfinite(out, ref, what=f"H={H} eps={eps}")
    ops.check_range(dev)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_edge_combine_fwd_nonfinite(gpu_device, kind):
    from gnnepcsaft_amd import ops
    dev = gpu_device
    g = R.hub()
    gp = _pack(g, dev)
    src, dst, code = g.csr()
    for H in (7, 36):
        P, Q, Te = R.values((g.N, H), 1), R.values((g.N, H), 2), R.values((g.R, H), 3)
        for relu in (False, True):
            for Ps, Qs, Ts in ((_poke(P, 0, 1, BAD[kind]), Q, Te), (P, _poke(Q, 1, H - 1, BAD[kind]), Te),
                               (P, Q, _poke(Te, int(code[0]), 0, BAD[kind]))):
                h1 = ops.edge_combine_fwd(Ps.to(dev), Qs.to(dev), Ts.to(dev), gp, relu)
                ref = R.edge_combine_fwd_ref(Ps, Qs, Ts, src, dst, code, relu)[0]
                assert int((~torch.isfinite(ref)).sum()) >= 1
                R.same_nonfinite(h1, ref, what=f"H={H} relu={relu}")
    ops.check_range(dev)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_pna_edge_fwd_h1_nonfinite(gpu_device, kind):
    """The fused edge kernel forms h1 with k_edge_combine_fwd's expression, ReLU included: the same non-finite entries."""
    from gnnepcsaft_amd import ops
    dev = gpu_device
    g = R.tail_empty()
    gp = _pack(g, dev)
    src, dst, code = g.csr()
    maxdeg = int(np.bincount(dst.numpy()).max())
    assert maxdeg <= 16
    T, F = 2, 32
    H = T * F
    P, Q, Te = R.values((g.N, H), 1), R.values((g.N, H), 2), R.values((g.R, H), 3)
    Ws = [(R.values((F, F), 40 + t) / F ** 0.5).to(dev) for t in range(T)]
    bs = [R.values((F,), 50 + t).to(dev) for t in range(T)]
    for Ps, Qs, Ts in ((_poke(P, int(dst[0]), 1, BAD[kind]), Q, Te), (P, _poke(Q, int(src[-1]), H - 1, BAD[kind]), Te),
                       (P, Q, _poke(Te, int(code[100]), F, BAD[kind]))):
        h1, _, _ = ops.pna_edge_fwd(Ps.to(dev), Qs.to(dev), Ts.to(dev), gp, T, F, Ws, bs, maxdeg)
        ref = R.edge_combine_fwd_ref(Ps, Qs, Ts, src, dst, code, True)[0]
        assert int((~torch.isfinite(ref)).sum()) >= 1
        R.same_nonfinite(h1, ref, what="fused h1")
        assert torch.equal(h1.cpu().nan_to_num(7.0, 8.0, 9.0),
                           ops.edge_combine_fwd(Ps.to(dev), Qs.to(dev), Ts.to(dev), gp, True).cpu().nan_to_num(7.0, 8.0, 9.0))
    ops.check_range(dev)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_by_code_sums_nonfinite(gpu_device, kind):
    """dP / dQ / dTe through the inverted index (H = 36, and 7 for the one-channel kernel) and through the table scatter
    (pos=None; direct flush at 65 codes and 200 edges, two-stage at 3000): both skip zeros when flushing, never a NaN."""
    from gnnepcsaft_amd import ops
    dev = gpu_device
    g = R.hub()
    gp = _pack(g, dev)
    src, dst, code = g.csr()
    for H in (7, 36):
        gr = _poke(R.values((g.E, H), 4), 129, H - 1, BAD[kind])
        refs = R.edge_combine_bwd_ref(gr, src, dst, code, g.N, g.R)
        for got, ref, what in zip(ops.edge_combine_bwd(gr.to(dev), gp, g.R), refs, ("dP", "dQ", "dTe")):
            assert int((~torch.isfinite(ref[0])).sum()) == 1
            R.same_nonfinite(got, ref[0], what=f"{what} H={H}")
        R.same_nonfinite(ops.bond_table_grad(gr.to(dev), gp, g.R, None), refs[2][0], what=f"dTe pos=None H={H}")
    for g in FALLBACK[:2]:
        gp = _pack(g, dev)
        gr = _poke(R.values((g.E, 7), 5), g.E - 1, 3, BAD[kind])
        R.same_nonfinite(ops.bond_table_grad(gr.to(dev), gp, g.R, None), R.sum_by(g.csr()[2], g.R, gr)[0],
                         what=f"dTe {g.name} R={g.R}")
    ops.check_range(dev)
