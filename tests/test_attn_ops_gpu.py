"""The attention kernels of csrc/gnx_attn.hip at op level (ops.transformer_attn_fwd / _bwd / _dle), entry by entry
against the fp64 references and derived bounds of tests/attn_ref.py, at every thread layout (NV = 1, 2, 4 chunks of 256
columns), head layout (C = 4 .. 1024: one lane per head, groups of lanes, a head over two, three and four chunks; 3, 5,
65, 129 and 256 heads), on hubs, nodes without edges, doubled edges, self-loops and the 128-entry chunk edges of
k_attn_dle, with inputs that make the softmax sharp ("sharp": spreads of 40 .. several hundred, alpha that underflows to
0) or put it at risk of overflow ("offset": a common score term of +-128), and with dropout masks across Philox blocks.

No tolerance here is a literal: every bound comes from tests/attn_ref.py, whose docstring derives it, and
tests/test_attn_ref_cpu.py shows that plain fp32 evaluations satisfy every bound and eight mutations do not.  The
backward is fed the reference alpha rounded to fp32, so it does not inherit the forward's error, and the four sums are
held to the fp64 sums of the kernel's own scratch read back.

Every test prints its worst err / bound per array and the worst so far per thread layout.  Recorded on an MI355X over
all layouts, graphs, input kinds and dropout rates (a record, not asserted):

    kernel          array    NV = 1   NV = 2   NV = 4
    k_attn_fwd      alpha    0.357    0.281    0.348
    k_attn_fwd      out      0.996    0.992    0.993   (the skip addition alone may use u |out|, the bound's last term)
    k_attn_bwd_dst  dscore   0.349    0.251    0.348
    k_attn_bwd_dst  alphad   0.667    0.667    0.667
    k_attn_bwd_dst  dq       0.514    0.536    0.544
    k_attn_bwd_src  dk       0.569    0.545    0.552
    k_attn_bwd_src  dv       0.545    0.541    0.615
    k_attn_dle      dLe      0.393    0.453    0.470   (both entry points)

The NV = 4 instantiations (H > 512), first run under test here, stayed inside every bound on every case.
"""
import math

import numpy as np
import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu

CASES = [(hw, g) for hw in A.ALL_LAYOUTS for g in A.graphs_for(hw)]
CASE_IDS = [f"{hw[0]}x{hw[1]}-{g.name}" for hw, g in CASES]
DROPOUT_CASES = [(hw, g, p) for hw in A.DROPOUT_LAYOUTS for g in A.graphs_for(hw) for p in A.DROPOUT_P]
DROPOUT_IDS = [f"{hw[0]}x{hw[1]}-{g.name}-p{p}" for hw, g, p in DROPOUT_CASES]
SEED, OFFSET = 0x9E3779B97F4A7C15, 3

_PACKS = {}
_ALPHA32 = {}  # (layout, graph, kind) -> reference alpha rounded to fp32 (it does not depend on the dropout mask)
WORST = {}


def _pack(g, dev):
    from gnnepcsaft_amd import ops
    if g.name not in _PACKS:
        _PACKS[g.name] = ops.pack_graph(g.edge_index.to(dev), g.edge_attr.to(dev), None, g.N, bond_dims=g.bond_dims)
    return _PACKS[g.name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _record(layout, ratios):
    nv = 1 if layout[0] <= 256 else 2 if layout[0] <= 512 else 4
    for n, r in ratios.items():
        WORST[f"NV{nv}.{n}"] = max(WORST.get(f"NV{nv}.{n}", 0.0), r)


def _report(what, ratios):
    print(what, {n: round(r, 3) for n, r in ratios.items()})
    print("worst so far", {n: round(r, 3) for n, r in sorted(WORST.items())})


def _forward(dev, layout, g, kind, p=0.0):
    """Forward on the GPU against the fp64 reference (the keep mask, if any, taken from the kernel as data); returns
    (worst ratios, keep mask on the CPU)."""
    from gnnepcsaft_amd import ops
    H, heads = layout
    gp = _pack(g, dev)
    src, dst, code = g.csr()
    inp = A.inputs(g, H, heads, kind)
    out, alpha, keep = ops.transformer_attn_fwd(inp.qkvs.to(dev), inp.Le.to(dev), gp, heads, p, SEED, OFFSET,
                                                want_mask=p > 0)
    out, alpha = out.cpu(), alpha.cpu()
    keep = None if keep is None else keep.cpu()
    fw = A.fwd_ref(inp.qkvs, inp.Le, src, dst, code, g.N, heads, keep, p, exact=inp.exact)
    _ALPHA32[(layout, g.name, kind)] = fw.alpha.float()
    what = f"{g.name} {H}x{heads} {kind} p={p}"
    ratios = {"alpha": A.assert_within(alpha, fw.alpha, fw.alpha_bound, what + " alpha"),
              "out": A.assert_within(out, fw.out, fw.out_bound, what + " out")}
    lone = fw.deg == 0
    assert torch.equal(_bits(out[lone]), _bits(inp.qkvs[:, 3 * H:][lone])), what + ": out != skip without in-edges"
    single = (fw.deg == 1)[dst]
    assert torch.equal(_bits(alpha[single]), _bits(torch.ones_like(alpha[single]))), what + ": alpha != 1 at D = 1"
    key = (dst * g.N + src) * A.CODES + code  # the copies of a doubled edge are neighbours under a stable sort
    order = torch.from_numpy(np.argsort(key.numpy(), kind="stable"))
    twin = key[order][1:] == key[order][:-1]
    if g.name == "loops_dups":
        assert int(twin.sum()) >= g.E // 2
    assert torch.equal(_bits(alpha[order][1:][twin]), _bits(alpha[order][:-1][twin])), what + ": doubled edges differ"
    return ratios, keep


def _alpha32(layout, g, kind):
    k = (layout, g.name, kind)
    if k not in _ALPHA32:
        src, dst, code = g.csr()
        inp = A.inputs(g, layout[0], layout[1], kind)
        _ALPHA32[k] = A.fwd_ref(inp.qkvs, inp.Le, src, dst, code, g.N, layout[1], exact=inp.exact).alpha.float()
    return _ALPHA32[k]


def _backward(dev, layout, g, kind, p=0.0):
    """(dq|dk|dv, scratch, dLe of that call, dLe of transformer_attn_dle on the same scratch), on the CPU."""
    from gnnepcsaft_amd import ops
    H, heads = layout
    gp = _pack(g, dev)
    inp = A.inputs(g, H, heads, kind)
    dout, qkvs, Le = inp.dout.to(dev), inp.qkvs.to(dev), inp.Le.to(dev)
    dqkv, scratch, dLe = ops.transformer_attn_bwd(dout, qkvs, Le, _alpha32(layout, g, kind).to(dev), gp, heads, p, SEED,
                                                  OFFSET)
    pos = gp.code_index(A.CODES) if g.E > 0 else None
    dLe2 = ops.transformer_attn_dle(dout, qkvs, scratch, Le, gp, heads, pos)
    ops.check_range(dev)
    return dqkv.cpu(), scratch.cpu(), dLe.cpu(), dLe2.cpu()


def _check_scratch(layout, g, kind, scratch, p=0.0, keep=None):
    H, heads = layout
    src, dst, code = g.csr()
    inp = A.inputs(g, H, heads, kind)
    alpha32 = _alpha32(layout, g, kind)
    sc = A.scratch_ref(inp.dout, inp.qkvs, inp.Le, alpha32, src, dst, code, g.N, heads, keep, p)
    what = f"{g.name} {H}x{heads} {kind} p={p}"
    dscore, alphad = scratch[0], scratch[1]
    ratios = {"dscore": A.assert_within(dscore, sc.dscore, sc.dscore_bound, what + " dscore"),
              "alphad": A.assert_within(alphad, sc.alphad, sc.alphad_bound, what + " alphad")}
    single = (A.in_degree(dst, g.N) == 1)[dst]
    assert bool((dscore[single] == 0.0).all()), what + ": dscore != 0 at D = 1"
    if p == 0.0:
        assert torch.equal(_bits(alphad), _bits(alpha32)), what + ": alphad is not alpha bit for bit"
    else:
        dropped = keep == 0
        assert bool((alphad[dropped] == 0.0).all()), what + ": alphad != 0 at a dropped entry"
        want = alpha32.double() / (1.0 - p)
        assert bool(((alphad.double() - want).abs()[~dropped] <= (2.0 * A.U * want + A.TINY)[~dropped]).all()), what
    return ratios


def _check_sums(layout, g, kind, dqkv, scratch, dLe, dLe2):
    H, heads = layout
    src, dst, code = g.csr()
    inp = A.inputs(g, H, heads, kind)
    sums = A.sums_ref(inp.dout, inp.qkvs, inp.Le, scratch[0], scratch[1], src, dst, code, g.N, heads)
    what = f"{g.name} {H}x{heads} {kind}"
    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    ratios = {"dq": A.assert_sum(dq, sums["dq"], "dq", what), "dk": A.assert_sum(dk, sums["dk"], "dk", what),
              "dv": A.assert_sum(dv, sums["dv"], "dv", what),
              "dLe": max(A.assert_sum(dLe, sums["dLe"], "dLe", what + " (attn_bwd)"),
                         A.assert_sum(dLe2, sums["dLe"], "dLe", what + " (attn_dle)"))}
    no_in = A.in_degree(dst, g.N) == 0
    no_out = A.in_degree(src, g.N) == 0
    assert bool((dq[no_in] == 0.0).all()), what + ": dq != 0 without in-edges"
    assert bool((dk[no_out] == 0.0).all()) and bool((dv[no_out] == 0.0).all()), what + ": dk|dv != 0 without out-edges"
    return ratios


def _merge(total, ratios):
    for n, r in ratios.items():
        total[n] = max(total.get(n, 0.0), r)


@pytest.mark.parametrize("layout,g", CASES, ids=CASE_IDS)
def test_forward(gpu_device, layout, g):
    total = {}
    for kind in A.KINDS:
        _merge(total, _forward(gpu_device, layout, g, kind)[0])
    _record(layout, total)
    _report(f"forward {layout} {g.name}", total)


@pytest.mark.parametrize("layout,g", CASES, ids=CASE_IDS)
def test_backward_scratch(gpu_device, layout, g):
    total = {}
    for kind in A.KINDS:
        _, scratch, _, _ = _backward(gpu_device, layout, g, kind)
        _merge(total, _check_scratch(layout, g, kind, scratch))
    _record(layout, total)
    _report(f"scratch {layout} {g.name}", total)


@pytest.mark.parametrize("layout,g", CASES, ids=CASE_IDS)
def test_backward_sums(gpu_device, layout, g):
    total = {}
    for kind in A.KINDS:
        _merge(total, _check_sums(layout, g, kind, *_backward(gpu_device, layout, g, kind)))
    _record(layout, total)
    _report(f"sums {layout} {g.name}", total)


@pytest.mark.parametrize("layout,g,p", DROPOUT_CASES, ids=DROPOUT_IDS)
def test_dropout(gpu_device, layout, g, p):
    """The mask of ``want_mask=True`` as data: forward and backward as above, and alphad is 0 exactly where the forward
    dropped the entry, so the backward regenerates the forward's mask entry for entry (more than four heads: more than
    one Philox block per edge; NV = 2 and 4: across chunks)."""
    total = {}
    for kind in A.KINDS:
        ratios, keep = _forward(gpu_device, layout, g, kind, p)
        _merge(total, ratios)
        n = keep.numel()
        if n >= 1000:
            frac = float(keep.double().mean())
            assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (frac, n)
        dqkv, scratch, dLe, dLe2 = _backward(gpu_device, layout, g, kind, p)
        _merge(total, _check_scratch(layout, g, kind, scratch, p, keep))
        _merge(total, _check_sums(layout, g, kind, dqkv, scratch, dLe, dLe2))
    _record(layout, total)
    _report(f"dropout {layout} {g.name} p={p}", total)


@pytest.mark.parametrize("heads,C", [(1, 12), (1, 1028), (2, 1024)], ids=["C12", "C1028", "H2048"])
def test_layout_refusal(gpu_device, heads, C):
    """check_layout is a host argument check: GnxError, nothing launched, for all three entries."""
    from gnnepcsaft_amd import _lib, ops
    dev = gpu_device
    g = A.main_graphs()[2]
    gp = _pack(g, dev)
    H = heads * C
    qkvs, Le = torch.zeros(g.N, 4 * H, device=dev), torch.zeros(A.CODES, H, device=dev)
    dout, alpha = torch.zeros(g.N, H, device=dev), torch.zeros(g.E, heads, device=dev)
    with pytest.raises(_lib.GnxError, match="head width"):
        ops.transformer_attn_fwd(qkvs, Le, gp, heads)
    with pytest.raises(_lib.GnxError, match="head width"):
        ops.transformer_attn_bwd(dout, qkvs, Le, alpha, gp, heads, want_dle=False)
    with pytest.raises(_lib.GnxError, match="head width"):
        ops.transformer_attn_dle(dout, qkvs, torch.zeros(2, g.E, heads, device=dev), Le, gp, heads,
                                 gp.code_index(A.CODES))
    ops.check_range(dev)
