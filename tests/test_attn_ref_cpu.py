"""The fp64 references and the bounds of tests/attn_ref.py, checked without a GPU:

* pin: composed with the five linear maps they equal the fp64 autograd of ``tests/transformer_ref.TransformerConv`` to
  1e-12 on out, dx, dBE and every parameter gradient (one case replays a given dropout mask);
* the "sharp" and "offset" inputs are what they claim, and their per-head dot products are exact in fp32 in any order
  (summed forwards, backwards and pairwise they equal the fp64 value bit for bit, and 4 sum |q k'| < 2^24 on the grid
  of quarters shows it for every other order), which is why their score bound drops the (C + 1) T term;
* a plain fp32 evaluation of every stage in torch on the CPU -- two-pass and online softmax, CSR order and every row's
  edges reversed -- lies inside every bound on every layout, graph, input kind and dropout rate of the GPU file, and
  over all of these no bound is vacuous (rho <= 1e-3; out and dscore bounds <= 1e-3 of the row's sum |term|);
* eight mutations of that fp32 evaluation each leave a bound in at least one entry, and the first three pass the
  norm-wise 1e-5 metric of tests/test_transformer_gpu.py on random(300, 1000) -- the reason for this file.
"""
import math
from typing import NamedTuple, Optional

import numpy as np
import pytest
import torch

from tests import attn_ref as A
from tests import graph_sum_ref as R
from tests.parity_util import rel_err
from tests.transformer_ref import TransformerConv

ARRAYS = ("alpha", "out", "dscore", "alphad", "dq", "dk", "dv", "dLe")


# ----------------------------------------------------------------------------------------------------------------------
# pin against fp64 autograd
# ----------------------------------------------------------------------------------------------------------------------
def _close(a, b, what):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), what


PIN = [(R.random(300, 1000), 0.0), (R.hub(400, 300), 0.25), (R.loops_dups(), 0.0)]


@pytest.mark.parametrize("H,heads", [(8, 2), (24, 3)])
@pytest.mark.parametrize("g,p", PIN, ids=[g.name for g, _ in PIN])
def test_references_match_fp64_autograd(g, p, H, heads):
    torch.manual_seed(1)
    conv = TransformerConv(H, H // heads, heads, dropout=p, edge_dim=H).double()
    x = torch.randn(g.N, H, dtype=torch.float64, requires_grad=True)
    BE = torch.randn(A.CODES, H, dtype=torch.float64, requires_grad=True)
    G = torch.randn(g.N, H, dtype=torch.float64)
    src, dst, code = g.csr()
    keep = A.keep_mask(g.E, heads, p) if p else None  # CSR order
    if keep is not None:
        conv.keep = torch.empty_like(keep)
        conv.keep[g.perm] = keep  # the restatement takes it in the original edge order
    out = conv(x, g.edge_index, BE.index_select(0, g.code))
    (out * G).sum().backward()

    lins = (conv.lin_query, conv.lin_key, conv.lin_value, conv.lin_skip)
    with torch.no_grad():
        qkvs = torch.cat([lin(x) for lin in lins], 1)
        Le = conv.lin_edge(BE)
    fw = A.fwd_ref(qkvs, Le, src, dst, code, g.N, heads, keep, p)
    sc = A.scratch_ref(G, qkvs, Le, fw.alpha, src, dst, code, g.N, heads, keep, p)
    sm = A.sums_ref(G, qkvs, Le, sc.dscore, sc.alphad, src, dst, code, g.N, heads)
    d = {"lin_query": sm["dq"][0], "lin_key": sm["dk"][0], "lin_value": sm["dv"][0], "lin_skip": G}
    _close(fw.out, out.detach(), "out")
    _close(sum(d[n] @ getattr(conv, n).weight.detach() for n in d), x.grad, "dx")
    _close(sm["dLe"][0] @ conv.lin_edge.weight.detach(), BE.grad, "dBE")
    _close(sm["dLe"][0].t() @ BE.detach(), conv.lin_edge.weight.grad, "lin_edge.weight")
    for n in d:
        _close(d[n].t() @ x.detach(), getattr(conv, n).weight.grad, n + ".weight")
        _close(d[n].sum(0), getattr(conv, n).bias.grad, n + ".bias")


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
LAYOUT_IDS = [f"{H}x{h}" for H, h in A.ALL_LAYOUTS]


def _sum_forwards(prod):  # prod [C, M] fp32: one fp32 addition per term, in exactly this order
    acc = torch.zeros_like(prod[0])
    for c in range(prod.size(0)):
        acc = acc + prod[c]
    return acc


def _sum_pairwise(prod):
    n = 1
    while n < prod.size(0):
        n *= 2
    prod = torch.cat([prod, torch.zeros(n - prod.size(0), prod.size(1))])
    while prod.size(0) > 1:
        prod = prod[0::2] + prod[1::2]
    return prod[0]


@pytest.mark.parametrize("H,heads", A.ALL_LAYOUTS, ids=LAYOUT_IDS)
def test_sharp_and_offset_dot_products_are_exact_in_fp32(H, heads):
    C = H // heads
    for g in A.graphs_for((H, heads)):
        src, dst, code = g.csr()
        for kind in ("sharp", "offset"):
            inp = A.inputs(g, H, heads, kind)
            assert inp.exact
            q, k = inp.qkvs[:, :H], inp.qkvs[:, H:2 * H]
            kp = k[src] + inp.Le[code]
            assert torch.equal(kp.double(), k.double()[src] + inp.Le.double()[code])
            prod = (q[dst] * kp).view(g.E, heads, C)
            p64 = q.double()[dst].view(g.E, heads, C) * kp.double().view(g.E, heads, C)
            assert torch.equal(prod.double(), p64)
            ref = p64.sum(-1).reshape(-1)
            # every term is a multiple of 1/4 and the absolute sum stays below 2^24 quarters: exact in ANY order
            assert torch.equal(p64 * 4, (p64 * 4).round())
            assert g.E == 0 or float(p64.abs().sum(-1).max()) * 4 < 2 ** 24
            t = prod.permute(2, 0, 1).reshape(C, -1).contiguous()
            for s in (_sum_forwards(t), _sum_forwards(t.flip(0)), _sum_pairwise(t)):
                assert s.dtype == torch.float32 and torch.equal(s.double(), ref), (g.name, kind)


@pytest.mark.parametrize("H,heads", A.ALL_LAYOUTS, ids=LAYOUT_IDS)
def test_sharp_and_offset_inputs_are_what_they_claim(H, heads):
    for g in A.main_graphs():
        src, dst, code = g.csr()
        inp = A.inputs(g, H, heads, "sharp")
        fw = A.fwd_ref(inp.qkvs, inp.Le, src, dst, code, g.N, heads, exact=True)
        sp = fw.spread.max(1).values
        assert bool(((sp >= 40) & (sp <= 90)).any()) and bool((sp > 110).any()), (g.name, float(sp.max()))
        assert bool((fw.alpha < 2.0 ** -150).any())  # rounds to exactly 0 in fp32
        assert bool((fw.alpha.float() == 0).any())
        inp = A.inputs(g, H, heads, "offset")
        fw = A.fwd_ref(inp.qkvs, inp.Le, src, dst, code, g.N, heads, exact=True)
        assert float(fw.score.abs().min()) >= 100.0 and float(fw.spread.max()) <= 20.0
        assert bool((fw.score > 100).any()) and bool((fw.score < -100).any())
        assert not bool(torch.isfinite(torch.exp(fw.score.float())).all())  # expf overflows without the maximum


# ----------------------------------------------------------------------------------------------------------------------
# fp32 evaluation of every stage in plain torch
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    """Inputs and references of one (graph, layout, kind, p); the backward is fed the reference alpha rounded to
    fp32."""

    def __init__(self, g, layout, kind, p=0.0):
        self.g, (self.H, self.heads), self.kind, self.p = g, layout, kind, p
        self.N, self.E = g.N, g.E
        self.edges = g.csr()
        self.inp = A.inputs(g, self.H, self.heads, kind)
        self.keep = A.keep_mask(g.E, self.heads, p) if p else None
        src, dst, code = self.edges
        i = self.inp
        self.fw = A.fwd_ref(i.qkvs, i.Le, src, dst, code, g.N, self.heads, self.keep, p, exact=i.exact)
        self.alpha32 = self.fw.alpha.float()
        self.sc = A.scratch_ref(i.dout, i.qkvs, i.Le, self.alpha32, src, dst, code, g.N, self.heads, self.keep, p)

    def true_sums(self):
        src, dst, code = self.edges
        i = self.inp
        return A.sums_ref(i.dout, i.qkvs, i.Le, self.sc.dscore, self.sc.alphad, src, dst, code, self.N, self.heads)


class Eval(NamedTuple):
    alpha: torch.Tensor
    out: torch.Tensor
    dscore: torch.Tensor
    alphad: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor
    dLe: torch.Tensor


def _by_rank(dst, N):
    """Edge ids grouped by their rank among the edges of the same row, in the order given."""
    E = int(dst.numel())
    if E == 0:
        return []
    order = torch.from_numpy(np.argsort(dst.numpy(), kind="stable"))
    start = torch.zeros(N + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    rank = torch.empty(E, dtype=torch.int64)
    rank[order] = torch.arange(E) - start[dst[order]]
    by = torch.from_numpy(np.argsort(rank.numpy(), kind="stable"))
    return list(by.split(torch.bincount(rank).tolist()))


def evaluate(case: Case, online: bool, reverse: bool = False, edges=None, keep=None, alpha_in=None,
             sqrt_c: Optional[float] = None, no_max: bool = False, s_without_dropout: bool = False,
             shift_head_at: Optional[int] = None, backward: bool = True) -> Eval:
    """Every stage in fp32.  ``edges`` / ``keep`` / ``alpha_in`` replace the case's own (mutations); ``reverse`` walks
    the edge arrays backwards, so every row's edges and every index sum are taken in the opposite order.  The online
    softmax walks every row edge by edge; the two-pass one and the backward sum with ``index_add_`` in the order of the
    edge arrays.  The backward does not depend on ``online``: ``backward=False`` leaves its arrays None."""
    src, dst, code = case.edges if edges is None else edges
    keep = case.keep if keep is None else keep
    alpha_in = case.alpha32 if alpha_in is None else alpha_in
    if reverse:
        src, dst, code, alpha_in = src.flip(0), dst.flip(0), code.flip(0), alpha_in.flip(0)
        keep = None if keep is None else keep.flip(0)
        if shift_head_at is not None:
            shift_head_at = int(src.numel()) - 1 - shift_head_at
    N, H, heads = case.N, case.H, case.heads
    C, E = H // heads, int(src.numel())
    f32 = torch.float32
    q, k, v, s = case.inp.qkvs.split(H, 1)
    dout, le = case.inp.dout, case.inp.Le[code]
    kp, vp = (k[src] + le).view(E, heads, C), (v[src] + le).view(E, heads, C)
    rc = torch.tensor(float(C) if sqrt_c is None else sqrt_c, dtype=f32)
    rc = rc.sqrt() if sqrt_c is None else rc
    sc = (q[dst].view(E, heads, C) * kp).sum(-1) / rc
    if case.p and keep is not None:
        one = torch.tensor(1.0, dtype=f32)
        d = keep.to(f32) * (one / (one - torch.tensor(case.p, dtype=f32)))
    else:
        d = torch.ones(E, heads, dtype=f32)
    l = torch.zeros(N, heads, dtype=f32)
    acc = torch.zeros(N, heads, C, dtype=f32)
    if no_max:
        m = torch.zeros(N, heads, dtype=f32)
    elif online:
        m = torch.full((N, heads), -math.inf, dtype=f32)
    else:
        m = torch.zeros(N, heads, dtype=f32).scatter_reduce(0, dst.view(-1, 1).expand(E, heads), sc, "amax",
                                                            include_self=False)
    if online and not no_max:
        for e in _by_rank(dst, N):
            rows = dst[e]
            mn = torch.maximum(m[rows], sc[e])
            r, w = torch.exp(m[rows] - mn), torch.exp(sc[e] - mn)
            l[rows] = l[rows] * r + w
            acc[rows] = acc[rows] * r.unsqueeze(-1) + (w * d[e]).unsqueeze(-1) * vp[e]
            m[rows] = mn
    else:
        w = torch.exp(sc - m[dst])
        l.index_add_(0, dst, w)
        acc.index_add_(0, dst, (w * d).unsqueeze(-1) * vp)
    inv = 1.0 / (l + 1e-16)
    out = (acc * inv.unsqueeze(-1)).view(N, H) + s
    alpha = torch.exp(sc - m[dst]) / (l[dst] + 1e-16)
    if reverse:
        alpha = alpha.flip(0)
    if not backward:
        return Eval(alpha, out, None, None, None, None, None, None)

    # backward, from the given alpha
    dot = (dout[dst].view(E, heads, C) * vp).sum(-1)
    da = dot * d
    S = torch.zeros(N, heads, dtype=f32).index_add_(0, dst, alpha_in * (dot if s_without_dropout else da))
    a_b = alpha_in
    if shift_head_at is not None:
        a_b = alpha_in.clone()
        a_b[shift_head_at] = alpha_in[shift_head_at].roll(-1)
    dscore = a_b * (da - S[dst]) / rc
    alphad = alpha_in * d
    ds, ad = dscore.repeat_interleave(C, dim=1), alphad.repeat_interleave(C, dim=1)
    tq, tg = ds * q[dst], ad * dout[dst]
    dq = torch.zeros(N, H, dtype=f32).index_add_(0, dst, ds * kp.view(E, H))
    dk = torch.zeros(N, H, dtype=f32).index_add_(0, src, tq)
    dv = torch.zeros(N, H, dtype=f32).index_add_(0, src, tg)
    dLe = torch.zeros(A.CODES, H, dtype=f32).index_add_(0, code, tq + tg)
    if reverse:
        dscore, alphad = dscore.flip(0), alphad.flip(0)
    return Eval(alpha, out, dscore, alphad, dq, dk, dv, dLe)


def compare(case: Case, ev: Eval, strict: bool):
    """Worst err / bound ratio per array; outside a bound: raises if ``strict``, else the ratio is inf."""
    src, dst, code = case.edges
    i, fw, sc = case.inp, case.fw, case.sc
    sums = None if ev.dscore is None else A.sums_ref(i.dout, i.qkvs, i.Le, ev.dscore, ev.alphad, src, dst, code,
                                                      case.N, case.heads)
    what = f"{case.g.name} {case.H}x{case.heads} {case.kind} p={case.p}"
    checks = {"alpha": lambda: A.assert_within(ev.alpha, fw.alpha, fw.alpha_bound, what + " alpha"),
              "out": lambda: A.assert_within(ev.out, fw.out, fw.out_bound, what + " out"),
              "dscore": lambda: A.assert_within(ev.dscore, sc.dscore, sc.dscore_bound, what + " dscore"),
              "alphad": lambda: A.assert_within(ev.alphad, sc.alphad, sc.alphad_bound, what + " alphad")}
    for n in ("dq", "dk", "dv", "dLe"):
        checks[n] = lambda n=n: A.assert_sum(getattr(ev, n), sums[n], n, what)
    res = {}
    for n in ARRAYS:
        if getattr(ev, n) is None:
            continue
        try:
            res[n] = checks[n]()
        except AssertionError:
            if strict:
                raise
            res[n] = math.inf
    return res


def _assert_not_vacuous(case: Case):
    fw, sc = case.fw, case.sc
    if case.E == 0:
        return
    assert float(fw.rho.max()) <= 1e-3, float(fw.rho.max())
    assert bool((fw.out_bound <= 1e-3 * fw.out_terms + 1e-30).all())
    assert bool((sc.dscore_bound <= 1e-3 * sc.dscore_terms + 2 * A.TINY).all())


CASES = [(hw, g) for hw in A.ALL_LAYOUTS for g in A.graphs_for(hw)]
WORST = {}


@pytest.mark.parametrize("layout,g", CASES, ids=[f"{hw[0]}x{hw[1]}-{g.name}" for hw, g in CASES])
def test_fp32_is_inside_every_bound_and_no_bound_is_vacuous(layout, g):
    rates = (0.0,) + (A.DROPOUT_P if layout in A.DROPOUT_LAYOUTS else ())
    for p in rates:
        for kind in A.KINDS:
            case = Case(g, layout, kind, p)
            _assert_not_vacuous(case)
            for online in (False, True):
                for reverse in (False, True):
                    res = compare(case, evaluate(case, online, reverse, backward=not online), strict=True)
                    for n, r in res.items():
                        WORST[n] = max(WORST.get(n, 0.0), r)
            if p == 0.0:  # alphad is alpha, bit for bit
                assert torch.equal(evaluate(case, True).alphad, case.alpha32)
    print({n: round(r, 3) for n, r in WORST.items()})


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
def _outside(res):
    return [n for n in ARRAYS if res.get(n) == math.inf]


def _passes_normwise(case: Case, ev: Eval):
    true = dict(alpha=case.fw.alpha, out=case.fw.out, dscore=case.sc.dscore, alphad=case.sc.alphad,
                **{n: r[0] for n, r in case.true_sums().items()})
    errs = {n: rel_err(getattr(ev, n), true[n]) for n in ARRAYS}
    assert max(errs.values()) <= 1e-5, errs


def _quiet_edge(case: Case, candidates, score_mut=None, quiet=True):
    """First candidate position whose largest alpha over the heads is at least 1e-30 and, if ``quiet``, at most 1e-8
    (and stays below 1e-8 under the mutated score): wrong beyond any rounding, and invisible next to the largest
    entry."""
    fw = case.fw
    dst = case.edges[1]
    m = A._row_max(dst, case.N, fw.score)
    top = fw.alpha.max(1).values
    ok = top >= 1e-30
    if quiet:
        ok &= top <= 1e-8
    if score_mut is not None:
        ok &= (score_mut - fw.score).abs().min(1).values >= 1.0
        if quiet:
            ok &= (score_mut - m[dst]).max(1).values <= -19.0
    for p in candidates.tolist():
        if bool(ok[p]):
            return p
    raise AssertionError("no quiet edge among the candidates")


def _scores(case: Case, src, code):
    q, k = case.inp.qkvs.double()[:, :case.H], case.inp.qkvs.double()[:, case.H:2 * case.H]
    C = case.H // case.heads
    kp = k[src] + case.inp.Le.double()[code]
    return (q[case.edges[1]] * kp).view(-1, case.heads, C).sum(-1) / math.sqrt(C)


def _without(t, p):
    return torch.cat([t[:p], t[p + 1:]])


def _with_zero_row(t, p):
    return torch.cat([t[:p], torch.zeros_like(t[:1]), t[p:]])


MUT_GRAPHS = [R.random(300, 1000), R.hub(400, 300)]


@pytest.mark.parametrize("g", MUT_GRAPHS, ids=[g.name for g in MUT_GRAPHS])
@pytest.mark.parametrize("layout", [(24, 3), (320, 5)], ids=["24x3", "320x5"])
def test_mutation_one_edge_dropped(g, layout):
    case = Case(g, layout, "sharp")
    src, dst, code = case.edges
    quiet = g.name.startswith("random")
    rows = torch.arange(case.E) if quiet else (dst == 0).nonzero().view(-1)  # the hub's edges
    p = _quiet_edge(case, rows, quiet=quiet)
    ev = evaluate(case, True, edges=tuple(_without(t, p) for t in case.edges), alpha_in=_without(case.alpha32, p))
    ev = ev._replace(alpha=_with_zero_row(ev.alpha, p), dscore=_with_zero_row(ev.dscore, p),
                     alphad=_with_zero_row(ev.alphad, p))
    compare(case, evaluate(case, True), strict=True)
    assert "alpha" in _outside(compare(case, ev, strict=False))
    if quiet:
        _passes_normwise(case, ev)


@pytest.mark.parametrize("g", MUT_GRAPHS, ids=[g.name for g in MUT_GRAPHS])
@pytest.mark.parametrize("layout", [(24, 3), (320, 5)], ids=["24x3", "320x5"])
@pytest.mark.parametrize("what", ["src", "code"])
def test_mutation_src_shifted_on_last_edge_of_a_row_or_bond_code_changed(g, layout, what):
    case = Case(g, layout, "sharp")
    src, dst, code = case.edges
    if what == "src":
        mut_src, mut_code = (src + 1) % case.N, code
        candidates = (torch.cumsum(torch.bincount(dst, minlength=case.N), 0) - 1)[case.fw.deg > 0]  # last of each row
    else:
        mut_src, mut_code = src, (code + 1) % A.CODES
        candidates = torch.arange(case.E)
    quiet = g.name.startswith("random")
    p = _quiet_edge(case, candidates, _scores(case, mut_src, mut_code), quiet=quiet)
    src2, code2 = src.clone(), code.clone()
    src2[p], code2[p] = mut_src[p], mut_code[p]
    ev = evaluate(case, True, edges=(src2, dst, code2))
    out = _outside(compare(case, ev, strict=False))
    assert "alpha" in out and "dscore" in out, out
    if quiet:
        _passes_normwise(case, ev)


@pytest.mark.parametrize("layout", [(8, 2), (320, 5), (1024, 256)], ids=["8x2", "320x5", "1024x256"])
def test_mutation_head_reads_the_next_heads_alpha(layout):
    case = Case(R.hub(400, 300), layout, "normal")
    p = int((case.edges[1] == 0).nonzero()[7])  # one edge of the hub
    out = _outside(compare(case, evaluate(case, True, shift_head_at=p), strict=False))
    assert "dscore" in out, out
    out = _outside(compare(case, evaluate(case, True, reverse=True, shift_head_at=p), strict=False))
    assert "dscore" in out, out


@pytest.mark.parametrize("layout", [(4, 1), (24, 3), (768, 1)], ids=["4x1", "24x3", "768x1"])
def test_mutation_c_for_sqrt_c(layout):
    C = layout[0] // layout[1]
    for kind in ("normal", "sharp"):
        case = Case(R.random(300, 1000), layout, kind)
        out = _outside(compare(case, evaluate(case, True, sqrt_c=float(C)), strict=False))
        assert "alpha" in out and "out" in out and "dscore" in out, (kind, out)


@pytest.mark.parametrize("layout", [(8, 2), (260, 65), (1024, 1)], ids=["8x2", "260x65", "1024x1"])
def test_mutation_no_maximum_subtraction_on_offset_inputs(layout):
    case = Case(R.random(300, 1000), layout, "offset")
    compare(case, evaluate(case, False), strict=True)
    for online in (False, True):
        ev = evaluate(case, online, no_max=True)
        assert not bool(torch.isfinite(ev.out).all())  # expf overflowed
        out = _outside(compare(case, ev, strict=False))
        assert "alpha" in out and "out" in out, out


@pytest.mark.parametrize("p", A.DROPOUT_P)
def test_mutation_row_sum_without_the_dropout_factor(p):
    case = Case(R.hub(400, 300), (8, 2), "normal", p)
    compare(case, evaluate(case, True), strict=True)
    out = _outside(compare(case, evaluate(case, True, s_without_dropout=True), strict=False))
    assert "dscore" in out, out


@pytest.mark.parametrize("flip_to", [0, 1])
def test_mutation_one_keep_mask_entry_flipped(flip_to):
    case = Case(R.random(300, 1000), (256, 64), "normal", 0.25)
    e, h = (case.keep != flip_to).nonzero()[500].tolist()
    keep = case.keep.clone()
    keep[e, h] = flip_to
    out = _outside(compare(case, evaluate(case, True, keep=keep), strict=False))
    assert "out" in out and "alphad" in out, out
