"""The fp64 references and the entry-wise bound of tests/graph_sum_ref.py, checked without a GPU:

* the references agree with the oracle (``oracle.pyg_restatement`` scatter / MaxAggregation and autograd of the fp64
  formulas) to 1e-12;
* plain fp32 evaluations of the same sums on the CPU -- in forward, reversed and shuffled edge order -- stay inside
  ``assert_entrywise`` on every graph the GPU file uses, so the bound does not reject a correct kernel;
* four one-edge mutations fail ``assert_entrywise`` while passing the norm-wise 1e-5 metric of tests/test_ops_gpu.py.
"""
import numpy as np
import pytest
import torch

from oracle import pyg_restatement as O
from tests import graph_sum_ref as R
from tests.parity_util import rel_err

PIN = [R.random(300, 1000), R.hub(), R.loops_dups()]
PIN_IDS = [g.name for g in PIN]
ALL = R.cases() + R.fallback_cases() + [R.hub(bond_dims=R.BOND_DIMS[r]) for r in (65, 300, 600)]
ALL_IDS = [f"{g.name}-R{g.R}" for g in ALL]
H = 5


def _close(a, b):
    assert a.shape == b.shape
    if a.numel():
        assert float((a.double() - b.double()).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# references against the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", PIN, ids=PIN_IDS)
@pytest.mark.parametrize("half", [False, True])
def test_edge_combine_ref_matches_oracle(g, half):
    src, dst, code = g.src, g.dst, g.code
    P, Q, Te = (R.values(s, 10 + i, half).double().requires_grad_(True) for i, s in enumerate([(g.N, H), (g.N, H), (g.R, H)]))
    gr = R.values((g.E, H), 13).double()
    for relu in (False, True):
        h = P[dst] + Q[src] + Te[code]
        h = h.relu() if relu else h
        _close(R.edge_combine_fwd_ref(P.detach().float(), Q.detach().float(), Te.detach().float(), src, dst, code,
                                      relu)[0], h.detach())
    h = P[dst] + Q[src] + Te[code]
    h.backward(gr)
    (dP, nP, _), (dQ, nQ, _), (dT, nT, _) = R.edge_combine_bwd_ref(gr.float(), src, dst, code, g.N, g.R)
    _close(dP, P.grad)
    _close(dQ, Q.grad)
    _close(dT, Te.grad)
    _close(dP, O.scatter(gr, dst, 0, g.N, "sum"))
    # the counts are the degrees (randn gradients have no zero entries)
    assert torch.equal(nP[:, 0], O.degree(dst, g.N, torch.float64)) and torch.equal(nQ[:, 0], O.degree(src, g.N, torch.float64))
    assert torch.equal(nT[:, 0], O.degree(code, g.R, torch.float64))


@pytest.mark.parametrize("g", PIN, ids=PIN_IDS)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.25, -1.0])
def test_gine_ref_matches_oracle(g, half, eps):
    src, dst, code = g.src, g.dst, g.code
    x = R.values((g.N, H), 20, half).double().requires_grad_(True)
    Le = R.values((g.R, H), 21, half).double().requires_grad_(True)
    dout = R.values((g.N, H), 22).double()
    out = O.scatter((x[src] + Le[code]).relu(), dst, 0, g.N, "sum") + (1 + eps) * x
    out.backward(dout)
    xf, Lf = x.detach().float(), Le.detach().float()
    _close(R.gine_fwd_ref(xf, Lf, src, dst, code, eps, g.N)[0], out.detach())
    (dx, _, _), (dLe, _, _) = R.gine_bwd_ref(dout.float(), xf, Lf, src, dst, code, eps, g.N)
    _close(dx, x.grad)
    _close(dLe, Le.grad)
    if half:  # exact zeros of x + Le occur, and autograd's relu gradient is 0 there: the strict mask
        assert int(((xf.double()[src] + Lf.double()[code]) == 0).sum()) > 0


def pool_sizes(name):
    return R.POOL_SIZES[name]


@pytest.mark.parametrize("sizes", ["edges", "many"])
@pytest.mark.parametrize("mode", ["add", "mean", "max"])
@pytest.mark.parametrize("kind", ["randn", "halves", "negative"])
def test_pool_ref_matches_oracle(sizes, mode, kind):
    sz = pool_sizes(sizes)
    N, B = sum(sz), len(sz)
    x = R.values((N, H), 30, kind == "halves")
    if kind == "negative":
        x = -x.abs() - 0.5
    x64 = x.double().requires_grad_(True)
    idx = R.segment_index(sz)
    agg = {"add": O.SumAggregation, "mean": O.MeanAggregation, "max": O.MaxAggregation}[mode]()
    out = agg(x64, idx, dim_size=B)
    _close(R.pool_fwd_ref(x, sz, mode)[0], out.detach())
    dout = R.values((B, H), 32)
    out.backward(dout.double())
    _close(R.pool_bwd_ref(dout, x, sz, mode)[0], x64.grad)
    if kind == "negative" and mode == "max":
        assert bool((out.detach()[torch.tensor(sz) > 0] < 0).all())  # never the zero fill


def test_embed_bwd_ref_matches_autograd():
    offsets = [0, 100, 250, 300]
    rng = np.random.default_rng(40)
    idx = torch.from_numpy(np.stack([rng.integers(0, offsets[k + 1] - offsets[k], 500) for k in range(3)], 1)).long()
    table = R.values((300, H), 41).double().requires_grad_(True)
    dout = R.values((500, H), 42)
    out = sum(table[idx[:, k] + offsets[k]] for k in range(3))
    out.backward(dout.double())
    _close(R.embed_bwd_ref(idx, offsets, dout)[0], table.grad)
    init = R.values((300, H), 43)
    _close(R.embed_bwd_ref(idx, offsets, dout, init)[0], table.grad + init.double())


# ----------------------------------------------------------------------------------------------------------------------
# fp32 on the CPU in three orders stays inside the bound, on every graph of the GPU file
# ----------------------------------------------------------------------------------------------------------------------
def _orders(E):
    fwd = torch.arange(E)
    return [fwd, fwd.flip(0), torch.from_numpy(np.random.default_rng(E).permutation(E))]


def _sum32(index, rows, terms, order):
    out = torch.zeros(rows, terms.size(1), dtype=torch.float32)
    index = index.tolist()
    for i in order.tolist():  # one fp32 addition per term, in exactly this order
        out[index[i]] += terms[i]
    return out


@pytest.mark.parametrize("g", ALL, ids=ALL_IDS)
@pytest.mark.parametrize("half", [False, True])
def test_fp32_in_any_order_is_inside_the_bound(g, half):
    src, dst, code = g.src, g.dst, g.code
    P, Q, Te = R.values((g.N, H), 50, half), R.values((g.N, H), 51, half), R.values((g.R, H), 52, half)
    gr = R.values((g.E, H), 53)
    for relu in (False, True):
        h32 = (P[dst] + Q[src]) + Te[code]
        ref, n, S = R.edge_combine_fwd_ref(P, Q, Te, src, dst, code, relu)
        R.assert_entrywise(h32.relu() if relu else h32, ref, n, S, extra=2, what="h1")
    refs = R.edge_combine_bwd_ref(gr, src, dst, code, g.N, g.R)
    eps = 0.25
    msg32 = (P[src] + Te[code]).relu()
    mask = R.gine_mask(P, Te, src, code)
    assert torch.equal(mask, (P[src] + Te[code]) > 0)  # the fp32 mask is the fp64 mask: nothing to exclude
    gm32 = Q[dst] * mask.float()
    fw = R.gine_fwd_ref(P, Te, src, dst, code, eps, g.N)
    bx, bl = R.gine_bwd_ref(Q, P, Te, src, dst, code, eps, g.N)
    k = torch.tensor(1.25, dtype=torch.float32)
    for order in _orders(g.E):
        for (ref, n, S), index, rows in zip(refs, (dst, src, code), (g.N, g.N, g.R)):
            R.assert_entrywise(_sum32(index, rows, gr, order), ref, n, S, what="edge combine bwd")
        R.assert_entrywise(_sum32(dst, g.N, msg32, order) + k * P, *fw, what="gine fwd")
        R.assert_entrywise(k * Q + _sum32(src, g.N, gm32, order), *bx, what="gine dx")
        R.assert_entrywise(_sum32(code, g.R, gm32, order), *bl, what="gine dLe")


@pytest.mark.parametrize("sizes", ["edges", "many"])
@pytest.mark.parametrize("mode", ["add", "mean"])
def test_fp32_pool_in_any_order_is_inside_the_bound(sizes, mode):
    sz = pool_sizes(sizes)
    N, B = sum(sz), len(sz)
    x = R.values((N, H), 60)
    idx = R.segment_index(sz)
    ref = R.pool_fwd_ref(x, sz, mode)
    cnt = torch.tensor(sz, dtype=torch.float32).clamp(min=1).view(-1, 1)
    for order in _orders(N):
        s = _sum32(idx, B, x, order)
        R.assert_entrywise(s / cnt if mode == "mean" else s, *ref, what=mode)
    dout = R.values((B, H), 61)
    g32 = dout[idx] / cnt[idx] if mode == "mean" else dout[idx]
    R.assert_entrywise(g32, *R.pool_bwd_ref(dout, x, sz, mode), what=mode + " bwd")


# ----------------------------------------------------------------------------------------------------------------------
# mutations: a single wrong edge in a small-magnitude row.  The gradient rows of one or two chosen nodes are scaled by
# 1e-6 (activations of very different magnitude in one batch are ordinary); a dropped, doubled or misdirected edge of
# such a node changes its own sums completely and the largest entry of the array by nothing that 1e-5 would see.
# ----------------------------------------------------------------------------------------------------------------------
SMALL = 1e-6


def _fails_entrywise_passes_normwise(mut64, ref, n, S):
    got = mut64.float()  # what a kernel with this bug would return, rounded once
    with pytest.raises(AssertionError, match="outside"):
        R.assert_entrywise(got, ref, n, S)
    assert rel_err(got, ref) <= 1e-5


def _hub_edge(g):
    """An edge into the hub (node 0), and its source."""
    p = int((g.dst == 0).nonzero()[0])
    return p, int(g.src[p])


@pytest.mark.parametrize("mutation", ["drop", "double"])
def test_mutation_one_hub_edge(mutation):
    g = R.hub()
    p, j = _hub_edge(g)
    scale = torch.ones(g.N)
    scale[j] = SMALL
    gr = R.values((g.E, H), 70) * scale[g.src].view(-1, 1)
    _, (dQ, n, S), _ = R.edge_combine_bwd_ref(gr, g.src, g.dst, g.code, g.N, g.R)
    R.assert_entrywise(dQ.float(), dQ, n, S)  # the unmutated sum passes
    edges = torch.arange(g.E)
    edges = edges[edges != p] if mutation == "drop" else torch.cat([edges, torch.tensor([p])])
    _fails_entrywise_passes_normwise(R.sum_by(g.src[edges], g.N, gr[edges])[0], dQ, n, S)


def test_mutation_src_shifted_on_last_edge_of_a_chunk():
    g = R.hub()
    src, dst, code = g.csr()
    pos = np.argsort(code.numpy(), kind="stable")  # the inverted index the by-code kernels walk in chunks of 128
    p = int(pos[127])
    j = int(src[p])
    j2 = (j + 1) % g.N
    scale = torch.ones(g.N)
    scale[j] = scale[j2] = SMALL
    gr = R.values((g.E, H), 71) * scale[src].view(-1, 1)
    _, (dQ, n, S), _ = R.edge_combine_bwd_ref(gr, src, dst, code, g.N, g.R)
    src_mut = src.clone()
    src_mut[p] = j2
    _fails_entrywise_passes_normwise(R.sum_by(src_mut, g.N, gr)[0], dQ, n, S)


def test_mutation_mask_not_strict_on_halves():
    """``>=`` for ``>`` in the ReLU mask.  Only the rows of code 7 can tie (every other row of Le is off the half grid
    by 1/4) and the edges of code 7 end in nodes whose output gradient is small: dLe[7] is the small-magnitude row."""
    g0 = R.hub()
    tied = 7
    small_nodes = torch.arange(g0.N) % 5 == 0
    code = torch.where(small_nodes[g0.dst], torch.full_like(g0.code, tied),
                       torch.where(g0.code == tied, torch.full_like(g0.code, tied + 1), g0.code))
    g = g0._replace(edge_attr=R.attr_of_code(code.numpy(), g0.bond_dims))
    assert torch.equal(g.code, code)
    x, Le = R.values((g.N, H), 72, True), R.values((g.R, H), 73, True) + 0.25
    Le[tied] -= 0.25
    dout = R.values((g.N, H), 74) * torch.where(small_nodes, SMALL, 1.0).view(-1, 1)
    pre = x.double()[g.src] + Le.double()[g.code]
    assert int((pre == 0).sum()) > 0 and bool((~(pre == 0).any(1) | (g.code == tied)).all())
    _, (dLe, n, S) = R.gine_bwd_ref(dout, x, Le, g.src, g.dst, g.code, 0.0, g.N)
    _, (mut, _, _) = R.gine_bwd_ref(dout, x, Le, g.src, g.dst, g.code, 0.0, g.N, strict=False)
    R.assert_entrywise(dLe.float(), dLe, n, S)
    _fails_entrywise_passes_normwise(mut, dLe, n, S)


def test_entrywise_rejects_nan_and_nonzero_where_all_terms_are_zero():
    ref, n, S = torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.float64)
    R.assert_entrywise(torch.tensor([[0.0, -0.0], [0.0, 0.0]]), ref, n, S)
    with pytest.raises(AssertionError, match=r"worst at \(1, 0\)"):
        R.assert_entrywise(torch.tensor([[0.0, 0.0], [1e-30, 0.0]]), ref, n, S)
    with pytest.raises(AssertionError):
        R.assert_entrywise(torch.tensor([[float("nan"), 0.0], [0.0, 0.0]]), ref + 1, n + 1, S + 1)
