"""Seeded graph builders, fp64 references and the entry-wise error bound for the index-sum kernels
(edge combine, GINE aggregate, segment pool, the by-code table sums and the embedding table gradient).

No GPU and no package import: ``tests/test_graph_sum_ref_cpu.py`` pins these references against the oracle and
``tests/test_graph_sums_gpu.py`` holds the kernels to them.

Every reference is written from the formula in the kernel's header comment with ``index_add_`` / ``scatter_reduce`` in
float64 on the CPU and returns, next to the value, the entry-wise count ``n`` of non-zero terms and ``S = sum |term|``.
``assert_entrywise`` then asks, for every entry,

    |got - ref| <= 1.01 (n + extra) 2^-24 S

the bound gamma_n sum|x_i| of an fp32 sum of n terms in ANY order (a summation tree with n leaves has n - 1 roundings
on the longest path, adding an exact zero rounds nothing, 1.01 covers 1 / (1 - n u) up to n = 10^5), so it holds for
sequential loops, register partial sums and atomics alike.  ``extra`` covers the roundings outside the sum (the x + Le
add of a message, (1 + eps) x, the division of a mean).  An entry whose terms are all zero must be exactly zero.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

U32 = 2.0 ** -24


class Graph(NamedTuple):
    name: str
    N: int
    edge_index: torch.Tensor  # int64 [2, E]
    edge_attr: torch.Tensor   # int64 [E, K]
    bond_dims: Tuple[int, ...]

    @property
    def E(self) -> int:
        return int(self.edge_index.size(1))

    @property
    def R(self) -> int:
        return int(np.prod(self.bond_dims))

    @property
    def src(self) -> torch.Tensor:
        return self.edge_index[0]

    @property
    def dst(self) -> torch.Tensor:
        return self.edge_index[1]

    @property
    def code(self) -> torch.Tensor:
        """Mixed-radix bond code of every edge (first feature most significant), int64 [E]."""
        c = torch.zeros(self.E, dtype=torch.int64)
        for k, d in enumerate(self.bond_dims):
            c = c * d + self.edge_attr[:, k]
        return c

    @property
    def perm(self) -> torch.Tensor:
        """Edge ids in CSR order: stably sorted by destination."""
        return torch.from_numpy(np.argsort(self.dst.numpy(), kind="stable"))

    def csr(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(src, dst, code) in CSR order, the order of every per-edge array of the kernels."""
        p = self.perm
        return self.src[p], self.dst[p], self.code[p]


def attr_of_code(code: np.ndarray, bond_dims: Sequence[int]) -> torch.Tensor:
    cols = []
    c = np.asarray(code, dtype=np.int64)
    for d in reversed(bond_dims):
        cols.append(c % d)
        c = c // d
    return torch.from_numpy(np.stack(cols[::-1], 1).reshape(len(code), len(bond_dims))).long()


def _graph(name, N, src, dst, code, bond_dims, rng, shuffle=True) -> Graph:
    src, dst, code = (np.asarray(a, dtype=np.int64) for a in (src, dst, code))
    if shuffle and len(src):
        o = rng.permutation(len(src))
        src, dst, code = src[o], dst[o], code[o]
    ei = torch.from_numpy(np.stack([src, dst]).reshape(2, len(src))).long()
    return Graph(name, int(N), ei, attr_of_code(code, bond_dims), tuple(int(d) for d in bond_dims))


def random(N: int, E: int, bond_dims=(5, 6, 2), seed: int = 0) -> Graph:
    rng = np.random.default_rng([1, N, E, seed])
    R = int(np.prod(bond_dims))
    return _graph(f"random{N}x{E}", N, rng.integers(0, N, E), rng.integers(0, N, E), rng.integers(0, R, E), bond_dims,
                  rng)


def hub(N: int = 400, deg: int = 300, bond_dims=(5, 6, 2), seed: int = 0) -> Graph:
    """Node 0 has in-degree ``deg``, node 1 out-degree ``deg``; nodes 2.. sit on a ring: in- and out-degree 2."""
    assert deg + 2 <= N
    rng = np.random.default_rng([2, N, deg, seed])
    R = int(np.prod(bond_dims))
    others = np.arange(2, deg + 2)
    ring = np.arange(2, N)
    src = np.concatenate([others, np.full(deg, 1), ring])
    dst = np.concatenate([np.zeros(deg, dtype=np.int64), others, np.roll(ring, -1)])
    return _graph(f"hub{N}x{deg}", N, src, dst, rng.integers(0, R, len(src)), bond_dims, rng)


def edgeless(N: int, bond_dims=(5, 6, 2)) -> Graph:
    rng = np.random.default_rng(3)
    return _graph(f"edgeless{N}", N, [], [], [], bond_dims, rng)


def loops_dups(N: int = 60, E: int = 150, bond_dims=(5, 6, 2), seed: int = 0) -> Graph:
    """Random edges and one self-loop on every third node, every edge (code included) present twice."""
    rng = np.random.default_rng([4, N, E, seed])
    R = int(np.prod(bond_dims))
    loops = np.arange(0, N, 3)
    src = np.concatenate([rng.integers(0, N, E), loops])
    dst = np.concatenate([rng.integers(0, N, E), loops])
    code = rng.integers(0, R, len(src))
    return _graph("loops_dups", N, np.tile(src, 2), np.tile(dst, 2), np.tile(code, 2), bond_dims, rng)


def tail_empty(N: int = 100, E: int = 260, bond_dims=(5, 6, 2), seed: int = 0) -> Graph:
    """The last 40 nodes have neither in- nor out-edges; node 0 has no out-edges."""
    rng = np.random.default_rng([5, N, E, seed])
    R = int(np.prod(bond_dims))
    return _graph("tail_empty", N, rng.integers(1, N - 40, E), rng.integers(0, N - 40, E), rng.integers(0, R, E),
                  bond_dims, rng)


def few_per_code(N: int = 50, bond_dims=(5, 6, 2), seed: int = 0) -> Graph:
    """Every one of the R codes is used by 1-3 edges: key runs shorter than the kernels' four items in flight."""
    rng = np.random.default_rng([6, N, seed])
    R = int(np.prod(bond_dims))
    code = np.repeat(np.arange(R), rng.integers(1, 4, R))
    return _graph("few_per_code", N, rng.integers(0, N, len(code)), rng.integers(0, N, len(code)), code, bond_dims, rng)


def one_code(N: int = 70, E: int = 300, bond_dims=(5, 6, 2), seed: int = 0) -> Graph:
    """Every edge has the same (last) code: one key run across all chunks."""
    rng = np.random.default_rng([7, N, E, seed])
    R = int(np.prod(bond_dims))
    return _graph("one_code", N, rng.integers(0, N, E), rng.integers(0, N, E), np.full(E, R - 1), bond_dims, rng)


BOND_DIMS = {1: (1,), 60: (5, 6, 2), 64: (8, 8), 65: (13, 5), 300: (300,), 600: (20, 30)}  # code space R -> bond_dims

# graph sizes of the segment pool: empty first and last segments, the 4-row loop with every remainder, one long segment;
# and 1000 graphs of 1-3 rows (the last thread block partial at every width)
POOL_SIZES = {"edges": [0, 1, 2, 3, 4, 5, 7, 8, 300, 0],
              "many": [int(v) for v in np.random.default_rng(31).integers(1, 4, 1000)]}

CHUNK_EDGES = (1, 3, 4, 5, 127, 128, 129, 257)  # around the 128-entry chunk, the 4 items in flight and one lane's share


def cases(bond_dims=(5, 6, 2)) -> List[Graph]:
    """Every graph of the GPU file for one code space (the CPU file runs the fp32 self-check on the same list)."""
    out = [random(300, 1000, bond_dims), hub(400, 300, bond_dims), edgeless(1, bond_dims), edgeless(50, bond_dims),
           loops_dups(bond_dims=bond_dims), tail_empty(bond_dims=bond_dims), few_per_code(bond_dims=bond_dims),
           one_code(bond_dims=bond_dims)]
    out += [random(40, E, bond_dims)._replace(name=f"chunk{E}") for E in CHUNK_EDGES]
    return out


def fallback_cases() -> List[Graph]:
    """Graphs of the table-scatter fallback (more than 64 codes): one row chunk, and 12 of them."""
    return [random(300, E, BOND_DIMS[R])._replace(name=f"random300x{E}") for R in (65, 300, 600) for E in (200, 3000)]


def halves(t: torch.Tensor) -> torch.Tensor:
    """Round to multiples of 1/2: sums of two such values are exact, so x + Le == 0 and max ties really occur."""
    return (t * 2).round() / 2


def values(shape, seed: int, half: bool = False) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g, dtype=torch.float32)
    return halves(t) if half else t


# ----------------------------------------------------------------------------------------------------------------------
# the bound
# ----------------------------------------------------------------------------------------------------------------------
Ref = Tuple[torch.Tensor, torch.Tensor, torch.Tensor]  # value (float64), n, S -- n and S broadcast against the value


def assert_entrywise(got: torch.Tensor, ref64: torch.Tensor, n, S, extra: int = 4, what: str = "") -> None:
    got64 = got.detach().cpu().double()
    ref64 = ref64.detach().cpu().double()
    assert got64.shape == ref64.shape, (what, tuple(got64.shape), tuple(ref64.shape))
    if ref64.numel() == 0:
        return
    n = torch.as_tensor(n, dtype=torch.float64).expand_as(ref64)
    S = torch.as_tensor(S, dtype=torch.float64).expand_as(ref64)
    err = (got64 - ref64).abs()
    bound = 1.01 * (n + extra) * U32 * S
    bad = ~(err <= bound) | ((S == 0) & (got64 != 0))  # ~(<=): a NaN in got fails
    if bool(bad.any()):
        over = torch.where(bad, err - bound, torch.full_like(err, -1.0))
        over = torch.where(torch.isnan(over), torch.full_like(over, float("inf")), over)
        i = int(over.argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref64.shape)))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} entries outside (n + {extra}) u S; worst at {idx}: "
            f"n={int(n.reshape(-1)[i])} S={float(S.reshape(-1)[i]):.9g} got={float(got64.reshape(-1)[i]):.9g} "
            f"ref={float(ref64.reshape(-1)[i]):.9g} err={float(err.reshape(-1)[i]):.3g} "
            f"bound={float(bound.reshape(-1)[i]):.3g}")


def same_nonfinite(got: torch.Tensor, ref64: torch.Tensor, what: str = "") -> None:
    """The NaN entries and the infinite entries of ``got`` are exactly the reference's."""
    got, ref64 = got.detach().cpu(), ref64.detach().cpu()
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    for name, f in (("NaN", torch.isnan), ("Inf", torch.isinf)):
        a, b = f(got), f(ref64)
        if not torch.equal(a, b):
            lost = (b & ~a).nonzero()[:4].tolist()
            made = (a & ~b).nonzero()[:4].tolist()
            raise AssertionError(f"{what}: {name} entries differ: reference has {int(b.sum())}, got {int(a.sum())}; "
                                 f"lost at {lost}, made up at {made}")


def sum_by(index: torch.Tensor, rows: int, terms: torch.Tensor) -> Ref:
    """out[index[i]] += terms[i] in float64, with the count of non-zero terms and the absolute sum per entry."""
    t = terms.double()
    z = torch.zeros(rows, t.size(1), dtype=torch.float64)
    return (z.clone().index_add_(0, index, t), z.clone().index_add_(0, index, (t != 0).double()),
            z.clone().index_add_(0, index, t.abs()))


# ----------------------------------------------------------------------------------------------------------------------
# PNA message assembly: h1[p] = relu(P[dst[p]] + Q[src[p]] + Te[code[p]]);  dP / dQ / dTe = sums of g by dst / src / code
# ----------------------------------------------------------------------------------------------------------------------
def edge_combine_fwd_ref(P, Q, Te, src, dst, code, relu: bool) -> Ref:
    a, b, e = P.double()[dst], Q.double()[src], Te.double()[code]
    r = a + b + e
    return (torch.relu(r) if relu else r), torch.full((1, 1), 3.0, dtype=torch.float64), a.abs() + b.abs() + e.abs()


def edge_combine_bwd_ref(g, src, dst, code, N: int, R: int) -> Tuple[Ref, Ref, Ref]:
    return sum_by(dst, N, g), sum_by(src, N, g), sum_by(code, R, g)


# ----------------------------------------------------------------------------------------------------------------------
# GINE: out[i] = (1 + eps) x[i] + sum_{p: dst[p] = i} relu(x[src[p]] + Le[code[p]])
# dx[j] = (1 + eps) dout[j] + sum_{p: src[p] = j} dout[dst[p]] [x[j] + Le[code[p]] > 0];  dLe[r] = the same terms by code
# ----------------------------------------------------------------------------------------------------------------------
def _k(eps: float) -> float:
    return float(np.float32(1.0) + np.float32(eps))  # the kernels form 1 + eps in fp32


def gine_mask(x, Le, src, code, strict: bool = True) -> torch.Tensor:
    """The ReLU mask in fp64 on the fp32 inputs.  It is the fp32 kernel's mask exactly: the rounded fp32 sum of two
    fp32 numbers has the sign of the exact sum (rounding is monotone and sums below the normal range are exact)."""
    pre = x.double()[src] + Le.double()[code]
    return (pre > 0) if strict else (pre >= 0)


def gine_fwd_ref(x, Le, src, dst, code, eps: float, N: int) -> Ref:
    msg = torch.relu(x.double()[src] + Le.double()[code])
    ref, n, S = sum_by(dst, N, msg)
    self_term = _k(eps) * x.double()
    return ref + self_term, n + (self_term != 0).double(), S + self_term.abs()


def gine_bwd_ref(dout, x, Le, src, dst, code, eps: float, N: int, strict: bool = True) -> Tuple[Ref, Ref]:
    gm = dout.double()[dst] * gine_mask(x, Le, src, code, strict).double()
    dx, n, S = sum_by(src, N, gm)
    self_term = _k(eps) * dout.double()
    return (dx + self_term, n + (self_term != 0).double(), S + self_term.abs()), sum_by(code, Le.size(0), gm)


# ----------------------------------------------------------------------------------------------------------------------
# contiguous segment pool (graph b = rows ptr[b] .. ptr[b+1]) and its backward
# ----------------------------------------------------------------------------------------------------------------------
def segment_index(sizes: Sequence[int]) -> torch.Tensor:
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(list(sizes), dtype=torch.int64))


def pool_fwd_ref(x, sizes: Sequence[int], mode: str) -> Ref:
    """add / mean: (value, n, S); max: the value is exact (n = 1, S = |value|), 0 for an empty segment."""
    B, idx = len(sizes), segment_index(sizes)
    if mode == "max":
        out = torch.zeros(B, x.size(1), dtype=torch.float64).scatter_reduce_(
            0, idx.view(-1, 1).expand(-1, x.size(1)), x.double(), reduce="amax", include_self=False)
        return out, torch.ones(1, 1, dtype=torch.float64), out.abs()
    ref, n, S = sum_by(idx, B, x)
    if mode == "mean":
        cnt = torch.tensor(list(sizes), dtype=torch.float64).clamp(min=1).view(-1, 1)
        ref, S = ref / cnt, S / cnt
    return ref, n, S


def pool_bwd_ref(dout, x, sizes: Sequence[int], mode: str) -> Ref:
    """add: dout[b]; mean: dout[b] / count; max: dout[b] / #ties on the rows equal to the maximum, where a maximum that
    is exactly 0 counts one more tie (torch's scatter_reduce backward counts the zero-filled output as a tie, also with
    include_self=False; k_pool_bwd documents and reproduces it).  One term per entry.  A NaN in a segment makes its
    maximum NaN and, in autograd, the gradient of every row of that segment and channel NaN."""
    idx = segment_index(sizes)
    g = dout.double()[idx]
    if mode == "mean":
        g = g / torch.tensor(list(sizes), dtype=torch.float64).clamp(min=1)[idx].view(-1, 1)
    elif mode == "max":
        mx = pool_fwd_ref(x, sizes, "max")[0]
        hit = x.double() == mx[idx]
        ties = torch.zeros_like(mx).index_add_(0, idx, hit.double()) + (mx == 0).double()
        g = torch.where(hit, g / ties[idx], torch.zeros_like(g))
        g = torch.where(torch.isnan(mx[idx]), mx[idx], g)  # a NaN maximum ties with nothing: autograd's g / 0 * 0
    return g, torch.ones(1, 1, dtype=torch.float64), g.abs()


# ----------------------------------------------------------------------------------------------------------------------
# embedding table gradient: dtable[offsets[k] + idx[n, k]] += dout[n]  (+ the table's initial content, if any)
# ----------------------------------------------------------------------------------------------------------------------
def embed_bwd_ref(idx, offsets: Sequence[int], dout, init: Optional[torch.Tensor] = None) -> Ref:
    K, R = len(offsets) - 1, int(offsets[-1])
    rows = torch.cat([idx[:, k] + int(offsets[k]) for k in range(K)])
    ref, n, S = sum_by(rows, R, dout.repeat(K, 1))
    if init is not None:
        ref, n, S = ref + init.double(), n + (init != 0).double(), S + init.double().abs()
    return ref, n, S
