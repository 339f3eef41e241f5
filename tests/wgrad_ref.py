"""Inputs, exact references, a CPU emulation of the split-operand arithmetic and mirrors of the host dispatch for the
weight-gradient kernels of gnx_wgrad.hip (dW[n,k] += sum_m dC[m,n] rs[m] A[m,k], dbias[n] += sum_m dC[m,n]).

No GPU and no package import: ``tests/test_wgrad_ref_cpu.py`` shows that these inputs tell a faithful kernel from a
damaged one, ``tests/test_wgrad_gpu.py`` holds the kernels to them.

Three kinds of input, each with a criterion that does not depend on the order of the fp32 atomics or on the CU count:

* ``int_case``: small integers.  fp32 MFMA, the six-term bf16 product (an integer |x| <= 8 is its own first bf16 piece)
  and fp32 atomics are all exact while every partial sum stays below 2^24, so the result must EQUAL the int64
  reference: any dropped, doubled or misplaced row, column, chunk or class shows as an integer difference.
* ``hot_rows_exact``: every dW entry has at most one non-zero term, a full-mantissa fp32 value times a power of two.
  The three bf16 pieces of the first times the single piece of the second add up to that product exactly (the partial
  sums a2 b, (a2 + a1) b, (a2 + a1 + a0) b are all fp32 numbers), so the result must EQUAL the fp32 product -- unless a
  piece is mis-staged or one of the terms a2 b0, a1 b0 (dC full) / a0 b1, a0 b2 (A full) is missing.
* ``hot_rows_dense``: four rows, both operands full-mantissa: entry-wise error against fp64 in units of
  u = 2^-24 of |dC|^T |A|, bounded by ``DENSE_BOUND_U`` (derivation at the constant).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

U32 = 2.0 ** -24

# the order in which mfma_3x3 (gnx_split.hpp) feeds the products (piece of dC, piece of A) to one accumulator
MFMA_3X3_TERMS: Tuple[Tuple[int, int], ...] = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))

# Entry-wise bound of the dense hot-row case, in units of u |dC|^T |A|:
#   * the three dropped cross terms a1 b2, a2 b1, a2 b2: <= (2^-9 2^-17 + 2^-17 2^-9 + 2^-17 2^-17) / 2^-24 < 2.1 u
#     (piece p of a value x is below 2^(-8p - 1) |x| ... 2^-9, 2^-17 for p = 1, 2);
#   * one rounding (<= 1 u of the running sum) per accumulator update of a slab that holds a hot row: six per slab;
#   * one rounding per atomic flush that adds a non-zero partial sum.
# Four rows in one slab: 2.1 + 6 + 1 = 9.1 u.  Four rows in four slabs of four chunks: 2.1 + 24 + 4 = 30.1 u.
DENSE_BOUND_U = 32.0


class IntCase(NamedTuple):
    dC: torch.Tensor            # fp32 [M, N], integers in [-8, 8]
    A: torch.Tensor             # fp32 [M, K], integers in [-8, 8]
    rowscale: Optional[torch.Tensor]  # fp32 [M] from {1, 2, 4} | None
    dW0: torch.Tensor           # fp32 [N, K], integer initial contents of dW
    db0: torch.Tensor           # fp32 [N], integer initial contents of dbias
    dW: torch.Tensor            # fp32 [N, K] = dW0 + dC^T (rs A), computed in int64
    db: torch.Tensor            # fp32 [N] = db0 + column sums of dC, computed in int64


INT_INIT_MAX = 100


def int_case(M: int, N: int, K: int, seed: int, rowscale: bool = False) -> IntCase:
    # |dC| |rs| |A| <= 8 * 4 * 8 = 64 * 4 per row: every partial sum of any subset of the terms, in any order, on top of
    # the initial value, is an integer below 2^24 and therefore an exact fp32 number
    assert 64 * 4 * M + INT_INIT_MAX < 2 ** 24, M
    g = torch.Generator().manual_seed(seed)
    dC = torch.randint(-8, 9, (M, N), generator=g)
    A = torch.randint(-8, 9, (M, K), generator=g)
    rs = torch.tensor([1, 2, 4])[torch.randint(0, 3, (M,), generator=g)] if rowscale else None
    dW0 = torch.randint(-INT_INIT_MAX, INT_INIT_MAX + 1, (N, K), generator=g)
    dW0[dW0 == 0] = 7  # non-zero everywhere: an entry the kernel overwrote instead of adding to would show
    db0 = torch.randint(1, INT_INIT_MAX + 1, (N,), generator=g)
    As = A if rs is None else A * rs[:, None]
    dW = dW0 + dC.T @ As
    db = db0 + dC.sum(0)
    assert int(dW.abs().max()) < 2 ** 24 and int(db.abs().max()) < 2 ** 24
    return IntCase(dC.float(), A.float(), None if rs is None else rs.float(), dW0.float(), db0.float(), dW.float(),
                   db.float())


def _full_mantissa(g: torch.Generator, *shape: int) -> torch.Tensor:
    """fp32 values with all 24 significand bits in use, spread over ~14 orders of magnitude."""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) *
            torch.exp(4 * torch.randn(*shape, generator=g, dtype=torch.float64))).float()


class HotRows(NamedTuple):
    dC: torch.Tensor    # fp32 [M, N], zero outside ``rows``
    A: torch.Tensor     # fp32 [M, K], zero outside ``rows``
    rows: Tuple[int, ...]
    ref: torch.Tensor   # exact: fp32 [N, K];  dense: fp64 [N, K]
    norm: Optional[torch.Tensor]  # dense only: |dC|^T |A| in fp64


def hot_rows_exact(M: int, N: int, K: int, rows: Sequence[int], role: str, seed: int = 0) -> HotRows:
    """``role`` = "dC" or "A": the operand that holds the full-mantissa values (hot row i only in the columns with
    col % len(rows) == i); the other one holds +-2^k, k in [-20, 20], in every column of the hot rows."""
    assert role in ("dC", "A") and len(set(rows)) == len(rows) and all(0 <= r < M for r in rows)
    g = torch.Generator().manual_seed(seed)
    L = len(rows)
    nf, np2 = (N, K) if role == "dC" else (K, N)
    full = torch.zeros(M, nf)
    pow2 = torch.zeros(M, np2)
    cols = torch.arange(nf)
    for i, r in enumerate(rows):
        v = _full_mantissa(g, nf)
        full[r] = torch.where(cols % L == i, v, torch.zeros(()))
        k = torch.randint(-20, 21, (np2,), generator=g)
        sign = torch.randint(0, 2, (np2,), generator=g) * 2 - 1
        pow2[r] = (sign * torch.exp2(k.double())).float()
    dC, A = (full, pow2) if role == "dC" else (pow2, full)
    idx = torch.tensor(list(rows))
    ref64 = dC[idx].double().T @ A[idx].double()   # at most one non-zero term per entry: exact in fp64
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), "the one-term products must be fp32 numbers"
    return HotRows(dC, A, tuple(rows), ref, None)


def hot_rows_dense(M: int, N: int, K: int, rows: Sequence[int], seed: int = 0) -> HotRows:
    assert len(rows) == 4 and len(set(rows)) == 4 and all(0 <= r < M for r in rows)
    g = torch.Generator().manual_seed(seed)
    dC, A = torch.zeros(M, N), torch.zeros(M, K)
    for r in rows:
        dC[r] = _full_mantissa(g, N)
        A[r] = _full_mantissa(g, K)
    idx = torch.tensor(list(rows))
    ref = dC[idx].double().T @ A[idx].double()
    norm = dC[idx].double().abs().T @ A[idx].double().abs()
    return HotRows(dC, A, tuple(rows), ref, norm)


def dense_error_u(dW: torch.Tensor, case: HotRows) -> float:
    """max |dW - ref64| / (|dC|^T |A|) in units of u = 2^-24."""
    return float(((dW.detach().double().cpu() - case.ref).abs() / case.norm).max()) / U32


def split_pieces(x: torch.Tensor, pieces: int = 3) -> List[torch.Tensor]:
    """split3 (gnx_split.hpp): round-to-nearest-even bf16 pieces of an fp32 tensor with exact fp32 remainders, as fp32
    tensors; pieces beyond ``pieces`` are zero (a damaged split)."""
    assert x.dtype is torch.float32
    p0 = x.bfloat16().float()
    r1 = x - p0
    p1 = r1.bfloat16().float()
    r2 = r1 - p1
    p2 = r2.bfloat16().float()
    assert torch.equal((p0.double() + p1.double() + p2.double()).float(), x)
    out = [p0, p1, p2]
    for p in range(pieces, 3):
        out[p] = torch.zeros_like(x)
    return out


def split_emulation(dC: torch.Tensor, A: torch.Tensor, terms: Sequence[Tuple[int, int]] = MFMA_3X3_TERMS,
                    pieces: int = 3, chunk_rows: Optional[int] = None) -> torch.Tensor:
    """dC^T A (fp32 [N, K]) the way wgrad3_body / wgrad3p_body compute it: both operands split into bf16 pieces; per
    16-row slab and per term of ``terms`` (in that order) one accumulator update acc = fl32(acc + sum of the slab's 16
    products), the 16 products of bf16 pieces summed without rounding (fp64 here: each has 16 significand bits); one
    accumulator per ``chunk_rows`` rows (None: one for all), the chunks' partial sums added to dW = 0 in fp32 one after
    the other.  Slabs whose operands are all zero are skipped, and so are all-zero chunks (adding an exact zero rounds
    nothing), which keeps the emulation cheap on the hot-row inputs."""
    M, N = dC.shape
    K = A.size(1)
    a, b = split_pieces(dC, pieces), split_pieces(A, pieces)
    chunk_rows = M if chunk_rows is None else chunk_rows
    assert chunk_rows % 16 == 0 or chunk_rows == M
    live = ((dC != 0).any(1) | (A != 0).any(1)).numpy()
    dW = torch.zeros(N, K)
    for c0 in range(0, M, chunk_rows):
        c1 = min(c0 + chunk_rows, M)
        acc, touched = torch.zeros(N, K), False
        for s0 in range(c0, c1, 16):
            s1 = min(s0 + 16, c1)
            if not live[s0:s1].any():
                continue
            touched = True
            for p, q in terms:
                acc = (acc.double() + a[p][s0:s1].double().T @ b[q][s0:s1].double()).float()
        if touched:
            dW = (dW.double() + acc.double()).float()
    return dW


# ---------------------------------------------------------------------------------------------------------------------
# mirrors of the host dispatch (gnx_wgrad.hip), so that a GPU test can assert that its shape reaches the kernel it
# claims to test.  ``wgs`` is the pinned GNX_OPT_WGRAD_WGS (> 0), which takes the CU count out of the arithmetic.
# ---------------------------------------------------------------------------------------------------------------------
BN, BK = 128, 32


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def wgrad_rows_per_block(M: int, N: int, K: int, wgs: int) -> int:
    # mirrors wgrad_launch: tiles, chunks, rows, the floor of 128 rows
    tiles = _cdiv(N, BN) * _cdiv(K, BN)
    target_wgs = wgs
    chunks = _cdiv(target_wgs, tiles)
    rows = _cdiv(_cdiv(M, chunks), BK) * BK
    if rows < 128:
        rows = 128
    return rows


def wgrad_kernel_name(M: int, N: int, K: int, wgs: int, *, vec: bool = True, rowscale: bool = False, split: bool = True,
                      pipe: bool = True, grouped: bool = False) -> str:
    # mirrors wgrad_split_enabled and the launch ladder at the end of wgrad_launch.  ``vec``: both operand views are
    # 16-byte aligned with leading dimensions that are multiples of 4 (vec_x && vec_y of wgrad_args_of); the shape
    # condition N % 4 == 0 && K % 4 == 0 is added here as there.  (Grouped calls also need M * ld < 2^32: always true
    # at test sizes.)
    rows = wgrad_rows_per_block(M, N, K, wgs)
    vec = vec and N % 4 == 0 and K % 4 == 0
    wsplit = (not rowscale) and M >= 4096 and split
    if wsplit and vec and not grouped and rows >= 512 and pipe:
        return "k_gemm_wgrad3p"
    if wsplit:
        return "k_gemm_wgrad3<true>" if grouped else "k_gemm_wgrad3<false>"
    return "k_gemm_wgrad<%s,%s>" % ("true" if vec else "false", "true" if grouped else "false")


def takes_wave_specialised(M: int, N: int, K: int, wgs: int, **kw) -> bool:
    return wgrad_kernel_name(M, N, K, wgs, **kw) == "k_gemm_wgrad3p"


def wgrad_chunks(M: int, rows: int) -> List[Tuple[int, int]]:
    """[begin, end) of the row chunks of an ungrouped launch with ``rows`` rows per workgroup."""
    return [(b, min(b + rows, M)) for b in range(0, M, rows)]


def wgrad_batched_plan(shapes: Sequence[Tuple[int, int, int]], wgs: int, *, any_rowscale: bool = False,
                       split: bool = True, pipe: bool = True) -> Tuple[str, List[int]]:
    """(kernel, rows per workgroup of every problem) of one gnx_gemm_wgrad_batched launch over ``shapes`` = (M, N, K)."""
    # mirrors gnx_gemm_wgrad_batched: total_cost, the per-problem chunk count from the pinned budget, the cap of one
    # chunk per 128 rows, rows rounded up to 32; the kernel follows wgrad_split_enabled(maxM, any_rowscale)
    total_cost = 0.0
    for M, N, K in shapes:
        total_cost += float(M) * float(_cdiv(N, BN) * _cdiv(K, BN))
    rows_out = []
    for M, N, K in shapes:
        tn, tk = _cdiv(N, BN), _cdiv(K, BN)
        M = M if M > 0 else 1
        budget = float(wgs)
        chunks = int(budget * (float(M) * tn * tk / total_cost) / (tn * tk) + 0.5)
        max_chunks = _cdiv(M, 128)
        if chunks > max_chunks:
            chunks = max_chunks
        if chunks < 1:
            chunks = 1
        rows_out.append(_cdiv(_cdiv(M, chunks), BK) * BK)
    wsplit = (not any_rowscale) and max(s[0] for s in shapes) >= 4096 and split
    name = "k_gemm_wgrad3p_batched" if wsplit and pipe else ("k_gemm_wgrad3_batched" if wsplit else
                                                             "k_gemm_wgrad_batched")
    return name, rows_out


# ---------------------------------------------------------------------------------------------------------------------
# graphs with prescribed in-degree classes (the grouped weight gradient sums the rows of each in-degree class)
# ---------------------------------------------------------------------------------------------------------------------
CLASS_CHUNK_ROWS = 1024  # ops.DegreeClasses.WGRAD_ROWS


class ClassGraph(NamedTuple):
    N: int
    D: int                     # number of classes = largest in-degree + 1
    edge_index: torch.Tensor   # int64 [2, E]
    degree: torch.Tensor       # int64 [N] in-degree of every node
    dperm: torch.Tensor        # int64 [N] nodes stably sorted by in-degree (what gnx_degree_classes builds)
    cls_ptr: torch.Tensor      # int64 [D + 1]

    def chunks(self) -> List[Tuple[int, int, int]]:
        """(first position in dperm, rows, class) of every chunk, as gnx_class_tiles lists them."""
        out = []
        for c in range(self.D):
            lo, hi = int(self.cls_ptr[c]), int(self.cls_ptr[c + 1])
            out += [(r, min(CLASS_CHUNK_ROWS, hi - r), c) for r in range(lo, hi, CLASS_CHUNK_ROWS)]
        return out


def graph_with_class_sizes(sizes: Sequence[int], seed: int) -> ClassGraph:
    """A graph in which exactly ``sizes[d]`` nodes have in-degree d (the last entry must be non-zero); which nodes is a
    seeded permutation, so the per-class row gather is not the identity; sources are random."""
    assert sizes[-1] > 0 and all(s >= 0 for s in sizes)
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    degree = np.repeat(np.arange(len(sizes)), sizes)[rng.permutation(N)]
    dst = np.repeat(np.arange(N), degree)
    dst = dst[rng.permutation(dst.size)]
    src = rng.integers(0, N, size=dst.size)
    cls_ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(np.asarray(sizes), out=cls_ptr[1:])
    return ClassGraph(N, len(sizes), torch.from_numpy(np.stack([src, dst])).long(), torch.from_numpy(degree).long(),
                      torch.from_numpy(np.argsort(degree, kind="stable")).long(), torch.from_numpy(cls_ptr))


def class_sums_int(dC: torch.Tensor, A: torch.Tensor, g: ClassGraph) -> torch.Tensor:
    """dW_cls[c] = sum over the nodes of in-degree c of dC[node]^T A[node], in int64, as fp32 [D, N, K]."""
    out = torch.zeros(g.D, dC.size(1), A.size(1), dtype=torch.int64)
    for c in range(g.D):
        sel = g.degree == c
        out[c] = dC[sel].long().T @ A[sel].long()
    assert int(out.abs().max()) < 2 ** 24
    return out.float()


# ---------------------------------------------------------------------------------------------------------------------
# PNA post-layer-0 effective weights (k_pna_weff_batched / k_pna_weff_bwd_batched, gnx_pack.hip)
# ---------------------------------------------------------------------------------------------------------------------
def degree_factors(D: int, avg_log: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """amp(d) = log(d + 1) / avg, att(d) = avg / log(max(d, 1) + 1) for d < D in fp64, avg rounded to fp32 as the
    kernels receive it."""
    avg = float(np.float32(avg_log))
    d = torch.arange(D, dtype=torch.float64)
    return torch.log(d + 1) / avg, avg / torch.log(d.clamp_min(1) + 1)


def weff_ref(W: torch.Tensor, F: int, D: int, avg_log: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Weff fp64 [D, F, 4F], S = |W1| + amp |W2| + att |W3|) from W [F, 13F]."""
    amp, att = degree_factors(D, avg_log)
    W = W.double()
    W1, W2, W3 = W[:, F:5 * F], W[:, 5 * F:9 * F], W[:, 9 * F:13 * F]
    ref = W1[None] + amp[:, None, None] * W2[None] + att[:, None, None] * W3[None]
    S = W1.abs()[None] + amp[:, None, None] * W2.abs()[None] + att[:, None, None] * W3.abs()[None]
    return ref, S


def weff_bwd_ref(dWeff: torch.Tensor, dW0: torch.Tensor, F: int, D: int, avg_log: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dW fp64 [F, 13F], S = |dW0| + sum_d |term|) after dW[:, F:5F] += sum_d dWeff[d], [:, 5F:9F] += sum_d amp(d)
    dWeff[d], [:, 9F:13F] += sum_d att(d) dWeff[d]; columns [0, F) are left alone."""
    amp, att = degree_factors(D, avg_log)
    v = dWeff.double()
    ref, S = dW0.double().clone(), dW0.double().abs()
    for blk, f in enumerate((torch.ones(D, dtype=torch.float64), amp, att)):
        sl = slice(F + 4 * F * blk, F + 4 * F * (blk + 1))
        ref[:, sl] += (f[:, None, None] * v).sum(0)
        S[:, sl] += (f[:, None, None] * v.abs()).sum(0)
    return ref, S
