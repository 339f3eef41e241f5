"""fp64 references, seeded inputs and entry-wise error bounds for the attention kernels of csrc/gnx_attn.hip
(k_attn_fwd, k_attn_bwd_dst, k_attn_bwd_src, k_attn_dle), at op level: q|k|v|skip, the bond table Le, the upstream
gradient and (backward) alpha are the inputs, taken as exact fp32 numbers.

No GPU and no package import: ``tests/test_attn_ref_cpu.py`` pins these references against the fp64 autograd of
``tests/transformer_ref.TransformerConv``, shows that plain fp32 evaluations stay inside every bound and that eight
mutations do not; ``tests/test_attn_ops_gpu.py`` holds the kernels to them.

Everything is in the CSR order of ``graph_sum_ref.Graph.csr()`` (edges stably sorted by destination), the order of the
kernels' per-edge arrays.  Notation: u = 2^-24, D the in-degree of row i, C = H / heads, k' = k_j + Le_c,
v' = v_j + Le_c, d_p the dropout factor of position p (0 or 1 / (1 - p); 1 without dropout).

Bounds, from the kernels' roundings (the library is built with -ffp-contract=off; expf within 1 ulp = 2u):

scores    s_p = <q_i, k'_p>_h / sqrt(C),  T_p = sum |q| |k'| / sqrt(C).
          delta_p = 1.01 u ((C + 1) T_p + 2 |s_p|): the add of k', the product and C - 1 additions on every term; the
          rounded sqrtf(C) and the division on the quotient.  Where the dot products are exact in fp32 in any order (the
          "sharp" and "offset" inputs; the CPU file proves it) only 1.01 u 2 |s_p| remains.
          delta_i = max_p delta_p,  spread_i = max_p s_p - min_p s_p  (per row and head).
alpha     alpha_p = exp(s_p - m) / (sum + 1e-16).
          rho_p = expm1(2 delta_i) + 1.01 u (4 D + 3 spread_i + 4), relative, plus 2^-125 absolute (a flushed or
          denormal result is not a failure).  Own count along the longest path of one term of the online sum l: per
          later edge the rescale r = expf(m - m') (2u), l r (u) and + w (u), i.e. 4 per edge; the arguments of those
          expf are rounded differences whose errors add up to u (m_final - s_p) <= u spread; the final expf(s_p - m)
          has u spread on its argument and 2u of its own, l + 1e-16 and the division one each: 4 D + 2 spread + 4 in
          all.  That is below 4 D + 3 spread + 4 in the spread term only, so that constant is kept, not raised.
out       out = sum alpha_p d_p v'_p + skip;
          |err| <= sum alpha_p d_p |v'_p| (max_p rho_p + 1.01 u (2 D + 8)) + u |out|.  acc and l are rescaled by the
          same computed r, so the error of r enters acc / l once (it is in rho); acc adds its own product and addition
          per edge (2 D), w d, v', (w d) v', 1 / x, acc inv and the spare (8), the skip addition u |out|.
          (+ 2^-125 sum d_p |v'_p|: where dropout removes the row's large alpha, only denormal terms remain.)
scratch   (alpha is an fp32 input here)  da_p = d_p <dout_i, v'_p>_h, A_p = d_p sum |dout| |v'|,
          eps_p = 1.01 (C + 3) u A_p;  S = sum alpha_r da_r,
          eps_S = sum alpha_r eps_r + 1.01 (D + 1) u sum alpha_r |da_r|;  dscore_p = alpha_p (da_p - S) / sqrt(C)
          within (alpha_p (eps_p + eps_S) + 4 u alpha_p (|da_p| + |S|)) / sqrt(C)
          (+ 2^-125 for a denormal alpha);  alphad_p = alpha_p d_p within 2 u alphad_p (+ 2^-125), and exactly 0 where
          the mask drops the entry: one rounding of 1 / (1 - p) and one of the product, each at most u / (1 + u).
sums      dq_i = sum dscore_p k'_p, dk_j = sum dscore_p q_dst, dv_j = sum alphad_p dout_dst,
          dLe_c = sum (dscore_p q_dst + alphad_p dout_dst), from a GIVEN scratch, as the (value, n, S) triples of
          ``graph_sum_ref`` for ``assert_entrywise``; extra = 3 for dq (k' and the product) and dLe, 2 for dk and dv.
          S carries n 2^-125 on top of sum |term|: the "sharp" inputs give denormal alpha, and a product below 2^-126
          is rounded to a multiple of 2^-149 (absolutely, at most 2^-150 per term), not relatively.  Entries without a
          non-zero term keep S = 0 and must be exactly 0.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from tests import graph_sum_ref as R

U = R.U32
TINY = 2.0 ** -125
CODES = 60  # rows of the bond table: the code space of graph_sum_ref's default bond_dims (5, 6, 2)

# (H, heads) by thread layout NV = ceil(H / 256) in {1, 2, 4}
LAYOUTS: Dict[int, List[Tuple[int, int]]] = {
    1: [(4, 1), (8, 2), (24, 3), (192, 3), (256, 1), (256, 64)],
    2: [(260, 65), (320, 5), (512, 1), (512, 2)],
    4: [(516, 129), (768, 1), (768, 3), (1024, 1), (1024, 2), (1024, 4), (1024, 256)],
}
ALL_LAYOUTS = [hw for nv in (1, 2, 4) for hw in LAYOUTS[nv]]
FULL_GRAPH_LAYOUTS = [(24, 3), (320, 5), (768, 1), (1024, 2)]  # every graph of graph_sum_ref.cases()
DROPOUT_LAYOUTS = [(8, 2), (256, 64), (320, 5), (768, 1), (1024, 256)]
DROPOUT_P = (0.25, 0.5)
KINDS = ("normal", "sharp", "offset")
EXTRA = {"dq": 3, "dk": 2, "dv": 2, "dLe": 3}

_CASES = R.cases()
_MAIN = [g for g in _CASES if g.name in ("random300x1000", "hub400x300", "tail_empty")]
assert len(_MAIN) == 3


def main_graphs() -> List[R.Graph]:
    return list(_MAIN)


def graphs_for(layout: Tuple[int, int]) -> List[R.Graph]:
    return list(_CASES) if tuple(layout) in FULL_GRAPH_LAYOUTS else list(_MAIN)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
class Inputs(NamedTuple):
    qkvs: torch.Tensor   # fp32 [N, 4H] = q | k | v | skip
    Le: torch.Tensor     # fp32 [CODES, H]
    dout: torch.Tensor   # fp32 [N, H]
    exact: bool          # per-head dot products <q, k'> are exact in fp32 in any order


def key_scale(C: int) -> float:
    """Scale of k and Le of the "normal" inputs: score std ~ 1 up to C = 256, smaller above, so that the term
    (C + 1) T_p of delta stays below 1e-3 / 2 (the CPU file asserts the resulting rho <= 1e-3)."""
    return min(0.7, 5000.0 / ((C + 1) * math.sqrt(C)))


def offset_magnitude(C: int) -> float:
    """A = 2^k with A^2 / sqrt(C) >= 128: the common score term of the "offset" inputs is +-A^2 / sqrt(C)."""
    k = 0
    while 4.0 ** k < 128.0 * math.sqrt(C):
        k += 1
    return 2.0 ** k


SHARP_ROW_SCALES = (1.0, 4.0, 16.0, 32.0)  # of q, by row; k and Le have scale 3: score std 4 .. 136 per row


def inputs(g: R.Graph, H: int, heads: int, kind: str) -> Inputs:
    """The seeded inputs of one graph, layout and kind (they depend on the graph through N only).  Shared, not copied:
    leave them unchanged."""
    return _inputs(g.N, H, heads, kind)


@functools.lru_cache(maxsize=6)
def _inputs(N: int, H: int, heads: int, kind: str) -> Inputs:
    C = H // heads
    base = 100 * (1 + KINDS.index(kind))
    q, k, Le = R.values((N, H), base + 1), R.values((N, H), base + 2), R.values((CODES, H), base + 3)
    v, skip, dout = R.values((N, H), base + 4), R.values((N, H), base + 5), R.values((N, H), base + 6)
    if kind == "normal":
        k, Le = k * key_scale(C), Le * key_scale(C)
    elif kind == "sharp":
        scale = torch.tensor(SHARP_ROW_SCALES)[torch.arange(N) % len(SHARP_ROW_SCALES)].view(-1, 1)
        q, k, Le = R.halves(q * scale), R.halves(k * 3.0), R.halves(Le * 3.0)
    elif kind == "offset":
        A = offset_magnitude(C)
        first = torch.arange(heads) * C  # first column of every head carries the common term
        sign = torch.where(torch.arange(N) % 4 == 3, -1.0, 1.0)
        q, k, Le = R.halves(q), R.halves(k * 0.5), R.halves(Le * 0.5)
        q[:, first] = (sign * A).view(-1, 1)
        k[:, first] = A
        Le[:, first] = 0.0
    else:
        raise ValueError(kind)
    return Inputs(torch.cat([q, k, v, skip], 1).contiguous(), Le.contiguous(), dout.contiguous(), kind != "normal")


def keep_mask(E: int, heads: int, p: float, seed: int = 0) -> torch.Tensor:
    """A seeded keep mask uint8 [E, heads] for the CPU file (the GPU file takes the kernel's own)."""
    gen = torch.Generator().manual_seed(7000 + seed)
    return (torch.rand(E, heads, generator=gen) >= p).to(torch.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------
def _split(qkvs: torch.Tensor):
    H = qkvs.size(1) // 4
    q, k, v, s = qkvs.double().split(H, 1)
    return q, k, v, s


def _row_sum(dst: torch.Tensor, N: int, t: torch.Tensor) -> torch.Tensor:
    return torch.zeros((N,) + tuple(t.shape[1:]), dtype=torch.float64).index_add_(0, dst, t)


def _row_max(dst: torch.Tensor, N: int, t: torch.Tensor) -> torch.Tensor:
    """Per row and head maximum of t [E, heads]; 0 on rows without edges."""
    idx = dst.view(-1, 1).expand_as(t)
    return torch.zeros(N, t.size(1), dtype=torch.float64).scatter_reduce(0, idx, t, "amax", include_self=False)


def factors(keep: Optional[torch.Tensor], p: float, E: int, heads: int) -> torch.Tensor:
    """d_p [E, heads] in float64."""
    if keep is None or p == 0.0:
        return torch.ones(E, heads, dtype=torch.float64)
    return keep.double() / (1.0 - p)


def in_degree(dst: torch.Tensor, N: int) -> torch.Tensor:
    return torch.bincount(dst, minlength=N)[:N]


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
class Forward(NamedTuple):
    score: torch.Tensor        # [E, heads]
    alpha: torch.Tensor        # [E, heads]
    out: torch.Tensor          # [N, H]
    rho: torch.Tensor          # [E, heads] relative bound on alpha
    alpha_bound: torch.Tensor  # [E, heads] rho alpha + 2^-125
    out_bound: torch.Tensor    # [N, H]
    out_terms: torch.Tensor    # [N, H] sum alpha d |v'| + |skip|
    spread: torch.Tensor       # [N, heads]
    deg: torch.Tensor          # [N]


def fwd_ref(qkvs, Le, src, dst, code, N: int, heads: int, keep: Optional[torch.Tensor] = None, p: float = 0.0,
            exact: bool = False) -> Forward:
    q, k, v, s = _split(qkvs)
    H = q.size(1)
    C = H // heads
    E = int(src.numel())
    le = Le.double()[code]
    kp, vp = (k[src] + le).view(E, heads, C), (v[src] + le).view(E, heads, C)
    prod = q[dst].view(E, heads, C) * kp
    rc = math.sqrt(C)
    score = prod.sum(-1) / rc
    T = prod.abs().sum(-1) / rc
    delta_p = 1.01 * U * ((0.0 if exact else (C + 1.0)) * T + 2.0 * score.abs())
    m = _row_max(dst, N, score)
    spread = m + _row_max(dst, N, -score)
    delta_i = _row_max(dst, N, delta_p)
    w = torch.exp(score - m[dst])
    l = _row_sum(dst, N, w)
    alpha = w / (l[dst] + 1e-16)
    deg = in_degree(dst, N)
    degf = deg.double().view(-1, 1)
    rho_row = torch.expm1(2.0 * delta_i) + 1.01 * U * (4.0 * degf + 3.0 * spread + 4.0)
    rho = rho_row[dst]
    d = factors(keep, p, E, heads)
    terms = (alpha * d).unsqueeze(-1) * vp
    A = _row_sum(dst, N, terms.abs())
    out = (_row_sum(dst, N, terms) + s.view(N, heads, C))
    out_bound = A * (rho_row + 1.01 * U * (2.0 * degf + 8.0)).unsqueeze(-1) + U * out.abs() \
        + TINY * _row_sum(dst, N, d.unsqueeze(-1) * vp.abs())
    return Forward(score, alpha, out.reshape(N, H), rho, rho * alpha + TINY, out_bound.reshape(N, H),
                   (A + s.view(N, heads, C).abs()).reshape(N, H), spread, deg)


# ----------------------------------------------------------------------------------------------------------------------
# backward scratch
# ----------------------------------------------------------------------------------------------------------------------
class Scratch(NamedTuple):
    dscore: torch.Tensor         # [E, heads]
    alphad: torch.Tensor         # [E, heads]
    dscore_bound: torch.Tensor
    alphad_bound: torch.Tensor
    dscore_terms: torch.Tensor   # alpha_p (A_p + sum alpha_r A_r) / sqrt(C)


def scratch_ref(dout, qkvs, Le, alpha, src, dst, code, N: int, heads: int, keep: Optional[torch.Tensor] = None,
                p: float = 0.0) -> Scratch:
    q, k, v, s = _split(qkvs)
    H = q.size(1)
    C = H // heads
    E = int(src.numel())
    a = alpha.double()
    vp = (v[src] + Le.double()[code]).view(E, heads, C)
    prod = dout.double()[dst].view(E, heads, C) * vp
    d = factors(keep, p, E, heads)
    da, A = d * prod.sum(-1), d * prod.abs().sum(-1)
    eps = 1.01 * (C + 3.0) * U * A
    S = _row_sum(dst, N, a * da)
    degf = in_degree(dst, N).double().view(-1, 1)
    eps_S = _row_sum(dst, N, a * eps) + 1.01 * (degf + 1.0) * U * _row_sum(dst, N, a * da.abs())
    rc = math.sqrt(C)
    dscore = a * (da - S[dst]) / rc
    bound = (a * (eps + eps_S[dst]) + 4.0 * U * a * (da.abs() + S[dst].abs())) / rc + TINY
    terms = a * (A + _row_sum(dst, N, a * A)[dst]) / rc
    alphad = a * d
    return Scratch(dscore, alphad, bound, torch.where(d == 0, torch.zeros_like(a), 2.0 * U * alphad + TINY), terms)


# ----------------------------------------------------------------------------------------------------------------------
# the four sums, from a given scratch
# ----------------------------------------------------------------------------------------------------------------------
def sums_ref(dout, qkvs, Le, dscore, alphad, src, dst, code, N: int, heads: int) -> Dict[str, R.Ref]:
    q, k, v, s = _split(qkvs)
    H = q.size(1)
    C = H // heads
    ds = dscore.double().repeat_interleave(C, dim=1)
    ad = alphad.double().repeat_interleave(C, dim=1)
    kp = k[src] + Le.double()[code]
    tq, tg = ds * q[dst], ad * dout.double()[dst]

    def gradual(ref: R.Ref) -> R.Ref:  # a product below 2^-126 is rounded to a multiple of 2^-149, not relatively
        return ref[0], ref[1], ref[2] + ref[1] * TINY

    return {"dq": gradual(R.sum_by(dst, N, ds * kp)), "dk": gradual(R.sum_by(src, N, tq)),
            "dv": gradual(R.sum_by(src, N, tg)),
            "dLe": gradual(R.sum_by(torch.cat([code, code]), Le.size(0), torch.cat([tq, tg])))}


# ----------------------------------------------------------------------------------------------------------------------
# checks; both return the worst err / bound ratio
# ----------------------------------------------------------------------------------------------------------------------
def _ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def assert_within(got: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """|got - ref| <= bound in every entry (a NaN in got fails)."""
    got64 = got.detach().cpu().double()
    assert got64.shape == ref64.shape, (what, tuple(got64.shape), tuple(ref64.shape))
    err = (got64 - ref64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        over = torch.where(bad, err - bound, torch.full_like(err, -1.0))
        over = torch.where(torch.isnan(over), torch.full_like(over, float("inf")), over)
        i = int(over.argmax())
        idx = tuple(int(x) for x in np.unravel_index(i, tuple(ref64.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} entries outside the bound; worst at {idx}: "
                             f"got={float(got64.reshape(-1)[i]):.9g} ref={float(ref64.reshape(-1)[i]):.9g} "
                             f"err={float(err.reshape(-1)[i]):.3g} bound={float(bound.reshape(-1)[i]):.3g}")
    return _ratio(err, bound)


def assert_sum(got: torch.Tensor, ref: R.Ref, name: str, what: str = "") -> float:
    """``graph_sum_ref.assert_entrywise`` with the extra of ``name``."""
    value, n, S = ref
    R.assert_entrywise(got, value, n, S, extra=EXTRA[name], what=f"{what} {name}")
    err = (got.detach().cpu().double() - value).abs()
    return _ratio(err, 1.01 * (n + EXTRA[name]) * U * S)
