// The per-item arithmetic of the PNA scatter-aggregate backward, spelled ONCE: k_pna_agg_bwd_rc (gnx_aggregate.hip) takes
// the four aggregate gradients of its item from dA in memory, k_pna_dA_agg_bwd (gnx_gemm.hip) from the accumulators of
// the dA product it has just computed.  An item is VEC consecutive channels of one destination node.
#pragma once
#include "gnx_common.hpp"

#include <cmath>

template <int VEC>
__device__ __forceinline__ void vload(float (&r)[VEC], const float* p) {
  if constexpr (VEC == 4) {
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    r[0] = v.x;
    r[1] = v.y;
    r[2] = v.z;
    r[3] = v.w;
  } else {
    r[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void vstore(float* p, const float (&r)[VEC]) {
  if constexpr (VEC == 4) {
    f32x4 v = {r[0], r[1], r[2], r[3]};
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    p[0] = r[0];
  }
}

// clamp / mask constants of [3P] StdAggregation: var.clamp(min=1e-5).sqrt(), masked to 0 where <= sqrt(1e-5)
#define STD_VAR_MIN 1e-5f
#define STD_MASK_AT 0.0031622776601683794f

// dm[p, c ..] for the messages p0 <= p < p1 (p1 > p0) of one node from the gradients of its mean / min / max / std:
//   dm = dmean/cnt + [m==min] dmin/#ties + [m==max] dmax/#ties + [std>0] dstd (m-mean)/(cnt std)
// mean / min / max / std are recomputed from the message rows with the forward's exact arithmetic (same bits, so the std
// mask decision is identical).  Two forms, the same operations in the same order per element:
//   pna_agg_bwd_item_loaded  1 <= deg <= 4 (every atom of an organic molecule): the three passes run on the node's
//                            messages a[0 .. deg) held in REGISTERS; dp = the item's first output row
//   pna_agg_bwd_item_loop    any degree: three passes over the rows in memory (re-read from L1 / L2)
// pna_agg_bwd_item picks the form and loads the messages of the first: mc = m + c, dmc = dm + c (the item's first channel),
// H = row stride of both.
template <int VEC>
__device__ __forceinline__ void pna_agg_bwd_item_loaded(const float (&gmean)[VEC], const float (&gmn)[VEC],
                                                        const float (&gmx)[VEC], const float (&gsd)[VEC], int deg,
                                                        const float (&a)[4][VEC], float* __restrict__ dp, int H, int centered) {
  float s[VEC], s2[VEC], mn[VEC], mx[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    s[v] = 0.f;
    s2[v] = 0.f;
    mn[v] = INFINITY;
    mx[v] = -INFINITY;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < deg) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        s[v] = __fadd_rn(s[v], a[e][v]);
        s2[v] = __fadd_rn(s2[v], __fmul_rn(a[e][v], a[e][v]));
        mn[v] = fminf(mn[v], a[e][v]);
        mx[v] = fmaxf(mx[v], a[e][v]);
      }
    }
  const float cnt = (float)deg;
  float mean[VEC], sd[VEC], nmn[VEC], nmx[VEC], c2[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    c2[v] = 0.f;
    mean[v] = __fdiv_rn(s[v], cnt);
    float mean2 = __fdiv_rn(s2[v], cnt);
    float var = __fsub_rn(mean2, __fmul_rn(mean[v], mean[v]));
    float o = __fsqrt_rn(fmaxf(var, STD_VAR_MIN));
    sd[v] = (o <= STD_MASK_AT) ? 0.f : o;
    nmn[v] = (mn[v] == 0.f) ? 1.f : 0.f;
    nmx[v] = (mx[v] == 0.f) ? 1.f : 0.f;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < deg) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        nmn[v] += (a[e][v] == mn[v]) ? 1.f : 0.f;
        nmx[v] += (a[e][v] == mx[v]) ? 1.f : 0.f;
        const float dv = a[e][v] - mean[v];
        c2[v] = fmaf(dv, dv, c2[v]);
      }
    }
  float k_mean[VEC], k_mn[VEC], k_mx[VEC], k_sd[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    k_mean[v] = gmean[v] / cnt;
    k_mn[v] = gmn[v] / nmn[v];
    k_mx[v] = gmx[v] / nmx[v];
    const float sdiv = (centered && c2[v] > 0.f) ? sqrtf(c2[v] / cnt) : sd[v];
    k_sd[v] = (sd[v] > 0.f) ? gsd[v] / (cnt * sdiv) : 0.f;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < deg) {
      float o[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float r = k_mean[v] + k_sd[v] * (a[e][v] - mean[v]);
        r += (a[e][v] == mn[v]) ? k_mn[v] : 0.f;
        r += (a[e][v] == mx[v]) ? k_mx[v] : 0.f;
        o[v] = r;
      }
      vstore<VEC>(dp + (int64_t)e * H, o);
    }
}

template <int VEC>
__device__ __forceinline__ void pna_agg_bwd_item_loop(const float (&gmean)[VEC], const float (&gmn)[VEC], const float (&gmx)[VEC],
                                                      const float (&gsd)[VEC], int p0, int p1, const float* __restrict__ mc,
                                                      float* __restrict__ dmc, int H, int centered) {
  float s[VEC], s2[VEC], mn[VEC], mx[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    s[v] = 0.f;
    s2[v] = 0.f;
    mn[v] = INFINITY;
    mx[v] = -INFINITY;
  }
  const float* mp = mc + (int64_t)p0 * H;
  for (int p = p0; p < p1; ++p, mp += H) {  // same order and roundings as k_pna_agg_fwd
    float a[VEC];
    vload<VEC>(a, mp);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      s[v] = __fadd_rn(s[v], a[v]);
      s2[v] = __fadd_rn(s2[v], __fmul_rn(a[v], a[v]));
      mn[v] = fminf(mn[v], a[v]);
      mx[v] = fmaxf(mx[v], a[v]);
    }
  }
  const float cnt = (float)(p1 - p0);
  float mean[VEC], sd[VEC], nmn[VEC], nmx[VEC], c2[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    c2[v] = 0.f;
    mean[v] = __fdiv_rn(s[v], cnt);
    float mean2 = __fdiv_rn(s2[v], cnt);
    float var = __fsub_rn(mean2, __fmul_rn(mean[v], mean[v]));
    float o = __fsqrt_rn(fmaxf(var, STD_VAR_MIN));
    sd[v] = (o <= STD_MASK_AT) ? 0.f : o;
    // torch's scatter_reduce(amin/amax) backward divides by (#src ties + [self == result]) with self = the zero-filled
    // output buffer, also under include_self=False: an extremum that is exactly 0 counts one extra tie.  The reference's
    // CPU path behaves that way (verified on torch 2.10: src [0,-1,0] -> grads [1/3,0,1/3]); reproduced here.
    nmn[v] = (mn[v] == 0.f) ? 1.f : 0.f;
    nmx[v] = (mx[v] == 0.f) ? 1.f : 0.f;
  }
  mp = mc + (int64_t)p0 * H;
  for (int p = p0; p < p1; ++p, mp += H) {
    float a[VEC];
    vload<VEC>(a, mp);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      nmn[v] += (a[v] == mn[v]) ? 1.f : 0.f;
      nmx[v] += (a[v] == mx[v]) ? 1.f : 0.f;
      const float dv = a[v] - mean[v];
      c2[v] = fmaf(dv, dv, c2[v]);
    }
  }
  float k_mean[VEC], k_mn[VEC], k_mx[VEC], k_sd[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    k_mean[v] = gmean[v] / cnt;
    k_mn[v] = gmn[v] / nmn[v];
    k_mx[v] = gmx[v] / nmx[v];
    // masked or not is the forward's decision (sd, bit for bit); the divisor is the centred two-pass std, free of the
    // cancellation error of mean(x^2) - mean(x)^2 (centered = 0: the forward's value, like the CPU path's backward)
    const float sdiv = (centered && c2[v] > 0.f) ? sqrtf(c2[v] / cnt) : sd[v];
    k_sd[v] = (sd[v] > 0.f) ? gsd[v] / (cnt * sdiv) : 0.f;
  }
  mp = mc + (int64_t)p0 * H;
  float* dp = dmc + (int64_t)p0 * H;
  for (int p = p0; p < p1; ++p, mp += H, dp += H) {
    float a[VEC], o[VEC];
    vload<VEC>(a, mp);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float r = k_mean[v] + k_sd[v] * (a[v] - mean[v]);
      r += (a[v] == mn[v]) ? k_mn[v] : 0.f;
      r += (a[v] == mx[v]) ? k_mx[v] : 0.f;
      o[v] = r;
    }
    vstore<VEC>(dp, o);
  }
}

template <int VEC>
__device__ __forceinline__ void pna_agg_bwd_item(const float (&gmean)[VEC], const float (&gmn)[VEC], const float (&gmx)[VEC],
                                                 const float (&gsd)[VEC], int p0, int p1, const float* __restrict__ mc,
                                                 float* __restrict__ dmc, int H, int centered) {
  // (measured and rejected, round 2: keeping the node's first 8 messages in registers for the three passes -- 71 vs 67 us at
  // cfg-2, 0.43 vs 0.59 of HBM as run at cfg-5: the extra 32 VGPRs cost more occupancy than the L1-resident re-reads cost)
  // (the same treatment of k_edge_combine_bwd's dQ gather and of k_gine_fwd / k_gine_bwd_dx -- indices, then rows, four at a time
  // -- was measured and rejected: cfg-3 20.15-20.23 vs 19.99-20.00 ms, cfg-2 neutral; those kernels sit at 0.76 of HBM with
  // one row in flight per thread and lose more occupancy to the 32 extra VGPRs than the loads gain)
  const int deg = p1 - p0;
  if (deg <= 4) {
    // the row's messages are loaded ONCE, all four loads in flight together (clamped addresses past the row's end)
    float a[4][VEC];
#pragma unroll
    for (int e = 0; e < 4; ++e) vload<VEC>(a[e], mc + (int64_t)(p0 + (e < deg ? e : 0)) * H);
    pna_agg_bwd_item_loaded<VEC>(gmean, gmn, gmx, gsd, deg, a, dmc + (int64_t)p0 * H, H, centered);
    return;
  }
  pna_agg_bwd_item_loop<VEC>(gmean, gmn, gmx, gsd, p0, p1, mc, dmc, H, centered);
}
