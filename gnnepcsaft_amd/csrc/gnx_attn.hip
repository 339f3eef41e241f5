// TransformerConv attention (ref: train/models.py:497-511; [3P] torch_geometric.nn.TransformerConv with concat=True,
// beta=False, root_weight=True, edge_dim=H): a segmented softmax over the destination-sorted CSR.
//
// Layout.  One wave per row (destination node in the forward and the destination-side backward, source node in the
// source-side backward); four rows per 256-thread workgroup.  Lane l holds columns [4 (64 k + l), +4) of chunk k,
// k < NV = ceil(H / 256), as float4.  A head = C consecutive columns = a group of G = min(C / 4, 64) lanes of one chunk,
// or (C > 256) all lanes of C / 256 consecutive chunks; per-head dot products reduce with __shfl_xor inside the group
// (and across those chunks).  Every lane of a group ends with the same bits, so the softmax state (running max and
// sum) is uniform over the group without a broadcast.  Per-(edge, head) values are written by the group's first lane
// ("writer"); a later pass of the same kernel reads them back in the SAME thread (program order, no cross-lane
// visibility question), and broadcasts with __shfl where the whole group needs them.
//
// Dropout on alpha (training only): keep(p, h) from Philox4x32-10 on the element e = p * heads + h, i.e. block
// (e / 4, offset) and word e % 4 under the key `seed` -- the scheme of gnx_dropout -- so the backward recomputes it.
#include "gnx_common.hpp"

#include <cmath>

namespace {

constexpr int kRowsPerBlock = 4;  // waves (rows) per 256-thread workgroup
constexpr int kDleChunk = 128;    // code-grouped CSR positions per workgroup of the bond-table gradient

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// per-lane view of the head layout (see the file comment)
template <int NV>
struct Heads {
  int col[NV];   // first column of this lane's float4 in chunk k
  int hd[NV];    // head of that float4
  bool act[NV];  // column inside [0, H)
  bool wr[NV];   // this lane writes the per-(edge, head) values of chunk k
  bool lead;     // first lane of its group in every chunk (reads the per-(edge, head) values back)
  int G, cpc;    // lanes per group inside a chunk; chunks per head (> 1 only for C > 256)
  __device__ Heads(int lane, int H, int C) {
    G = C / 4 < 64 ? C / 4 : 64;
    cpc = C > 256 ? C / 256 : 1;
    lead = (lane & (G - 1)) == 0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      col[k] = 4 * (64 * k + lane);
      act[k] = col[k] < H;
      hd[k] = col[k] / C;
      wr[k] = act[k] && lead && (k % cpc) == 0;
    }
  }
  // per-chunk partial -> per-head total, identical bits on every lane of the head
  __device__ __forceinline__ void reduce(float (&s)[NV]) const {
#pragma unroll
    for (int k = 0; k < NV; ++k)
      for (int o = 1; o < G; o <<= 1) s[k] += __shfl_xor(s[k], o, 64);
    if (cpc > 1) {
      float t[NV];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        t[k] = 0.f;
#pragma unroll
        for (int k2 = 0; k2 < NV; ++k2)
          if (k2 / cpc == k / cpc) t[k] += s[k2];
      }
#pragma unroll
      for (int k = 0; k < NV; ++k) s[k] = t[k];
    }
  }
};

// dropout factor of every chunk's head on edge e: 0 or 1 / (1 - p); one Philox block per distinct e * heads + h >> 2
template <int NV>
__device__ __forceinline__ void keep_factors(float (&d)[NV], const Heads<NV>& L, int64_t e, int heads, float p,
                                             float inv_keep, uint64_t seed, uint64_t offset) {
  int64_t blk = -1;
  uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int64_t el = e * heads + L.hd[k];
    if ((el >> 2) != blk) {
      blk = el >> 2;
      c[0] = (uint32_t)blk;
      c[1] = (uint32_t)((uint64_t)blk >> 32);
      c[2] = (uint32_t)offset;
      c[3] = (uint32_t)(offset >> 32);
      philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    }
    const int w = (int)(el & 3);
    const uint32_t r = w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : c[3];
    d[k] = ((float)(r >> 8) * 5.9604644775390625e-8f >= p) ? inv_keep : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// forward: one wave per destination row i, online softmax (each K / V row gathered once), then a pass over the row's
// raw scores (saved in alpha) that turns them into alpha = exp(score - max) / (sum + 1e-16).
// ---------------------------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(256) k_attn_fwd(const float* __restrict__ qkvs, const float* __restrict__ Le,
                                                  const int* __restrict__ rowptr, const int* __restrict__ src,
                                                  const int* __restrict__ code, int64_t N, int H, int heads, int C,
                                                  float sqrt_c, float p, float inv_keep, uint64_t seed, uint64_t offset,
                                                  float* __restrict__ out, float* __restrict__ alpha,
                                                  uint8_t* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (i >= N) return;  // uniform over the wave
  const Heads<NV> L(lane, H, C);
  const int64_t ld = 4 * (int64_t)H;
  f32x4 q[NV], acc[NV];
  float m[NV], l[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    q[k] = L.act[k] ? ld4(qkvs + i * ld + L.col[k]) : f32x4{0.f, 0.f, 0.f, 0.f};
    acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[k] = -INFINITY;
    l[k] = 0.f;
  }
  const int p0 = rowptr[i], p1 = rowptr[i + 1];
  for (int e = p0; e < p1; ++e) {
    const int64_t j = src[e], c = code[e];
    float s[NV];
    f32x4 v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (L.act[k]) {
        const f32x4 le = ld4(Le + c * H + L.col[k]);
        const f32x4 kk = ld4(qkvs + j * ld + H + L.col[k]) + le;
        v[k] = ld4(qkvs + j * ld + 2 * H + L.col[k]) + le;
        s[k] = dot4(q[k], kk);
      } else {
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        s[k] = 0.f;
      }
    }
    L.reduce(s);
    float d[NV];
    if (p > 0.f) {
      keep_factors<NV>(d, L, e, heads, p, inv_keep, seed, offset);
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) d[k] = 1.f;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      s[k] = s[k] / sqrt_c;
      if (L.wr[k]) {
        alpha[(int64_t)e * heads + L.hd[k]] = s[k];  // raw score until the row is done
        if (keep != nullptr) keep[(int64_t)e * heads + L.hd[k]] = d[k] != 0.f ? 1 : 0;
      }
      const float mn = fmaxf(m[k], s[k]);
      const float r = expf(m[k] - mn), w = expf(s[k] - mn);
      l[k] = l[k] * r + w;
      acc[k] = acc[k] * r + (w * d[k]) * v[k];
      m[k] = mn;
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if (L.act[k]) {
      const float inv = 1.0f / (l[k] + 1e-16f);
      st4(out + i * H + L.col[k], acc[k] * inv + ld4(qkvs + i * ld + 3 * H + L.col[k]));
    }
  }
  for (int e = p0; e < p1; ++e) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (L.wr[k]) {
        float* a = alpha + (int64_t)e * heads + L.hd[k];
        *a = expf(*a - m[k]) / (l[k] + 1e-16f);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward, destination side: one wave per row i.
//   pass A: dalpha_p = d_p <dout_i, v_j + Le_c>,  S = sum_row alpha_p dalpha_p      (dalpha_p parked in dscore)
//   pass B: dscore_p = alpha_p (dalpha_p - S) / sqrt(C),  dq_i = sum_p dscore_p (k_j + Le_c)
// scratch: dscore[E, heads] and alphad[E, heads] = d_p alpha_p (what the source side and dLe need).
// ---------------------------------------------------------------------------------------------------------------
template <int NV>
__global__ void __launch_bounds__(256) k_attn_bwd_dst(const float* __restrict__ dout, const float* __restrict__ qkvs,
                                                      const float* __restrict__ Le, const float* __restrict__ alpha,
                                                      const int* __restrict__ rowptr, const int* __restrict__ src,
                                                      const int* __restrict__ code, int64_t N, int H, int heads, int C,
                                                      float sqrt_c, float p, float inv_keep, uint64_t seed,
                                                      uint64_t offset, float* __restrict__ dqkv,
                                                      float* __restrict__ dscore, float* __restrict__ alphad) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (i >= N) return;
  const Heads<NV> L(lane, H, C);
  const int64_t ld = 4 * (int64_t)H;
  f32x4 g[NV], dq[NV];
  float S[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    g[k] = L.act[k] ? ld4(dout + i * H + L.col[k]) : f32x4{0.f, 0.f, 0.f, 0.f};
    dq[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    S[k] = 0.f;
  }
  const int p0 = rowptr[i], p1 = rowptr[i + 1];
  for (int e = p0; e < p1; ++e) {
    const int64_t j = src[e], c = code[e];
    float da[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
      da[k] = L.act[k] ? dot4(g[k], ld4(qkvs + j * ld + 2 * H + L.col[k]) + ld4(Le + c * H + L.col[k])) : 0.f;
    L.reduce(da);
    float d[NV];
    if (p > 0.f) {
      keep_factors<NV>(d, L, e, heads, p, inv_keep, seed, offset);
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) d[k] = 1.f;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const float a = L.act[k] ? alpha[(int64_t)e * heads + L.hd[k]] : 0.f;  // hd >= heads past column H
      da[k] *= d[k];
      S[k] += a * da[k];
      if (L.wr[k]) {
        dscore[(int64_t)e * heads + L.hd[k]] = da[k];
        alphad[(int64_t)e * heads + L.hd[k]] = a * d[k];
      }
    }
  }
  for (int e = p0; e < p1; ++e) {
    const int64_t j = src[e], c = code[e];
    float ds[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {  // reads of every chunk first: a writer overwrites dalpha with dscore below
      ds[k] = 0.f;
      if (L.lead && L.act[k]) {
        const int64_t o = (int64_t)e * heads + L.hd[k];
        ds[k] = alpha[o] * (dscore[o] - S[k]) / sqrt_c;
      }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (L.wr[k]) dscore[(int64_t)e * heads + L.hd[k]] = ds[k];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      ds[k] = __shfl(ds[k], lane & ~(L.G - 1), 64);
      if (L.act[k]) dq[k] = dq[k] + ds[k] * (ld4(qkvs + j * ld + H + L.col[k]) + ld4(Le + c * H + L.col[k]));
    }
  }
  const int64_t ldg = 3 * (int64_t)H;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (L.act[k]) st4(dqkv + i * ldg + L.col[k], dq[k]);
}

// backward, source side: one wave per node j over the CSR positions leaving it (colptr / cpos, ascending):
//   dk_j = sum dscore_p q_dst,  dv_j = sum alphad_p dout_dst.  Fixed order, no atomics.
template <int NV>
__global__ void __launch_bounds__(256) k_attn_bwd_src(const float* __restrict__ dout, const float* __restrict__ qkvs,
                                                      const int* __restrict__ colptr, const int* __restrict__ cpos,
                                                      const int* __restrict__ dst, int64_t N, int H, int heads, int C,
                                                      const float* __restrict__ dscore,
                                                      const float* __restrict__ alphad, float* __restrict__ dqkv) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (j >= N) return;
  const Heads<NV> L(lane, H, C);
  const int64_t ld = 4 * (int64_t)H;
  f32x4 dk[NV], dv[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) dk[k] = dv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int c0 = colptr[j], c1 = colptr[j + 1];
  for (int t = c0; t < c1; ++t) {
    const int64_t e = cpos[t];
    const int64_t i = dst[e];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (L.act[k]) {
        const int64_t o = e * heads + L.hd[k];
        dk[k] = dk[k] + dscore[o] * ld4(qkvs + i * ld + L.col[k]);
        dv[k] = dv[k] + alphad[o] * ld4(dout + i * H + L.col[k]);
      }
    }
  }
  const int64_t ldg = 3 * (int64_t)H;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if (L.act[k]) {
      st4(dqkv + j * ldg + H + L.col[k], dk[k]);
      st4(dqkv + j * ldg + 2 * H + L.col[k], dv[k]);
    }
  }
}

// dLe[c] += sum over the CSR positions with bond code c of dscore_p q_dst + alphad_p dout_dst, through the inverted
// index (positions stably grouped by code): a workgroup walks kDleChunk consecutive entries, a thread owns 4 channels and
// sums in registers, one atomic add per channel and key run (as k_gine_dle_segment_sum).
__global__ void __launch_bounds__(256) k_attn_dle(const float* __restrict__ dout, const float* __restrict__ qkvs,
                                                  const int* __restrict__ pos, const int* __restrict__ dst,
                                                  const int* __restrict__ key, int64_t E, int H, int heads, int C,
                                                  const float* __restrict__ dscore, const float* __restrict__ alphad,
                                                  float* __restrict__ dLe) {
  const int G = H / 4;
  const int lanes = 256 / G > 0 ? 256 / G : 1;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  if (rl >= lanes) return;
  const int col = cg * 4, hd = col / C;
  const int64_t ld = 4 * (int64_t)H;
  const int64_t i0 = (int64_t)blockIdx.x * kDleChunk;
  const int64_t i1 = i0 + kDleChunk < E ? i0 + kDleChunk : E;
  const int64_t per = (i1 - i0 + lanes - 1) / lanes;
  const int64_t a = i0 + (int64_t)rl * per;
  const int64_t b = a + per < i1 ? a + per : i1;
  if (a >= b) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int cur = key[pos[a]];
  for (int64_t t = a; t < b; ++t) {
    const int64_t e = pos[t];
    const int k = key[e];
    if (k != cur) {
      float* o = dLe + (int64_t)cur * H + col;
      atomicAdd(o, acc.x);
      atomicAdd(o + 1, acc.y);
      atomicAdd(o + 2, acc.z);
      atomicAdd(o + 3, acc.w);
      acc = f32x4{0.f, 0.f, 0.f, 0.f};
      cur = k;
    }
    const int64_t i = dst[e];
    const int64_t o = e * heads + hd;
    acc = acc + dscore[o] * ld4(qkvs + i * ld + col) + alphad[o] * ld4(dout + i * H + col);
  }
  float* o = dLe + (int64_t)cur * H + col;
  atomicAdd(o, acc.x);
  atomicAdd(o + 1, acc.y);
  atomicAdd(o + 2, acc.z);
  atomicAdd(o + 3, acc.w);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// H = heads * C with C % 4 == 0 and the group layout of the file comment (C / 4 a power of two up to 64, or C a
// multiple of 256); H <= 1024 (NV <= 4)
int32_t check_layout(const char* fn, int64_t H, int32_t heads, int32_t C) {
  GNX_CHECK_ARG(heads > 0 && C > 0 && H == (int64_t)heads * C, "%s: heads=%d x C=%d", fn, heads, C);
  GNX_CHECK_ARG(C % 4 == 0 && ((C <= 256 && ((C / 4) & (C / 4 - 1)) == 0) || C % 256 == 0) && H <= 1024,
                "%s: head width C=%d must be 4 x a power of two up to 256 or a multiple of 256, and H=%lld <= 1024", fn,
                C, (long long)H);
  return GNX_OK;
}

template <int NV>
void launch_fwd(gnx_handle* h, gnx_prof_scope& prof, const float* qkvs, const float* Le, const int32_t* rowptr,
                const int32_t* src, const int32_t* code, int64_t N, int H, int heads, int C, float p, uint64_t seed,
                uint64_t offset, float* out, float* alpha, uint8_t* keep) {
  GNX_LAUNCH_TIMED(prof, k_attn_fwd<NV>, dim3((unsigned)gnx_cdiv(N, kRowsPerBlock)), dim3(256), 0, h->stream, qkvs, Le,
                   rowptr, src, code, N, H, heads, C, sqrtf((float)C), p, 1.0f / (1.0f - p), seed, offset, out, alpha,
                   keep);
}

template <int NV>
void launch_bwd(gnx_handle* h, const float* dout, const float* qkvs, const float* Le, const float* alpha,
                const int32_t* rowptr, const int32_t* src, const int32_t* dst, const int32_t* code,
                const int32_t* colptr, const int32_t* cpos, int64_t N, int H, int heads, int C, float p, uint64_t seed,
                uint64_t offset, float* dqkv, float* dscore, float* alphad) {
  const dim3 grid((unsigned)gnx_cdiv(N, kRowsPerBlock));
  hipLaunchKernelGGL(k_attn_bwd_dst<NV>, grid, dim3(256), 0, h->stream, dout, qkvs, Le, alpha, rowptr, src, code, N, H,
                     heads, C, sqrtf((float)C), p, 1.0f / (1.0f - p), seed, offset, dqkv, dscore, alphad);
  hipLaunchKernelGGL(k_attn_bwd_src<NV>, grid, dim3(256), 0, h->stream, dout, qkvs, colptr, cpos, dst, N, H, heads, C,
                     dscore, alphad, dqkv);
}

}  // namespace

extern "C" int32_t gnx_transformer_attn_fwd(gnx_handle* h, const float* qkvs, const float* Le, const int32_t* rowptr,
                                            const int32_t* src, const int32_t* code, int64_t N, int64_t E,
                                            int32_t heads, int32_t C, float p, uint64_t seed, uint64_t offset,
                                            float* out, float* alpha, uint8_t* keep) {
  GNX_CHECK_ARG(h && N >= 0 && E >= 0, "gnx_transformer_attn_fwd: bad argument");
  const int64_t H = (int64_t)heads * C;
  if (int32_t st = check_layout("gnx_transformer_attn_fwd", H, heads, C)) return st;
  GNX_CHECK_ARG(p >= 0.f && p < 1.f, "gnx_transformer_attn_fwd: p=%g not in [0,1)", (double)p);
  if (N == 0) return GNX_OK;
  GNX_CHECK_ARG(qkvs && Le && rowptr && out && (E == 0 || (src && code && alpha)),
                "gnx_transformer_attn_fwd: NULL argument");
  GNX_CHECK_ARG(aligned16(qkvs) && aligned16(Le) && aligned16(out), "gnx_transformer_attn_fwd: float operands must be "
                "16-byte aligned");
  // q|k|v|s read once, out written, alpha written (+ the row pass over alpha), two indices per edge
  gnx_prof_scope prof(h, GNX_K_ATTN_FWD, 4.0 * (5.0 * N * H + E * heads) + 8.0 * E, 0.0, 0.0, true);
  if (H <= 256)
    launch_fwd<1>(h, prof, qkvs, Le, rowptr, src, code, N, (int)H, heads, C, p, seed, offset, out, alpha, keep);
  else if (H <= 512)
    launch_fwd<2>(h, prof, qkvs, Le, rowptr, src, code, N, (int)H, heads, C, p, seed, offset, out, alpha, keep);
  else
    launch_fwd<4>(h, prof, qkvs, Le, rowptr, src, code, N, (int)H, heads, C, p, seed, offset, out, alpha, keep);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_transformer_attn_dle(gnx_handle* h, const float* dout, const float* qkvs, const float* scratch,
                                            const int32_t* dst, const int32_t* code, const int32_t* code_pos, int64_t E,
                                            int32_t heads, int32_t C, int32_t R, float* dLe) {
  GNX_CHECK_ARG(h && E >= 0 && R > 0, "gnx_transformer_attn_dle: bad argument");
  const int64_t H = (int64_t)heads * C;
  if (int32_t st = check_layout("gnx_transformer_attn_dle", H, heads, C)) return st;
  if (E == 0) return GNX_OK;
  GNX_CHECK_ARG(dout && qkvs && scratch && dst && code && code_pos && dLe, "gnx_transformer_attn_dle: NULL argument");
  GNX_CHECK_ARG(aligned16(dout) && aligned16(qkvs), "gnx_transformer_attn_dle: float operands must be 16-byte aligned");
  // gathers of q and dout per edge, two scratch values and three indices per edge
  gnx_prof_scope prof(h, GNX_K_KEY_SEGMENT_SUM, 8.0 * E * H + 8.0 * E * heads + 12.0 * E, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_attn_dle, dim3((unsigned)gnx_cdiv(E, kDleChunk)), dim3(256), 0, h->stream, dout, qkvs,
                   code_pos, dst, code, E, (int)H, heads, C, scratch, scratch + E * heads, dLe);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_transformer_attn_bwd(gnx_handle* h, const float* dout, const float* qkvs, const float* Le,
                                            const float* alpha, const int32_t* rowptr, const int32_t* src,
                                            const int32_t* dst, const int32_t* code, const int32_t* colptr,
                                            const int32_t* cpos, const int32_t* code_pos, int64_t N, int64_t E,
                                            int32_t heads, int32_t C, int32_t R, float p, uint64_t seed,
                                            uint64_t offset, float* dqkv, float* scratch, float* dLe) {
  GNX_CHECK_ARG(h && N >= 0 && E >= 0, "gnx_transformer_attn_bwd: bad argument");
  const int64_t H = (int64_t)heads * C;
  if (int32_t st = check_layout("gnx_transformer_attn_bwd", H, heads, C)) return st;
  GNX_CHECK_ARG(p >= 0.f && p < 1.f, "gnx_transformer_attn_bwd: p=%g not in [0,1)", (double)p);
  if (N == 0) return GNX_OK;
  GNX_CHECK_ARG(dout && qkvs && Le && rowptr && colptr && dqkv &&
                    (E == 0 || (alpha && src && dst && code && cpos && scratch)),
                "gnx_transformer_attn_bwd: NULL argument");
  GNX_CHECK_ARG(aligned16(dout) && aligned16(qkvs) && aligned16(Le) && aligned16(dqkv),
                "gnx_transformer_attn_bwd: float operands must be 16-byte aligned");
  float* dscore = scratch;
  float* alphad = scratch == nullptr ? nullptr : scratch + E * heads;
  {
    // read dout, q|k|v once, alpha; write dq|dk|dv; the two scratch arrays written and read once; indices
    gnx_prof_scope prof(h, GNX_K_ATTN_BWD, 4.0 * (7.0 * N * H + 5.0 * E * heads) + 16.0 * E);
    if (H <= 256)
      launch_bwd<1>(h, dout, qkvs, Le, alpha, rowptr, src, dst, code, colptr, cpos, N, (int)H, heads, C, p, seed, offset,
                    dqkv, dscore, alphad);
    else if (H <= 512)
      launch_bwd<2>(h, dout, qkvs, Le, alpha, rowptr, src, dst, code, colptr, cpos, N, (int)H, heads, C, p, seed, offset,
                    dqkv, dscore, alphad);
    else
      launch_bwd<4>(h, dout, qkvs, Le, alpha, rowptr, src, dst, code, colptr, cpos, N, (int)H, heads, C, p, seed, offset,
                    dqkv, dscore, alphad);
    GNX_LAUNCH_CHECK();
  }
  if (dLe != nullptr) return gnx_transformer_attn_dle(h, dout, qkvs, scratch, dst, code, code_pos, E, heads, C, R, dLe);
  return GNX_OK;
}
