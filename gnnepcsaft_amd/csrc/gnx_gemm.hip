// Dense feature x weight contractions on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD).
//
// Shapes on this path are tall-skinny: M = #edges or #nodes (1e5..1e6), N = 32..512, K = 32..13*F.  The base kernels:
//   k_gemm       tiled 128 x 128 x 32, multi-segment (K-concatenated operands with per-row scale), optional row
//                gather/scatter over degree-class tiles with per-class weights.
//   k_gemm_ws    weights-stationary persistent kernel for ONE segment with K, N <= 128 (the most frequent shape):
//                the weight image stays in LDS for the workgroup's lifetime, 64-row A tiles stream through a double
//                buffer, one barrier per tile.
// Their split-operand forms and the small / mid-size products follow; the weight gradients are in gnx_wgrad.hip.
//
// Lesson baked into the structure (measured, tools/gemm_diag.py + the ISA): any runtime-conditional global load in the
// epilogue ("if (mask) v *= mask[...]", "if (accumulate) v += C[...]") makes hipcc put `s_waitcnt vmcnt(0)` in front of
// EVERY store (3 per store in the first version of this file), serialising the 64 stores of a thread and draining the
// next tile's prefetch.  The epilogue kind is therefore a template parameter, its loads are issued unconditionally
// (clamped addresses) in one batch before they are used, and there are no loads between stores.
//
// LDS images:
//   "row-k" image  T[row][k]  (A always; B when the weight is [n][k], i.e. NT): row stride 36 (tiled) / 132 (ws) floats,
//        i.e. an odd number of 16-B slots.  A lane (i = l&31, h = l>>5) fetches k = 8*kk + 4*h .. +3 with ONE ds_read_b128
//        and feeds element t to MFMA step t, i.e. MFMA step (kk,t) contracts k in {8kk+t, 8kk+4+t}: the k order inside
//        a tile is permuted identically for A and B, which only reorders an exact-fp32 sum; the odd slot stride makes
//        the 16 lanes of every ds_read_b128 group hit 16 distinct 16-byte slots (MI355X_MICROARCH.md, LDS table).
//   "k-row" image  T[k][col]  (B when the weight is [k][n], i.e. NN; both operands of the weight gradient):
//        row stride 128 floats, read with ds_read_b32 (32 consecutive columns per half-wave: conflict-free).
#include "gnx_gemm_plan.hpp"
#include "gnx_pna_agg_item.hpp"
#include "gnx_split.hpp"

#include <cstdlib>
#include <type_traits>

#define MAX_SEGS 4

enum { EPI_PLAIN = 0, EPI_ACCUM = 1, EPI_MASK = 2 };

// Calls f(B_TRANS, EPI) with the run-time (b_trans, epi) pair turned into compile-time constants (std::integral_constant).
template <typename F>
static auto epi_dispatch(bool bt, int epi, F&& f) {
  auto with_bt = [&](auto BT) {
    if (epi == EPI_MASK) return f(BT, std::integral_constant<int, EPI_MASK>{});
    if (epi == EPI_ACCUM) return f(BT, std::integral_constant<int, EPI_ACCUM>{});
    return f(BT, std::integral_constant<int, EPI_PLAIN>{});
  };
  return bt ? with_bt(std::true_type{}) : with_bt(std::false_type{});
}

struct seg_dev {
  const float* a;
  const float* rs;
  const float* b;
  int64_t lda;
  int64_t ldb;
  int64_t cls_stride;  // grouped mode: B of class c starts at b + c * cls_stride (0 = class-independent)
  int k;
  int vec_a;  // 1: float4 loads allowed on A (16B-aligned rows)
  int vec_b;
};

struct gemm_args {
  seg_dev seg[MAX_SEGS];
  int nseg;
  int64_t M;
  int N;
  const float* bias;
  const float* mask;
  int64_t ldmask;
  float* C;
  int64_t ldc;
  int relu;
  // grouped mode (degree classes): workgroup b handles rows row_index[tile_info[3b] .. +tile_info[3b+1]) with the
  // class-tile_info[3b+2] weights; workgroups >= *ntiles exit.  NULL tile_info = plain row tiles.
  const int* row_index;
  const int* tile_info;
  const int* ntiles;
  int ny;  // column tiles (k_gemm3's 1-D grid)
  const __bf16* bsplit;  // k_gemm3: split weight images (k_split_weights)
  int Npad, Kpad;
  int koff[MAX_SEGS];  // padded k offset of every segment inside the images
  int steps;           // K-tiles per output tile
};

// Epilogue of one 32x32 accumulator tile (C/D map: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)).
// rows[r] = global row of accumulator register r (-1 = padding); every lane of a half-wave shares it.
template <int EPI>
__device__ __forceinline__ void epilogue_tile(const f32x16& acc, const int (&rows)[16], int gc, int N, float bv,
                                              int relu, const float* __restrict__ mask, int64_t ldmask,
                                              float* __restrict__ C, int64_t ldc) {
  const bool col_ok = gc < N;
  const int gcc = col_ok ? gc : 0;
  float extra[16];
  if constexpr (EPI != EPI_PLAIN) {
    // one batch of unconditional loads (clamped rows), one wait, then the stores
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t gr = rows[r] < 0 ? 0 : rows[r];
      extra[r] = (EPI == EPI_MASK) ? mask[gr * ldmask + gcc] : C[gr * ldc + gcc];
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bv;
    if constexpr (EPI == EPI_ACCUM) v += extra[r];
    v = relu ? fmaxf(v, 0.f) : v;
    if constexpr (EPI == EPI_MASK) v = (extra[r] > 0.f) ? v : 0.f;
    if (col_ok && rows[r] >= 0) C[(int64_t)rows[r] * ldc + gc] = v;
  }
}

// VEC = every operand is 16-B aligned with leading dimensions / k / class strides multiples of 4 (always true for the
// model's shapes): loads are unconditional float4 from clamped addresses + a select, so all 8 loads of a K-tile are in
// flight together.  VEC = false keeps the generic element-wise path (odd shapes; correctness only).
template <bool B_TRANS, int EPI, bool VEC>
__global__ void __launch_bounds__(256, 2) k_gemm(gemm_args g) {
  __shared__ __attribute__((aligned(16))) float As[BM * LDK];
  __shared__ __attribute__((aligned(16))) float Bs[B_TRANS ? BN * LDK : BK * LDN];
  __shared__ int rid[BM];  // global row of every tile row (-1 = padding)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * BN;
  int cls = 0;
  if (g.tile_info != nullptr) {
    if ((int)blockIdx.x >= g.ntiles[0]) return;
    const int p0 = g.tile_info[3 * blockIdx.x], pr = g.tile_info[3 * blockIdx.x + 1];
    cls = g.tile_info[3 * blockIdx.x + 2];
    if (tid < BM) rid[tid] = (tid < pr) ? g.row_index[p0 + tid] : -1;
  } else {
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    if (tid < BM) rid[tid] = (m0 + tid < g.M) ? (int)(m0 + tid) : -1;
  }
  __syncthreads();

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // staging registers
  f32x4 ra[4], rb[4];

  // loader geometry for the row-k image: 8 lanes cover one 128-B row, 32 rows per pass, 4 passes
  const int lr = tid >> 3;        // 0..31
  const int lk = (tid & 7) * 4;   // 0..28
  // loader geometry for the k-row image (NN B): 32 lanes cover 128 columns, 8 k-rows per pass, 4 passes
  const int br = tid >> 5;        // 0..7
  const int bc = (tid & 31) * 4;  // 0..124
  int grow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) grow[i] = rid[lr + 32 * i];
  int okmask = 0;   // VEC: validity bits of ra[0..3] (bits 0-3) and rb[0..3] (bits 4-7) of the tile in flight
  float rsv[4] = {1.f, 1.f, 1.f, 1.f};

  auto load_tile = [&](const seg_dev& s, int k0) {
    const float* sb = s.b + (int64_t)cls * s.cls_stride;
    if constexpr (VEC) {
      // raw loads only: the select / row scale are applied in store_tile, so nothing consumes the loaded registers
      // before the MFMAs of the current tile have been issued (a select here makes hipcc wait for the loads at once)
      const int kcol = k0 + lk;
      const bool k_ok = kcol < s.k;
      const int kc = k_ok ? kcol : 0;
      okmask = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = grow[i] >= 0 ? grow[i] : 0;
        ra[i] = *reinterpret_cast<const f32x4*>(s.a + row * s.lda + kc);
        rsv[i] = *(s.rs != nullptr ? s.rs + row : &c_one);
        okmask |= (k_ok && grow[i] >= 0) ? (1 << i) : 0;
      }
      if (B_TRANS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gn = n0 + lr + 32 * i;
          rb[i] = *reinterpret_cast<const f32x4*>(sb + (int64_t)(gn < g.N ? gn : 0) * s.ldb + kc);
          okmask |= (k_ok && gn < g.N) ? (16 << i) : 0;
        }
      } else {
        const int nn = n0 + bc;
        const bool n_ok = nn < g.N;
        const int nc = n_ok ? nn : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int kr = k0 + br + 8 * i;
          rb[i] = *reinterpret_cast<const f32x4*>(sb + (int64_t)(kr < s.k ? kr : 0) * s.ldb + nc);
          okmask |= (n_ok && kr < s.k) ? (16 << i) : 0;
        }
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t gm = grow[i];
      int kv = s.k - (k0 + lk);
      kv = gm >= 0 ? kv : 0;
      f32x4 v = ld4(s.a + gm * s.lda + k0 + lk, s.vec_a, kv);
      if (s.rs != nullptr && kv > 0) {
        float sc = s.rs[gm];
        v.x *= sc;
        v.y *= sc;
        v.z *= sc;
        v.w *= sc;
      }
      ra[i] = v;
    }
    if (B_TRANS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int r = lr + 32 * i;
        int gn = n0 + r;
        int kv = s.k - (k0 + lk);
        kv = gn < g.N ? kv : 0;
        rb[i] = ld4(sb + (int64_t)gn * s.ldb + k0 + lk, s.vec_b, kv);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int kr = br + 8 * i;
        int nv = g.N - (n0 + bc);
        nv = (k0 + kr) < s.k ? nv : 0;
        rb[i] = ld4(sb + (int64_t)(k0 + kr) * s.ldb + n0 + bc, s.vec_b, nv);
      }
    }
  };

  auto store_tile = [&]() {
    if constexpr (VEC) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 v = ra[i];
        v.x *= rsv[i];
        v.y *= rsv[i];
        v.z *= rsv[i];
        v.w *= rsv[i];
        ra[i] = ((okmask >> i) & 1) ? v : z;
        rb[i] = ((okmask >> (4 + i)) & 1) ? rb[i] : z;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int r = lr + 32 * i;
      *reinterpret_cast<f32x4*>(&As[r * LDK + lk]) = ra[i];
    }
    if (B_TRANS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int r = lr + 32 * i;
        *reinterpret_cast<f32x4*>(&Bs[r * LDK + lk]) = rb[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int kr = br + 8 * i;
        *reinterpret_cast<f32x4*>(&Bs[kr * LDN + bc]) = rb[i];
      }
    }
  };

  // flattened (segment, k0) tile list
  int s_idx = 0, k0 = 0;
  load_tile(g.seg[0], 0);
  bool more = true;
  while (more) {
    __syncthreads();  // previous compute finished reading LDS
    store_tile();
    __syncthreads();
    // advance and prefetch the next tile into registers
    k0 += BK;
    if (k0 >= g.seg[s_idx].k) {
      ++s_idx;
      k0 = 0;
    }
    more = s_idx < g.nseg;
    if (more) load_tile(g.seg[s_idx], k0);

#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      f32x4 a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        a[mi] = *reinterpret_cast<const f32x4*>(&As[(wm * 64 + mi * 32 + li) * LDK + kk * 8 + 4 * lh]);
      if (B_TRANS) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          b[ni] = *reinterpret_cast<const f32x4*>(&Bs[(wn * 64 + ni * 32 + li) * LDK + kk * 8 + 4 * lh]);
      } else {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const float* p = &Bs[(kk * 8 + 4 * lh) * LDN + wn * 64 + ni * 32 + li];
          b[ni].x = p[0];
          b[ni].y = p[LDN];
          b[ni].z = p[2 * LDN];
          b[ni].w = p[3 * LDN];
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][t], b[ni][t], acc[mi][ni], 0, 0, 0);
    }
  }

#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    int rows[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rows[r] = rid[wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int gc = n0 + wn * 64 + ni * 32 + li;
      const float bv = (g.bias != nullptr && gc < g.N) ? g.bias[gc] : 0.f;
      epilogue_tile<EPI>(acc[mi][ni], rows, gc, g.N, bv, g.relu, g.mask, g.ldmask, g.C, g.ldc);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Weights-stationary persistent GEMM: ONE segment, K <= 128, N <= 128, M = #nodes or #edges.
//   LDS: B image [128][132] (NT) or [128][128] (NN) + 2 x A image [64][132]  = 135 KB (dynamic), 1 workgroup / CU.
//   512 threads: wave w owns the 32x32 MFMA tile at rows (w>>2)*32, columns (w&3)*32 (16 accumulators); two waves per
//   SIMD cover each other's LDS-read latency and epilogue.
// One workgroup per CU keeps the whole weight image in LDS and streams 64-row A tiles through a double buffer: the next
// tile's global loads and the previous tile's stores are in flight while the MFMAs of the current tile run, with ONE
// barrier per tile and none inside the K loop.
// ---------------------------------------------------------------------------------------------------------------
#define WS_BM 64
#define WS_LD 132  // 33 x 16 B: odd -> the 16 lanes of every ds_read_b128 group hit distinct 16-B slots

struct ws_args {
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  int64_t M;
  int N, K;
  const float* bias;
  const float* mask;
  int64_t ldmask;
  float* C;
  int64_t ldc;
  int relu;
  int ntiles;
};

// full-tile epilogue of one 32x32 accumulator tile: no row checks, one base pointer, constant row strides
template <int EPI>
__device__ __forceinline__ void epilogue_tile_full(const f32x16& acc, int64_t row0, int gc, int N, float bv, int relu,
                                                   const float* __restrict__ mask, int64_t ldmask,
                                                   float* __restrict__ C, int64_t ldc) {
  if (gc >= N) return;
  float* cp = C + row0 * ldc + gc;
  float extra[16];
  if constexpr (EPI != EPI_PLAIN) {
    const float* ep = (EPI == EPI_MASK) ? mask + row0 * ldmask + gc : cp;
    const int64_t lde = (EPI == EPI_MASK) ? ldmask : ldc;
#pragma unroll
    for (int r = 0; r < 16; ++r) extra[r] = ep[((r & 3) + 8 * (r >> 2)) * lde];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bv;
    if constexpr (EPI == EPI_ACCUM) v += extra[r];
    v = relu ? fmaxf(v, 0.f) : v;
    if constexpr (EPI == EPI_MASK) v = (extra[r] > 0.f) ? v : 0.f;
    cp[((r & 3) + 8 * (r >> 2)) * ldc] = v;
  }
}

template <bool B_TRANS, int EPI>
__global__ void __launch_bounds__(512, 1) k_gemm_ws(ws_args g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Bs = lds;
  float* As = lds + 128 * WS_LD;  // two buffers of WS_BM * WS_LD
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;       // 8 waves: two per SIMD hide each other's LDS / epilogue latency
  const int wr = (wave >> 2) * 32, wc = (wave & 3) * 32;  // one 32x32 MFMA tile per wave
  const int li = lane & 31, lh = lane >> 5;
  const int kgroups = (g.K + 7) >> 3;

  // ---- weight image, once per workgroup (zero-filled to 128 x 128); addresses clamped, values selected
  {
    const int r = tid >> 5, c4 = (tid & 31) * 4;  // 16 rows per pass, 8 passes
    const int rmax = B_TRANS ? g.N : g.K, cmax = B_TRANS ? g.K : g.N;
    const bool c_ok = c4 < cmax;
    const int cc = c_ok ? c4 : 0;
#pragma unroll 4
    for (int i = 0; i < 8; ++i) {
      const int rr = r + 16 * i;
      const bool ok = c_ok && rr < rmax;
      f32x4 v = *reinterpret_cast<const f32x4*>(g.B + (int64_t)(rr < rmax ? rr : 0) * g.ldb + cc);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      v = ok ? v : z;
      *reinterpret_cast<f32x4*>(&Bs[rr * (B_TRANS ? WS_LD : 128) + c4]) = v;
    }
  }

  // ---- A tile loader: 32 lanes cover one 512-B row, 16 rows per pass, 4 passes; clamped addresses, no branches
  const int ar = tid >> 5, ak = (tid & 31) * 4;
  const bool ak_ok = ak < g.K;
  const int akc = ak_ok ? ak : 0;
  f32x4 ra[4];
  int okmask = 0;  // validity of ra[] of the tile in flight; applied at LDS-store time so the loads stay in flight
  auto load_a = [&](int tile) {
    const int64_t m0 = (int64_t)tile * WS_BM;
    okmask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t gm = m0 + ar + 16 * i;
      ra[i] = *reinterpret_cast<const f32x4*>(g.A + (gm < g.M ? gm : g.M - 1) * g.lda + akc);
      okmask |= (ak_ok && gm < g.M) ? (1 << i) : 0;
    }
  };
  auto store_a = [&](float* buf) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f32x4*>(&buf[(ar + 16 * i) * WS_LD + ak]) = ((okmask >> i) & 1) ? ra[i] : z;
  };

  const int gc = wc + li;
  const float bv = (g.bias != nullptr && gc < g.N) ? g.bias[gc] : 0.f;

  int tile = blockIdx.x;  // grid <= ntiles
  int cur = 0;
  load_a(tile);
  store_a(As);
  __syncthreads();

  while (tile < g.ntiles) {
    const int next = tile + gridDim.x;
    const bool has_next = next < g.ntiles;
    if (has_next) load_a(next);  // wave-uniform branch; loads stay in flight during the MFMAs below
    const int64_t m0 = (int64_t)tile * WS_BM;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* Ap = As + cur * (WS_BM * WS_LD) + (wr + li) * WS_LD + 4 * lh;
    const float* Bp = B_TRANS ? Bs + (wc + li) * WS_LD + 4 * lh : Bs + (4 * lh) * 128 + wc + li;
    auto frag_b = [&](int kk) {
      f32x4 b;
      if (B_TRANS) {
        b = *reinterpret_cast<const f32x4*>(Bp + kk * 8);
      } else {
        const float* p = Bp + kk * 8 * 128;
        b.x = p[0];
        b.y = p[128];
        b.z = p[256];
        b.w = p[384];
      }
      return b;
    };
    // software-pipelined fragment reads: the reads of group kk+1 are issued before the MFMAs of group kk
    f32x4 a0 = *reinterpret_cast<const f32x4*>(Ap), b0 = frag_b(0);
    for (int kk = 0; kk < kgroups; kk += 2) {
      const int k1 = (kk + 1 < kgroups) ? kk + 1 : kk;
      f32x4 a1 = *reinterpret_cast<const f32x4*>(Ap + k1 * 8), b1 = frag_b(k1);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[t], b0[t], acc, 0, 0, 0);
      const int k2 = (kk + 2 < kgroups) ? kk + 2 : kk;
      a0 = *reinterpret_cast<const f32x4*>(Ap + k2 * 8);
      b0 = frag_b(k2);
      if (kk + 1 < kgroups) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[t], b1[t], acc, 0, 0, 0);
      }
    }

    // epilogue (stores stay in flight under the next tile's MFMAs)
    if (m0 + WS_BM <= g.M) {
      epilogue_tile_full<EPI>(acc, m0 + wr + 4 * lh, gc, g.N, bv, g.relu, g.mask, g.ldmask, g.C, g.ldc);
    } else {
      int rows[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t gr = m0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
        rows[r] = gr < g.M ? (int)gr : -1;
      }
      epilogue_tile<EPI>(acc, rows, gc, g.N, bv, g.relu, g.mask, g.ldmask, g.C, g.ldc);
    }

    if (has_next) store_a(As + (cur ^ 1) * (WS_BM * WS_LD));
    __syncthreads();
    cur ^= 1;
    tile = next;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Split-operand weights-stationary GEMM (the default for the shapes k_gemm_ws covers).
//
// fp32 MFMA runs at 1/16 of the bf16 MFMA rate on CDNA4, so the exact-fp32 kernel above is matrix-core bound at ~55 %
// of the fp32 peak while HBM idles.  Here every fp32 operand is written EXACTLY as a sum of three bf16 values
// (x = x1 + x2 + x3: round-to-nearest 8-bit pieces of a 24-bit significand, remainders exact) and the product is
//     a.b ~= a1.b1 + (a1.b2 + a2.b1 + a2.b2 + a1.b3 + a3.b1)          six v_mfma_f32_32x32x16_bf16 = 6/16 of the
// fp32-MFMA time.  Every bf16 x bf16 product is exact in fp32 and the accumulation is fp32; the three dropped terms
// (a2.b3, a3.b2, a3.b3) are <= 2^-25 |a||b|, i.e. below the rounding of the fp32 accumulation itself.  The leading
// term and the five correction terms use separate accumulators (added once at the end) so the corrections are not
// absorbed by the rounding of the large partial sum.  Inf operands give NaN (inf - inf in the remainder).
//
//   * B (<= 128 x 128 weights) lives in REGISTERS: wave w owns output columns (w&3)*32.., its B fragments for all
//     eight 16-deep k-slabs are 3 x 8 x 4 = 96 VGPRs, split once per launch.  No LDS traffic for B at all.
//   * A: 64-row tiles, split when staged: LDS holds three bf16 images [64][128 (+8 pad)] per buffer, two buffers
//     (102 KB).  Row stride 272 B = 17 x 16 B (odd) -> conflict-free ds_read_b128 fragments.
//   * per 16-deep slab a wave issues 3 ds_read_b128 and 6 MFMAs; the kernel is HBM-bound (A in, C out): the marginal
//     cost of 64 more rows per CU is 4.1 us at every size from 2 to 20 tiles per CU (= 4 TB/s of mixed read + write
//     traffic), and neither a second tile of loads in flight (hand-counted asm loads) nor software-pipelined fragment
//     reads moved it; a launch has ~8 us of fixed cost (weight fragments, first tile, drain) on top.
//     Round 2 (same-box A/B, tools/ws3_scaling.py): two register stages of A loads (tiles t+G and t+2G in flight, 64 KB
//     per CU) and a branch-free 8-slab loop for K = 128 (the tile's 48 MFMAs and 24 fragment reads in ONE basic block
//     instead of eight) each changed nothing (25.1 vs 25.2-26.4 us at 81 920 rows, 42-44 vs 40-43 us at 163 840): the
//     kernel moves 64 KB per 64-row tile and CU in 4.1-4.5 us = 14-16 GB/s per CU of mixed read + write traffic, and
//     that -- not latency, issue order or the matrix pipe (96 MFMAs per SIMD and tile = 1.3-1.7 us) -- is its bound.
//     Also measured and rejected: the same kernel as TWO 256-thread workgroups per CU (wave = 64 rows x 32 columns, one LDS
//     stage each, two barriers per tile; built on the idea that the eight waves of this workgroup are barrier-locked into
//     the same phase): bit-identical, 26.7 vs 25.2 us at 81 920 rows, 91.5 vs 87.7 us at 327 680.  With the C stores
//     removed this kernel needs 3.3 us per tile (67 vs 86 us at 327 680 rows), i.e. the on-CU work of a tile -- 96 MFMAs
//     per SIMD (1.3-1.7 us) + the split of 2 x 16 floats per lane (0.6 us) + 48 KB of LDS stores + 192 KB of fragment
//     reads -- adds up whoever issues it: tools/ubench/wave_specialised_overlap.hip shows the same for different waves of one
//     SIMD (0.91 us of MFMAs + 0.84 us of split and LDS stores -> 1.41-1.46 us together).  The split-operand formulation
//     itself, not this kernel's structure, sets the per-tile time; what would remove work is a producer that writes the
//     three bf16 images instead of fp32 (no split, half the staging LDS traffic in every consumer).
// ---------------------------------------------------------------------------------------------------------------
//
// Round 3, measured and rejected: the split of tile t + G issued BETWEEN the MFMA slabs of tile t (two register stages of
// loads, the k_gemm3p scheme; bit-identical): 27.4 vs 27.2 us at 81 920 rows, 42.3 vs 43.6 at 163 840, +1.5 us at 8 192
// rows, step 6.87 vs 6.91 ms with / without the predicate-free form either way -- the split is not what bounds a tile.
#ifdef WS_STAMP  // diagnostic build only (tools/ubench/gemm_ws3_stamp.hip): phase cycle sums of wave 0 per workgroup
__device__ unsigned long long* ws_stamp_buf = nullptr;
#define WS_AT(i)                                     \
  do {                                               \
    __builtin_amdgcn_sched_barrier(0);               \
    const unsigned long long tn_ = clock64();        \
    tacc[i] += tn_ - tprev;                          \
    tprev = tn_;                                     \
    __builtin_amdgcn_sched_barrier(0);               \
  } while (0)
#else
#define WS_AT(i)
#endif
//
// FAST (N == 128, 16-byte aligned C / mask, no accumulate): a predicate-free tile loop.  The result tile is transposed
// 4 x 4 inside every quad of lanes (two DPP exchange stages: lane = column, four rows per register group -> lane = row,
// four columns) and leaves as four 16-byte stores per lane, 8 full 128-byte lines per wave instruction; a partial last
// tile repeats row M - 1 (same inputs -> same value to the same address) and the next tile's loads are always issued
// (past the end: the current tile again), so no branch sits between the loads of tile t + G and their first use and the
// wait in front of the split is an exact vmcnt(stores issued since) -- with the predicated 4-byte epilogue hipcc could
// not count the stores and drained ALL of them (write acknowledgements, ~1 us) before every split.
// NW = waves per workgroup: 8 (64-row tiles, one workgroup per CU) or 4 (32-row tiles, TWO workgroups per CU with their
// own barriers, so that one can issue loads / stores while the other multiplies: in-kernel stamps of the 8-wave form give
// a tile 6.2 k cycles = loads 0.8 k + fragment reads and 48 MFMAs 2.2 k + epilogue 1.2 k + split 0.7 k + barrier 1.3 k, all
// eight waves in the same phase -- tools/ubench/gemm_ws3_stamp.hip).  The same arithmetic per row either way.
template <bool B_TRANS, int EPI, bool FAST, int NW>
__global__ void __launch_bounds__(64 * NW, NW == 8 ? 1 : 2) k_gemm_ws3(ws_args g) {
  constexpr int RS = 2 * NW;               // rows per loader pass (32 lanes per row)
  constexpr int TM = 4 * RS;               // rows per tile: 64 / 32
  constexpr int PIECE = TM * W3_LDB;       // one bf16 image of a tile
  constexpr int BUF = 3 * PIECE;           // the three images
  extern __shared__ __attribute__((aligned(16))) unsigned char lds3[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 2) * 32, wc = (wave & 3) * 32;
  const int li = lane & 31, lh = lane >> 5;
  const int nslab = (g.K + 15) >> 4;
  const int gc = wc + li;

  // ---- A tile loader: 32 lanes cover one 512-B row with consecutive float4 (whole cache lines per wave instruction:
  // a wave load touches 2 rows = 8 lines; 16 lanes x 2 float4 per row touched 16 half-used lines per instruction and
  // was bound by line operations in the texture path), 16 rows per pass, 4 passes
  const int ar = tid >> 5, ak = (tid & 31) * 4;
  const bool ak_ok = ak < g.K;
  const int akc = ak_ok ? ak : 0;
  f32x4 ra[4];
  int okmask = 0;
  auto load_a = [&](int tile) {
    const int64_t m0 = (int64_t)tile * TM;
    okmask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t gm = m0 + ar + RS * i;
      ra[i] = *reinterpret_cast<const f32x4*>(g.A + (gm < g.M ? gm : g.M - 1) * g.lda + akc);
      okmask |= (ak_ok && (FAST || gm < g.M)) ? (1 << i) : 0;  // FAST: rows past the end repeat row M - 1
    }
  };
  typedef __attribute__((ext_vector_type(2))) float f32x2;  // 8-byte LDS word (four bf16)
  auto store_a = [&](unsigned char* buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // rows ar + 2 RS h and ar + 2 RS h + RS: four k each -> one split3 of 8 values
      float x[8];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) x[4 * q + j] = ((okmask >> (2 * h + q)) & 1) ? ra[2 * h + q][j] : 0.f;
      bf16x8 pc[3];
      split3(x, pc[0], pc[1], pc[2]);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(&pc[p]);
        unsigned char* q = buf + p * PIECE + (ar + 2 * RS * h) * W3_LDB + ak * 2;
        *reinterpret_cast<f32x2*>(q) = f32x2{w.x, w.y};
        *reinterpret_cast<f32x2*>(q + RS * W3_LDB) = f32x2{w.z, w.w};
      }
    }
  };

  const float bv = (g.bias != nullptr && gc < g.N) ? g.bias[gc] : 0.f;
  int tile = blockIdx.x;  // grid <= ntiles
  int cur = 0;
  load_a(tile);  // in flight while the weight fragments are fetched and split

  // ---- this wave's B fragments, split once: lane holds column gc, k = 16 s + 8 lh + j
  bf16x8 b1[8], b2[8], b3[8];
  {
    const bool n_ok = gc < g.N;
    const int gcc = n_ok ? gc : 0;
    if (!B_TRANS) {
      // W[k][n]: stage the zero-filled 128 x 128 image in LDS with coalesced float4 loads (the A buffers are not in
      // use yet); the fragment below is then a conflict-free column read instead of 64 strided global loads per lane
      float* wl = reinterpret_cast<float*>(lds3);
      const int r = tid >> 5, c4 = (tid & 31) * 4;
      const bool c_ok = c4 < g.N;
#pragma unroll
      for (int i = 0; i < 128 / RS; ++i) {
        const int rr = r + RS * i;
        f32x4 v = *reinterpret_cast<const f32x4*>(g.B + (int64_t)(rr < g.K ? rr : 0) * g.ldb + (c_ok ? c4 : 0));
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(wl + rr * 128 + c4) = (c_ok && rr < g.K) ? v : z;
      }
      __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      float x[8];
      const int k0 = 16 * s + 8 * lh;
      if (B_TRANS) {  // W[n][k]: 8 consecutive floats of row gc
        const int ka = (k0 < g.K) ? k0 : 0, kb = (k0 + 4 < g.K) ? k0 + 4 : 0;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(g.B + (int64_t)gcc * g.ldb + ka);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(g.B + (int64_t)gcc * g.ldb + kb);
        const bool ok0 = n_ok && k0 < g.K, ok1 = n_ok && k0 + 4 < g.K;  // K % 4 == 0
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          x[j] = ok0 ? v0[j] : 0.f;
          x[4 + j] = ok1 ? v1[j] : 0.f;
        }
      } else {  // W[k][n]: column gc of 8 consecutive rows of the staged image
        const float* wl = reinterpret_cast<const float*>(lds3);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = wl[(k0 + j) * 128 + gc];
      }
      split3(x, b1[s], b2[s], b3[s]);
    }
    if (!B_TRANS) {
      // the image is overwritten by the first A tile.  The fragments are CONSUMED here: hipcc may otherwise sink the LDS
      // reads above to below this barrier (seen in the ISA of a software-pipelined form of this kernel: both barriers
      // back to back, the reads among the first tile's split), where they race with the other waves' stores of that tile
#pragma unroll
      for (int s = 0; s < 8; ++s) asm volatile("" ::"v"(b1[s]), "v"(b2[s]), "v"(b3[s]));
      __syncthreads();
    }
  }

  store_a(lds3);
  __syncthreads();

  // FAST epilogue geometry (see above)
  const int qj = li & 3, colq = wc + (li >> 2) * 4;
  f32x4 bv4 = {0.f, 0.f, 0.f, 0.f};
  if (FAST && g.bias != nullptr)
#pragma unroll
    for (int e = 0; e < 4; ++e) bv4[e] = g.bias[colq + e];
  const float floor_v = g.relu ? 0.f : -__builtin_inff();
  auto quad_swap = [&](float& x, float& y, auto CTRL, bool hi) {
    const float send = hi ? x : y;
    const float got = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), decltype(CTRL)::value, 0xf, 0xf, true));
    x = hi ? got : x;
    y = hi ? y : got;
  };
  using XOR1 = std::integral_constant<int, 0xB1>;  // quad_perm [1,0,3,2]
  using XOR2 = std::integral_constant<int, 0x4E>;  // quad_perm [2,3,0,1]

#ifdef WS_STAMP
  unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long tprev = clock64();
  int ntile_done = 0;
#endif
  while (tile < g.ntiles) {
    const int next = tile + gridDim.x;
    const bool has_next = next < g.ntiles;
    if (FAST) {
      load_a(has_next ? next : tile);
      __builtin_amdgcn_sched_barrier(0);  // (hipcc sinks these loads below the MFMA slabs otherwise)
    } else if (has_next) {
      load_a(next);
    }
    const int64_t m0 = (int64_t)tile * TM;

    f32x16 acc, corr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] = 0.f;
      corr[r] = 0.f;
    }
    const unsigned char* ap = lds3 + cur * BUF + (wr + li) * W3_LDB + 16 * lh;
    WS_AT(0);  // issue of the next tile's loads
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s < nslab) {
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap + 32 * s);
        const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(ap + 32 * s + PIECE);
        const bf16x8 a3 = *reinterpret_cast<const bf16x8*>(ap + 32 * s + 2 * PIECE);
        corr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3[s], corr, 0, 0, 0);
        corr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1[s], corr, 0, 0, 0);
        corr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2[s], corr, 0, 0, 0);
        corr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2[s], corr, 0, 0, 0);
        corr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1[s], corr, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[s], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += corr[r];
    WS_AT(1);  // fragment reads + 48 MFMAs

    if constexpr (FAST) {
      const int64_t rbase = m0 + wr + 4 * lh + qj, rlast = g.M - 1;
      f32x4 ex[4];
      if constexpr (EPI == EPI_MASK) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int64_t gr = rbase + 8 * gq < rlast ? rbase + 8 * gq : rlast;
          ex[gq] = *reinterpret_cast<const f32x4*>(g.mask + gr * g.ldmask + colq);
        }
      }
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        float c0 = acc[4 * gq], c1 = acc[4 * gq + 1], c2 = acc[4 * gq + 2], c3 = acc[4 * gq + 3];
        quad_swap(c0, c1, XOR1{}, (qj & 1) != 0);
        quad_swap(c2, c3, XOR1{}, (qj & 1) != 0);
        quad_swap(c0, c2, XOR2{}, (qj & 2) != 0);
        quad_swap(c1, c3, XOR2{}, (qj & 2) != 0);
        f32x4 v = {c0 + bv4.x, c1 + bv4.y, c2 + bv4.z, c3 + bv4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], floor_v);
        if constexpr (EPI == EPI_MASK)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (ex[gq][e] > 0.f) ? v[e] : 0.f;
        const int64_t gr = rbase + 8 * gq < rlast ? rbase + 8 * gq : rlast;
        *reinterpret_cast<f32x4*>(g.C + gr * g.ldc + colq) = v;
      }
    } else if (m0 + TM <= g.M) {
      epilogue_tile_full<EPI>(acc, m0 + wr + 4 * lh, gc, g.N, bv, g.relu, g.mask, g.ldmask, g.C, g.ldc);
    } else {
      int rows[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t gr = m0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
        rows[r] = gr < g.M ? (int)gr : -1;
      }
      epilogue_tile<EPI>(acc, rows, gc, g.N, bv, g.relu, g.mask, g.ldmask, g.C, g.ldc);
    }

    WS_AT(2);  // epilogue (transpose + stores)
    if (has_next) store_a(lds3 + (cur ^ 1) * BUF);
    WS_AT(3);  // wait for the next tile's loads + split + LDS stores
    __syncthreads();
    WS_AT(4);  // barrier
    cur ^= 1;
    tile = next;
#ifdef WS_STAMP
    ++ntile_done;
#endif
  }
#ifdef WS_STAMP
  if (tid == 0 && ws_stamp_buf != nullptr) {
    for (int i = 0; i < 5; ++i) ws_stamp_buf[(size_t)blockIdx.x * 8 + i] = tacc[i];
    ws_stamp_buf[(size_t)blockIdx.x * 8 + 5] = (unsigned long long)ntile_done;
  }
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// Split-operand tiled GEMM (same contract as k_gemm<.., VEC = true>: multi-segment, row scale, grouped rows; see the
// split-operand notes at k_gemm_ws3).
//   * weights: split once per call by k_split_weights into zero-padded bf16 images [class][3][n][k] (either source
//     layout), so the B tiles are plain 16-B copies global(L2) -> LDS;
//   * activations: split when a K-tile is staged (the only conversion work left in the loop, ~6 VALU ops / element);
//   * LDS  A3[3][128][32 (+8 pad)] bf16, B3[3][128 n][32 k (+8)] bf16, row stride 80 B = 5 x 16 B (odd -> conflict-free
//     ds_read_b128), 60 KB per workgroup, two workgroups per CU.
// Per 16-deep slab a wave (64 x 64 outputs) reads 12 fragments and issues 24 bf16 MFMAs (fp32: 64 MFMAs, 2x the time
// each): 6/16 of the matrix-core time of k_gemm.
// ---------------------------------------------------------------------------------------------------------------

// Weight images for k_gemm3: every segment's B (either layout, any class) is split ONCE per call into three bf16
// images, zero padded (n to 128, every segment's k to 32, segments concatenated) and stored TILE-MAJOR
// [class][n tile][k tile][piece][128][32]: a workgroup copies the 24 KB of a K-tile global -> LDS with fully coalesced
// 16-byte loads (8 cache lines per wave instruction), no conversion work and no bounds checks.
struct split_args {
  seg_dev seg[MAX_SEGS];
  int koff[MAX_SEGS + 1];  // padded k offset of every segment; koff[nseg] = Kpad
  int nseg;
  int N, Npad, Kpad, D;
  int frag;  // 1: fragment-major blocks [slab][piece][n / 32][lane][8] (k_gemm3p), 0: [piece][128 n][32 k] (k_gemm3)
  __bf16* out;
};

// One item of a split: thread `idx` of D * Npad * Kpad / 8 converts 8 consecutive k of one (class, column) and stores its three
// pieces.  seg_of(si) names segment si's weights as a split_src; koff[q] (q <= nseg) are the padded k offsets.  Shared by
// the per-call kernel and the batched one, so both write the same bytes.
struct split_src {
  const float* b;
  int64_t ldb, cls_stride;
  int k;
};

template <bool B_TRANS, typename SegOf>
__device__ __forceinline__ void split_weights_item(int64_t idx, int nseg, const int* koff, SegOf seg_of, int N, int Npad,
                                                   int Kpad, int D, int frag, __bf16* out) {
  const int kgroups = Kpad >> 3;
  const int64_t total = (int64_t)D * Npad * kgroups;
  if (idx >= total) return;
  int c, n, kg;
  if (B_TRANS) {  // W[n][k]: k fastest
    kg = (int)(idx % kgroups);
    n = (int)((idx / kgroups) % Npad);
    c = (int)(idx / ((int64_t)kgroups * Npad));
  } else {  // W[k][n]: n fastest
    n = (int)(idx % Npad);
    kg = (int)((idx / Npad) % kgroups);
    c = (int)(idx / ((int64_t)kgroups * Npad));
  }
  const int kk = kg * 8;
  int si = 0, kbase = 0;  // the segment kk falls into and its padded offset (the offsets grow with q)
#pragma unroll
  for (int q = 1; q < MAX_SEGS; ++q)
    if (q < nseg && kk >= koff[q]) {
      si = q;
      kbase = koff[q];
    }
  const split_src sg = seg_of(si);
  const int kl = kk - kbase;
  const float* sb = sg.b + (int64_t)c * sg.cls_stride;
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool ok = n < N && kl + j < sg.k;
    const int64_t off = B_TRANS ? (int64_t)n * sg.ldb + kl + j : (int64_t)(kl + j) * sg.ldb + n;
    x[j] = ok ? sb[ok ? off : 0] : 0.f;
  }
  bf16x8 p1, p2, p3;
  split3(x, p1, p2, p3);
  // tile-major: [class][n tile][k tile][piece][128 n][32 k] -> the 24 KB of one (n tile, k tile) are contiguous
  const int NT = Npad / BN, KT = Kpad / BK;
  __bf16* blk = out + ((((int64_t)c * NT + n / BN) * KT + kk / BK) * 3) * (BN * BK);
  if (frag) {
    // MFMA B operand of column n, k = 16 slab + 8 half .. +7: lane = 32 half + n % 32 of the (slab, piece, n / 32) fragment
    const int nl = n % BN, kl2 = kk % BK;
    const int64_t lane_off = ((int64_t)(nl >> 5) * 64 + ((kl2 >> 3) & 1) * 32 + (nl & 31)) * 8;
    const int64_t pstride = 4 * 64 * 8, sbase = (int64_t)(kl2 >> 4) * 3 * pstride;
    *reinterpret_cast<bf16x8*>(blk + sbase + lane_off) = p1;
    *reinterpret_cast<bf16x8*>(blk + sbase + pstride + lane_off) = p2;
    *reinterpret_cast<bf16x8*>(blk + sbase + 2 * pstride + lane_off) = p3;
    return;
  }
  __bf16* o = blk + (n % BN) * BK + (kk % BK);
  *reinterpret_cast<bf16x8*>(o) = p1;
  *reinterpret_cast<bf16x8*>(o + BN * BK) = p2;
  *reinterpret_cast<bf16x8*>(o + 2 * BN * BK) = p3;
}

template <bool B_TRANS>
__global__ void __launch_bounds__(256) k_split_weights(split_args g) {
  split_weights_item<B_TRANS>((int64_t)blockIdx.x * 256 + threadIdx.x, g.nseg, g.koff,
                              [&](int si) {
                                const seg_dev& s = g.seg[si];
                                return split_src{s.b, s.ldb, s.cls_stride, s.k};
                              },
                              g.N, g.Npad, g.Kpad, g.D, g.frag, g.out);
}

// The splits of many products in ONE launch (gnx_split_weights_batched: every PNA layer's images, once per step):
// blockIdx.y = problem, blockIdx.x covers that problem's D * Npad * Kpad / 8 items (the grid is as wide as the largest
// problem; blocks past a problem's end return).  A problem is what a split needs of a call -- per segment b, ldb, the class
// stride and k; N, the class count, the layout and the image address -- 120 bytes, so 32 of them travel in the
// kernel-argument block (4 KB): no descriptor buffer on the device, no copy.  Npad, Kpad and the k offsets follow from
// N and k as in gemm_plan_of.
#define SPLIT_MAX_BATCH 32
struct split_batch_seg {
  const float* b;
  int64_t cls_stride;
  int32_t ldb, k;
};
struct split_batch_prob {
  split_batch_seg seg[MAX_SEGS];
  __bf16* out;
  int32_t N, D;
  int32_t nseg;
  int32_t layout;  // bit 0: B_TRANS, bit 1: fragment-major
};
struct split_batch_args {
  split_batch_prob p[SPLIT_MAX_BATCH];
  int32_t n;
};
static_assert(sizeof(split_batch_prob) == 120 && sizeof(split_batch_args) <= 4096, "split_batch_args: kernel-argument limit");

__global__ void __launch_bounds__(256) k_split_weights_batched(split_batch_args b) {
  const split_batch_prob& p = b.p[blockIdx.y];
  int koff[MAX_SEGS + 1];
  koff[0] = 0;
#pragma unroll
  for (int s = 0; s < MAX_SEGS; ++s) koff[s + 1] = koff[s] + (s < p.nseg ? (p.seg[s].k + BK - 1) / BK * BK : 0);
  const int Npad = (p.N + BN - 1) / BN * BN, Kpad = koff[MAX_SEGS];
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  auto seg_of = [&](int si) {
    const split_batch_seg& s = p.seg[si];
    return split_src{s.b, (int64_t)s.ldb, s.cls_stride, s.k};
  };
  if (p.layout & 1)
    split_weights_item<true>(idx, p.nseg, koff, seg_of, p.N, Npad, Kpad, p.D, (p.layout >> 1) & 1, p.out);
  else
    split_weights_item<false>(idx, p.nseg, koff, seg_of, p.N, Npad, Kpad, p.D, (p.layout >> 1) & 1, p.out);
}

// Persistent workgroups (two per CU): workgroup w walks the virtual tile ids w, w + G, w + 2G, ...  A virtual id v maps
// to (row tile, column tile) so that the column tiles of one row tile get ids 8 apart = the same XCD (ids are dealt
// round-robin to the 8 XCDs and G % 8 == 0): the shared A rows hit that XCD's L2.  Row tiles grow with v, so the first
// invalid tile ends the walk.  The loads of the next tile (its row ids, then its first K-tile) are issued while the
// current tile is still multiplying, so a workgroup waits on a cold pipeline only once.
//
// Where a workgroup's time goes (s_memtime stamps around the phases, post-layer-0 shape, 25 K-tiles per workgroup on
// average): issuing the 10 loads of a K-tile 20 % (the waves stall AT the load instructions: 40 KB per K-tile through
// the CU's 64 B/clk vector-memory path, shared by both resident workgroups), split + LDS store incl. the wait for the
// data 22 %, LDS reads + MFMA issue 17 % + 7 % waiting for the other waves' MFMAs at the barrier, epilogue 6 %, tile
// switch / prologue the rest.  The phases of one workgroup are serial; only the two resident workgroups overlap.
//
// Measured dead ends on MI355X (kept out of the code, recorded here): a 512-thread double-buffered variant with
// hand-counted inline-asm loads, the same with the loads interleaved between MFMAs, and a loader/multiply
// wave-specialised variant were all correct and all 3-20 % SLOWER than this two-barrier form; their phase ablations
// were additive (load + split + MFMA time), i.e. the phases did not overlap inside one workgroup whatever the
// structure, while two independent workgroups per CU do overlap each other.
//
// Round 2 measured the pieces one by one (tools/ubench/*.hip, tools/gemm3_kslope.py, ablations of a software-pipelined
// rewrite that is NOT in the tree):
//   * the matrix pipe: 48 bf16 MFMAs take 0.65 us per wave at 2.4 GHz, 0.84-0.87 us with random operands on all 256 CUs
//     (the power management holds the clock near 1.8 GHz; <= 128 active CUs or constant operands are not throttled);
//     that is the floor of a K-tile, against 1.5-1.7 us (A inside the Infinity Cache) and 1.85-2.1 us (A streamed from
//     HBM) that a K-tile costs a CU in this kernel.  A lone workgroup finishes a tile in 34 us, two sharing a CU need
//     75 us for their two tiles: the second workgroup per CU hides epilogues and tile switches, not the K loop;
//   * the same wave can overlap its split (VALU) with its MFMAs: 48 MFMAs + the split of 32 floats take 0.78 us where
//     the parts take 0.65 + 0.60 us;
//   * a rewrite with ONE workgroup per CU, one barrier per K-tile, the split / LDS stores of K-tile j+2 and the global
//     loads of K-tile j+4 issued inside the MFMA block of K-tile j, B fragments fetched straight from a fragment-major
//     weight image into registers and a three-stage LDS ring for A reached 1.15 us per K-tile with A in the Infinity
//     Cache (MFMAs alone 0.75, + fragment reads and loads 1.06, + split and LDS stores 1.15) but 1.8-1.9 us from HBM
//     and ~20 us more per launch in prologue / epilogues that no second workgroup hides: not faster (111 vs 113-122 us
//     on post-layer 0).  Pinning the order of MFMA groups, fragment reads and LDS stores with sched_barrier and a
//     1 x 4 instead of a 2 x 2 wave grid (B read once per workgroup: L2 serves ~70 GB/s per CU, the Infinity Cache
//     ~33, HBM ~24) did not move these numbers;
//   * the same pipeline with TWO workgroups per CU (two-stage ring, no cross-barrier fragment prefetch, 218 VGPRs) is
//     k_gemm3p below: 0.9 us per K-tile and CU once both workgroups are in their K loops (the MFMA floor), 1.1 / 1.4 us
//     per K-tile over whole launches (Infinity Cache / HBM) against 1.75 / 2.0 us here.  It takes the products with
//     >= 12 K-tiles per tile; this kernel keeps the shorter ones (equal speed at 4 and 8 K-tiles, shorter prologue).
template <int EPI>
__global__ void __launch_bounds__(256, 2) k_gemm3(gemm_args g) {
  __shared__ __attribute__((aligned(16))) unsigned char A3[G3_OP];
  __shared__ __attribute__((aligned(16))) unsigned char B3[G3_OP];
  __shared__ int rid[BM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  // loader geometry.  A: 8 lanes cover one 128-byte row segment (one cache line), 32 rows per pass, 4 passes: every
  // wave instruction touches 8 whole lines (two lanes per row = 32 lines per instruction, each line hit by four
  // instructions, was texture-path bound).  B: the 24 KB K-tile of the tile-major image is read linearly.
  const int lrow = tid >> 3, lk4 = (tid & 7) * 4;
  const int NT = g.Npad / BN, KT = g.Kpad / BK;

  const int ny = g.ny, G = gridDim.x;
  const bool grouped = g.tile_info != nullptr;
  const int nrt = grouped ? g.ntiles[0] : (int)((g.M + BM - 1) / BM);
  auto row_tile_of = [&](int v) { return (v / (8 * ny)) * 8 + ((v % (8 * ny)) & 7); };
  auto n0_of = [&](int v) { return ((v % (8 * ny)) >> 3) * BN; };

  // tile context: cur = tile being multiplied, nxt = the following one (row ids in flight), ti2 = tile_info of the
  // one after that (two-level dependency tile_info -> row_index, each level fetched one tile ahead)
  int v_cur = blockIdx.x;
  if (row_tile_of(v_cur) >= nrt) return;
  int grow[4], cls, n0, grow_n[4] = {-1, -1, -1, -1}, ridt_n = -1, cls_n = 0, n0_n = 0, ti2_p0 = 0, ti2_pr = 0, ti2_cls = 0;
  bool valid_n;
  auto fetch_ti = [&](int v, int& p0, int& pr, int& c) {  // tile_info triple (clamped; callers check validity)
    const int rt = row_tile_of(v);
    const int rtc = rt < nrt ? rt : 0;
    p0 = g.tile_info[3 * rtc];
    pr = g.tile_info[3 * rtc + 1];
    c = g.tile_info[3 * rtc + 2];
  };
  auto fetch_rows = [&](int v, int p0, int pr, int c, int (&gr)[4], int& rt_id, int& cl) {
    const int t = tid < BM ? tid : 0;
    if (grouped) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = lrow + 32 * q;
        gr[q] = g.row_index[p0 + (r < pr ? r : 0)];
        gr[q] = r < pr ? gr[q] : -1;
      }
      rt_id = g.row_index[p0 + (t < pr ? t : 0)];
      rt_id = t < pr ? rt_id : -1;
      cl = c;
    } else {
      const int64_t m0 = (int64_t)row_tile_of(v) * BM;
#pragma unroll
      for (int q = 0; q < 4; ++q) gr[q] = (m0 + lrow + 32 * q < g.M) ? (int)(m0 + lrow + 32 * q) : -1;
      rt_id = (m0 + t < g.M) ? (int)(m0 + t) : -1;
      cl = 0;
    }
  };
  {
    int p0 = 0, pr = 0, c = 0, rt_id;
    if (grouped) fetch_ti(v_cur, p0, pr, c);
    fetch_rows(v_cur, p0, pr, c, grow, rt_id, cls);
    n0 = n0_of(v_cur);
    if (tid < BM) rid[tid] = rt_id;
    valid_n = row_tile_of(v_cur + G) < nrt;
    if (valid_n) {
      if (grouped) fetch_ti(v_cur + G, p0, pr, c);
      fetch_rows(v_cur + G, p0, pr, c, grow_n, ridt_n, cls_n);
      n0_n = n0_of(v_cur + G);
    }
    if (grouped) fetch_ti(v_cur + 2 * G, ti2_p0, ti2_pr, ti2_cls);
  }
  __syncthreads();

  // one accumulator per 32x32 tile (the register budget of a 128x128 tile does not allow k_gemm_ws3's separate
  // correction accumulators): 6 roundings per 16 k instead of the 16 of the fp32 MFMA chain
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 ra[4];   // A K-tile of the next stage (fp32, split at store time): rows lrow + 32 q, k lk4..+3
  f32x4 rb[6];   // B K-tile of the next stage: six 16-byte words of the contiguous [3][128][32] bf16 block
  int kvalid_a = 0;  // per-pass validity bits of ra, applied at store time

  // Load cursor state kept in registers: indexing g.seg[] / g.koff[] with a run-time index is a kernarg load + wait,
  // and the row byte offsets are 64-bit multiplies -- both are paid when the segment (or tile) changes, not per K-tile
  // (measured with s_memtime: the "issue the loads" phase was 24 % of the workgroup's lifetime before this).
  const float* rowp[4];   // this thread's four A rows in the current segment (k = 0)
  int rowv = 0;           // validity bits of the four rows
  int segK = 0;
  const __bf16* bptr = nullptr;  // this thread's 16-byte slot in the B block of the cursor's K-tile
  auto enter_segment = [&](int s_i, const int (&gr)[4]) {
    const seg_dev& s = g.seg[s_i];
    rowv = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      rowp[q] = s.a + (int64_t)(gr[q] >= 0 ? gr[q] : 0) * s.lda;
      rowv |= gr[q] >= 0 ? (1 << q) : 0;
    }
    segK = s.k;
  };
  auto enter_tile = [&](const int (&gr)[4], int cl, int nn0) {
    enter_segment(0, gr);
    bptr = g.bsplit + (((int64_t)cl * NT + nn0 / BN) * KT * 3) * (BN * BK) + tid * 8;
  };
  auto load_ab = [&](int k0) {  // K-tile at (current segment, k0); the B blocks of a tile are consecutive
    const int k = k0 + lk4;
    const bool k_ok = k < segK;
    const int kc = k_ok ? k : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) ra[q] = *reinterpret_cast<const f32x4*>(rowp[q] + kc);
    kvalid_a = k_ok ? rowv : 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) rb[j] = *reinterpret_cast<const f32x4*>(bptr + j * 2048);
    bptr += 3 * (BN * BK);
  };

  typedef __attribute__((ext_vector_type(2))) float f32x2;  // 8-byte LDS word (four bf16)
  auto store_tile = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // rows (lrow + 64 h, lrow + 64 h + 32): four k each -> one split3 of 8 values
      float xa[8];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) xa[4 * q + j] = ((kvalid_a >> (2 * h + q)) & 1) ? ra[2 * h + q][j] : 0.f;
      bf16x8 pc[3];
      split3(xa, pc[0], pc[1], pc[2]);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(&pc[p]);
        unsigned char* qa = A3 + p * G3_PIECE + (lrow + 64 * h) * G3_LDB + lk4 * 2;
        *reinterpret_cast<f32x2*>(qa) = f32x2{w.x, w.y};
        *reinterpret_cast<f32x2*>(qa + 32 * G3_LDB) = f32x2{w.z, w.w};
      }
    }
    // B: chunk c = j * 256 + tid of the contiguous [piece][128][32] block -> piece j / 2, row (j & 1) * 64 + tid / 4
#pragma unroll
    for (int j = 0; j < 6; ++j)
      *reinterpret_cast<f32x4*>(B3 + (j >> 1) * G3_PIECE + ((j & 1) * 64 + (tid >> 2)) * G3_LDB + (tid & 3) * 16) = rb[j];
  };

  auto compute = [&]() {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      bf16x8 a[2][3], b[2][3];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int p = 0; p < 3; ++p)
          a[mi][p] = *reinterpret_cast<const bf16x8*>(A3 + p * G3_PIECE + (wm * 64 + mi * 32 + li) * G3_LDB + 32 * sl + 16 * lh);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int p = 0; p < 3; ++p)
          b[ni][p] = *reinterpret_cast<const bf16x8*>(B3 + p * G3_PIECE + (wn * 64 + ni * 32 + li) * G3_LDB + 32 * sl + 16 * lh);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) mfma_3x3(acc[mi][ni], a[mi], b[ni]);
    }
  };

  // bias of the current tile's columns (fetched at the tile switch, consumed in the epilogue)
  float bv[2];
  auto fetch_bias = [&](int nn0) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int gc = nn0 + wn * 64 + ni * 32 + li;
      bv[ni] = (g.bias != nullptr && gc < g.N) ? g.bias[gc] : 0.f;
    }
  };
  fetch_bias(n0);

  int s1 = 0, k1 = 0;  // (segment, k) of the K-tile held in ra / rb
  enter_tile(grow, cls, n0);
  load_ab(0);
  while (true) {
    __syncthreads();  // previous multiply finished reading LDS
    store_tile();
    __syncthreads();
    // advance to the next K-tile; past the last segment it is the next tile's first K-tile
    k1 += BK;
    bool last = false;
    if (k1 >= segK) {
      ++s1;
      k1 = 0;
      last = s1 >= g.nseg;
      if (!last) enter_segment(s1, grow);
    }
    if (!last) {
      load_ab(k1);
    } else if (valid_n) {
      enter_tile(grow_n, cls_n, n0_n);
      load_ab(0);
    }
    compute();
    if (!last) continue;

    // ---- tile finished: epilogue, then switch to the next tile's context
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      int rows[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) rows[r] = rid[wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int gc = n0 + wn * 64 + ni * 32 + li;
        epilogue_tile<EPI>(acc[mi][ni], rows, gc, g.N, bv[ni], g.relu, g.mask, g.ldmask, g.C, g.ldc);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
      }
    }
    if (!valid_n) break;
    __syncthreads();  // every wave has read rid[] of the finished tile
    v_cur += G;
#pragma unroll
    for (int q = 0; q < 4; ++q) grow[q] = grow_n[q];
    cls = cls_n;
    n0 = n0_n;
    if (tid < BM) rid[tid] = ridt_n;  // ordered before its first use by the two barriers of the next stage
    fetch_bias(n0);
    s1 = 0;
    k1 = 0;
    valid_n = row_tile_of(v_cur + G) < nrt;
    if (valid_n) {
      fetch_rows(v_cur + G, ti2_p0, ti2_pr, ti2_cls, grow_n, ridt_n, cls_n);
      n0_n = n0_of(v_cur + G);
    }
    if (grouped) fetch_ti(v_cur + 2 * G, ti2_p0, ti2_pr, ti2_cls);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Software-pipelined form of k_gemm3 (same contract, same arithmetic, same tile walk, two workgroups per CU).
//   * B never touches LDS: k_split_weights writes the images FRAGMENT-major, so a lane fetches its 16-byte MFMA operand
//     straight from L2 (a wave reads 1 KB contiguous per fragment); wave w multiplies all 128 rows by the 32 columns
//     32 w .., so the four waves read disjoint fragments (24 KB per K-tile and workgroup) and a slab's registers are
//     refilled with the next K-tile's fragments right after its MFMAs are issued;
//   * A: global loads three K-tiles ahead (two register stages), split + ds_write ONE K-tile ahead into the other half
//     of a two-stage LDS ring, inside the MFMA block of the current K-tile; ONE barrier per K-tile;
//   * every load of the loop is unconditional (clamped addresses, validity applied at LDS-store time): a load inside a
//     conditional block makes the compiler's s_waitcnt insertion fall back to vmcnt(0), i.e. exposes the memory latency;
//   * the second workgroup of the CU covers what one workgroup cannot hide: the LDS round trip behind the barrier,
//     prologue, epilogue and tile switch.
// Needs >= 4 K-tiles per output tile (the load cursor is at most one tile ahead of the multiply); used from 8.
// Bit-identical to k_gemm3 (same MFMAs, same operands, same order per accumulator: tests/test_gemm_split_gpu.py).
// Measured (tools/gemm3_diag.py, same box, us per launch, k_gemm3 -> k_gemm3p): post-layer 0 (K = 640) at 81 920 rows
// 104 -> 97, at 131 072 rows 167 -> 151, at 655 360 rows 744 -> 643 (0.40 of the bf16 peak); K = 384 product 71.5 -> 62.7;
// a lone workgroup's K-tile 1.36 us.  In-kernel wall-clock stamps (65 536 rows, one tile per workgroup, K = 640): prologue
// 3.4-5.1 us, K loop 2.0 us per K-tile in the CU's first workgroup and 2.4 us in its second (= 1.1-1.2 us per K-tile and CU
// against the 0.87 us MFMA floor), epilogue (64 four-byte stores per lane) 3.0-5.0 us, workgroup lifetime 48-57 us inside a
// 65 us kernel (dispatch of 2048 waves and the final write-back are the rest); on top of that cfg-2's 640 tiles meet 512
// workgroups; whole step (tools/ab_bench.py base / nopipe): cfg-2 7.75 vs 7.82 ms, cfg-4's batch 27.2 vs 27.5.
// ---------------------------------------------------------------------------------------------------------------
#define G3P_STAGES 2
#define G3P_MIN_KTILES 8  // shorter K: the two-barrier kernel is as fast (measured at 4 K-tiles) and has the shorter prologue; at 8
                         // K-tiles (cfg-3's 256-wide GINE layers, 327 680 rows) the pipelined kernel is worth 0.34 of the 19.4 ms step
#define G3P_LDS(MI) (G3P_STAGES * 3 * 32 * (MI) * G3_LDB + 2 * 32 * (MI) * 4)

// MI = 32-row blocks per tile (4: 128-row tiles; 3: 96-row tiles, taken when 128-row tiles leave the last round of the
// persistent workgroups mostly idle: cfg-2's 81 920 rows are 640 tiles for 512 workgroup slots).  Same arithmetic per row.
// Measured (round 3, same-box A/B of the cfg-2 step, 6.97-7.05 ms): 96-row tiles -0.01...-0.02 ms only -- the CU, not the
// workgroup slot, is the unit to balance (854 x 0.75 tiles are the same 2.5 tile-equivalents per CU as 640, and a workgroup
// alone on its CU runs nearly twice as fast); 160-row tiles (MI = 5: exactly two per CU, a fifth less B traffic per row, but
// 248 VGPRs and 76 KB of LDS) were +0.06 ms and are not instantiated.
template <int EPI, int MI>
__global__ void __launch_bounds__(256, 2) k_gemm3p(gemm_args g) {
  constexpr int TM = 32 * MI;             // rows per tile
  constexpr int PIECE = TM * G3_LDB;      // one bf16 image of a TM x 32 K-tile
  constexpr int OP = 3 * PIECE;           // the three images
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_p[];
  unsigned char* const Abuf = lds_p;                                  // [2][OP]
  int* const rid = reinterpret_cast<int*>(lds_p + G3P_STAGES * OP);   // [2][TM]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // wave w multiplies ALL 128 rows by the 32 columns w*32..: the four waves read disjoint B fragments (24 KB per
  // K-tile and workgroup from L2; a 2 x 2 wave grid reads every fragment twice, and at ~70 GB/s per CU from L2 plus
  // ~30 GB/s per CU for A that, not the matrix pipe, bounds the K-tile)
  const int li = lane & 31, lh = lane >> 5;
  const int lrow = tid >> 3, lk4 = (tid & 7) * 4;
  const int NT = g.Npad / BN, KT = g.Kpad / BK;

  const int ny = g.ny, G = gridDim.x;
  const bool grouped = g.tile_info != nullptr;
  const int nrt = grouped ? g.ntiles[0] : (int)((g.M + TM - 1) / TM);
  auto row_tile_of = [&](int v) { return (v / (8 * ny)) * 8 + ((v % (8 * ny)) & 7); };
  auto n0_of = [&](int v) { return ((v % (8 * ny)) >> 3) * BN; };

  int v_l = blockIdx.x;  // tile of the A load cursor (the multiply is at most one tile behind it)
  if (row_tile_of(v_l) >= nrt) return;

  auto fetch_ti = [&](int v, int& p0, int& pr, int& c) {
    const int rt = row_tile_of(v);
    const int rtc = rt < nrt ? rt : 0;
    p0 = g.tile_info[3 * rtc];
    pr = g.tile_info[3 * rtc + 1];
    c = g.tile_info[3 * rtc + 2];
  };
  // row ids of a tile: RAW loaded values; the r < rows select is applied where the ids are consumed, a tile later (a
  // select right here would wait for these loads, and with them for every K-tile load in flight, at each tile switch)
  auto fetch_rows = [&](int v, int p0, int pr, int c, int (&gr)[MI], int& rt_id, int& cl) {
    const int t = tid < TM ? tid : 0;
    if (grouped) {
#pragma unroll
      for (int q = 0; q < MI; ++q) {
        const int r = lrow + 32 * q;
        gr[q] = g.row_index[p0 + (r < pr ? r : 0)];
      }
      rt_id = g.row_index[p0 + (t < pr ? t : 0)];
      cl = c;
    } else {
      const int64_t m0 = (int64_t)row_tile_of(v) * TM;
#pragma unroll
      for (int q = 0; q < MI; ++q) gr[q] = (int)(m0 + lrow + 32 * q);
      rt_id = (int)(m0 + t);
      cl = 0;
    }
  };
  auto rows_in_tile = [&](int v, int pr) {
    return grouped ? pr : (int)min((int64_t)TM, g.M - (int64_t)row_tile_of(v) * TM);
  };

  // A cursor's tile (cgrow), the tile after it (grow_n ..: row ids fetched one tile ahead, its tile_info two ahead), and
  // what the multiply / the B cursor take over when they reach the tile the A cursor has entered (ridt_p, n0_p, cls_p)
  int cgrow[MI], grow_n[MI] = {}, ridt_n = 0, pr_n = 0, cls_n = 0, n0_n = 0, ti2_p0 = 0, ti2_pr = 0, ti2_cls = 0;
  int n0_c, ridt_p = -1, n0_p = 0, cls_p = 0;
  bool valid_n, pend = false, cursor_valid = true;
  int tpar = 0, cls0 = 0;
  {
    int p0 = 0, pr = 0, c = 0, rt_id, cl;
    if (grouped) fetch_ti(v_l, p0, pr, c);
    fetch_rows(v_l, p0, pr, c, cgrow, rt_id, cl);
    {
      const int nr = rows_in_tile(v_l, pr);
#pragma unroll
      for (int q = 0; q < MI; ++q) cgrow[q] = (lrow + 32 * q < nr) ? cgrow[q] : -1;
      if (tid < TM) rid[tid] = tid < nr ? rt_id : -1;
    }
    n0_c = n0_of(v_l);
    valid_n = row_tile_of(v_l + G) < nrt;
    if (valid_n) {
      if (grouped) fetch_ti(v_l + G, p0, pr, c);
      fetch_rows(v_l + G, p0, pr, c, grow_n, ridt_n, cls_n);
      pr_n = rows_in_tile(v_l + G, pr);
      n0_n = n0_of(v_l + G);
    }
    if (grouped) fetch_ti(v_l + 2 * G, ti2_p0, ti2_pr, ti2_cls);
    cls0 = cl;
  }

  f32x16 acc[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  f32x4 ra[2][MI];          // A K-tiles in flight (fp32), two register stages
  int kvalid[2] = {0, 0};
  bf16x8 bfr[2][3];        // B fragments [slab][piece]: a slab is refilled (next K-tile) right after its MFMAs

  // ---- A cursor
  const float* rowp[MI];
  int rowv = 0, segK = 0, s1 = 0, k1 = 0;
  auto enter_segment = [&](int s_i) {
    const seg_dev& s = g.seg[s_i];
    rowv = 0;
#pragma unroll
    for (int q = 0; q < MI; ++q) {
      rowp[q] = s.a + (int64_t)(cgrow[q] >= 0 ? cgrow[q] : 0) * s.lda;
      rowv |= cgrow[q] >= 0 ? (1 << q) : 0;
    }
    segK = s.k;
  };
  auto load_a = [&](auto PC) {  // K-tile at the cursor -> register stage P (always issued)
    constexpr int P = decltype(PC)::value;
    const int k = k1 + lk4;
    const bool k_ok = k < segK;
    const int kc = k_ok ? k : 0;
#pragma unroll
    for (int q = 0; q < MI; ++q) ra[P][q] = *reinterpret_cast<const f32x4*>(rowp[q] + kc);
    kvalid[P] = (k_ok && cursor_valid) ? rowv : 0;
  };
  auto cursor_step = [&]() {
    if (!cursor_valid) return;
    k1 += BK;
    if (k1 < segK) return;
    ++s1;
    k1 = 0;
    if (s1 < g.nseg) {
      enter_segment(s1);
      return;
    }
    s1 = 0;
    if (valid_n) {
#pragma unroll
      for (int q = 0; q < MI; ++q) cgrow[q] = (lrow + 32 * q < pr_n) ? grow_n[q] : -1;
      enter_segment(0);
      ridt_p = tid < pr_n ? ridt_n : -1;
      n0_p = n0_n;
      cls_p = cls_n;
      pend = true;
      v_l += G;
      valid_n = row_tile_of(v_l + G) < nrt;
      if (valid_n) {
        fetch_rows(v_l + G, ti2_p0, ti2_pr, ti2_cls, grow_n, ridt_n, cls_n);
        pr_n = rows_in_tile(v_l + G, ti2_pr);
        n0_n = n0_of(v_l + G);
      }
      if (grouped) fetch_ti(v_l + 2 * G, ti2_p0, ti2_pr, ti2_cls);
    } else {
      cursor_valid = false;  // the loads go on over the last tile's first K-tile and are never multiplied
      enter_segment(0);
    }
  };

  // ---- B cursor: this lane's 16-byte slot of the fragment-major block [slab][piece][ni 0..3][lane][8] of a K-tile
  const __bf16* bptr;
  int kb = 0;
  bool b_valid = true;
  auto b_tile_base = [&](int cl, int nn0) {
    return g.bsplit + (((int64_t)cl * NT + nn0 / BN) * KT * 3) * (BN * BK) + (wave * 64 + lane) * 8;
  };
  auto load_b = [&](int sl) {
#pragma unroll
    for (int p = 0; p < 3; ++p) bfr[sl][p] = *reinterpret_cast<const bf16x8*>(bptr + ((sl * 3 + p) * 4 * 64) * 8);
  };
  auto b_step = [&]() {
    if (!b_valid) return;
    bptr += 3 * (BN * BK);
    if (++kb < KT) return;
    kb = 0;
    if (pend) {
      bptr = b_tile_base(cls_p, n0_p);
    } else {
      b_valid = false;
      bptr = b_tile_base(0, 0);
    }
  };

  typedef __attribute__((ext_vector_type(2))) float f32x2;
  auto store_a = [&](auto PC, unsigned char* A3) {  // register stage P -> LDS stage at A3
    constexpr int P = decltype(PC)::value;
#pragma unroll
    for (int h = 0; h < (MI + 1) / 2; ++h) {
      float xa[8];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xa[4 * q + j] = (2 * h + q < MI && ((kvalid[P] >> (2 * h + q)) & 1)) ? ra[P][2 * h + q < MI ? 2 * h + q : 0][j] : 0.f;
      bf16x8 pc[3];
      split3(xa, pc[0], pc[1], pc[2]);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(&pc[p]);
        unsigned char* qa = A3 + p * PIECE + (lrow + 64 * h) * G3_LDB + lk4 * 2;
        *reinterpret_cast<f32x2*>(qa) = f32x2{w.x, w.y};
        if (2 * h + 1 < MI) *reinterpret_cast<f32x2*>(qa + 32 * G3_LDB) = f32x2{w.z, w.w};
      }
    }
  };
  const int afrag = li * G3_LDB + 16 * lh;  // this lane's fragment offset inside an image (mi = 0, slab 0)
  auto read_a1 = [&](const unsigned char* A3, int sl, int mi, bf16x8 (&a)[3]) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
      a[p] = *reinterpret_cast<const bf16x8*>(A3 + p * PIECE + afrag + mi * 32 * G3_LDB + 32 * sl);
  };
  auto read_a = [&](const unsigned char* A3, int sl, bf16x8 (&a)[MI][3]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) read_a1(A3, sl, mi, a[mi]);
  };
  float bv;
  auto fetch_bias = [&](int nn0) {
    const int gc = nn0 + wave * 32 + li;
    bv = (g.bias != nullptr && gc < g.N) ? g.bias[gc] : 0.f;
  };
  fetch_bias(n0_c);

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;

  // ---- prologue: A K-tile 0 in LDS stage 0; K-tiles 1, 2 in flight (register stages 1, 0); B K-tile 0 in flight
  enter_segment(0);
  bptr = b_tile_base(cls0, n0_c);
  load_a(I0{});
  cursor_step();
  load_a(I1{});
  cursor_step();
  load_b(0);
  load_b(1);
  b_step();
  store_a(I0{}, Abuf);
  load_a(I0{});
  cursor_step();
  __syncthreads();

  int kc = 0;
  bool done = false;
  auto iteration = [&](auto SC, auto PC) {  // S = j & 1: LDS stage of K-tile j; P = 1 - S: register stage of K-tile j + 1
    const unsigned char* const Ac = Abuf + decltype(SC)::value * OP;
    unsigned char* const As = Abuf + decltype(PC)::value * OP;
    // multiply K-tile j || split K-tile j + 1 into the other LDS stage || refill each slab's B fragments (K-tile j + 1)
    bf16x8 af[MI][3];
    read_a(Ac, 0, af);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      mfma_3x3(acc[mi], af[mi], bfr[0]);
      read_a1(Ac, 1, mi, af[mi]);
    }
    load_b(0);
    store_a(PC, As);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) mfma_3x3(acc[mi], af[mi], bfr[1]);
    load_b(1);
    b_step();
    load_a(PC);  // A K-tile j + 3 (register stage P was stored just above)
    if (++kc == KT) {  // tile finished
      const int* rt = rid + tpar * TM;
      const int gc = n0_c + wave * 32 + li;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        int rows[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rows[r] = rt[mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
        epilogue_tile<EPI>(acc[mi], rows, gc, g.N, bv, g.relu, g.mask, g.ldmask, g.C, g.ldc);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
      }
      if (!pend) {
        done = true;
        return;
      }
      // take over the tile the A cursor entered three K-tiles ago (other rid stage: its last readers were the epilogue
      // of the tile before this one)
      tpar ^= 1;
      if (tid < TM) rid[tpar * TM + tid] = ridt_p;
      n0_c = n0_p;
      fetch_bias(n0_c);
      pend = false;
      kc = 0;
    }
    cursor_step();
    __syncthreads();
  };
  while (true) {
    iteration(I0{}, I1{});
    if (done) break;
    iteration(I1{}, I0{});
    if (done) break;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Activation-stationary split product for SHORT K, WIDE N (one segment, 96 < K <= 128, N a multiple of 128 and >= 256:
// dA = g . W_eff(d)^T of post-layer 0, K = 128 -> N = 512, per degree class).  k_gemm3 gives every (row tile, column
// tile) pair its own workgroup, so the same 128 x 128 activation tile is loaded and split N / 128 times; with 4 K-tiles
// per tile the split costs as much as the MFMAs.  Here a workgroup owns a 64-row tile: loads + splits it ONCE into LDS
// (three bf16 images, 64 rows x 272 B, 51 KB: three workgroups per CU), then walks the column tiles; wave w multiplies
// all 64 rows by the columns 32 w .. of the column tile, its B fragments coming straight from the fragment-major weight
// image in L2 (k_split_weights, frag = 1) through a two-K-tile register ring that is refilled right after each slab's
// MFMAs and runs on across column-tile boundaries (every load unconditional: past the end the last K-tile is re-read).
// No predicates anywhere in the column loop, so every s_waitcnt of the ring is exact (vmcnt counts loads AND stores in
// order; behind a data-dependent number of stores hipcc waits for all of them):
//   * a partial tile repeats its last valid row (same inputs -> same outputs -> the same value stored to the same
//     address more than once);
//   * N % 128 == 0 and all element offsets below 2^30 are launch conditions (else k_gemm3 runs), so a store is a
//     uniform base + a 32-bit lane offset read from LDS (row * ldc, computed once per tile).
// Same MFMAs, same operands, same order per accumulator as k_gemm3: bit-identical results.
// A grouped call's 128-row class tiles (gnx_class_tiles) are taken as two 64-row halves.
// ---------------------------------------------------------------------------------------------------------------
#define AS_BM 64
#define AS_LDA 272                  // bytes per image row: 128 bf16 + 16 (row stride = 17 x 16 B: conflict-free ds_read_b128)
#define AS_PIECE (AS_BM * AS_LDA)
#define AS_LDS (3 * AS_PIECE + 2 * AS_BM * 4)

#ifdef AS_STAMP  // diagnostic build only (tools/ubench/gemm_as3_stamp.hip): per-workgroup phase cycle sums
__device__ unsigned long long* as_stamp_buf = nullptr;
#define AS_AT(i)                                     \
  do {                                               \
    __builtin_amdgcn_sched_barrier(0);               \
    const unsigned long long tn_ = clock64();        \
    tacc[i] += tn_ - tprev;                          \
    tprev = tn_;                                     \
    __builtin_amdgcn_sched_barrier(0);               \
  } while (0)
#else
#define AS_AT(i)
#endif

template <int EPI>
__global__ void __launch_bounds__(256, 3) k_gemm_as3(gemm_args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_as[];
#ifdef AS_STAMP
  unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0};
  const unsigned long long tstart = clock64();
  unsigned long long tprev = tstart;
#endif
  unsigned char* const A3 = lds_as;
  unsigned* const roff = reinterpret_cast<unsigned*>(lds_as + 3 * AS_PIECE);              // row * ldc
  unsigned* const moff = reinterpret_cast<unsigned*>(lds_as + 3 * AS_PIECE + AS_BM * 4);  // row * ldmask

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int NT = g.Npad / BN;
  const bool grouped = g.tile_info != nullptr;

  int p0, pr, cls = 0;
  if (grouped) {
    const int t = blockIdx.x >> 1, half = blockIdx.x & 1;
    if (t >= g.ntiles[0]) return;
    p0 = g.tile_info[3 * t] + AS_BM * half;
    pr = g.tile_info[3 * t + 1] - AS_BM * half;
    cls = g.tile_info[3 * t + 2];
    if (pr <= 0) return;
    pr = pr < AS_BM ? pr : AS_BM;
  } else {
    const int64_t m0 = (int64_t)blockIdx.x * AS_BM;
    p0 = (int)m0;
    pr = (int)min((int64_t)AS_BM, g.M - m0);
  }

  // ---- A tile: 32 lanes cover one 512-byte row, 8 rows per pass, 8 passes; B ring: K-tile 0 of column tile 0
  const seg_dev& s = g.seg[0];
  const int lr = tid >> 5, k4 = (tid & 31) * 4;
  const bool k_ok = k4 < s.k;
  int grow[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = lr + 8 * q;
    const int idx = p0 + (r < pr ? r : pr - 1);
    grow[q] = grouped ? g.row_index[idx] : idx;
  }
  int my_row = 0;
  if (tid < AS_BM) {
    const int idx = p0 + (tid < pr ? tid : pr - 1);
    my_row = grouped ? g.row_index[idx] : idx;
  }
  f32x4 ra[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) ra[q] = *reinterpret_cast<const f32x4*>(s.a + (int64_t)grow[q] * s.lda + (k_ok ? k4 : 0));

  const int total_kt = NT * 4;
  const __bf16* const bbase = g.bsplit + ((int64_t)cls * NT * 4 * 3) * (BN * BK) + (wave * 64 + lane) * 8;
  bf16x8 bq[2][2][3];  // [K-tile parity][slab][piece]
  auto load_b = [&](int slot, int sl, int j) {
    const __bf16* p = bbase + (int64_t)(j < total_kt ? j : total_kt - 1) * (3 * BN * BK);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) bq[slot][sl][pc] = *reinterpret_cast<const bf16x8*>(p + ((sl * 3 + pc) * 4 * 64) * 8);
  };
  load_b(0, 0, 0);
  load_b(0, 1, 0);
  AS_AT(0);  // tile info, row ids, issue of the A loads

  typedef __attribute__((ext_vector_type(2))) float f32x2;
  if (tid < AS_BM) {
    roff[tid] = (unsigned)my_row * (unsigned)g.ldc;
    moff[tid] = (unsigned)my_row * (unsigned)g.ldmask;
  }
#pragma unroll
  for (int q = 0; q < 8; q += 2) {
    float xa[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xa[j] = k_ok ? ra[q][j] : 0.f;
      xa[4 + j] = k_ok ? ra[q + 1][j] : 0.f;
    }
    bf16x8 pc[3];
    split3(xa, pc[0], pc[1], pc[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(&pc[p]);
      unsigned char* qa = A3 + p * AS_PIECE + (lr + 8 * q) * AS_LDA + k4 * 2;
      *reinterpret_cast<f32x2*>(qa) = f32x2{w.x, w.y};
      *reinterpret_cast<f32x2*>(qa + 8 * AS_LDA) = f32x2{w.z, w.w};
    }
  }
  load_b(1, 0, 1);  // (after the split: held across it, the second K-tile's 24 registers spill)
  load_b(1, 1, 1);
  AS_AT(1);  // wait for A, split, LDS stores
  __syncthreads();
  AS_AT(2);

  // A fragments come from LDS for every slab (one slab ahead of its MFMAs).  The offset is made opaque per column tile:
  // the tile is loop-invariant, and hoisting its 48 fragments (192 VGPRs) out of the column loop spills.  (The OFFSET,
  // not the pointer: an opaque pointer loses its LDS address space and turns the reads into flat loads.)
  int afrag = li * AS_LDA + 16 * lh;
  bf16x8 af[2][2][3];  // [slab parity][mi][piece]
  auto read_a = [&](int slot, int off, int ks) {  // ks = 16-deep slab 0..7 of the K = 128 tile
    const unsigned char* base = A3 + off;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        af[slot][mi][p] = *reinterpret_cast<const bf16x8*>(base + p * AS_PIECE + mi * 32 * AS_LDA + ks * 32);
  };
  read_a(0, afrag, 0);

  // Epilogue geometry.  The MFMA result has lane = column, 4 consecutive ROWS per register group; a 4 x 4 transpose
  // inside every quad of lanes (two DPP exchange stages) turns that into lane = (row 8g + 4 lh + j, columns 4c .. 4c+3)
  // with j = li & 3, c = li >> 2: one 16-byte store per group, 8 lanes per 128-byte line, 8 full lines per wave
  // instruction (the 4-byte stores of the untransposed layout reached 2.2 TB/s: the epilogue took as long as the MFMAs).
  const int qj = li & 3;
  const unsigned lc = (unsigned)(wave * 32 + (li >> 2) * 4);
  unsigned ro[2][4], mo[2][4];  // row * ldc (row * ldmask) of this lane's 8 stores per column tile
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      ro[mi][gq] = roff[mi * 32 + 8 * gq + 4 * lh + qj] + lc;
      mo[mi][gq] = moff[mi * 32 + 8 * gq + 4 * lh + qj] + lc;
    }
  // bias of the NEXT column tile is fetched a tile ahead (unconditional, from a zero vector when there is none)
  const float* const bias_p = g.bias != nullptr ? g.bias : c_zero4;
  const int bias_on = g.bias != nullptr ? 1 : 0;
  auto bias_at = [&](int nt_) { return *reinterpret_cast<const f32x4*>(bias_p + (bias_on ? nt_ * BN + (int)lc : 0)); };
  f32x4 bv = bias_at(0);
  const float floor_v = g.relu ? 0.f : -__builtin_inff();
  asm volatile("" ::"v"(bv));  // waited for HERE: pending at the loop entry it would cost a vmcnt(0) in every iteration
  // exchange within lane pairs (xor 1) / across pairs (xor 2) of a quad: x and y swap their off-diagonal elements
  auto quad_swap = [&](float& x, float& y, auto CTRL, bool hi) {
    const float send = hi ? x : y;
    const float got = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), decltype(CTRL)::value, 0xf, 0xf, true));
    x = hi ? got : x;
    y = hi ? y : got;
  };
  using XOR1 = std::integral_constant<int, 0xB1>;  // quad_perm [1,0,3,2]
  using XOR2 = std::integral_constant<int, 0x4E>;  // quad_perm [2,3,0,1]

  for (int nt = 0; nt < NT; ++nt) {
    asm volatile("" : "+v"(afrag));
    f32x16 acc[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
    const f32x4 bv_next = bias_at(nt + 1 < NT ? nt + 1 : nt);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int kt = ks >> 1, sl = ks & 1;
      read_a((ks + 1) & 1, afrag, (ks + 1) & 7);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) mfma_3x3(acc[mi], af[ks & 1][mi], bq[kt & 1][sl]);
      load_b(kt & 1, sl, nt * 4 + kt + 2);
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("" ::"v"(bv_next));  // touched here, where the number of younger loads is static
    AS_AT(3);  // fragment reads + MFMAs of a column tile
    float* const cbase = g.C + nt * BN;
    const float* const mbase = (EPI == EPI_MASK ? g.mask : g.C) + nt * BN;
    // every load of the accumulate / mask operand precedes every store: a repeated row (partial tile) must read the
    // ORIGINAL C in all its copies (same wave, same address, program order), or it would be accumulated more than once
    f32x4 extra[2][4];
    if constexpr (EPI != EPI_PLAIN) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          extra[mi][gq] = *reinterpret_cast<const f32x4*>(mbase + (EPI == EPI_MASK ? mo[mi][gq] : ro[mi][gq]));
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        float c0 = acc[mi][4 * gq], c1 = acc[mi][4 * gq + 1], c2 = acc[mi][4 * gq + 2], c3 = acc[mi][4 * gq + 3];
        quad_swap(c0, c1, XOR1{}, (qj & 1) != 0);
        quad_swap(c2, c3, XOR1{}, (qj & 1) != 0);
        quad_swap(c0, c2, XOR2{}, (qj & 2) != 0);
        quad_swap(c1, c3, XOR2{}, (qj & 2) != 0);
        f32x4 v = {c0 + bv.x, c1 + bv.y, c2 + bv.z, c3 + bv.w};
        if constexpr (EPI == EPI_ACCUM) v += extra[mi][gq];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], floor_v);
        if constexpr (EPI == EPI_MASK)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (extra[mi][gq][e] > 0.f) ? v[e] : 0.f;
        *reinterpret_cast<f32x4*>(cbase + ro[mi][gq]) = v;
      }
    bv = bv_next;
    AS_AT(4);  // epilogue
  }
#ifdef AS_STAMP
  if (tid == 0 && as_stamp_buf != nullptr) {
    for (int i = 0; i < 5; ++i) as_stamp_buf[(size_t)blockIdx.x * 8 + i] = tacc[i];
    as_stamp_buf[(size_t)blockIdx.x * 8 + 5] = tstart;
    as_stamp_buf[(size_t)blockIdx.x * 8 + 6] = clock64();
  }
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// dA product + PNA scatter-aggregate backward of one tower in ONE launch: dA = g Weff(d) ([N, 4F], the layer backward's
// largest intermediate) is consumed by exactly one kernel, k_pna_agg_bwd_rc, which reads it straight back.  Here the
// k_gemm_as3 product runs on a 32-ROW tile (one 32 x 32 accumulator per wave and column tile instead of two), the
// quad-transposed result of each of the FOUR column tiles -- column tile nt = aggregator nt (mean | min | max | std) of
// the tower's F = 128 channels -- stays in registers (64 per lane), and after the last column tile a lane holds, for each
// of its four (row 8 gq + 4 lh + j, channels 32 wave + 4 (li >> 2) .. +3) items, exactly the four inputs one thread of
// k_pna_agg_bwd_rc<4> loads from dA: it runs pna_agg_bwd_item on them and writes ge.  dA is never written.
// Same MFMAs, same operands, same order per accumulator, the same bias / floor operations behind them as k_gemm_as3, the
// same item arithmetic as k_pna_agg_bwd_rc: bit-identical to the pair.  The row's degree is read from rowptr.
// Price: the weight image streams from L2 once per 32 rows instead of once per 64; two workgroups per CU (<= 256
// registers per lane) so that one's aggregate phase (loads and stores) runs beside the other's matrix phase.
// Grouped calls only; a table's 96- or 128-row class tile is taken as up to four 32-row parts.
// ---------------------------------------------------------------------------------------------------------------
#define DAF_BM 32
#define DAF_PIECE (DAF_BM * AS_LDA)
#define DAF_LDS (3 * DAF_PIECE + DAF_BM * 4)

struct daf_args {
  const float* m;     // messages fp32[E, H] in CSR order, already offset to the tower's first channel
  const int* rowptr;  // int32[N + 1]
  float* ge;          // message gradient fp32[E, H], offset like m
  int H;              // row stride of m and ge
  int centered;       // GNX_OPT_STD_BWD_CENTERED
};

__global__ void __launch_bounds__(256, 2) k_pna_dA_agg_bwd(gemm_args g, daf_args x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_daf[];
  unsigned char* const A3 = lds_daf;
  int* const rown = reinterpret_cast<int*>(lds_daf + 3 * DAF_PIECE);  // node of every tile row (a partial tile repeats its last)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  constexpr int NT = 4;

  const int t = blockIdx.x >> 2, part = blockIdx.x & 3;
  if (t >= g.ntiles[0]) return;
  const int p0 = g.tile_info[3 * t] + DAF_BM * part;
  int pr = g.tile_info[3 * t + 1] - DAF_BM * part;
  const int cls = g.tile_info[3 * t + 2];
  if (pr <= 0) return;
  pr = pr < DAF_BM ? pr : DAF_BM;

  // ---- A tile: 32 lanes cover one 512-byte row, 8 rows per pass, 4 passes; B ring: K-tile 0 of column tile 0
  const seg_dev& s = g.seg[0];
  const int lr = tid >> 5, k4 = (tid & 31) * 4;
  f32x4 ra[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = lr + 8 * q;
    const int row = g.row_index[p0 + (r < pr ? r : pr - 1)];
    ra[q] = *reinterpret_cast<const f32x4*>(s.a + (int64_t)row * s.lda + k4);
  }
  if (tid < DAF_BM) rown[tid] = g.row_index[p0 + (tid < pr ? tid : pr - 1)];

  constexpr int total_kt = NT * 4;
  const __bf16* const bbase = g.bsplit + ((int64_t)cls * NT * 4 * 3) * (BN * BK) + (wave * 64 + lane) * 8;
  bf16x8 bq[2][2][3];  // [K-tile parity][slab][piece]
  auto load_b = [&](int slot, int sl, int j) {
    const __bf16* p = bbase + (int64_t)(j < total_kt ? j : total_kt - 1) * (3 * BN * BK);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) bq[slot][sl][pc] = *reinterpret_cast<const bf16x8*>(p + ((sl * 3 + pc) * 4 * 64) * 8);
  };
  load_b(0, 0, 0);
  load_b(0, 1, 0);

  typedef __attribute__((ext_vector_type(2))) float f32x2;
#pragma unroll
  for (int q = 0; q < 4; q += 2) {
    float xa[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xa[j] = ra[q][j];
      xa[4 + j] = ra[q + 1][j];
    }
    bf16x8 pc[3];
    split3(xa, pc[0], pc[1], pc[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(&pc[p]);
      unsigned char* qa = A3 + p * DAF_PIECE + (lr + 8 * q) * AS_LDA + k4 * 2;
      *reinterpret_cast<f32x2*>(qa) = f32x2{w.x, w.y};
      *reinterpret_cast<f32x2*>(qa + 8 * AS_LDA) = f32x2{w.z, w.w};
    }
  }
  load_b(1, 0, 1);
  load_b(1, 1, 1);
  __syncthreads();

  // this lane's four items: tile row 8 gq + 4 lh + (li & 3), channels lc .. lc + 3; their message runs, fetched now so
  // that the aggregate phase starts with its addresses known (rows past the tile's end: an empty run)
  const int qj = li & 3;
  const int lc = wave * 32 + (li >> 2) * 4;
  int e0[4], e1[4];
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const int r = 8 * gq + 4 * lh + qj;
    const int node = rown[r];
    e0[gq] = x.rowptr[node];
    e1[gq] = r < pr ? x.rowptr[node + 1] : e0[gq];
  }
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) asm volatile("" ::"v"(e0[gq]), "v"(e1[gq]));  // waited for HERE, not inside the ring

  int afrag = li * AS_LDA + 16 * lh;
  bf16x8 af[2][3];  // [slab parity][piece]
  auto read_a = [&](int slot, int off, int ks) {  // ks = 16-deep slab 0..7 of the K = 128 tile
    const unsigned char* base = A3 + off;
#pragma unroll
    for (int p = 0; p < 3; ++p) af[slot][p] = *reinterpret_cast<const bf16x8*>(base + p * DAF_PIECE + ks * 32);
  };
  read_a(0, afrag, 0);

  const f32x4 bv = *reinterpret_cast<const f32x4*>(c_zero4);  // (k_gemm_as3's bias add and floor: -0 + 0 = +0 like there)
  const float floor_v = g.relu ? 0.f : -__builtin_inff();
  asm volatile("" ::"v"(bv));
  auto quad_swap = [&](float& a, float& b, auto CTRL, bool hi) {
    const float send = hi ? a : b;
    const float got = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), decltype(CTRL)::value, 0xf, 0xf, true));
    a = hi ? got : a;
    b = hi ? b : got;
  };
  using XOR1 = std::integral_constant<int, 0xB1>;  // quad_perm [1,0,3,2]
  using XOR2 = std::integral_constant<int, 0x4E>;  // quad_perm [2,3,0,1]

  // the messages of the four items, register form (1 <= degree <= 4; a node without messages reads row 0, a longer run its
  // first four rows: never used).  Offsets fit 32 bits (launch condition).
  const float* const mc = x.m + lc;
  float am[4][4][4];  // [item][message][channel]
  auto load_messages = [&]() {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int deg = e1[gq] - e0[gq];
#pragma unroll
      for (int e = 0; e < 4; ++e) vload<4>(am[gq][e], mc + (deg > 0 ? (e0[gq] + (e < deg ? e : 0)) * x.H : 0));
    }
  };

  f32x4 kept[NT][4];  // [aggregator][item]: the transposed dA tile
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    asm volatile("" : "+v"(afrag));
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int kt = ks >> 1, sl = ks & 1;
      read_a((ks + 1) & 1, afrag, (ks + 1) & 7);
      __builtin_amdgcn_sched_barrier(0);
      mfma_3x3(acc, af[ks & 1], bq[kt & 1][sl]);
      load_b(kt & 1, sl, nt * 4 + kt + 2);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float c0 = acc[4 * gq], c1 = acc[4 * gq + 1], c2 = acc[4 * gq + 2], c3 = acc[4 * gq + 3];
      quad_swap(c0, c1, XOR1{}, (qj & 1) != 0);
      quad_swap(c2, c3, XOR1{}, (qj & 1) != 0);
      quad_swap(c0, c2, XOR2{}, (qj & 2) != 0);
      quad_swap(c1, c3, XOR2{}, (qj & 2) != 0);
      f32x4 v = {c0 + bv.x, c1 + bv.y, c2 + bv.z, c3 + bv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], floor_v);
      kept[nt][gq] = v;
    }
  }

  // ---- aggregate backward on the kept tile: the messages of all four items are fetched at once (16 loads of 16 bytes in
  // flight per lane; the ring's and the accumulators' registers are free by now).  (measured: one item at a time 116.4 us per
  // launch at the cfg-2 layer shape, all four here 113.7, all four in front of the last column tile's MFMAs 114.6 at 250
  // VGPRs, in front of the third tile 3 VGPRs spilled; the two launches 147.2)
  load_messages();
  float* const gec = x.ge + lc;
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const int deg = e1[gq] - e0[gq];
    if (deg <= 0) continue;
    float gmean[4], gmn[4], gmx[4], gsd[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gmean[e] = kept[0][gq][e];
      gmn[e] = kept[1][gq][e];
      gmx[e] = kept[2][gq][e];
      gsd[e] = kept[3][gq][e];
    }
    if (deg <= 4)
      pna_agg_bwd_item_loaded<4>(gmean, gmn, gmx, gsd, deg, am[gq], gec + (int64_t)e0[gq] * x.H, x.H, x.centered);
    else
      pna_agg_bwd_item_loop<4>(gmean, gmn, gmx, gsd, e0[gq], e1[gq], mc, gec, x.H, x.centered);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Mid-size product (M < 4096 rows and few 128 x 128 tiles: a 32-graph batch's 640 atoms / 1 280 bonds): the whole gnx_gemm
// contract (segments, row scale, degree-class grouping, every epilogue) on 16 x 16 output patches, one output per thread,
// the k-ordered fp32 fmaf chain of k_gemm_small_batched.  The tiled kernel gives such a problem 5-10 workgroups that walk K
// serially, two barriers per 32 k: 40 us per launch, 78 launches = 3.3 of the 4.4 ms of a cfg-1 (B = 32) step; here
// M / 16 x N / 16 workgroups stage 128 k per barrier pair with 16-byte loads and read LDS 16 bytes at a time.
// ---------------------------------------------------------------------------------------------------------------
#define MID_T 16
#define MID_KC 128
#define MID_LD (MID_KC + 4)

template <bool B_TRANS, int EPI>
__global__ void __launch_bounds__(256) k_gemm_mid(gemm_args g) {
  __shared__ __attribute__((aligned(16))) float As[MID_T][MID_LD];
  __shared__ __attribute__((aligned(16))) float Bs[MID_T][MID_LD];  // Bs[n][k]
  __shared__ int rid[MID_T];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int n0 = blockIdx.y * MID_T;
  int cls = 0;
  if (g.tile_info != nullptr) {  // a 128-row class tile = eight 16-row patches
    const int t = blockIdx.x >> 3, sub = blockIdx.x & 7;
    if (t >= g.ntiles[0]) return;
    const int p0 = g.tile_info[3 * t] + MID_T * sub, pr = g.tile_info[3 * t + 1] - MID_T * sub;
    cls = g.tile_info[3 * t + 2];
    if (pr <= 0) return;
    if (tid < MID_T) rid[tid] = tid < pr ? g.row_index[p0 + tid] : -1;
  } else {
    const int64_t m0 = (int64_t)blockIdx.x * MID_T;
    if (tid < MID_T) rid[tid] = (m0 + tid < g.M) ? (int)(m0 + tid) : -1;
  }
  __syncthreads();

  // chunk = 128 k of one segment; the NEXT chunk's granules are fetched into registers while this one is multiplied
  f32x4 ra[2], rb[2];
  auto fetch = [&](int si, int k0) {
    const seg_dev& s = g.seg[si];
    const float* __restrict__ sb = s.b + (int64_t)cls * s.cls_stride;
    const bool va = s.vec_a && (s.k % 4 == 0), vb = s.vec_b && (B_TRANS ? (s.k % 4 == 0) : (g.N % 4 == 0));
    const int kc = (s.k - k0) < MID_KC ? (s.k - k0) : MID_KC;
    // A[rows][k0 .. k0+kc): 512 four-float granules, two per thread, consecutive threads along k
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gi = tid + 256 * j, r = gi >> 5, k4 = (gi & 31) * 4;
      const int row = rid[r];
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row >= 0 && k4 < kc) {
        const float* ap = s.a + (int64_t)row * s.lda + k0 + k4;
        if (va) {
          v = *reinterpret_cast<const f32x4*>(ap);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (k4 + e < kc) ? ap[e] : 0.f;
        }
        if (s.rs != nullptr) {
          const float rs = s.rs[row];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rs * v[e];
        }
      }
      ra[j] = v;
    }
    if (B_TRANS) {  // B[n][k]: the same shape as A
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int gi = tid + 256 * j, r = gi >> 5, k4 = (gi & 31) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n0 + r < g.N && k4 < kc) {
          const float* bp = sb + (int64_t)(n0 + r) * s.ldb + k0 + k4;
          if (vb) {
            v = *reinterpret_cast<const f32x4*>(bp);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (k4 + e < kc) ? bp[e] : 0.f;
          }
        }
        rb[j] = v;
      }
    } else {  // B[k][n]: four granules per k row, transposed into Bs[n][k] at store time
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int gi = tid + 256 * j, k = gi >> 2, c4 = (gi & 3) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < kc && n0 + c4 < g.N) {
          const float* bp = sb + (int64_t)(k0 + k) * s.ldb + n0 + c4;
          if (vb) {
            v = *reinterpret_cast<const f32x4*>(bp);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (n0 + c4 + e < g.N) ? bp[e] : 0.f;
          }
        }
        rb[j] = v;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gi = tid + 256 * j;
      *reinterpret_cast<f32x4*>(&As[gi >> 5][(gi & 31) * 4]) = ra[j];
      if (B_TRANS) {
        *reinterpret_cast<f32x4*>(&Bs[gi >> 5][(gi & 31) * 4]) = rb[j];
      } else {
        const int k = gi >> 2, c4 = (gi & 3) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[c4 + e][k] = rb[j][e];
      }
    }
  };

  float acc = 0.f;
  int si = 0, k0 = 0;
  fetch(0, 0);
  while (true) {
    stage();
    __syncthreads();
    const int kc = (g.seg[si].k - k0) < MID_KC ? (g.seg[si].k - k0) : MID_KC;
    int sn = si, kn = k0 + MID_KC;
    if (kn >= g.seg[si].k) {
      ++sn;
      kn = 0;
    }
    const bool more = sn < g.nseg;
    if (more) fetch(sn, kn);
    const int kend = (kc + 3) & ~3;
    for (int k = 0; k < kend; k += 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&As[ty][k]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[tx][k]);
      acc = fmaf(a.x, b.x, acc);
      acc = fmaf(a.y, b.y, acc);
      acc = fmaf(a.z, b.z, acc);
      acc = fmaf(a.w, b.w, acc);
    }
    if (!more) break;
    __syncthreads();
    si = sn;
    k0 = kn;
  }
  const int gm = rid[ty], gn = n0 + tx;
  if (gm >= 0 && gn < g.N) {
    float v = acc + (g.bias != nullptr ? g.bias[gn] : 0.f);
    float* cp = g.C + (int64_t)gm * g.ldc + gn;
    if constexpr (EPI == EPI_ACCUM) v += *cp;
    v = g.relu ? fmaxf(v, 0.f) : v;
    if constexpr (EPI == EPI_MASK) v = (g.mask[(int64_t)gm * g.ldmask + gn] > 0.f) ? v : 0.f;
    *cp = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Small products (M <= 256: the 60-row bond-table chain  BondEmb -> edge_encoder -> pre-layer-0 slice and its
// gradients).  The tiled kernel spends ~22 us of pure load/barrier latency on such a problem in ONE workgroup; here a
// 16 x 16 output patch per 256-thread workgroup stages its A rows and B rows/columns in LDS once and every thread does
// one K-long dot product (the k-ordered fmaf chain of the fp32 MFMA): ~M/16 * N/16 workgroups in parallel, a few
// microseconds.  One segment, no row scale / mask.
// Up to GNX_SMALL_BATCH independent problems in ONE launch (the bond-table chain, the merged lin o last-post weights
// and their gradients for ALL layers of a model; VERDICT r2 #4: ~360 launches per step, 54 of them 16 x 16-patch
// products of ~8 us each); gnx_gemm's own small path (GNX_OPT_GEMM_MID = 0) is a batch of one.  blockIdx.y = problem,
// blockIdx.x = output patch.  Either operand may be read transposed (the weight gradients of these tiny layers are
// A^T B products), the result may be accumulated plainly (problems of one launch must then write disjoint outputs) or
// with fp32 atomics.
// ---------------------------------------------------------------------------------------------------------------
#define SM_T 16
#define SM_KC 128  // K chunk staged per pass

struct small_batch_args {
  gnx_small_prob p[GNX_SMALL_BATCH];
  int n;
};

__global__ void __launch_bounds__(256) k_gemm_small_batched(small_batch_args b) {
  __shared__ float As[SM_T][SM_KC + 1];
  __shared__ float Bs[SM_T][SM_KC + 1];
  const gnx_small_prob& q = b.p[blockIdx.y];
  const int M = q.M, N = q.N, K = q.K;
  const int nt = (N + SM_T - 1) / SM_T, mt = (M + SM_T - 1) / SM_T;
  if ((int)blockIdx.x >= nt * mt) return;  // (uniform per workgroup: before any barrier)
  const int m0 = (blockIdx.x / nt) * SM_T, n0 = (blockIdx.x % nt) * SM_T;
  const bool at = (q.flags & GNX_SB_A_TRANS) != 0, bt = (q.flags & GNX_SB_B_TRANS) != 0;
  const float* __restrict__ A = q.A;
  const float* __restrict__ B = q.B;
  const int64_t lda = q.lda, ldb = q.ldb;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc = 0.f;
  for (int k0 = 0; k0 < K; k0 += SM_KC) {
    const int kc = (K - k0) < SM_KC ? (K - k0) : SM_KC;
    if (!at) {  // A[m][k]: consecutive threads along k
      for (int i = threadIdx.x; i < SM_T * SM_KC; i += 256) {
        const int r = i / SM_KC, k = i % SM_KC;
        As[r][k] = (m0 + r < M && k < kc) ? A[(int64_t)(m0 + r) * lda + k0 + k] : 0.f;
      }
    } else {  // A[k][m]: consecutive threads along m
      for (int i = threadIdx.x; i < SM_T * SM_KC; i += 256) {
        const int k = i / SM_T, r = i % SM_T;
        As[r][k] = (m0 + r < M && k < kc) ? A[(int64_t)(k0 + k) * lda + m0 + r] : 0.f;
      }
    }
    if (bt) {  // B[n][k]
      for (int i = threadIdx.x; i < SM_T * SM_KC; i += 256) {
        const int r = i / SM_KC, k = i % SM_KC;
        Bs[r][k] = (n0 + r < N && k < kc) ? B[(int64_t)(n0 + r) * ldb + k0 + k] : 0.f;
      }
    } else {  // B[k][n]
      for (int i = threadIdx.x; i < SM_T * SM_KC; i += 256) {
        const int k = i / SM_T, r = i % SM_T;
        Bs[r][k] = (n0 + r < N && k < kc) ? B[(int64_t)(k0 + k) * ldb + n0 + r] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < SM_KC; ++k) acc = fmaf(As[ty][k], Bs[tx][k], acc);
    __syncthreads();
  }
  const int gm = m0 + ty, gn = n0 + tx;
  if (gm < M && gn < N) {
    float v = acc + (q.bias != nullptr ? q.bias[gn] : 0.f);
    float* cp = q.C + (int64_t)gm * q.ldc + gn;
    if (q.flags & GNX_SB_ATOMIC) {
      atomicAdd(cp, v);
    } else {
      if (q.flags & GNX_SB_ACCUMULATE) v += *cp;
      *cp = (q.flags & GNX_SB_RELU) ? fmaxf(v, 0.f) : v;
    }
  }
}

extern "C" int32_t gnx_gemm_small_batched(gnx_handle* h, int32_t nprob, const gnx_small_prob* probs) {
  GNX_CHECK_ARG(h && nprob >= 0 && (probs || nprob == 0), "gnx_gemm_small_batched: bad argument");
  for (int32_t i0 = 0; i0 < nprob; i0 += GNX_SMALL_BATCH) {
    small_batch_args b;
    b.n = nprob - i0 < GNX_SMALL_BATCH ? nprob - i0 : GNX_SMALL_BATCH;
    int maxt = 0;
    double bytes = 0.0, flops = 0.0;
    for (int i = 0; i < b.n; ++i) {
      const gnx_small_prob& q = probs[i0 + i];
      GNX_CHECK_ARG(q.A && q.B && q.C && q.M > 0 && q.N > 0 && q.K > 0, "gnx_gemm_small_batched: problem %d is empty or NULL",
                    i0 + i);
      GNX_CHECK_ARG(!((q.flags & GNX_SB_ATOMIC) && (q.flags & GNX_SB_RELU)), "gnx_gemm_small_batched: atomic + relu");
      b.p[i] = q;
      const int t = (int)(gnx_cdiv(q.M, SM_T) * gnx_cdiv(q.N, SM_T));
      maxt = t > maxt ? t : maxt;
      bytes += 4.0 * ((double)q.M * (q.K + q.N) + (double)q.N * q.K);
      flops += 2.0 * q.M * q.N * q.K;
    }
    for (int i = b.n; i < GNX_SMALL_BATCH; ++i) b.p[i] = b.p[0];
    gnx_prof_scope prof(h, GNX_K_GEMM_SMALL, bytes, flops, 0.0);
    hipLaunchKernelGGL(k_gemm_small_batched, dim3((unsigned)maxt, (unsigned)b.n), dim3(256), 0, h->stream, b);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

// Host side of gnx_gemm / gnx_gemm_grouped / gnx_gemm_grouped_rows: check the arguments, ask gnx_gemm_plan.hpp which kernel
// the call takes, launch from the plan.  The plan's copies of the kernels' geometry:
static_assert(PLAN_MAX_SEGS == MAX_SEGS && PLAN_BM == BM && PLAN_BN == BN && PLAN_BK == BK, "plan / tiled kernel geometry");
static_assert(PLAN_EPI_PLAIN == EPI_PLAIN && PLAN_EPI_ACCUM == EPI_ACCUM && PLAN_EPI_MASK == EPI_MASK, "plan / epilogue kinds");
static_assert(PLAN_WS_BM == WS_BM && PLAN_WS_LDS == sizeof(float) * (128 * WS_LD + 2 * WS_BM * WS_LD), "plan / k_gemm_ws");
static_assert(PLAN_WS_BM == W3_BM && PLAN_WS3_LDS8 == 2 * W3_BUF, "plan / k_gemm_ws3");
static_assert(PLAN_G3P_MIN_KTILES == G3P_MIN_KTILES && plan_g3p_lds(3) == G3P_LDS(3) && plan_g3p_lds(4) == G3P_LDS(4), "plan / k_gemm3p");
static_assert(PLAN_AS_BM == AS_BM && PLAN_AS_LDS == AS_LDS, "plan / k_gemm_as3");
static_assert(PLAN_PATCH == MID_T && PLAN_PATCH == SM_T, "plan / k_gemm_mid, k_gemm_small_batched");

static int32_t gemm_check(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, int64_t M, int32_t N, const float* mask,
                          int64_t ldmask, const float* C, int64_t ldc, int32_t flags, int32_t tile_rows) {
  GNX_CHECK_ARG(h && segs && C, "gnx_gemm: NULL argument");
  GNX_CHECK_ARG(tile_rows == 0 || tile_rows == 96 || tile_rows == 128, "gnx_gemm: tile_rows=%d not in {0, 96, 128}", tile_rows);
  GNX_CHECK_ARG(nseg >= 1 && nseg <= MAX_SEGS, "gnx_gemm: nseg=%d not in [1,%d]", nseg, MAX_SEGS);
  GNX_CHECK_ARG(M >= 0 && N > 0 && ldc >= N, "gnx_gemm: bad shape M=%lld N=%d ldc=%lld", (long long)M, N, (long long)ldc);
  GNX_CHECK_ARG(!((flags & GNX_GEMM_RELU) && (flags & GNX_GEMM_ACCUMULATE)), "gnx_gemm: relu+accumulate rejected");
  GNX_CHECK_ARG(!(mask && (flags & GNX_GEMM_ACCUMULATE)), "gnx_gemm: mask+accumulate rejected");
  GNX_CHECK_ARG(mask == nullptr || ldmask >= N, "gnx_gemm: ldmask < N");
  if (M == 0) return GNX_OK;
  const bool bt = (flags & GNX_GEMM_B_TRANS) != 0;
  for (int s = 0; s < nseg; ++s) {
    const gnx_gemm_seg& in = segs[s];
    GNX_CHECK_ARG(in.a && in.b && in.k > 0, "gnx_gemm: segment %d: NULL operand or k<=0", s);
    GNX_CHECK_ARG(in.lda >= in.k, "gnx_gemm: segment %d: lda < k", s);
    GNX_CHECK_ARG(bt ? in.ldb >= in.k : in.ldb >= N, "gnx_gemm: segment %d: ldb too small", s);
  }
  return GNX_OK;
}

static int32_t gemm_launch(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                           int32_t num_classes, int64_t M, int32_t N, const float* bias, const float* mask, int64_t ldmask, float* C,
                           int64_t ldc, int32_t flags, const int32_t* row_index, const int32_t* tile_info,
                           const int32_t* ntiles, int64_t max_tiles, void* ws, size_t ws_bytes, int32_t tile_rows = 0) {
  const int32_t st = gemm_check(h, nseg, segs, M, N, mask, ldmask, C, ldc, flags, tile_rows);
  if (st != GNX_OK) return st;
  const gemm_plan p = gemm_plan_of(nseg, segs, cls_strides, num_classes, M, N, bias, mask, ldmask, C, ldc, flags, tile_info,
                                   max_tiles, ws, tile_rows, h->opt, h->num_cus);
  if (p.images && ws_bytes < p.image_bytes) {
    gnx_set_error("gnx_gemm: workspace of %zu bytes, the split weight images need %zu", ws_bytes, p.image_bytes);
    return GNX_E_WORKSPACE;
  }
  GNX_CHECK_ARG(!p.images || aligned16(ws), "gnx_gemm: workspace must be 16-byte aligned");
  if (p.kernel == GNX_GEMM_KERNEL_NONE && p.prof_id == GNX_K_NONE) return GNX_OK;

  const int relu = (flags & GNX_GEMM_RELU) ? 1 : 0;
  __bf16* const images = reinterpret_cast<__bf16*>(ws);
  gemm_args g = {{},      nseg, M, N, bias, mask, ldmask, C, ldc, relu, row_index, tile_info, ntiles, p.ny, images, p.Npad,
                 p.Kpad, {},   p.Kpad / BK};  // the tiled kernels and k_gemm_mid
  split_args sa = {{}, {}, nseg, N, p.Npad, p.Kpad, p.classes, p.frag, images};
  for (int s = 0; s < MAX_SEGS; ++s) {
    seg_dev d = {nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0};
    if (s < nseg) {
      const gnx_gemm_seg& in = segs[s];
      const int64_t cs = cls_strides ? cls_strides[s] : 0;
      d = seg_dev{in.a, in.rowscale, in.b, in.lda, in.ldb, cs, in.k, plan_vec_a(in), plan_vec_b(in, cs)};
    }
    g.seg[s] = sa.seg[s] = d;
    g.koff[s] = p.koff[s];
  }
  for (int s = 0; s <= MAX_SEGS; ++s) sa.koff[s] = p.koff[s];
  const gnx_gemm_seg& s0 = segs[0];  // the one segment of the weights-stationary kernels and of k_gemm_small_batched
  const ws_args w = {s0.a, s0.lda, s0.b, s0.ldb, M, N, s0.k, bias, mask, ldmask, C, ldc, relu, p.row_tiles};

  gnx_prof_scope prof(h, p.prof_id, p.bytes, p.flops, p.mfma);
  if (p.run_split) {
    const dim3 gs((unsigned)gnx_cdiv((int64_t)sa.D * sa.Npad * (sa.Kpad / 8), 256));
    if (p.bt)
      hipLaunchKernelGGL(k_split_weights<true>, gs, dim3(256), 0, h->stream, sa);
    else
      hipLaunchKernelGGL(k_split_weights<false>, gs, dim3(256), 0, h->stream, sa);
    ++h->split_launches;
  }
  if (p.stop_after_split || p.kernel == GNX_GEMM_KERNEL_NONE) {
    GNX_LAUNCH_CHECK();
    return GNX_OK;
  }
  const dim3 grid(p.grid_x, p.grid_y), block(p.block);
  // one launch per kernel kind, instantiated where COND holds; LDS_LIMIT > 0: raised on the kernel's first launch
#define GEMM_CASE(KIND, COND, KERNEL, ARGS, LDS_LIMIT)                                               \
  case KIND:                                                                                         \
    if constexpr (COND) {                                                                            \
      if constexpr ((LDS_LIMIT) > 0)                                                                 \
        if (const hipError_t e = gnx_raise_lds_limit<&KERNEL>(LDS_LIMIT); e != hipSuccess) return e; \
      hipLaunchKernelGGL((KERNEL), grid, block, p.lds, h->stream, ARGS);                             \
    }                                                                                                \
    return hipSuccess
  const hipError_t lds_limit = epi_dispatch(p.bt, p.epi, [&](auto BT, auto EPI) -> hipError_t {
    constexpr bool no_rmw = EPI != EPI_ACCUM;  // the predicate-free forms have no accumulate epilogue (the plan never asks)
    switch (p.kernel) {
      GEMM_CASE(GNX_GEMM_KERNEL_WS, true, (k_gemm_ws<BT, EPI>), w, 160 * 1024);
      GEMM_CASE(GNX_GEMM_KERNEL_WS3, true, (k_gemm_ws3<BT, EPI, false, 8>), w, 160 * 1024);
      GEMM_CASE(GNX_GEMM_KERNEL_WS3_FAST8, no_rmw, (k_gemm_ws3<BT, EPI, true, 8>), w, 160 * 1024);
      GEMM_CASE(GNX_GEMM_KERNEL_WS3_FAST4, no_rmw, (k_gemm_ws3<BT, EPI, true, 4>), w, 64 * 1024);
      GEMM_CASE(GNX_GEMM_KERNEL_MID, true, (k_gemm_mid<BT, EPI>), g, 0);
      GEMM_CASE(GNX_GEMM_KERNEL_AS3, true, (k_gemm_as3<EPI>), g, (int)AS_LDS);
      GEMM_CASE(GNX_GEMM_KERNEL_GEMM3P_96, true, (k_gemm3p<EPI, 3>), g, 0);
      GEMM_CASE(GNX_GEMM_KERNEL_GEMM3P_128, true, (k_gemm3p<EPI, 4>), g, 0);
      GEMM_CASE(GNX_GEMM_KERNEL_GEMM3, true, (k_gemm3<EPI>), g, 0);
      GEMM_CASE(GNX_GEMM_KERNEL_TILED_VEC, true, (k_gemm<BT, EPI, true>), g, 0);
      GEMM_CASE(GNX_GEMM_KERNEL_TILED_GENERIC, true, (k_gemm<BT, EPI, false>), g, 0);
      default: {  // GNX_GEMM_KERNEL_SMALL: a batch of one
        small_batch_args b;
        for (int i = 0; i < GNX_SMALL_BATCH; ++i)
          b.p[i] = {w.A, w.lda, w.B, w.ldb, bias, C, ldc, (int32_t)M, N, w.K,
                    (p.bt ? GNX_SB_B_TRANS : 0) | (relu ? GNX_SB_RELU : 0) | ((flags & GNX_GEMM_ACCUMULATE) ? GNX_SB_ACCUMULATE : 0)};
        b.n = 1;
        hipLaunchKernelGGL(k_gemm_small_batched, grid, block, 0, h->stream, b);
        return hipSuccess;
      }
    }
  });
#undef GEMM_CASE
  GNX_HIP(lds_limit);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

// The splits of `n` products in ceil(n / SPLIT_MAX_BATCH) launches of k_split_weights_batched on the bound stream (declared
// in gnx_common.hpp; gnx_pna_split_all is the caller).  Every image is written whole by its own problem's workgroups.
int32_t gnx_split_weights_batched(gnx_handle* h, int32_t n, const gemm_split_problem* probs) {
  GNX_CHECK_ARG(h && (n == 0 || probs) && n >= 0, "gnx_split_weights_batched: bad argument");
  double bytes = 0.0;
  for (int i = 0; i < n; ++i) {
    const gemm_split_problem& q = probs[i];
    GNX_CHECK_ARG(q.nseg >= 1 && q.nseg <= MAX_SEGS && q.N > 0 && q.classes >= 1 && q.out && aligned16(q.out),
                  "gnx_split_weights_batched: problem %d: bad shape or image address", i);
    for (int s = 0; s < q.nseg; ++s)
      GNX_CHECK_ARG(q.b[s] && q.k[s] > 0 && q.ldb[s] > 0 && q.ldb[s] <= INT32_MAX,
                    "gnx_split_weights_batched: problem %d, segment %d: NULL weights, k <= 0 or ldb out of range", i, s);
  }
  for (int i0 = 0; i0 < n; i0 += SPLIT_MAX_BATCH) {
    split_batch_args b = {};
    b.n = n - i0 < SPLIT_MAX_BATCH ? n - i0 : SPLIT_MAX_BATCH;
    int64_t widest = 0;
    for (int i = 0; i < b.n; ++i) {
      const gemm_split_problem& q = probs[i0 + i];
      split_batch_prob& d = b.p[i];
      int64_t kpad = 0;
      for (int s = 0; s < q.nseg; ++s) {
        d.seg[s] = split_batch_seg{q.b[s], q.cls_stride[s], (int32_t)q.ldb[s], q.k[s]};
        kpad += plan_kpad(q.k[s]);
      }
      d.out = reinterpret_cast<__bf16*>(q.out);
      d.N = q.N;
      d.D = q.classes;
      d.nseg = q.nseg;
      d.layout = (q.bt ? 1 : 0) | (q.frag ? 2 : 0);
      const int64_t items = (int64_t)q.classes * (gnx_cdiv(q.N, BN) * BN) * (kpad / 8);
      widest = items > widest ? items : widest;
      bytes += 6.0 * items * 8 + 4.0 * q.classes * q.N * kpad;
    }
    gnx_prof_scope prof(h, GNX_K_GEMM_TILED, bytes, 0.0, 0.0);
    hipLaunchKernelGGL(k_split_weights_batched, dim3((unsigned)gnx_cdiv(widest, 256), (unsigned)b.n), dim3(256), 0, h->stream, b);
    ++h->split_batched_launches;
    bytes = 0.0;
  }
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_gemm(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, int64_t M, int32_t N,
                            const float* bias, const float* mask, int64_t ldmask, float* C, int64_t ldc, int32_t flags,
                            void* ws, size_t ws_bytes) {
  return gemm_launch(h, nseg, segs, nullptr, 1, M, N, bias, mask, ldmask, C, ldc, flags, nullptr, nullptr, nullptr, 0,
                     ws, ws_bytes);
}

extern "C" size_t gnx_gemm_workspace_bytes(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs,
                                           const int64_t* cls_strides, int32_t num_classes, int64_t M, int32_t N,
                                           const float* mask, int32_t flags, int32_t grouped) {
  if (h == nullptr || segs == nullptr || nseg < 1 || nseg > MAX_SEGS || M < 0 || N <= 0) return 0;
  static const int32_t a_table = 0;  // (only its NULL-ness is looked at)
  return gemm_plan_of(nseg, segs, cls_strides, num_classes, M, N, nullptr, mask, N, nullptr, N, flags, grouped ? &a_table : nullptr,
                      1, nullptr, 0, h->opt, h->num_cus)
      .image_bytes;
}

extern "C" int32_t gnx_gemm_split_counts(gnx_handle* h, int64_t* per_call, int64_t* batched) {
  GNX_CHECK_ARG(h && per_call && batched, "gnx_gemm_split_counts: NULL argument");
  *per_call = h->split_launches;
  *batched = h->split_batched_launches;
  return GNX_OK;
}

extern "C" int32_t gnx_gemm_tile_rows(gnx_handle* h, int64_t M, int32_t N) {
  if (h == nullptr || M <= 0 || N <= 0) return 128;
  return gemm_plan_tile_rows(M, N, h->opt[GNX_OPT_GEMM_TILE_ROWS], h->num_cus > 0 ? h->num_cus : 256);
}

extern "C" int32_t gnx_gemm_plan(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                                 int32_t num_classes, int64_t M, int32_t N, const float* bias, const float* mask, int64_t ldmask,
                                 float* C, int64_t ldc, int32_t flags, const int32_t* row_index, const int32_t* tile_info,
                                 const int32_t* ntiles, int64_t max_tiles, void* ws, size_t ws_bytes, int32_t tile_rows,
                                 gnx_gemm_plan_info* out) {
  GNX_CHECK_ARG(out, "gnx_gemm_plan: NULL argument");
  const bool grouped = cls_strides || row_index || tile_info || ntiles;
  GNX_CHECK_ARG(!grouped || (cls_strides && row_index && tile_info && ntiles && max_tiles > 0 && num_classes >= 1 && num_classes <= 4096),
                "gnx_gemm_plan: grouped call with a NULL array, max_tiles <= 0 or num_classes not in [1,4096]");
  const int32_t st = gemm_check(h, nseg, segs, M, N, mask, ldmask, C, ldc, flags, tile_rows);
  if (st != GNX_OK) return st;
  (void)ws_bytes;
  const gemm_plan p = gemm_plan_of(nseg, segs, cls_strides, grouped ? num_classes : 1, M, N, bias, mask, ldmask, C, ldc, flags,
                                   tile_info, max_tiles, ws, tile_rows, h->opt, h->num_cus);
  *out = gnx_gemm_plan_info{p.kernel, p.tile_rows, p.grid_x, p.grid_y, p.block, p.run_split ? 1 : 0, p.image_bytes};
  return GNX_OK;
}

extern "C" int32_t gnx_gemm_grouped(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                                    int32_t num_classes, int64_t M, int32_t N, const float* bias, const float* mask,
                                    int64_t ldmask, float* C, int64_t ldc, int32_t flags, const int32_t* row_index,
                                    const int32_t* tile_info, const int32_t* ntiles, int64_t max_tiles, void* ws,
                                    size_t ws_bytes) {
  GNX_CHECK_ARG(cls_strides && row_index && tile_info && ntiles && max_tiles > 0, "gnx_gemm_grouped: NULL argument");
  GNX_CHECK_ARG(num_classes >= 1 && num_classes <= 4096, "gnx_gemm_grouped: num_classes=%d not in [1,4096]", num_classes);
  return gemm_launch(h, nseg, segs, cls_strides, num_classes, M, N, bias, mask, ldmask, C, ldc, flags, row_index,
                     tile_info, ntiles, max_tiles, ws, ws_bytes);
}

static_assert(PLAN_DAF_BM == DAF_BM && PLAN_DAF_LDS == DAF_LDS, "plan / k_pna_dA_agg_bwd");

extern "C" int32_t gnx_pna_da_aggregate_bwd(gnx_handle* h, const float* weff_t, int32_t T, int32_t F, int32_t D, int32_t t,
                                            const float* g, const float* dA, const float* m, const int32_t* rowptr, int64_t N,
                                            int64_t E, float* ge, const int32_t* dperm, const int32_t* tiles,
                                            const int32_t* ntiles, int64_t max_tiles, void* image, const gnx_gemm_image* rec,
                                            void* ws, size_t ws_bytes, int32_t* fused) {
  GNX_CHECK_ARG(h && fused, "gnx_pna_da_aggregate_bwd: NULL argument");
  *fused = 0;
  GNX_CHECK_ARG(T >= 1 && F >= 1 && D >= 1 && D <= 4096 && t >= 0 && t < T && N >= 0 && E >= 0,
                "gnx_pna_da_aggregate_bwd: bad shape T=%d F=%d D=%d t=%d N=%lld E=%lld", T, F, D, t, (long long)N, (long long)E);
  GNX_CHECK_ARG(weff_t && g && dA && rowptr && dperm && tiles && ntiles && max_tiles > 0, "gnx_pna_da_aggregate_bwd: NULL argument");
  GNX_CHECK_ARG(E == 0 || (m && ge), "gnx_pna_da_aggregate_bwd: NULL messages");
  if (N == 0 || E == 0) return GNX_OK;
  const int64_t H = (int64_t)T * F;
  const pna_product q = pna_dA_product(weff_t, T, F, D, t, g, const_cast<float*>(dA));
  // the images: gnx_pna_split_all's where this call's plan gives the record they were written under, else split into ws
  int32_t extra = 0;
  void* img = ws;
  size_t img_bytes = ws_bytes;
  if (image != nullptr && rec != nullptr && rec->image_bytes > 0) {
    const gemm_plan p = pna_product_plan(q, N, GNX_GEMM_PRESPLIT, image, max_tiles, h->opt, h->num_cus);
    if (p.images && gemm_image_equal(gemm_image_of(p), *rec)) {
      extra = GNX_GEMM_PRESPLIT;
      img = image;
      img_bytes = (size_t)rec->image_bytes;
    }
  }
  const pna_dA_agg_plan f = pna_dA_agg_plan_of(q, N, E, H, m, ge, extra, img, max_tiles, h->opt, h->num_cus);
  if (!f.fused) return GNX_OK;
  const gemm_plan& p = f.product;
  if (img_bytes < p.image_bytes) {
    gnx_set_error("gnx_pna_da_aggregate_bwd: workspace of %zu bytes, the split weight images need %zu", img_bytes, p.image_bytes);
    return GNX_E_WORKSPACE;
  }
  GNX_CHECK_ARG(aligned16(img), "gnx_pna_da_aggregate_bwd: workspace must be 16-byte aligned");
  if (p.run_split) {
    const int32_t st = gemm_launch(h, q.nseg, q.seg, q.stride, q.classes, N, q.N, nullptr, nullptr, 0, q.C, q.ldc, GNX_GEMM_SPLIT_ONLY,
                                   dperm, tiles, ntiles, max_tiles, img, img_bytes);
    if (st != GNX_OK) return st;
  }
  gemm_args ga = {{},    1,     N,      q.N,    nullptr, nullptr,
                  0,     q.C,   q.ldc,  0,      dperm,   tiles,
                  ntiles, p.ny, reinterpret_cast<__bf16*>(img), p.Npad, p.Kpad, {}, p.Kpad / BK};
  for (int s = 0; s < MAX_SEGS; ++s) {
    ga.seg[s] = seg_dev{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0};
    ga.koff[s] = p.koff[s];
  }
  const gnx_gemm_seg& in = q.seg[0];
  ga.seg[0] = seg_dev{in.a, nullptr, in.b, in.lda, in.ldb, q.stride[0], in.k, plan_vec_a(in), plan_vec_b(in, q.stride[0])};
  const daf_args x = {m + (int64_t)t * F, rowptr, ge + (int64_t)t * F, (int)H, h->opt[GNX_OPT_STD_BWD_CENTERED]};
  gnx_prof_scope prof(h, GNX_K_PNA_AGG_BWD, f.bytes, f.flops, f.mfma, true);
  GNX_LAUNCH_TIMED(prof, k_pna_dA_agg_bwd, dim3(f.grid_x), dim3(256), f.lds, h->stream, ga, x);
  GNX_LAUNCH_CHECK();
  *fused = 1;
  return GNX_OK;
}

extern "C" int32_t gnx_gemm_grouped_rows(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                                         int32_t num_classes, int64_t M, int32_t N, const float* bias, const float* mask,
                                         int64_t ldmask, float* C, int64_t ldc, int32_t flags, const int32_t* row_index,
                                         const int32_t* tile_info, const int32_t* ntiles, int64_t max_tiles, void* ws,
                                         size_t ws_bytes, int32_t tile_rows) {
  GNX_CHECK_ARG(cls_strides && row_index && tile_info && ntiles && max_tiles > 0, "gnx_gemm_grouped_rows: NULL argument");
  GNX_CHECK_ARG(num_classes >= 1 && num_classes <= 4096, "gnx_gemm_grouped_rows: num_classes=%d not in [1,4096]", num_classes);
  GNX_CHECK_ARG(tile_rows == 96 || tile_rows == 128, "gnx_gemm_grouped_rows: tile_rows=%d not in {96, 128}", tile_rows);
  return gemm_launch(h, nseg, segs, cls_strides, num_classes, M, N, bias, mask, ldmask, C, ldc, flags, row_index,
                     tile_info, ntiles, max_tiles, ws, ws_bytes, tile_rows);
}
