// Weight gradients of the dense products (gnx_gemm.hip): the fp32-MFMA kernel, the split-operand kernels (two-barrier and
// wave-specialised) and their batched forms, which run several same-shaped problems in one launch.
#include "gnx_split.hpp"
#include "gnx_wgrad_plan.hpp"

static_assert(WGRAD_PLAN_BN == BN, "gnx_wgrad_plan.hpp: dW tile");

// ---------------------------------------------------------------------------------------------------------------
// Weight gradient  dW[n,k] += sum_m dC[m,n] * rs[m]*A[m,k]   (both operands k-row images: the contraction index m is the
// row of both).  grid = (M chunks, n tiles, k tiles); fp32 atomics into dW; the k-tile-0 workgroups also reduce dbias.
// ---------------------------------------------------------------------------------------------------------------
struct wgrad_args {
  const float* X;  // dC [M, N]
  int64_t ldx;
  const float* Y;  // A  [M, K]
  int64_t ldy;
  const float* rs;
  int64_t M;
  int N, K;
  float* dW;
  int64_t lddw;
  float* dbias;
  int64_t rows_per_block;
  int vec_x, vec_y;
  // grouped mode: blockIdx.x = chunk; rows row_index[chunk_info[3b] .. +chunk_info[3b+1]) add into dW + class * stride
  const int* row_index;
  const int* chunk_info;
  const int* nchunks;
  int64_t dw_cls_stride;
  const float* zero;  // 16 readable zero bytes (k_gemm_wgrad3p: target of masked-out loads)
};

template <bool VEC, bool GROUPED>
__device__ __forceinline__ void wgrad_body(const wgrad_args& g, const int bx, const int by, const int bz, float* Xs,
                                           float* Ys) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = by * BN;  // dW row tile (output features)
  const int c0 = bz * BN;  // dW col tile (input features)
  if (n0 >= g.N || c0 >= g.K) return;
  int64_t r_begin = (int64_t)bx * g.rows_per_block;
  int64_t r_end = r_begin + g.rows_per_block;
  if (r_end > g.M) r_end = g.M;
  float* dW = g.dW;
  if constexpr (GROUPED) {
    if (bx >= g.nchunks[0]) return;
    r_begin = g.chunk_info[3 * bx];
    r_end = r_begin + g.chunk_info[3 * bx + 1];
    dW += (int64_t)g.chunk_info[3 * bx + 2] * g.dw_cls_stride;
  }
  if (r_begin >= r_end) return;  // (workgroup-uniform) nothing to contribute: skip the zero-valued atomic flush

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float bsum = 0.f;  // threads 0..127: column n0+tid of dC

  const int br = tid >> 5;
  const int bc = (tid & 31) * 4;
  f32x4 rx[4], ry[4];
  int okmask = 0;
  float rsv[4] = {1.f, 1.f, 1.f, 1.f};

  auto load_tile = [&](int64_t r0) {
    if constexpr (VEC) {
      // raw loads; select / row scale deferred to the LDS store (see k_gemm)
      const int xn = n0 + bc, yk = c0 + bc;
      const bool x_ok = xn < g.N, y_ok = yk < g.K;
      const int xc = x_ok ? xn : 0, yc = y_ok ? yk : 0;
      int64_t rowi[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t pos = r0 + br + 8 * i;
        const int64_t pc = pos < r_end ? pos : r_begin;  // clamped (r_begin < r_end here)
        rowi[i] = GROUPED ? (int64_t)g.row_index[pc] : pc;
      }
      okmask = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool rv = r0 + br + 8 * i < r_end;
        rx[i] = *reinterpret_cast<const f32x4*>(g.X + rowi[i] * g.ldx + xc);
        ry[i] = *reinterpret_cast<const f32x4*>(g.Y + rowi[i] * g.ldy + yc);
        rsv[i] = *(g.rs != nullptr ? g.rs + rowi[i] : &c_one);
        okmask |= (rv && x_ok) ? (1 << i) : 0;
        okmask |= (rv && y_ok) ? (16 << i) : 0;
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t gm = r0 + br + 8 * i;
      bool rv = gm < r_end;
      if (GROUPED && rv) gm = g.row_index[gm];
      int nv = rv ? g.N - (n0 + bc) : 0;
      rx[i] = ld4(g.X + gm * g.ldx + n0 + bc, g.vec_x, nv);
      int kv = rv ? g.K - (c0 + bc) : 0;
      f32x4 v = ld4(g.Y + gm * g.ldy + c0 + bc, g.vec_y, kv);
      if (g.rs != nullptr && rv) {
        float sc = g.rs[gm];
        v.x *= sc;
        v.y *= sc;
        v.z *= sc;
        v.w *= sc;
      }
      ry[i] = v;
    }
  };

  int64_t r0 = r_begin;
  if (r0 < r_end) load_tile(r0);
  while (r0 < r_end) {
    __syncthreads();
    if constexpr (VEC) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 v = ry[i];
        v.x *= rsv[i];
        v.y *= rsv[i];
        v.z *= rsv[i];
        v.w *= rsv[i];
        rx[i] = ((okmask >> i) & 1) ? rx[i] : z;
        ry[i] = ((okmask >> (4 + i)) & 1) ? v : z;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int kr = br + 8 * i;
      *reinterpret_cast<f32x4*>(&Xs[kr * LDN + bc]) = rx[i];
      *reinterpret_cast<f32x4*>(&Ys[kr * LDN + bc]) = ry[i];
    }
    __syncthreads();
    r0 += BK;
    if (r0 < r_end) load_tile(r0);

    if (g.dbias != nullptr && bz == 0 && tid < BN) {
#pragma unroll 8
      for (int r = 0; r < BK; ++r) bsum += Xs[r * LDN + tid];
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      f32x4 a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const float* p = &Xs[(kk * 8 + 4 * lh) * LDN + wm * 64 + mi * 32 + li];
        a[mi].x = p[0];
        a[mi].y = p[LDN];
        a[mi].z = p[2 * LDN];
        a[mi].w = p[3 * LDN];
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const float* p = &Ys[(kk * 8 + 4 * lh) * LDN + wn * 64 + ni * 32 + li];
        b[ni].x = p[0];
        b[ni].y = p[LDN];
        b[ni].z = p[2 * LDN];
        b[ni].w = p[3 * LDN];
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
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int gc = c0 + wn * 64 + ni * 32 + li;
      if (gc >= g.K) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int gr = n0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gr >= g.N) continue;
        atomicAdd(dW + (int64_t)gr * g.lddw + gc, acc[mi][ni][r]);
      }
    }
  if (g.dbias != nullptr && bz == 0 && tid < BN && n0 + tid < g.N) atomicAdd(g.dbias + n0 + tid, bsum);
}

template <bool VEC, bool GROUPED>
__global__ void __launch_bounds__(256, 2) k_gemm_wgrad(wgrad_args g) {
  __shared__ __attribute__((aligned(16))) float Xs[BK * LDN];
  __shared__ __attribute__((aligned(16))) float Ys[BK * LDN];
  wgrad_body<VEC, GROUPED>(g, blockIdx.x, blockIdx.y, blockIdx.z, Xs, Ys);
}

// ---------------------------------------------------------------------------------------------------------------
// Split-operand weight gradient (same contract as wgrad_body<true, GROUPED> without a row scale; see the split-operand
// notes at k_gemm_ws3).  dW[n,k] = sum_m dC[m,n] A[m,k] contracts over the ROW index of both operands, so both bf16
// images must be column-major for the matrix core (a lane needs 8 consecutive m of one column).  The transpose is done
// by the loader: thread = (column tid & 127, 16 rows), 16 four-byte loads per operand and 32-row step (each wave
// instruction reads 256 contiguous bytes of one row); the 16 values of a column are split and stored with two
// ds_write_b128 per image into [3][128 columns][32 m (+8 pad)] -- the same images and the same multiply loop as
// k_gemm3.  The fp32-MFMA version above runs at ~70 TF and was the largest group of kernels of the step.
// ---------------------------------------------------------------------------------------------------------------
template <bool GROUPED>
__device__ __forceinline__ void wgrad3_body(const wgrad_args& g, const int bx, const int by, const int bz,
                                            unsigned char* A3, unsigned char* B3, unsigned* offs) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = by * BN;  // dW row tile (output features)
  const int c0 = bz * BN;  // dW col tile (input features)
  if (n0 >= g.N || c0 >= g.K) return;
  int64_t r_begin = (int64_t)bx * g.rows_per_block;
  int64_t r_end = r_begin + g.rows_per_block;
  if (r_end > g.M) r_end = g.M;
  float* dW = g.dW;
  if constexpr (GROUPED) {
    if (bx >= g.nchunks[0]) return;
    r_begin = g.chunk_info[3 * bx];
    r_end = r_begin + g.chunk_info[3 * bx + 1];
    dW += (int64_t)g.chunk_info[3 * bx + 2] * g.dw_cls_stride;
  }
  if (r_begin >= r_end) return;  // (workgroup-uniform) nothing to contribute: skip the zero-valued atomic flush

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float bsum = 0.f;  // column n0 + col of dC, this thread's 16-row half

  const int col = tid & 127, rh = (tid >> 7) * 16;
  const bool x_ok = n0 + col < g.N, y_ok = c0 + col < g.K;
  const float* xp = g.X + (x_ok ? n0 + col : 0);
  const float* yp = g.Y + (y_ok ? c0 + col : 0);
  float gx[16], gy[16];
  int nvalid = 0;  // valid rows among this thread's 16 of the tile in flight

  // GROUPED: rows are gathered through row_index.  The element offsets row * ld of a step's 32 rows are computed once
  // per workgroup (threads 0..31, two steps ahead, into a double-buffered LDS array offs[parity][X|Y][32]) instead of
  // 32 index loads + 32 64-bit multiplies per thread and step; the host guarantees M * ld < 2^32.
  auto stage_offsets = [&](int64_t r0, int par) {
    if constexpr (GROUPED) {
      if (tid < 32) {
        const int64_t pos = r0 + tid < r_end ? r0 + tid : r_begin;
        const unsigned row = (unsigned)g.row_index[pos];
        offs[par * 64 + tid] = row * (unsigned)g.ldx;
        offs[par * 64 + 32 + tid] = row * (unsigned)g.ldy;
      }
    }
  };
  auto load_tile = [&](int64_t r0, int par) {
    const int64_t first = r0 + rh;
    const int64_t left = r_end - first;
    nvalid = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
    if constexpr (GROUPED) {
      const unsigned* ox = offs + par * 64 + rh;
      const unsigned* oy = ox + 32;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        gx[j] = xp[ox[j]];
        gy[j] = yp[oy[j]];
      }
    } else if (r0 + BK <= r_end) {  // full step (workgroup-uniform): one 64-bit product per operand, uniform strides
      const float* xb = xp + first * g.ldx;
      const float* yb = yp + first * g.ldy;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        gx[j] = xb[j * g.ldx];
        gy[j] = yb[j * g.ldy];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int64_t row = first + j < r_end ? first + j : r_begin;  // clamped (r_begin < r_end here)
        gx[j] = xp[row * g.ldx];
        gy[j] = yp[row * g.ldy];
      }
    }
  };

  auto store_tile = [&]() {
#pragma unroll
    for (int hgrp = 0; hgrp < 2; ++hgrp) {
      float xa[8], ya[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = 8 * hgrp + j < nvalid;
        xa[j] = (ok && x_ok) ? gx[8 * hgrp + j] : 0.f;
        ya[j] = (ok && y_ok) ? gy[8 * hgrp + j] : 0.f;
        bsum += xa[j];
      }
      bf16x8 p1, p2, p3;
      split3(xa, p1, p2, p3);
      unsigned char* q = A3 + col * G3_LDB + (rh + 8 * hgrp) * 2;
      *reinterpret_cast<bf16x8*>(q) = p1;
      *reinterpret_cast<bf16x8*>(q + G3_PIECE) = p2;
      *reinterpret_cast<bf16x8*>(q + 2 * G3_PIECE) = p3;
      split3(ya, p1, p2, p3);
      q = B3 + col * G3_LDB + (rh + 8 * hgrp) * 2;
      *reinterpret_cast<bf16x8*>(q) = p1;
      *reinterpret_cast<bf16x8*>(q + G3_PIECE) = p2;
      *reinterpret_cast<bf16x8*>(q + 2 * G3_PIECE) = p3;
    }
  };

  int64_t r0 = r_begin;
  int par = 0;
  stage_offsets(r0, 0);
  stage_offsets(r0 + BK, 1);
  if constexpr (GROUPED) __syncthreads();
  load_tile(r0, 0);
  while (r0 < r_end) {
    __syncthreads();  // previous multiply finished reading LDS (and the offsets staged during it are visible)
    store_tile();
    __syncthreads();
    r0 += BK;
    par ^= 1;
    if (r0 < r_end) load_tile(r0, par);
    // offsets of the step after that one go into the other buffer (last read one step ago, two barriers back)
    if (r0 + BK < r_end) stage_offsets(r0 + BK, par ^ 1);
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
  }

#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int gc = c0 + wn * 64 + ni * 32 + li;
      if (gc >= g.K) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int gr = n0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gr >= g.N) continue;
        atomicAdd(dW + (int64_t)gr * g.lddw + gc, acc[mi][ni][r]);
      }
    }
  if (g.dbias != nullptr && bz == 0 && x_ok) atomicAdd(g.dbias + n0 + col, bsum);
}

template <bool GROUPED>
__global__ void __launch_bounds__(256, 2) k_gemm_wgrad3(wgrad_args g) {
  __shared__ __attribute__((aligned(16))) unsigned char A3[G3_OP];
  __shared__ __attribute__((aligned(16))) unsigned char B3[G3_OP];
  __shared__ __attribute__((aligned(16))) unsigned offs[128];
  wgrad3_body<GROUPED>(g, blockIdx.x, blockIdx.y, blockIdx.z, A3, B3, offs);
}

// ---------------------------------------------------------------------------------------------------------------
// Wave-specialised split-operand weight gradient (same contract and arithmetic as wgrad3_body for 16-byte aligned
// operands with N, K multiples of 4), ONE 512-thread workgroup per CU -- the weight-gradient launches are sized to one
// workgroup per CU anyway, and in the two-barrier body above such a lone workgroup runs its phases back to back: 32
// four-byte loads per thread, wait, split, LDS stores, barrier, fragment reads, 48 MFMAs, barrier = 2.5-2.8 us per
// 32-row step against 0.65-0.87 us of MFMA time (SQ_VALU_MFMA_BUSY_CYCLES: 0.20-0.26 of the matrix pipe; ablations:
// split + LDS stores alone 1.0 us, fragment reads + MFMAs alone 1.27 us, and the compiler keeps the two apart even
// inside one basic block).  Here the phases belong to different waves of the same SIMD, which the hardware overlaps:
//   * waves 0..3 multiply: fragment reads + 48 MFMAs per step out of the LDS stage of step j (2 x 2 tiles of 64 x 64);
//   * waves 4..7 stage: threads 256..383 dC, 384..511 A -- eight 16-byte loads each (8 rows x 4 columns) issued five
//     steps ahead into four register stages (128 KB in flight per CU), always unconditional (invalid rows / columns read a zero line instead of
//     being masked), split column by column and written as 16-byte LDS words into the [column][32 m] bf16 images of
//     step j + 1 (two-stage ring, 120 KB); they also accumulate the bias gradient;
//   * ONE barrier per step joins the two groups.
// Rows gathered by degree class: a first grouped form of this structure (one workgroup per 1024-row chunk, LDS-staged row
// offsets) was built, correct, and SLOWER than wgrad3_body<true> (145 vs 123 us per launch: 1024 rows = 32 steps are too
// short for its prologue).  k_gemm_wgrad3p_grouped below walks merged runs of consecutive chunks instead; its figures
// are at its launch in wgrad_launch.
// Measured (tools/wgrad_ab.py, a layer's eight 81 920 x 128 x 128 problems in one launch = 671 MB): 235 -> 205 us (3.4 -> 3.9
// TB/s); K = 512: 111 -> 94 us.  Ablations of this kernel: the loads alone 124 us (the HBM floor), + the multiply waves
// 132 us, + the staging waves' split and stores instead 138 us, both 195-205 us: the two groups slow each other down.
// tools/ubench/wave_specialised_overlap.hip isolates that: per step, multiply waves alone 0.91 us, staging waves alone
// 0.60 us (split) / 0.84 us (+ the twelve ds_write_b128), both 1.04 us without and 1.41-1.46 us with the LDS stores --
// the 16-byte LDS stores, not the split, are what the MFMA waves feel; 1.45 us is this structure's floor, the kernel
// runs at 2.2 us (loads, masks, address arithmetic, bias sums on top).
// ---------------------------------------------------------------------------------------------------------------
#define WG3P_LDS (4 * G3_OP)
#define WG3P_NST 4  // register stages of the staging waves (must be 4: the prologue and the unrolled loop assume it)

// The three pieces of wgrad3p_body that k_gemm_wgrad3p_grouped below runs unchanged.  wgrad3p_body keeps its own inline
// copy: routed through these functions the batched kernel comes out with a different schedule of its fragment waits
// (38 more s_waitcnt), and that schedule has not been measured.
// A staging thread's eight rows of one column: split and written as one 16-byte word per bf16 image
__device__ __forceinline__ void wg3p_store_column(const float (&xa)[8], unsigned char* dst) {
  bf16x8 p1, p2, p3;
  split3(xa, p1, p2, p3);
  *reinterpret_cast<bf16x8*>(dst) = p1;
  *reinterpret_cast<bf16x8*>(dst + G3_PIECE) = p2;
  *reinterpret_cast<bf16x8*>(dst + 2 * G3_PIECE) = p3;
}

// One 32-row step of a multiply wave (wave 0..3 owns the 64 x 64 quadrant (wave >> 1, wave & 1) of the 128 x 128 tile):
// fragment reads + 48 MFMAs out of the LDS stage `stage` = [dC images | A images].
__device__ __forceinline__ void wg3p_multiply_step(f32x16 (&acc)[2][2], const unsigned char* stage, const int wave,
                                                   const int lane) {
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const unsigned char* const A3 = stage;
  const unsigned char* const B3 = A3 + G3_OP;
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
}

// fp32 atomics of a multiply wave's quadrant into dW (rows n0.., columns c0..)
__device__ __forceinline__ void wg3p_flush(const f32x16 (&acc)[2][2], const wgrad_args& g, float* dW, const int n0,
                                           const int c0, const int wave, const int lane) {
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int gc = c0 + wn * 64 + ni * 32 + li;
      if (gc >= g.K) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int gr = n0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gr >= g.N) continue;
        atomicAdd(dW + (int64_t)gr * g.lddw + gc, acc[mi][ni][r]);
      }
    }
}

__device__ __forceinline__ void wgrad3p_body(const wgrad_args& g, const int bx, const int by, const int bz,
                                             unsigned char* lds) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int n0 = by * BN;  // dW row tile (output features)
  const int c0 = bz * BN;  // dW col tile (input features)
  if (n0 >= g.N || c0 >= g.K) return;
  int64_t r_begin = (int64_t)bx * g.rows_per_block;
  int64_t r_end = r_begin + g.rows_per_block;
  if (r_end > g.M) r_end = g.M;
  float* const dW = g.dW;
  if (r_begin >= r_end) return;
  const int64_t nsteps = (r_end - r_begin + BK - 1) / BK;

  if (wave < 4) {
    // ================================================================ multiply waves
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    __syncthreads();  // the staging waves' prologue
    for (int64_t j = 0; j < nsteps; ++j) {
      const unsigned char* const A3 = lds + (j & 1) * 2 * G3_OP;
      const unsigned char* const B3 = A3 + G3_OP;
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
      __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        int gc = c0 + wn * 64 + ni * 32 + li;
        if (gc >= g.K) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int gr = n0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (gr >= g.N) continue;
          atomicAdd(dW + (int64_t)gr * g.lddw + gc, acc[mi][ni][r]);
        }
      }
    return;
  }

  // ================================================================== staging waves
  const int lt = tid - 256;
  const int role = lt >> 7;  // 0: dC (dW rows n0..), 1: A (dW columns c0..)
  const int c4 = (lt & 31) * 4, rg = (lt >> 5) & 3;
  const bool col_ok = role ? (c0 + c4 < g.K) : (n0 + c4 < g.N);  // N, K multiples of 4: the quad is valid as a whole
  const float* const base = (role ? g.Y + (col_ok ? c0 + c4 : 0) : g.X + (col_ok ? n0 + c4 : 0));
  const float* const zero = g.zero;  // 16 zero bytes: what an invalid row or column quad reads
  const int64_t ld = role ? g.ldy : g.ldx;
  const int img = role * G3_OP;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};  // role 0: column sums of dC (bias gradient)

  f32x4 v[WG3P_NST][8];  // register stages: the loads of WG3P_NST steps in flight (32 KB per stage and workgroup)

  auto load_step = [&](auto PC, int64_t r0) {
    constexpr int P = decltype(PC)::value;
    const int64_t left = r_end - (r0 + rg * 8);
    const int nval = (left >= 8 && col_ok) ? 8 : ((left > 0 && col_ok) ? (int)left : 0);
    const float* p = base + (r0 + rg * 8) * ld;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[P][j] = *reinterpret_cast<const f32x4*>(j < nval ? p + j * ld : zero);
  };
  auto store_step = [&](auto PC, unsigned char* stage) {
    constexpr int P = decltype(PC)::value;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float xa[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) xa[j] = v[P][j][q];
      if (role == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[q] += xa[j];
      }
      bf16x8 p1, p2, p3;
      split3(xa, p1, p2, p3);
      unsigned char* dst = stage + img + (c4 + q) * G3_LDB + rg * 16;
      *reinterpret_cast<bf16x8*>(dst) = p1;
      *reinterpret_cast<bf16x8*>(dst + G3_PIECE) = p2;
      *reinterpret_cast<bf16x8*>(dst + 2 * G3_PIECE) = p3;
    }
  };
  auto row_of = [&](int64_t step) { return r_begin + step * BK; };

  // ---- prologue: steps 0 .. 3 loaded, step 0 split into LDS stage 0, step 4 loaded into its register stage
  load_step(std::integral_constant<int, 0>{}, row_of(0));
  load_step(std::integral_constant<int, 1>{}, row_of(1));
  load_step(std::integral_constant<int, 2>{}, row_of(2));
  load_step(std::integral_constant<int, 3>{}, row_of(3));
  store_step(std::integral_constant<int, 0>{}, lds);
  load_step(std::integral_constant<int, 0>{}, row_of(4));
  __syncthreads();

  // iteration j (K = j % NST): split register stage (K + 1) % NST = step j + 1 into LDS stage (j + 1) & 1, then refill
  // that register stage with step j + 1 + NST
  auto iteration = [&](auto KC, int64_t j) {
    constexpr int K = decltype(KC)::value;
    constexpr int P = (K + 1) % WG3P_NST;
    store_step(std::integral_constant<int, P>{}, lds + ((K + 1) & 1) * 2 * G3_OP);
    load_step(std::integral_constant<int, P>{}, row_of(j + 1 + WG3P_NST));
    __syncthreads();
  };
  for (int64_t j = 0; j < nsteps; j += 4) {
    iteration(std::integral_constant<int, 0>{}, j);
    if (j + 1 >= nsteps) break;
    iteration(std::integral_constant<int, 1>{}, j + 1);
    if (j + 2 >= nsteps) break;
    iteration(std::integral_constant<int, 2>{}, j + 2);
    if (j + 3 >= nsteps) break;
    iteration(std::integral_constant<int, 3>{}, j + 3);
  }
  if (g.dbias != nullptr && bz == 0 && role == 0 && col_ok) {
#pragma unroll
    for (int q = 0; q < 4; ++q) atomicAdd(g.dbias + n0 + c4 + q, bsum[q]);
  }
}

__global__ void __launch_bounds__(512, 1) k_gemm_wgrad3p(wgrad_args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_w[];
  wgrad3p_body(g, blockIdx.x, blockIdx.y, blockIdx.z, lds_w);
}

// ---------------------------------------------------------------------------------------------------------------
// Per-degree-class form of the wave-specialised kernel (no row scale, no bias gradient; 16-byte aligned operands, N and K
// multiples of 4, M * ld < 2^32).  Workgroup (w, by, bz) owns the chunks [w S, min((w + 1) S, nchunks)) of the chunk table
// (S = chunks_per_range, fixed on the host from max_chunks; nchunks is read here, on the device).  Chunks of one class
// are consecutive ranges of row_index, so consecutive owned chunks of the same class whose positions touch form ONE run
// [p0, p0 + len): per run the accumulators are zeroed, wgrad3p_body's prologue and pipelined loop run over
// ceil(len / 32) steps, and the tile is flushed once into dW + class * dw_cls_stride.
//
// Barriers: both wave roles derive the run list from the same scalars (readfirstlane of the chunk table), and per run
// both pass 2 + nsteps barriers: A (the ring below is filled), B (the staging prologue: step 0 is in LDS stage 0), one
// per step.  The barrier that ends a run's last step orders every fragment read of that run before the next run's
// prologue stores into LDS stage 0 and before its ring fill.
//
// Row gather: the staging waves read row row_index[p0 + i] for position i of the run.  Vector-memory loads return in
// order, so a staging wave that waited for an index load would also wait for the four steps of row loads in front of
// it.  The row numbers therefore reach the staging waves through LDS (its own counter): a ring of WG3G_RING = 16 steps x
// 32 row numbers.  The staging waves fill steps 0..15 at the start of a run (barrier A); after that the MULTIPLY waves,
// which have no other load in flight, fetch eight steps at a time: step 8m + 3 loads the row numbers of steps
// 8m + 16 .. 8m + 23 (thread = position), step 8m + 4 stores them over steps 8m .. 8m + 7, last read (by the loads of step
// i + 5 in step i) in step 8m + 2 and next needed in step 8m + 11.  Positions at or past the end of the run read the
// zero line, as rows past r_end do in wgrad3p_body; the ring entry of such a position is a valid row that nobody loads.
// ---------------------------------------------------------------------------------------------------------------
#define WG3G_RING 16
#define WG3G_LDS (WG3P_LDS + WG3G_RING * BK * 4)

struct wgrad_grouped_args {
  wgrad_args g;
  int chunks_per_range;  // S: blockIdx.x = range of this many consecutive chunks
  int max_chunks;        // ... of a table of this many chunks (nchunks[0] is clamped to it)
};

__global__ void __launch_bounds__(512, 1) k_gemm_wgrad3p_grouped(wgrad_grouped_args ga) {
  const wgrad_args& g = ga.g;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_wg[];
  unsigned char* const lds = lds_wg;
  unsigned* const ring = reinterpret_cast<unsigned*>(lds_wg + WG3P_LDS);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int n0 = blockIdx.y * BN;  // dW row tile (output features)
  const int c0 = blockIdx.z * BN;  // dW col tile (input features)
  if (n0 >= g.N || c0 >= g.K) return;
  const int c_begin = (int)blockIdx.x * ga.chunks_per_range;
  int nch = __builtin_amdgcn_readfirstlane(g.nchunks[0]);
  nch = nch < ga.max_chunks ? nch : ga.max_chunks;
  const int c_end = c_begin + ga.chunks_per_range < nch ? c_begin + ga.chunks_per_range : nch;
  auto info = [&](int i) { return __builtin_amdgcn_readfirstlane(g.chunk_info[i]); };
  // the run that starts at chunk c: [p0, p0 + len) of row_index, class cls; c moves to the first chunk behind it
  auto next_run = [&](int& c, int& p0, int& len, int& cls) {
    p0 = info(3 * c);
    len = info(3 * c + 1);
    cls = info(3 * c + 2);
    for (++c; c < c_end && info(3 * c + 2) == cls && info(3 * c) == p0 + len; ++c) len += info(3 * c + 1);
  };
  // row number of position i of the run (clamped: the row of a position past the run is never loaded)
  auto row_at = [&](int p0, int len, int i) { return (unsigned)g.row_index[p0 + (i < len ? i : 0)]; };

  if (wave < 4) {
    // ================================================================ multiply waves
    for (int c = c_begin; c < c_end;) {
      int p0, len, cls;
      next_run(c, p0, len, cls);
      if (len <= 0) continue;
      const int nsteps = (len + BK - 1) / BK;
      f32x16 acc[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
      __syncthreads();  // A
      __syncthreads();  // B
      unsigned pend = 0;
      for (int j = 0; j < nsteps; ++j) {
        if ((j & 7) == 3) pend = row_at(p0, len, (j + 13) * BK + tid);
        wg3p_multiply_step(acc, lds + (j & 1) * 2 * G3_OP, wave, lane);
        if ((j & 7) == 4) ring[((j + 12) & (WG3G_RING - 1)) * BK + tid] = pend;
        __syncthreads();
      }
      wg3p_flush(acc, g, g.dW + (int64_t)cls * g.dw_cls_stride, n0, c0, wave, lane);
    }
    return;
  }

  // ================================================================== staging waves
  const int lt = tid - 256;
  const int role = lt >> 7;  // 0: dC (dW rows n0..), 1: A (dW columns c0..)
  const int c4 = (lt & 31) * 4, rg = (lt >> 5) & 3;
  const bool col_ok = role ? (c0 + c4 < g.K) : (n0 + c4 < g.N);  // N, K multiples of 4: the quad is valid as a whole
  const float* const base = (role ? g.Y + (col_ok ? c0 + c4 : 0) : g.X + (col_ok ? n0 + c4 : 0));
  const float* const zero = g.zero;
  const unsigned ld = (unsigned)(role ? g.ldy : g.ldx);
  const int img = role * G3_OP;
  int len = 0;  // of the current run

  f32x4 v[WG3P_NST][8];

  auto load_step = [&](auto PC, int step) {
    constexpr int P = decltype(PC)::value;
    const int left = len - (step * BK + rg * 8);
    const int nval = (left >= 8 && col_ok) ? 8 : ((left > 0 && col_ok) ? left : 0);
    const unsigned* const rr = ring + (step & (WG3G_RING - 1)) * BK + rg * 8;
    const split_u32x4 ra = *reinterpret_cast<const split_u32x4*>(rr);
    const split_u32x4 rb = *reinterpret_cast<const split_u32x4*>(rr + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned off = (j < 4 ? ra[j & 3] : rb[j & 3]) * ld;  // row * ld < 2^32 (host)
      v[P][j] = *reinterpret_cast<const f32x4*>(j < nval ? base + off : zero);
    }
  };
  auto store_step = [&](auto PC, unsigned char* stage) {
    constexpr int P = decltype(PC)::value;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float xa[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) xa[j] = v[P][j][q];
      wg3p_store_column(xa, stage + img + (c4 + q) * G3_LDB + rg * 16);
    }
  };
  // step j (K = j % NST): as in wgrad3p_body
  auto iteration = [&](auto KC, int j) {
    constexpr int K = decltype(KC)::value;
    constexpr int P = (K + 1) % WG3P_NST;
    store_step(std::integral_constant<int, P>{}, lds + ((K + 1) & 1) * 2 * G3_OP);
    load_step(std::integral_constant<int, P>{}, j + 1 + WG3P_NST);
    __syncthreads();
  };

  for (int c = c_begin; c < c_end;) {
    int p0, cls;
    next_run(c, p0, len, cls);
    if (len <= 0) continue;
    const int nsteps = (len + BK - 1) / BK;
    ring[lt] = row_at(p0, len, lt);
    ring[256 + lt] = row_at(p0, len, 256 + lt);
    __syncthreads();  // A
    load_step(std::integral_constant<int, 0>{}, 0);
    load_step(std::integral_constant<int, 1>{}, 1);
    load_step(std::integral_constant<int, 2>{}, 2);
    load_step(std::integral_constant<int, 3>{}, 3);
    store_step(std::integral_constant<int, 0>{}, lds);
    load_step(std::integral_constant<int, 0>{}, 4);
    __syncthreads();  // B
    for (int j = 0; j < nsteps; j += 4) {
      iteration(std::integral_constant<int, 0>{}, j);
      if (j + 1 >= nsteps) break;
      iteration(std::integral_constant<int, 1>{}, j + 1);
      if (j + 2 >= nsteps) break;
      iteration(std::integral_constant<int, 2>{}, j + 2);
      if (j + 3 >= nsteps) break;
      iteration(std::integral_constant<int, 3>{}, j + 3);
    }
  }
}

// Several independent weight gradients in ONE launch (a layer's same-shaped dW = g^T a products): blockIdx.x =
// problem * chunks + chunk.  With P problems sharing the grid every workgroup owns a P x longer row range, so the
// per-problem atomic flush shrinks P x at equal parallelism (a lone 128x128 dW over 82k rows flushes 33 MB of fp32
// atomics for 17 us of MFMA work).
#define WGRAD_MAX_BATCH 8
struct wgrad_batch_args {
  wgrad_args p[WGRAD_MAX_BATCH];
  int nprob;
  // 1-D work list: problem i owns workgroups [wg_off[i], wg_off[i+1]) = its row chunks x its 128x128 output tiles.
  // Chunk counts are per problem (proportional to its share of the work): one uniform count starved the small
  // problems of a batch that also held a 512x512 one (cfg-5: 32 workgroups busy on 256 CUs, 26 TF).
  int wg_off[WGRAD_MAX_BATCH + 1];
  int tiles_k[WGRAD_MAX_BATCH];  // column tiles of dW
  int tiles[WGRAD_MAX_BATCH];    // row tiles x column tiles of dW
};

// (problem, chunk, dW row tile, dW column tile) of a workgroup of the 1-D batched grid
__device__ __forceinline__ void wgrad_batch_locate(const wgrad_batch_args& b, int w, int& prob, int& chunk, int& by,
                                                   int& bz) {
  prob = 0;
#pragma unroll
  for (int i = 1; i < WGRAD_MAX_BATCH; ++i) prob += (i < b.nprob && w >= b.wg_off[i]) ? 1 : 0;
  int off = b.wg_off[0], tiles = b.tiles[0], tk = b.tiles_k[0];
#pragma unroll
  for (int i = 1; i < WGRAD_MAX_BATCH; ++i)
    if (i == prob) {
      off = b.wg_off[i];
      tiles = b.tiles[i];
      tk = b.tiles_k[i];
    }
  const int local = w - off;
  chunk = local / tiles;
  const int t = local - chunk * tiles;
  by = t / tk;
  bz = t - by * tk;
}

__global__ void __launch_bounds__(256, 2) k_gemm_wgrad_batched(wgrad_batch_args b) {
  __shared__ __attribute__((aligned(16))) float Xs[BK * LDN];
  __shared__ __attribute__((aligned(16))) float Ys[BK * LDN];
  int prob, chunk, by, bz;
  wgrad_batch_locate(b, blockIdx.x, prob, chunk, by, bz);
  // copy the selected descriptor (wave-uniform index) so the body sees scalars
  wgrad_args g = b.p[0];
#pragma unroll
  for (int i = 1; i < WGRAD_MAX_BATCH; ++i)
    if (i == prob) g = b.p[i];
  wgrad_body<true, false>(g, chunk, by, bz, Xs, Ys);
}

__global__ void __launch_bounds__(256, 2) k_gemm_wgrad3_batched(wgrad_batch_args b) {
  __shared__ __attribute__((aligned(16))) unsigned char A3[G3_OP];
  __shared__ __attribute__((aligned(16))) unsigned char B3[G3_OP];
  int prob, chunk, by, bz;
  wgrad_batch_locate(b, blockIdx.x, prob, chunk, by, bz);
  wgrad_args g = b.p[0];
#pragma unroll
  for (int i = 1; i < WGRAD_MAX_BATCH; ++i)
    if (i == prob) g = b.p[i];
  wgrad3_body<false>(g, chunk, by, bz, A3, B3, nullptr);
}

__global__ void __launch_bounds__(512, 1) k_gemm_wgrad3p_batched(wgrad_batch_args b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_wb[];
  int prob, chunk, by, bz;
  wgrad_batch_locate(b, blockIdx.x, prob, chunk, by, bz);
  wgrad_args g = b.p[0];
#pragma unroll
  for (int i = 1; i < WGRAD_MAX_BATCH; ++i)
    if (i == prob) g = b.p[i];
  wgrad3p_body(g, chunk, by, bz, lds_wb);
}

// The descriptor of one whole-range weight gradient (callers set rows_per_block and, grouped, the class fields).
static wgrad_args wgrad_args_of(const gnx_handle* h, const gnx_wgrad_prob& q) {
  wgrad_args g = {};
  g.X = q.dC;
  g.ldx = q.lddc;
  g.Y = q.A;
  g.ldy = q.lda;
  g.rs = q.rowscale;
  g.M = q.M;
  g.N = q.N;
  g.K = q.K;
  g.dW = q.dW;
  g.lddw = q.lddw;
  g.dbias = q.dbias;
  g.vec_x = aligned16(q.dC) && (q.lddc % 4 == 0);
  g.vec_y = aligned16(q.A) && (q.lda % 4 == 0);
  g.zero = h->d_zero;
  return g;
}

static bool wgrad_split_enabled(const gnx_handle* h, int64_t M, bool any_rowscale) {
  return wgrad_plan_split_enabled(h->opt, M, any_rowscale);
}

static int32_t wgrad_launch(gnx_handle* h, const float* dC, int64_t lddc, const float* A, int64_t lda,
                            const float* rowscale, int64_t M, int32_t N, int32_t K, float* dW, int64_t lddw,
                            float* dbias, const int32_t* row_index, const int32_t* chunk_info, const int32_t* nchunks,
                            int64_t max_chunks, int64_t dw_cls_stride) {
  GNX_CHECK_ARG(h && dC && A && dW, "gnx_gemm_wgrad: NULL argument");
  GNX_CHECK_ARG(M >= 0 && N > 0 && K > 0 && lddc >= N && lda >= K && lddw >= K, "gnx_gemm_wgrad: bad shape");
  if (M == 0) return GNX_OK;
  wgrad_args g = wgrad_args_of(h, gnx_wgrad_prob{dC, lddc, A, lda, rowscale, dW, lddw, dbias, M, N, K});
  int64_t tiles = gnx_cdiv(N, BN) * gnx_cdiv(K, BN);
  // aim for ~512 workgroups; at least 128 rows each (4 K-steps) so the atomic flush stays amortised
  // default: one workgroup per CU.  Measured on cfg-2 (tools/ab_bench.py, same box): 512 / 1024 workgroups cost 0.4 ms
  // per step more -- every workgroup flushes its 128 x 128 partial sum with fp32 atomics, and a weight-gradient launch
  // that fills every CU slot starves the input-gradient chain it overlaps with on the main stream.
  const int64_t target_wgs = h->opt[GNX_OPT_WGRAD_WGS] > 0 ? h->opt[GNX_OPT_WGRAD_WGS] : (h->num_cus > 0 ? h->num_cus : 256);
  int64_t chunks = gnx_cdiv(target_wgs, tiles);
  int64_t rows = gnx_cdiv(gnx_cdiv(M, chunks), BK) * BK;
  if (rows < 128) rows = 128;
  g.rows_per_block = rows;
  g.row_index = row_index;
  g.chunk_info = chunk_info;
  g.nchunks = nchunks;
  g.dw_cls_stride = dw_cls_stride;
  dim3 grid((unsigned)(chunk_info ? max_chunks : gnx_cdiv(M, rows)), (unsigned)gnx_cdiv(N, BN), (unsigned)gnx_cdiv(K, BN));
  const bool vec = g.vec_x && g.vec_y && (N % 4 == 0) && (K % 4 == 0);
  const bool offs32 = (uint64_t)M * (uint64_t)lddc < (1ull << 32) && (uint64_t)M * (uint64_t)lda < (1ull << 32);
  const bool wsplit = wgrad_split_enabled(h, M, rowscale != nullptr) && (!chunk_info || offs32);
  const double wfl = 2.0 * (double)M * N * K;
  gnx_prof_scope prof(h, GNX_K_GEMM_WGRAD, 4.0 * M * ((double)N + K) + 4.0 * N * K, wfl, wsplit ? 6.0 * wfl : 0.0);
  // (short row ranges -- the readout's 4096-row problems -- keep the two-barrier kernel: 14.7 vs 24 us)
  wgrad_grouped_plan p = {};
  if (chunk_info) p = wgrad_grouped_plan_of(dC, lddc, A, lda, M, N, K, max_chunks, h->opt);
  if (p.kernel == GNX_WGRAD_KERNEL_SPLIT3P_GROUPED) {
    // Per-class gradient over merged class runs, at most WGRAD_GROUPED_WGS workgroups (ranges x output tiles).  Measured
    // on one MI355X, builds alternating (profiles/wgrad_grouped_pipe_ab.json; cfg-2: 82 chunks in a table of 85, K = 512):
    //   budget   grid      alone (tools/wgrad_ab.py | single-stream trace)   cfg-2 step   cfg-5 step
    //   k_gemm_wgrad3<true>  85 x 4      107.9 | 122.4 us                       6.397 ms     55.97 ms
    //       64   15 x 4, S = 6           241.6 us                               6.565        57.60
    //      128   29 x 4, S = 3           127.3 | 136.5 us                       6.322        55.34
    //      256   43 x 4, S = 2            93.8 | 104.6 us                       6.320        55.19
    // A workgroup takes 1.3 - 1.5 us per 32-row step whatever the budget, so alone the launch is as fast as it has
    // workgroups; at 128 it is slower alone than the kernel it replaces and the step is still faster, because it leaves
    // the CUs to the main stream.  256 is the default: same cfg-2 step as 128, faster alone and at cfg-5.
    grid.x = p.grid_x;
    GNX_HIP(gnx_raise_lds_limit<&k_gemm_wgrad3p_grouped>((int)WG3G_LDS));
    hipLaunchKernelGGL(k_gemm_wgrad3p_grouped, grid, dim3(512), WG3G_LDS, h->stream,
                       wgrad_grouped_args{g, p.chunks_per_range, (int)max_chunks});
  } else if (wsplit && vec && !chunk_info && rows >= 512 && h->opt[GNX_OPT_WGRAD_PIPE] != 0) {
    GNX_HIP(gnx_raise_lds_limit<&k_gemm_wgrad3p>((int)WG3P_LDS));
    hipLaunchKernelGGL(k_gemm_wgrad3p, grid, dim3(512), WG3P_LDS, h->stream, g);
  } else if (wsplit) {
    if (chunk_info)
      hipLaunchKernelGGL((k_gemm_wgrad3<true>), grid, dim3(256), 0, h->stream, g);
    else
      hipLaunchKernelGGL((k_gemm_wgrad3<false>), grid, dim3(256), 0, h->stream, g);
  } else if (chunk_info) {
    if (vec)
      hipLaunchKernelGGL((k_gemm_wgrad<true, true>), grid, dim3(256), 0, h->stream, g);
    else
      hipLaunchKernelGGL((k_gemm_wgrad<false, true>), grid, dim3(256), 0, h->stream, g);
  } else {
    if (vec)
      hipLaunchKernelGGL((k_gemm_wgrad<true, false>), grid, dim3(256), 0, h->stream, g);
    else
      hipLaunchKernelGGL((k_gemm_wgrad<false, false>), grid, dim3(256), 0, h->stream, g);
  }
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_gemm_wgrad(gnx_handle* h, const float* dC, int64_t lddc, const float* A, int64_t lda,
                                  const float* rowscale, int64_t M, int32_t N, int32_t K, float* dW, int64_t lddw,
                                  float* dbias) {
  return wgrad_launch(h, dC, lddc, A, lda, rowscale, M, N, K, dW, lddw, dbias, nullptr, nullptr, nullptr, 0, 0);
}

extern "C" int32_t gnx_gemm_wgrad_grouped(gnx_handle* h, const float* dC, int64_t lddc, const float* A, int64_t lda,
                                          int64_t M, int32_t N, int32_t K, float* dW_cls, int64_t lddw,
                                          int64_t dw_cls_stride, const int32_t* row_index, const int32_t* chunk_info,
                                          const int32_t* nchunks, int64_t max_chunks) {
  GNX_CHECK_ARG(row_index && chunk_info && nchunks && max_chunks > 0, "gnx_gemm_wgrad_grouped: NULL argument");
  return wgrad_launch(h, dC, lddc, A, lda, nullptr, M, N, K, dW_cls, lddw, nullptr, row_index, chunk_info, nchunks,
                      max_chunks, dw_cls_stride);
}

extern "C" int32_t gnx_gemm_wgrad_grouped_plan(gnx_handle* h, int64_t lddc, int64_t lda, const float* dC, const float* A,
                                               int64_t M, int32_t N, int32_t K, int64_t max_chunks,
                                               gnx_wgrad_grouped_plan_info* out) {
  GNX_CHECK_ARG(h && dC && A && out && max_chunks > 0, "gnx_gemm_wgrad_grouped_plan: NULL argument");
  GNX_CHECK_ARG(M >= 0 && N > 0 && K > 0 && lddc >= N && lda >= K, "gnx_gemm_wgrad_grouped_plan: bad shape");
  const wgrad_grouped_plan p = wgrad_grouped_plan_of(dC, lddc, A, lda, M, N, K, max_chunks, h->opt);
  const bool pipe = p.kernel == GNX_WGRAD_KERNEL_SPLIT3P_GROUPED;
  *out = gnx_wgrad_grouped_plan_info{p.kernel,
                                     p.ranges,
                                     p.chunks_per_range,
                                     p.kernel == GNX_WGRAD_KERNEL_NONE ? 0u : p.grid_x,
                                     (uint32_t)gnx_cdiv(N, BN),
                                     (uint32_t)gnx_cdiv(K, BN),
                                     pipe ? 512u : 256u};
  return GNX_OK;
}

extern "C" int32_t gnx_gemm_wgrad_batched(gnx_handle* h, int32_t nprob, const gnx_wgrad_prob* probs) {
  GNX_CHECK_ARG(h && probs && nprob >= 1 && nprob <= WGRAD_MAX_BATCH, "gnx_gemm_wgrad_batched: nprob must be in [1,%d]",
                WGRAD_MAX_BATCH);
  wgrad_batch_args b;
  int64_t maxM = 0;
  int maxN = 0, maxK = 0;
  for (int i = 0; i < nprob; ++i) {
    const gnx_wgrad_prob& q = probs[i];
    GNX_CHECK_ARG(q.dC && q.A && q.dW && q.M >= 0 && q.N > 0 && q.K > 0 && q.lddc >= q.N && q.lda >= q.K && q.lddw >= q.K,
                  "gnx_gemm_wgrad_batched: problem %d: bad argument", i);
    b.p[i] = wgrad_args_of(h, q);
    GNX_CHECK_ARG(b.p[i].vec_x && b.p[i].vec_y && (q.N % 4 == 0) && (q.K % 4 == 0),
                  "gnx_gemm_wgrad_batched: problem %d is not 16-byte aligned / multiple-of-4 shaped", i);
    if (q.M > maxM) maxM = q.M;
    if (q.N > maxN) maxN = q.N;
    if (q.K > maxK) maxK = q.K;
  }
  for (int i = nprob; i < WGRAD_MAX_BATCH; ++i) b.p[i] = b.p[0];
  if (maxM == 0) return GNX_OK;
  // ~1024 workgroups in total, shared out by work (rows x output tiles); every chunk is a multiple of 32 rows
  double total_cost = 0.0;
  for (int i = 0; i < nprob; ++i)
    total_cost += (double)b.p[i].M * (double)(gnx_cdiv(b.p[i].N, BN) * gnx_cdiv(b.p[i].K, BN));
  int off = 0;
  for (int i = 0; i < WGRAD_MAX_BATCH; ++i) {
    b.wg_off[i] = off;
    b.tiles[i] = 1;
    b.tiles_k[i] = 1;
    if (i >= nprob) continue;
    const int tn = (int)gnx_cdiv(b.p[i].N, BN), tk = (int)gnx_cdiv(b.p[i].K, BN);
    const int64_t M = b.p[i].M > 0 ? b.p[i].M : 1;
    // workgroups of the launch: at most one per CU, and at least ~5120 rows of a 128 x 128 output tile each (every
    // workgroup ends with a 64 KB fp32 atomic flush and, on its CU, displaces the main stream's workgroups: at cfg-2's
    // 650 k row-tiles per layer 160 workgroups beat 256 by 1.7 % of the step in round 2; with round 3's shorter main
    // stream 128 beat 160 / 96 / 192 / 256: 6.765 vs 6.836 / 6.932 / 6.880 / 6.880 ms; at cfg-3/4/5's sizes 256 are best)
    const double cus_d = (double)(h->num_cus > 0 ? h->num_cus : 256);
    double auto_budget = total_cost / 5120.0;
    auto_budget = auto_budget < cus_d / 4 ? cus_d / 4 : (auto_budget > cus_d ? cus_d : auto_budget);
    const double budget = h->opt[GNX_OPT_WGRAD_WGS] > 0 ? (double)h->opt[GNX_OPT_WGRAD_WGS] : auto_budget;
    int64_t chunks = (int64_t)(budget * ((double)M * tn * tk / total_cost) / (tn * tk) + 0.5);
    const int64_t max_chunks = gnx_cdiv(M, 128);
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks < 1) chunks = 1;
    const int64_t rows = gnx_cdiv(gnx_cdiv(M, chunks), BK) * BK;
    chunks = gnx_cdiv(M, rows);  // no empty chunks
    b.p[i].rows_per_block = rows;
    b.tiles[i] = tn * tk;
    b.tiles_k[i] = tk;
    off += (int)chunks * tn * tk;
  }
  b.wg_off[WGRAD_MAX_BATCH] = off;
  for (int i = nprob; i < WGRAD_MAX_BATCH; ++i) b.wg_off[i] = off;
  b.nprob = nprob;
  dim3 grid((unsigned)off);
  bool any_rs = false;
  for (int i = 0; i < nprob; ++i) any_rs = any_rs || probs[i].rowscale != nullptr;
  double wby = 0.0, wfl = 0.0;
  for (int i = 0; i < nprob; ++i) {
    wby += 4.0 * probs[i].M * ((double)probs[i].N + probs[i].K) + 4.0 * probs[i].N * probs[i].K;
    wfl += 2.0 * (double)probs[i].M * probs[i].N * probs[i].K;
  }
  gnx_prof_scope prof(h, GNX_K_GEMM_WGRAD_BATCHED, wby, wfl, wgrad_split_enabled(h, maxM, any_rs) ? 6.0 * wfl : 0.0);
  if (wgrad_split_enabled(h, maxM, any_rs) && h->opt[GNX_OPT_WGRAD_PIPE] != 0) {
    GNX_HIP(gnx_raise_lds_limit<&k_gemm_wgrad3p_batched>((int)WG3P_LDS));
    hipLaunchKernelGGL(k_gemm_wgrad3p_batched, grid, dim3(512), WG3P_LDS, h->stream, b);
  } else if (wgrad_split_enabled(h, maxM, any_rs))
    hipLaunchKernelGGL(k_gemm_wgrad3_batched, grid, dim3(256), 0, h->stream, b);
  else
    hipLaunchKernelGGL(k_gemm_wgrad_batched, grid, dim3(256), 0, h->stream, b);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}
