// Which kernel a per-degree-class weight gradient (gnx_gemm_wgrad_grouped) takes and how k_gemm_wgrad3p_grouped shares out
// the chunk table, decided on the host without HIP: wgrad_launch (gnx_wgrad.hip) launches from it and
// gnx_gemm_wgrad_grouped_plan returns its fields.  Plain C++17 so that tests/wgrad_grouped_plan_probe.cpp can pin it on a
// machine without a GPU.  Pointers are looked at for 16-byte alignment only.
#pragma once
#include <cstdint>

#include "gnx.h"

constexpr int64_t WGRAD_PLAN_BN = 128;            // dW tile (gnx_wgrad.hip asserts it against BN)
constexpr int64_t WGRAD_SPLIT_MIN_ROWS = 4096;    // below it the fp32-MFMA kernels run
// Workgroup budget of k_gemm_wgrad3p_grouped when GNX_OPT_WGRAD_WGS is 0 (the measured table is at its launch).
constexpr int64_t WGRAD_GROUPED_WGS = 256;

struct wgrad_grouped_plan {
  int kernel = GNX_WGRAD_KERNEL_NONE;  // GNX_WGRAD_KERNEL_*
  int ranges = 1;                      // max(1, budget / output tiles)
  int chunks_per_range = 1;            // S = ceil(max_chunks / ranges)
  unsigned grid_x = 0;                 // ceil(max_chunks / S) <= ranges (k_gemm_wgrad3p_grouped), else max_chunks
};

static inline int64_t wgrad_plan_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool wgrad_plan_vec(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

// the split-operand weight-gradient kernels take over for large row counts (GNX_GEMM_SPLIT=0: fp32 MFMA everywhere)
static inline bool wgrad_plan_split_enabled(const int* opt, int64_t M, bool any_rowscale) {
  if (any_rowscale || M < WGRAD_SPLIT_MIN_ROWS) return false;
  return opt[GNX_OPT_GEMM_SPLIT] != 0;
}

// Arguments as gnx_gemm_wgrad_grouped's, checked by the caller (max_chunks > 0); opt = gnx_handle::opt.
static inline wgrad_grouped_plan wgrad_grouped_plan_of(const float* dC, int64_t lddc, const float* A, int64_t lda, int64_t M,
                                                       int32_t N, int32_t K, int64_t max_chunks, const int* opt) {
  const bool vec = wgrad_plan_vec(dC, lddc) && wgrad_plan_vec(A, lda) && N % 4 == 0 && K % 4 == 0;
  // the grouped split kernels keep row * ld in 32 bits
  const bool offs32 = (uint64_t)M * (uint64_t)lddc < (1ull << 32) && (uint64_t)M * (uint64_t)lda < (1ull << 32);
  const bool wsplit = wgrad_plan_split_enabled(opt, M, false) && offs32;
  const int64_t tiles = wgrad_plan_cdiv(N, WGRAD_PLAN_BN) * wgrad_plan_cdiv(K, WGRAD_PLAN_BN);
  const int64_t budget = opt[GNX_OPT_WGRAD_WGS] > 0 ? opt[GNX_OPT_WGRAD_WGS] : WGRAD_GROUPED_WGS;
  wgrad_grouped_plan p;
  p.ranges = (int)(budget / tiles > 1 ? budget / tiles : 1);
  p.chunks_per_range = (int)wgrad_plan_cdiv(max_chunks, p.ranges);
  if (M == 0)
    p.kernel = GNX_WGRAD_KERNEL_NONE;
  else if (wsplit && vec && opt[GNX_OPT_WGRAD_PIPE] != 0)
    p.kernel = GNX_WGRAD_KERNEL_SPLIT3P_GROUPED;
  else if (wsplit)
    p.kernel = GNX_WGRAD_KERNEL_SPLIT3;
  else
    p.kernel = vec ? GNX_WGRAD_KERNEL_F32_VEC : GNX_WGRAD_KERNEL_F32_GENERIC;
  if (p.kernel == GNX_WGRAD_KERNEL_SPLIT3P_GROUPED)
    p.grid_x = (unsigned)wgrad_plan_cdiv(max_chunks, p.chunks_per_range);
  else if (p.kernel != GNX_WGRAD_KERNEL_NONE)
    p.grid_x = (unsigned)max_chunks;
  return p;
}
