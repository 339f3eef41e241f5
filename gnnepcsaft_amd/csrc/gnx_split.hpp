// Device pieces shared by the products (gnx_gemm.hip), the weight gradients (gnx_wgrad.hip), the embedding backward
// (gnx_embed.hip) and the fused edge kernels (gnx_fused.hip): the tile geometry and loads of the fp32 products, and the
// split-operand helpers -- an fp32 value written EXACTLY as the sum of three bf16 pieces (see the notes at k_gemm_ws3) and
// the MFMA sequence that multiplies two such values.
#pragma once
#include "gnx_common.hpp"

// 128 x 128 output tiles, 32-deep K-tiles (LDS images: see the top of gnx_gemm.hip)
#define BM 128
#define BN 128
#define BK 32
#define LDK 36    // row stride of the row-k image
#define LDN 128   // row stride of the k-row image

__device__ __forceinline__ f32x4 ld4(const float* p, bool vec, int valid) {
  // valid = number of in-range elements (0..4) starting at p
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (valid >= 4 && vec) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
    if (valid > 0) v.x = p[0];
    if (valid > 1) v.y = p[1];
    if (valid > 2) v.z = p[2];
    if (valid > 3) v.w = p[3];
  }
  return v;
}

// Row scale of segments that have none (pointer-select, no branch).  A __device__ (global address space) variable on
// purpose: selecting between a kernel-argument pointer and a __constant__ address yields a GENERIC pointer, i.e. a
// flat_load, and one outstanding flat load turns every counted s_waitcnt vmcnt(N) of the loop into vmcnt(0).  `inline`:
// one definition for all translation units that use them, still writable (a `static` one could be folded to a constant).
inline __device__ float c_one = 1.0f;
inline __device__ __attribute__((aligned(16))) float c_zero4[4] = {0.f, 0.f, 0.f, 0.f};

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
#define W3_BM 64
#define W3_LDB 272                    // bytes per row of one bf16 image
#define W3_PIECE (W3_BM * W3_LDB)     // 17408 B
#define W3_BUF (3 * W3_PIECE)         // 52224 B

// bf16 images of a 128 x 32 K-tile (k_gemm3, the split weight gradients)
#define G3_LDB 80                   // bytes per image row
#define G3_PIECE (128 * G3_LDB)     // 10240 B: one bf16 image of a 128 x 32 K-tile
#define G3_OP (3 * G3_PIECE)        // the three images of one operand

// Two elements at a time: ONE v_cvt_pk_bf16_f32 per pair and piece, the piece's fp32 value taken out of the packed word by a
// shift (low half) / a mask (high half): 46 VALU instructions per 8 elements.  The element-wise form compiled to 62 (a
// conversion per element plus packing moves), and with the SLP vectoriser on to 44 that contain packed-f32 subtractions,
// which issue badly beside MFMAs (build.py).  Same roundings either way (round-to-nearest-even pieces, exact remainders).
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float split_f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned split_u32x4;
__device__ __forceinline__ void split3(const float (&x)[8], bf16x8& p1, bf16x8& p2, bf16x8& p3) {
  split_u32x4 w1, w2, w3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const split_f32x2 v = {x[2 * q], x[2 * q + 1]};
    const unsigned u1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    const split_f32x2 r1 = {v.x - __builtin_bit_cast(float, u1 << 16), v.y - __builtin_bit_cast(float, u1 & 0xFFFF0000u)};
    const unsigned u2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
    const split_f32x2 r2 = {r1.x - __builtin_bit_cast(float, u2 << 16), r1.y - __builtin_bit_cast(float, u2 & 0xFFFF0000u)};
    w1[q] = u1;
    w2[q] = u2;
    w3[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
  }
  p1 = __builtin_bit_cast(bf16x8, w1);
  p2 = __builtin_bit_cast(bf16x8, w2);
  p3 = __builtin_bit_cast(bf16x8, w3);
}

// One 16-deep slab of the split-operand product (a[p], b[p] = piece p of split3; the three terms below the fp32 rounding
// are dropped, see k_gemm_ws3): six bf16 MFMAs into one accumulator, the smallest terms first.
__device__ __forceinline__ void mfma_3x3(f32x16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}
