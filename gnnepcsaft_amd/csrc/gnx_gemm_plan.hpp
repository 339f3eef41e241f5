// Which kernel a gnx_gemm / gnx_gemm_grouped / gnx_gemm_grouped_rows call takes, decided ONCE, on the host, without HIP:
// gemm_plan_of() turns a call's arguments into a gemm_plan, gemm_launch (gnx_gemm.hip) checks the arguments, asks for the
// plan and launches from it, and gnx_gemm_workspace_bytes / gnx_gemm_tile_rows / gnx_gemm_plan return its fields.  Plain
// C++17 so that tests/gemm_plan_probe.cpp can pin the decision table on a machine without a GPU.  Pointers are looked at
// for NULL-ness and 16-byte alignment only.  No heap use: this runs once per product, > 100 times per step.
//
// The decision table, in the order gemm_plan_of takes it, is in DESIGN.md section 4 ("Which product kernel a call takes").
#pragma once
#include <cstddef>
#include <cstdint>

#include "gnx.h"

// Tile geometry the decision depends on; gnx_gemm.hip asserts every value against the kernels' own constants.
constexpr int PLAN_MAX_SEGS = 4;
constexpr int PLAN_BM = 128, PLAN_BN = 128, PLAN_BK = 32;  // tiled kernels
constexpr int PLAN_WS_BM = 64;                             // k_gemm_ws, k_gemm_ws3 with 8 waves (4 waves: half of it)
constexpr size_t PLAN_WS_LDS = 4 * (128 * 132 + 2 * 64 * 132);  // k_gemm_ws: the weight image and two A tiles, row stride 132
constexpr size_t PLAN_WS3_LDS8 = 2 * 3 * 64 * 272;         // k_gemm_ws3, 8 waves: two stages of three bf16 images of a tile
constexpr size_t PLAN_WS3_LDS4 = 64 * 1024;                // 4 waves: at least what the NN weight staging image needs
constexpr int PLAN_G3P_MIN_KTILES = 8;
constexpr size_t plan_g3p_lds(int mi) { return (size_t)(2 * 3 * 32 * mi * 80 + 2 * 32 * mi * 4); }
constexpr int PLAN_AS_BM = 64;
constexpr size_t PLAN_AS_LDS = 3 * 64 * 272 + 2 * 64 * 4;
constexpr int PLAN_PATCH = 16;           // k_gemm_mid and k_gemm_small_batched: 16 x 16 outputs per workgroup
constexpr int PLAN_WGS_PER_CU = 2;       // persistent workgroups of k_gemm3 / k_gemm3p
constexpr int64_t PLAN_SPLIT_MIN_ROWS = 4096, PLAN_WS_MIN_ROWS = 8192;

enum { PLAN_EPI_PLAIN = 0, PLAN_EPI_ACCUM = 1, PLAN_EPI_MASK = 2 };

struct gemm_plan {
  int kernel = GNX_GEMM_KERNEL_NONE;  // GNX_GEMM_KERNEL_*: with stop_after_split, the kernel the images are for
  bool bt = false;
  int epi = PLAN_EPI_PLAIN;
  unsigned grid_x = 0, grid_y = 1, block = 256;
  size_t lds = 0;          // dynamic LDS bytes
  int tile_rows = 0;       // rows per workgroup tile
  int row_tiles = 0;       // ws_args.ntiles (weights-stationary kernels)
  int ny = 1;              // column tiles of 128
  size_t image_bytes = 0;  // what gnx_gemm_workspace_bytes answers (whether or not this call brought a workspace)
  bool images = false;     // the kernel reads split weight images: image_bytes > 0 and a workspace
  int Npad = 0, Kpad = 0, koff[PLAN_MAX_SEGS + 1] = {0, 0, 0, 0, 0}, frag = 0, classes = 1;
  bool run_split = false;         // launch k_split_weights first (images, and not GNX_GEMM_PRESPLIT)
  bool stop_after_split = false;  // GNX_GEMM_SPLIT_ONLY
  int prof_id = GNX_K_NONE;
  double bytes = 0.0, flops = 0.0, mfma = 0.0;
};

static inline int64_t plan_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool plan_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool plan_vec_a(const gnx_gemm_seg& s) { return plan_aligned16(s.a) && s.lda % 4 == 0; }
static inline bool plan_vec_b(const gnx_gemm_seg& s, int64_t cls_stride) {
  return plan_aligned16(s.b) && s.ldb % 4 == 0 && cls_stride % 4 == 0;
}
static inline int plan_kpad(int64_t k) { return (int)(plan_cdiv(k, PLAN_BK) * PLAN_BK); }

// Bytes of the split weight images of `classes` weight sets with N columns and kpad = sum of plan_kpad(k) over the
// segments: N padded to 128, three bf16 pieces.
static inline size_t gemm_plan_image_bytes(int64_t classes, int64_t N, int64_t kpad) {
  return (size_t)((classes > 0 ? classes : 1) * 3 * (plan_cdiv(N, PLAN_BN) * PLAN_BN) * kpad) * 2;
}

// Row-tile height of the pipelined tiled product for M rows x N columns: 96 where that shortens the longest workgroup's
// walk (rounds x tile height; persistent workgroups, PLAN_WGS_PER_CU per CU), else 128 (ties keep 128, the most measured
// shape).  forced = GNX_OPT_GEMM_TILE_ROWS.
static inline int gemm_plan_tile_rows(int64_t M, int32_t N, int forced, int cus) {
  if (forced == 96 || forced == 128) return forced;
  const int64_t ny = plan_cdiv(N, PLAN_BN), slots = (int64_t)PLAN_WGS_PER_CU * cus;
  const int64_t c128 = plan_cdiv(plan_cdiv(M, 128) * ny, slots) * 128, c96 = plan_cdiv(plan_cdiv(M, 96) * ny, slots) * 96;
  return c96 < c128 ? 96 : 128;
}

// Workgroups of k_gemm3 / k_gemm3p for row_tiles x ny tiles: PLAN_WGS_PER_CU per CU at the most, a multiple of 8 * ny
// (the XCD-aware tile walk needs it).
static inline unsigned gemm_plan_persistent_grid(int64_t row_tiles, unsigned ny, int cus) {
  const unsigned unit = 8u * ny, all = (unsigned)(plan_cdiv(row_tiles, 8) * unit);
  unsigned slots = (unsigned)(PLAN_WGS_PER_CU * cus) / unit * unit;
  if (slots < unit) slots = unit;
  return all > slots ? slots : all;
}

// Arguments as gemm_launch's (tile_info == NULL: an ungrouped call; ws is the caller's workspace or NULL); opt =
// gnx_handle::opt, num_cus <= 0 counts as 256.  The arguments have passed gemm_launch's checks.
static inline gemm_plan gemm_plan_of(int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides, int32_t num_classes,
                                     int64_t M, int32_t N, const float* bias, const float* mask, int64_t ldmask, const float* C,
                                     int64_t ldc, int32_t flags, const int32_t* tile_info, int64_t max_tiles, const void* ws,
                                     int32_t tile_rows, const int* opt, int num_cus) {
  gemm_plan p;
  p.bt = (flags & GNX_GEMM_B_TRANS) != 0;
  const bool accumulate = (flags & GNX_GEMM_ACCUMULATE) != 0;
  p.epi = mask ? PLAN_EPI_MASK : (accumulate ? PLAN_EPI_ACCUM : PLAN_EPI_PLAIN);
  if (M == 0) return p;
  const int cus = num_cus > 0 ? num_cus : 256;
  const bool grouped = tile_info != nullptr, split_only = (flags & GNX_GEMM_SPLIT_ONLY) != 0;
  const bool out_aligned = plan_aligned16(C) && ldc % 4 == 0 && (mask == nullptr || (plan_aligned16(mask) && ldmask % 4 == 0));
  double ktot = 0.0;
  for (int s = 0; s < nseg; ++s) ktot += segs[s].k;
  p.flops = 2.0 * (double)M * N * ktot;
  const double io = 4.0 * M * (ktot + N), rmw = (mask || accumulate) ? 4.0 * M * N : 0.0;

  // The weights-stationary shape: one segment with M >= 8192, 32 <= K, N <= 128 (multiples of 4), aligned operands, no row
  // scale and not mask + accumulate (ungrouped calls only).
  const gnx_gemm_seg& s0 = segs[0];
  if (!grouped && nseg == 1 && M >= PLAN_WS_MIN_ROWS && s0.rowscale == nullptr && s0.k >= 32 && s0.k <= 128 && N >= 32 &&
      N <= 128 && s0.k % 4 == 0 && N % 4 == 0 && plan_vec_a(s0) && plan_vec_b(s0, 0) && !(mask != nullptr && accumulate)) {
    if (split_only) return p;  // (the weights live in registers or LDS there: no images)
    const bool split = opt[GNX_OPT_GEMM_SPLIT] != 0;
    const int fast = (split && p.epi != PLAN_EPI_ACCUM && N == 128 && out_aligned) ? opt[GNX_OPT_GEMM_WS_FAST] : 0;
    p.kernel = !split ? GNX_GEMM_KERNEL_WS : fast == 2 ? GNX_GEMM_KERNEL_WS3_FAST4 : fast ? GNX_GEMM_KERNEL_WS3_FAST8 : GNX_GEMM_KERNEL_WS3;
    const int waves = fast == 2 ? 4 : 8;
    p.tile_rows = PLAN_WS_BM * waves / 8;
    p.row_tiles = (int)plan_cdiv(M, p.tile_rows);
    const int wgs = cus * (8 / waves);
    p.grid_x = (unsigned)(p.row_tiles < wgs ? p.row_tiles : wgs);
    p.block = 64u * waves;
    p.lds = !split ? PLAN_WS_LDS : waves == 4 ? PLAN_WS3_LDS4 : PLAN_WS3_LDS8;
    p.prof_id = GNX_K_GEMM_WS;
    p.bytes = io + rmw + 4.0 * N * ktot;
    p.mfma = split ? 6.0 * p.flops : 0.0;
    return p;
  }
  if (split_only && M < PLAN_SPLIT_MIN_ROWS) return p;  // (no split path below 4096 rows)
  if (!grouped && nseg == 1 && M <= 256 && mask == nullptr && segs[0].rowscale == nullptr && opt[GNX_OPT_GEMM_MID] == 0) {
    // (k_gemm_mid computes the same k-ordered chain with 16-byte staging loads and the next chunk prefetched: 3-4 us
    // instead of 7-10 us for a 20-row product)
    p.kernel = GNX_GEMM_KERNEL_SMALL;
    p.tile_rows = PLAN_PATCH;
    p.grid_x = (unsigned)(plan_cdiv(M, PLAN_PATCH) * plan_cdiv(N, PLAN_PATCH));
    p.prof_id = GNX_K_GEMM_SMALL;
    p.bytes = 4.0 * ((double)M * (segs[0].k + N) + (double)N * segs[0].k);
    return p;
  }
  p.ny = (int)plan_cdiv(N, PLAN_BN);
  if (opt[GNX_OPT_GEMM_MID] != 0 && M < PLAN_SPLIT_MIN_ROWS && plan_cdiv(M, PLAN_BM) * p.ny <= 48) {
    // few 128 x 128 tiles: 16 x 16 patches on many workgroups instead (a grouped call's max_tiles is an upper bound with
    // one partial tile per class, so the row count decides; every 128-row tile of its table is 8 patches high)
    p.kernel = GNX_GEMM_KERNEL_MID;
    p.tile_rows = PLAN_PATCH;
    p.grid_x = (unsigned)(grouped ? max_tiles * (PLAN_BM / PLAN_PATCH) : plan_cdiv(M, PLAN_PATCH));
    p.grid_y = (unsigned)plan_cdiv(N, PLAN_PATCH);
    p.prof_id = GNX_K_GEMM_SMALL;
    p.bytes = io + 4.0 * N * ktot;
    return p;
  }

  // Tiled kernels.  The split-operand ones (M >= 4096, >= 2 K-tiles, no row scale, aligned operands) read split weight
  // images from the caller's workspace; row-scaled segments (the 4-segment post-layer 0 of hub-heavy batches), odd shapes
  // and a call without a workspace stay on the exact-fp32 MFMA kernel.
  p.classes = num_classes > 0 ? num_classes : 1;
  bool vec = true, can_split = opt[GNX_OPT_GEMM_SPLIT] != 0 && M >= PLAN_SPLIT_MIN_ROWS;
  for (int s = 0; s < nseg; ++s) {
    const gnx_gemm_seg& in = segs[s];
    const bool aligned = plan_vec_a(in) && plan_vec_b(in, cls_strides ? cls_strides[s] : 0) && in.k % 4 == 0 && (p.bt || N % 4 == 0);
    vec = vec && aligned;
    can_split = can_split && aligned && in.rowscale == nullptr && in.k > 0;
    p.koff[s] = p.Kpad;
    p.Kpad += plan_kpad(in.k);
  }
  for (int s = nseg; s <= PLAN_MAX_SEGS; ++s) p.koff[s] = p.Kpad;
  p.Npad = p.ny * PLAN_BN;
  const int ktiles = p.Kpad / PLAN_BK;
  if (can_split && ktiles >= 2) p.image_bytes = gemm_plan_image_bytes(p.classes, N, p.Kpad);
  p.images = p.image_bytes > 0 && ws != nullptr;
  p.prof_id = GNX_K_GEMM_TILED;
  p.bytes = io + rmw + 4.0 * N * ktot * p.classes;
  p.mfma = p.images ? 6.0 * p.flops : 0.0;
  const int64_t row_tiles = grouped ? max_tiles : plan_cdiv(M, PLAN_BM);
  if (!p.images) {
    if (split_only) return p;  // (this call takes a kernel that needs no images)
    p.kernel = vec ? GNX_GEMM_KERNEL_TILED_VEC : GNX_GEMM_KERNEL_TILED_GENERIC;
    p.tile_rows = PLAN_BM;
    p.grid_x = (unsigned)row_tiles;
    p.grid_y = (unsigned)p.ny;
    return p;
  }
  p.run_split = (flags & GNX_GEMM_PRESPLIT) == 0;  // (else the caller ran this very split before: SPLIT_ONLY, same arguments)
  p.stop_after_split = split_only;
  const bool as3 = opt[GNX_OPT_GEMM_AS] != 0 && nseg == 1 && p.Kpad == 4 * PLAN_BK && N >= 2 * PLAN_BN && N % PLAN_BN == 0 &&
                   (double)M * (double)(ldc > ldmask ? ldc : ldmask) + (double)N < 1073741824.0 && out_aligned &&
                   (bias == nullptr || plan_aligned16(bias));
  const bool pipe = opt[GNX_OPT_GEMM_PIPE] != 0 && ktiles >= PLAN_G3P_MIN_KTILES;
  p.frag = (pipe || as3) ? 1 : 0;
  if (as3) {  // one 64-row tile per workgroup, all column tiles
    p.kernel = GNX_GEMM_KERNEL_AS3;
    p.tile_rows = PLAN_AS_BM;
    p.grid_x = (unsigned)(grouped ? max_tiles * (PLAN_BM / PLAN_AS_BM) : plan_cdiv(M, PLAN_AS_BM));
    p.lds = PLAN_AS_LDS;
  } else if (pipe) {  // tile height: a grouped call's is what its tile table was built with (the caller's, or 128)
    p.tile_rows = tile_rows ? tile_rows : grouped ? PLAN_BM : gemm_plan_tile_rows(M, N, opt[GNX_OPT_GEMM_TILE_ROWS], cus);
    p.kernel = p.tile_rows == 96 ? GNX_GEMM_KERNEL_GEMM3P_96 : GNX_GEMM_KERNEL_GEMM3P_128;
    p.grid_x = gemm_plan_persistent_grid(grouped ? row_tiles : plan_cdiv(M, p.tile_rows), (unsigned)p.ny, cus);
    p.lds = plan_g3p_lds(p.tile_rows / 32);
  } else {
    p.kernel = GNX_GEMM_KERNEL_GEMM3;
    p.tile_rows = PLAN_BM;
    p.grid_x = gemm_plan_persistent_grid(row_tiles, (unsigned)p.ny, cus);
  }
  return p;
}

// ---------------------------------------------------------------------------------------------------------------
// Split weight images as data: what a plan says about the images it reads, and what a split needs of the call.
// ---------------------------------------------------------------------------------------------------------------

// The record of a plan's images (gnx_gemm_image, gnx.h: it crosses the C ABI next to the image pointer).  Two calls whose
// records are equal read images of the same size and layout; image_bytes == 0: the call reads none.
static inline gnx_gemm_image gemm_image_of(const gemm_plan& p) {
  gnx_gemm_image r = {};
  if (p.image_bytes == 0) return r;
  r.image_bytes = p.image_bytes;
  r.classes = p.classes;
  r.Npad = p.Npad;
  r.Kpad = p.Kpad;
  for (int s = 0; s <= PLAN_MAX_SEGS; ++s) r.koff[s] = p.koff[s];
  r.frag = p.frag;
  r.bt = p.bt ? 1 : 0;
  return r;
}
static inline bool gemm_image_equal(const gnx_gemm_image& a, const gnx_gemm_image& b) {
  bool eq = a.image_bytes == b.image_bytes && a.classes == b.classes && a.Npad == b.Npad && a.Kpad == b.Kpad && a.frag == b.frag &&
            a.bt == b.bt;
  for (int s = 0; s <= PLAN_MAX_SEGS; ++s) eq = eq && a.koff[s] == b.koff[s];
  return eq;
}

// One problem of gnx_split_weights_batched (gnx_gemm.hip): the weights of a call whose plan has images, and where they go.
struct gemm_split_problem {
  const float* b[PLAN_MAX_SEGS];
  int64_t ldb[PLAN_MAX_SEGS], cls_stride[PLAN_MAX_SEGS];
  int32_t k[PLAN_MAX_SEGS];
  int32_t nseg, N, classes, frag, bt;
  void* out;
};
static inline gemm_split_problem gemm_split_problem_of(const gemm_plan& p, int32_t nseg, const gnx_gemm_seg* segs,
                                                       const int64_t* cls_strides, int32_t N, void* out) {
  gemm_split_problem q = {};
  for (int s = 0; s < nseg; ++s) {
    q.b[s] = segs[s].b;
    q.ldb[s] = segs[s].ldb;
    q.cls_stride[s] = cls_strides ? cls_strides[s] : 0;
    q.k[s] = segs[s].k;
  }
  q.nseg = nseg;
  q.N = N;
  q.classes = p.classes;
  q.frag = p.frag;
  q.bt = p.bt ? 1 : 0;
  q.out = out;
  return q;
}

// ---------------------------------------------------------------------------------------------------------------
// The three products of a PNAConv layer that read split weight images, as argument lists.  gnx_pna_conv_fwd / _bwd run
// them, gnx_pna_split_all plans them: both build them HERE, so they cannot disagree about what a product's weights are.
//   post-layer 0   z = x W0^T + A Weff(d)^T   grouped by degree class, [n][k] weights, N = F, K = F + 4F
//   dA             dA = g Weff(d)             grouped by degree class, [k][n] weights, N = 4F, K = F
//   dx             dx = g Wx + dP Wi + dQ Wj  three segments,          [k][n] weights, N = F, K = 3F
// P = the layer's parameter pointers (gnx_pna_bwd_args' order), t = the tower; operand / output pointers are the caller's.
// At split time only their alignment is looked at (pna_stand_in).
// ---------------------------------------------------------------------------------------------------------------
struct pna_product {
  int32_t nseg = 0;
  gnx_gemm_seg seg[3] = {};
  int64_t stride[3] = {0, 0, 0};
  bool grouped = false;
  int32_t classes = 1, N = 0, flags = 0, tile_rows = 0;  // tile_rows != 0: gnx_gemm_grouped_rows
  const float* bias = nullptr;
  float* C = nullptr;
  int64_t ldc = 0;
};

static inline gnx_gemm_seg pna_seg(const float* a, int64_t lda, const float* b, int64_t ldb, int32_t k) {
  gnx_gemm_seg s;
  s.a = a;
  s.lda = lda;
  s.rowscale = nullptr;
  s.b = b;
  s.ldb = ldb;
  s.k = k;
  s._pad = 0;
  return s;
}

// a 256-byte aligned address that is never dereferenced: stands in for an activation when only the weights are known
static inline float* pna_stand_in() { return reinterpret_cast<float*>(static_cast<uintptr_t>(1) << 20); }

static inline pna_product pna_post0_product(const float* const* P, const float* weff_t, int T, int F, int pre, int post, int D,
                                            int t, const float* x, const float* A, float* z0, int tile_rows) {
  const int H = T * F, k = 4 + t * 2 * (pre + post) + 2 * pre;
  pna_product q;
  q.nseg = 2;
  q.seg[0] = pna_seg(x + t * F, H, P[k], 13 * F, F);
  q.seg[1] = pna_seg(A + (int64_t)t * 4 * F, (int64_t)T * 4 * F, weff_t, 4 * F, 4 * F);
  q.stride[1] = (int64_t)4 * F * F;
  q.grouped = true;
  q.classes = D;
  q.N = F;
  q.flags = GNX_GEMM_B_TRANS | (post > 1 ? GNX_GEMM_RELU : 0);
  q.tile_rows = tile_rows == 96 ? 96 : 128;
  q.bias = P[k + 1];
  q.C = z0 + t * F;
  q.ldc = H;
  return q;
}

static inline pna_product pna_dA_product(const float* weff_t, int T, int F, int D, int t, const float* g, float* dA) {
  pna_product q;
  q.nseg = 1;
  q.seg[0] = pna_seg(g + t * F, (int64_t)T * F, weff_t, 4 * F, F);
  q.stride[0] = (int64_t)4 * F * F;
  q.grouped = true;
  q.classes = D;
  q.N = 4 * F;
  q.C = dA + (int64_t)t * 4 * F;
  q.ldc = (int64_t)T * 4 * F;
  return q;
}

static inline pna_product pna_dx_product(const float* const* P, int T, int F, int pre, int post, int t, const float* g_post0,
                                         const float* dP, const float* dQ, float* dx) {
  const int H = T * F, k0 = 4 + t * 2 * (pre + post), kp = k0 + 2 * pre;
  pna_product q;
  q.nseg = 3;
  q.seg[0] = pna_seg(g_post0 + t * F, H, P[kp], 13 * F, F);
  q.seg[1] = pna_seg(dP + t * F, H, P[k0], 3 * F, F);
  q.seg[2] = pna_seg(dQ + t * F, H, P[k0] + F, 3 * F, F);
  q.N = F;
  q.C = dx + t * F;
  q.ldc = H;
  return q;
}

// The plan of such a product over M rows: what gemm_launch computes for pna_product's call (a grouped call's table is
// looked at for NULL-ness and max_tiles only, and max_tiles moves grid sizes alone).
static inline gemm_plan pna_product_plan(const pna_product& q, int64_t M, int32_t extra_flags, const void* ws, int64_t max_tiles,
                                         const int* opt, int num_cus) {
  static const int32_t a_table = 0;
  return gemm_plan_of(q.nseg, q.seg, q.grouped ? q.stride : nullptr, q.grouped ? q.classes : 1, M, q.N, q.bias, nullptr, 0, q.C,
                      q.ldc, q.flags | extra_flags, q.grouped ? &a_table : nullptr, max_tiles, ws, q.grouped ? q.tile_rows : 0, opt,
                      num_cus);
}

// Where the images of L layers x T towers lie in one slab: per (layer, tower) post-layer 0, dA, dx back to back, each
// region as long as its plan's image_bytes (a multiple of 24 KB, so every region stays 256-byte aligned); a product
// without images takes no room.  Returns the slab's size; fills out[l] when out != NULL (pointers relative to slab;
// slab == NULL: offsets from 0, for the size query).  params: L x (4 + T 2 (pre + post)) pointers, weff: L x T.
static inline size_t pna_images_layout(int L, int T, int F, int pre, int post, int D, int64_t N, int tile_rows,
                                       const float* const* params, const float* const* weff, const int* opt, int num_cus,
                                       void* slab, gnx_pna_layer_images* out, gemm_split_problem* probs, int* nprobs) {
  const int np = 4 + T * 2 * (pre + post);
  const uintptr_t base = reinterpret_cast<uintptr_t>(slab);
  float* const act = pna_stand_in();
  size_t off = 0;
  int n = 0;
  for (int l = 0; l < L; ++l) {
    const float* const* P = params + (size_t)l * np;
    gnx_pna_layer_images li = {};
    for (int t = 0; t < T; ++t) {
      const float* w = weff[(size_t)l * T + t];
      const pna_product prod[3] = {pna_post0_product(P, w, T, F, pre, post, D, t, act, act, act, tile_rows),
                                   pna_dA_product(w, T, F, D, t, act, act), pna_dx_product(P, T, F, pre, post, t, act, act, act, act)};
      void** const ptr[3] = {&li.post0[t], &li.dA[t], &li.dx[t]};
      gnx_gemm_image* const rec[3] = {&li.post0_rec[t], &li.dA_rec[t], &li.dx_rec[t]};
      for (int i = 0; i < 3; ++i) {
        const pna_product& q = prod[i];
        // (any non-NULL workspace: its alignment is checked where the images are written, not in the plan)
        const gemm_plan p = pna_product_plan(q, N, GNX_GEMM_SPLIT_ONLY, act, 1, opt, num_cus);
        if (!p.images || !p.run_split) continue;
        *rec[i] = gemm_image_of(p);
        void* const image = reinterpret_cast<void*>(base + off);
        *ptr[i] = image;
        if (probs) probs[n] = gemm_split_problem_of(p, q.nseg, q.seg, q.grouped ? q.stride : nullptr, q.N, image);
        ++n;
        off += p.image_bytes;
      }
    }
    if (out) out[l] = li;
  }
  if (nprobs) *nprobs = n;
  return off;
}

// ---------------------------------------------------------------------------------------------------------------
// dA product + scatter-aggregate backward in ONE launch (k_pna_dA_agg_bwd, gnx_gemm.hip): whether a tower's call takes it.
// The fused kernel is k_gemm_as3's product on 32-row tiles with the four column tiles (mean | min | max | std of the
// tower's F = 128 channels) kept in registers, so it is eligible only where the dA product itself takes k_gemm_as3 from
// split images, grouped by degree class, with exactly four column tiles and the plain epilogue; the message operands must
// allow 16-byte lane accesses, and every element offset must fit 32 bits.  Everything else keeps the two launches.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PLAN_DAF_BM = 32;                                        // rows per workgroup of k_pna_dA_agg_bwd
constexpr size_t PLAN_DAF_LDS = 3 * PLAN_DAF_BM * 272 + PLAN_DAF_BM * 4;  // three bf16 images of the tile + its row ids

struct pna_dA_agg_plan {
  bool fused = false;
  gemm_plan product;  // the plan of the dA product alone (what the two-launch path runs; its images are the fused kernel's)
  unsigned grid_x = 0;
  size_t lds = 0;
  double bytes = 0.0, flops = 0.0, mfma = 0.0;
};

// q = pna_dA_product(...) of one tower; N nodes, E messages, H = T F = row stride of m and ge.  extra_flags / ws as
// pna_product_plan's.
static inline pna_dA_agg_plan pna_dA_agg_plan_of(const pna_product& q, int64_t N, int64_t E, int64_t H, const float* m,
                                                 const float* ge, int32_t extra_flags, const void* ws, int64_t max_tiles,
                                                 const int* opt, int num_cus) {
  pna_dA_agg_plan f;
  f.product = pna_product_plan(q, N, extra_flags, ws, max_tiles, opt, num_cus);
  const gemm_plan& p = f.product;
  const int F = q.seg[0].k;
  f.fused = opt[GNX_OPT_DA_AGG_FUSED] != 0 && p.kernel == GNX_GEMM_KERNEL_AS3 && p.images && !p.stop_after_split && q.grouped &&
            max_tiles > 0 && F == PLAN_BN && q.N == 4 * PLAN_BN && p.epi == PLAN_EPI_PLAIN && q.bias == nullptr &&
            (q.flags & GNX_GEMM_RELU) == 0 && m != nullptr && ge != nullptr && plan_aligned16(m) && plan_aligned16(ge) &&
            H % 4 == 0 && H >= F && (double)(E + 1) * (double)H < 2147483648.0 && (double)N * (double)q.seg[0].lda < 2147483648.0 &&
            max_tiles * (PLAN_BM / PLAN_DAF_BM) < 2147483648LL;
  if (!f.fused) return f;
  f.grid_x = (unsigned)(max_tiles * (PLAN_BM / PLAN_DAF_BM));
  f.lds = PLAN_DAF_LDS;
  // the gradient rows 4NF, the messages read and their gradient written 8EF, row pointers and the class permutation
  f.bytes = 4.0 * N * F + 8.0 * E * F + 4.0 * E + 8.0 * N;
  f.flops = p.flops;
  f.mfma = p.mfma;
  return f;
}
