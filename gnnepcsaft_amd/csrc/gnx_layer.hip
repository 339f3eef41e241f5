// Native launch sequence of one PNAConv backward (gnx_pna_conv_bwd): the ~35 launches that
// gnnepcsaft_amd/functional.py::PNAConvFn.backward issues one by one from Python (0.32 ms of host time per layer, 5.5 ms
// per cfg-2 step, against 7.9 ms of GPU time) are issued here from ONE call -- same kernels, same streams, same order.
// It only composes the public entry points of gnx.h; nothing below touches a kernel directly.
//
// Reference semantics: the backward of [3P] torch_geometric.nn.PNAConv as built at
// /root/reference/gnnepcsaft/train/models.py:445-457 (restructured as DESIGN.md §4 describes: node-level P/Q products +
// 60-row bond table for pre-layer 0, per-degree-class effective weights for post-layer 0, lin o last post layer merged).
#include "gnx_common.hpp"
#include "gnx_gemm_plan.hpp"

#include <algorithm>
#include <vector>

namespace {

inline gnx_gemm_seg seg(const float* a, int64_t lda, const float* b, int64_t ldb, int32_t k) { return pna_seg(a, lda, b, ldb, k); }

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct WgradQueue {
  std::vector<gnx_wgrad_prob> q;
  void add(const float* dC, int64_t lddc, const float* A, int64_t lda, int64_t M, int32_t N, int32_t K, float* dW,
           int64_t lddw, float* dbias) {
    if (M <= 0) return;
    gnx_wgrad_prob p;
    p.dC = dC;
    p.lddc = lddc;
    p.A = A;
    p.lda = lda;
    p.rowscale = nullptr;
    p.dW = dW;
    p.lddw = lddw;
    p.dbias = dbias;
    p.M = M;
    p.N = N;
    p.K = K;
    q.push_back(p);
  }
  // up to 8 problems per launch, largest row counts first (problems of similar size share a launch)
  int32_t flush(gnx_handle* h) {
    std::stable_sort(q.begin(), q.end(), [](const gnx_wgrad_prob& a, const gnx_wgrad_prob& b) { return a.M > b.M; });
    for (size_t i = 0; i < q.size(); i += 8) {
      const int32_t n = (int32_t)std::min<size_t>(8, q.size() - i);
      const int32_t st = gnx_gemm_wgrad_batched(h, n, q.data() + i);
      if (st != GNX_OK) return st;
    }
    q.clear();
    return GNX_OK;
  }
};

#define GNX_TRY(call)                 \
  do {                                \
    const int32_t st_ = (call);       \
    if (st_ != GNX_OK) return st_;    \
  } while (0)

// runs `body` on side stream `which` (forked from the current point of the bound stream), restoring the stream on any exit
template <class F>
int32_t on_side(gnx_handle* h, int which, bool enabled, F body) {
  if (!enabled) return body();
  GNX_TRY(gnx_side_begin_n(h, which));
  const int32_t st = body();
  (void)gnx_side_end(h);
  return st;
}

// the degree-class table a grouped product runs over
struct class_tiles {
  const int32_t *dperm, *tiles, *ntiles;
  int64_t max_tiles;
};

int32_t run_product(gnx_handle* h, const pna_product& q, int64_t M, const class_tiles& ct, int32_t extra_flags, void* ws,
                    size_t ws_bytes) {
  if (!q.grouped) return gnx_gemm(h, q.nseg, q.seg, M, q.N, q.bias, nullptr, 0, q.C, q.ldc, q.flags | extra_flags, ws, ws_bytes);
  if (q.tile_rows)
    return gnx_gemm_grouped_rows(h, q.nseg, q.seg, q.stride, q.classes, M, q.N, q.bias, nullptr, 0, q.C, q.ldc, q.flags | extra_flags,
                                 ct.dperm, ct.tiles, ct.ntiles, ct.max_tiles, ws, ws_bytes, q.tile_rows);
  return gnx_gemm_grouped(h, q.nseg, q.seg, q.stride, q.classes, M, q.N, q.bias, nullptr, 0, q.C, q.ldc, q.flags | extra_flags, ct.dperm,
                          ct.tiles, ct.ntiles, ct.max_tiles, ws, ws_bytes);
}

// One of the layer's three image-reading products.  `image` / `rec` (gnx_pna_split_all) are used only if the plan of THIS call
// gives the very record the images were written under; any difference -- another row count, a changed option, an operand
// that is not aligned after all -- and the product splits in place into the scratch, as it does without images.
int32_t run_with_image(gnx_handle* h, const pna_product& q, int64_t M, const class_tiles& ct, void* image,
                       const gnx_gemm_image* rec, void* scratch, size_t scratch_bytes) {
  if (image != nullptr && rec != nullptr && rec->image_bytes > 0) {
    const gemm_plan p = pna_product_plan(q, M, GNX_GEMM_PRESPLIT, image, ct.max_tiles, h->opt, h->num_cus);
    if (p.images && gemm_image_equal(gemm_image_of(p), *rec))
      return run_product(h, q, M, ct, GNX_GEMM_PRESPLIT, image, (size_t)rec->image_bytes);
  }
  return run_product(h, q, M, ct, 0, scratch, scratch_bytes);
}

}  // namespace

// upper bound of the split-weight images any product of the layer's forward or backward needs (gnx_gemm_workspace_bytes): the
// degree-class product dA = g Weff(d) (D classes, N = 4F, K = F) and the 3-segment dx product (N = F, K = 3F)
// The workspace is one scratch that every product of the layer splits into in turn (a product whose images came from
// gnx_pna_split_all does not touch it).
static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

extern "C" size_t gnx_pna_conv_bwd_workspace_bytes(int32_t T, int32_t F, int32_t D) {
  const int64_t H = (int64_t)T * F;
  const size_t grouped = gemm_plan_image_bytes(D, 4 * (int64_t)F, plan_kpad(F));
  const size_t dx = gemm_plan_image_bytes(1, F, 3 * plan_kpad(F));
  const size_t lin = gemm_plan_image_bytes(1, H, plan_kpad(H));  // lin / merged product, H x H
  // forward: post-layer 0 by degree class, z = x W0^T + A Weff(d)^T  (N = F, K = F + 4F)
  const size_t post0 = gemm_plan_image_bytes(D, F, plan_kpad(F) + plan_kpad(4 * (int64_t)F));
  return align256(std::max(std::max(grouped, post0), std::max(dx, lin)) + 256);
}

extern "C" int32_t gnx_pna_conv_bwd(gnx_handle* h, const gnx_pna_bwd_args* a) { return gnx_pna_conv_bwd_images(h, a, nullptr); }

extern "C" int32_t gnx_pna_conv_bwd_images(gnx_handle* h, const gnx_pna_bwd_args* a, const gnx_pna_layer_images* im) {
  GNX_CHECK_ARG(h && a, "gnx_pna_conv_bwd: NULL argument");
  const int T = a->T, F = a->F, pre = a->pre_layers, post = a->post_layers, R = a->R, D = a->D;
  const int64_t N = a->N, E = a->E;
  const int H = T * F;
  GNX_CHECK_ARG(T >= 1 && F >= 1 && pre >= 1 && pre <= GNX_PNA_MAX_LAYERS && post >= 1 && post <= GNX_PNA_MAX_LAYERS &&
                    T <= GNX_PNA_MAX_TOWERS && D >= 1 && R >= 1,
                "gnx_pna_conv_bwd: bad layer shape T=%d F=%d pre=%d post=%d D=%d R=%d", T, F, pre, post, D, R);
  GNX_CHECK_ARG(a->params && a->grads && a->dout && a->x && a->A && a->dx && a->acc_buf, "gnx_pna_conv_bwd: NULL array");
  const bool side = a->use_side_streams != 0;
  const int per = 2 * (pre + post);
  auto pidx = [&](int t, bool is_pre, int i) { return 4 + t * per + 2 * (is_pre ? i : pre + i); };
  const float* const* P = a->params;
  float* const* G = a->grads;
  const float* lin_w = P[2];
  WgradQueue wq;

  // the two tiled products of this backward that read split weight images (dA per degree class, the 3-segment dx) take them
  // from `im` where gnx_pna_split_all wrote them for this very shape, and split in place otherwise
  const class_tiles ct = {a->dperm, a->tiles, a->ntiles, a->max_tiles};

  // ---- lin (or lin o last post layer): dgrad into gbuf[0]
  // every gradient buffer of the chain is distinct: the queued weight-gradient problems read them at flush time
  int gi = 0;
  float* g = a->gbuf[gi];
  const float* z_last = a->zs[a->n_z - 1];
  int last_hidden;
  const bool tail = (a->flags & GNX_PNA_BWD_LAST_OF_PASS) != 0;  // nothing follows this layer on the main stream (see the flush below)
  const bool defer = (a->flags & GNX_PNA_BWD_DEFER_SMALL) != 0;  // small accumulators pre-zeroed by the caller, their consumers
                                                                 // run in gnx_pna_stack_finish for all layers at once
  // with side streams the per-class weight gradients of post-layer 0 are forked BEHIND the aggregate backward, not in front of
  // it (a memory-bound kernel they slow down a lot: 135 us beside them, 55 alone): 6.640 -> 6.609 ms, cfg-5 55.88 -> 55.63; at
  // the END of the layer they were worse (6.662 vs 6.579)
  std::vector<std::function<int32_t()>> class_wgrads;
  if (a->merged) {
    if (!defer) {
      GNX_TRY(gnx_fill(h, a->dWm, (int64_t)H * H, 0.f));
      GNX_TRY(gnx_fill(h, a->dbm, H, 0.f));
    }
    wq.add(a->dout, H, z_last, H, N, H, H, a->dWm, H, a->dbm);
    gnx_gemm_seg s = seg(a->dout, H, a->Wm, H, H);
    GNX_TRY(gnx_gemm(h, 1, &s, N, H, nullptr, z_last, H, g, H, 0, a->ws, a->ws_bytes));
    last_hidden = post - 2;
  } else {
    wq.add(a->dout, H, z_last, H, N, H, H, G[2], H, G[3]);
    gnx_gemm_seg s = seg(a->dout, H, lin_w, H, H);
    GNX_TRY(gnx_gemm(h, 1, &s, N, H, nullptr, nullptr, 0, g, H, 0, a->ws, a->ws_bytes));
    last_hidden = post - 1;
  }
  // ---- hidden post layers last..1: dgrad masked by the relu'd input activation
  for (int i = last_hidden; i >= 1; --i) {
    const float* a_prev = a->zs[i - 1];
    for (int t = 0; t < T; ++t) {
      const int k = pidx(t, false, i);
      wq.add(g + t * F, H, a_prev + t * F, H, N, F, F, G[k], F, G[k + 1]);
      gnx_gemm_seg s = seg(g + t * F, H, P[k], F, F);
      GNX_TRY(gnx_gemm(h, 1, &s, N, F, nullptr, a_prev + t * F, H, a->gbuf[gi + 1] + t * F, H, 0, a->ws, a->ws_bytes));
    }
    g = a->gbuf[++gi];
  }
  // ---- post layer 0: x-part weight gradient (queued), per-class weight gradient (side stream 0), dA
  // dA and the scatter-aggregate backward behind it run as ONE launch per tower (gnx_pna_da_aggregate_bwd: dA stays in
  // registers) as long as every tower's call is eligible; the first that is not sends the whole layer down the two-launch path
  int ei = 0;
  float* ge = a->gebuf[ei];
  const float* m_last = a->hs[a->n_h - 1];
  bool fused_agg = true;
  auto dA_product = [&](int t) -> int32_t {
    return run_with_image(h, pna_dA_product(a->weff[t], T, F, D, t, g, a->dA), N, ct, im ? im->dA[t] : nullptr,
                          im ? &im->dA_rec[t] : nullptr, a->ws, a->ws_bytes);
  };
  for (int t = 0; t < T; ++t) {
    const int k = pidx(t, false, 0);
    const float* gt = g + t * F;
    const float* At = a->A + (int64_t)t * 4 * F;
    float* dWp = G[k];
    wq.add(gt, H, a->x + t * F, H, N, F, F, dWp, 13 * F, G[k + 1]);
    float* dWeff = a->dWeff + (int64_t)t * D * F * 4 * F;
    if (!defer) GNX_TRY(gnx_fill(h, dWeff, (int64_t)D * F * 4 * F, 0.f));
    auto class_wgrad = [&, gt, At, dWeff, dWp]() -> int32_t {
      GNX_TRY(gnx_gemm_wgrad_grouped(h, gt, H, At, (int64_t)T * 4 * F, N, F, 4 * F, dWeff, 4 * F, (int64_t)F * 4 * F, a->dperm,
                                     a->chunks, a->nchunks, a->max_chunks));
      return defer ? GNX_OK : gnx_pna_weff_bwd(h, dWeff, F, D, a->avg_deg_log, dWp, 13 * F);
    };
    if (side)
      class_wgrads.push_back(class_wgrad);
    else
      GNX_TRY(class_wgrad());
    if (fused_agg) {
      int32_t took = 0;
      GNX_TRY(gnx_pna_da_aggregate_bwd(h, a->weff[t], T, F, D, t, g, a->dA, m_last, a->rowptr, N, E, ge, a->dperm, a->tiles,
                                       a->ntiles, a->max_tiles, im ? im->dA[t] : nullptr, im ? &im->dA_rec[t] : nullptr, a->ws,
                                       a->ws_bytes, &took));
      fused_agg = took != 0;
      if (!fused_agg)
        for (int u = 0; u < t; ++u) GNX_TRY(dA_product(u));  // (towers already done wrote their columns of ge: rewritten below)
    }
    if (!fused_agg) GNX_TRY(dA_product(t));
  }
  const float* g_post0 = g;  // gradient w.r.t. post-layer 0's output: also an operand of dx below
  // (the last layer of the pass keeps the weight gradients queued so far for the end of the layer as well: launched HERE,
  // beside the edge backward, they compete with it on the main stream: 6.612 vs 6.554 ms)
  // ---- scatter-aggregate backward, then the pre layers last..1
  if (!fused_agg) GNX_TRY(gnx_pna_aggregate_bwd(h, a->dA, m_last, a->A, a->rowptr, N, E, T, F, ge));
  for (auto& fn : class_wgrads) GNX_TRY(on_side(h, 0, side, fn));
  // With two pre layers (the reference's default) the masked input gradient of pre-layer 1, the destination sums dP and the
  // bond-table sums dTe come from ONE pass over the message gradient (gnx_pna_edge_bwd); only dQ is a pass of its own.
  bool fused_bwd = pre == 2 && a->etile_info != nullptr && E > 0 && F % 4 == 0 && F <= 128 &&
                   R <= 64 && a16(ge) && a16(a->hs[0]) && a16(a->gebuf[1]) && a16(a->dP) && a16(a->dTe);
  for (int t = 0; t < T && fused_bwd; ++t) fused_bwd = a16(P[pidx(t, true, 1)]);
  if (fused_bwd) {
    const float* W1[GNX_PNA_MAX_TOWERS];
    for (int t = 0; t < T; ++t) {
      const int k = pidx(t, true, 1);
      W1[t] = P[k];
      wq.add(ge + t * F, H, a->hs[0] + t * F, H, E, F, F, G[k], F, G[k + 1]);
    }
    if (!defer) GNX_TRY(gnx_fill(h, a->dTe, (int64_t)R * H, 0.f));
    GNX_TRY(gnx_pna_edge_bwd(h, ge, a->hs[0], a->code, a->rowptr, a->etile_info, a->etile_w, N, E, T, F, R, W1, a->gebuf[1], a->dP,
                             a->dTe));
    ge = a->gebuf[++ei];
    GNX_TRY(gnx_edge_combine_bwd(h, ge, a->rowptr, a->colptr, a->cpos, a->code, N, E, H, 0, nullptr, a->dQ, nullptr, nullptr, 0));
  } else {
    for (int i = pre - 1; i >= 1; --i) {
      const float* h_prev = a->hs[i - 1];
      for (int t = 0; t < T; ++t) {
        const int k = pidx(t, true, i);
        wq.add(ge + t * F, H, h_prev + t * F, H, E, F, F, G[k], F, G[k + 1]);
        gnx_gemm_seg s = seg(ge + t * F, H, P[k], F, F);
        GNX_TRY(gnx_gemm(h, 1, &s, E, F, nullptr, h_prev + t * F, H, a->gebuf[ei + 1] + t * F, H, 0, a->ws, a->ws_bytes));
      }
      ge = a->gebuf[++ei];
    }
    // ---- message assembly backward: dP, dQ; input gradient
    GNX_TRY(gnx_edge_combine_bwd(h, ge, a->rowptr, a->colptr, a->cpos, a->code, N, E, H, 0, a->dP, a->dQ, nullptr, nullptr, 0));
  }
  for (int t = 0; t < T; ++t) {
    float* dW0 = G[pidx(t, true, 0)];
    wq.add(a->dP + t * F, H, a->x + t * F, H, N, F, F, dW0, 3 * F, nullptr);
    wq.add(a->dQ + t * F, H, a->x + t * F, H, N, F, F, dW0 + F, 3 * F, nullptr);
  }
  // the queue is complete: with side streams the batched weight gradients start HERE, beside the dx product (matrix-bound),
  // instead of behind it, beside the next layer's BatchNorm backward (memory-bound): 6.578 -> 6.541 ms, cfg-5 56.03 -> 55.90
  auto flush_batched = [&]() -> int32_t {
    // the LAST layer of a backward pass has the chip to itself: its batched weight gradients take every CU instead of the
    // workgroup budget that leaves room for the main stream (the end of a step waits for exactly this launch): 6.760 -> 6.687 ms
    const int wgs_saved = h->opt[GNX_OPT_WGRAD_WGS];
    if (tail && wgs_saved == 0) h->opt[GNX_OPT_WGRAD_WGS] = h->num_cus > 0 ? h->num_cus : 256;
    const int32_t fst = wq.flush(h);
    h->opt[GNX_OPT_WGRAD_WGS] = wgs_saved;
    return fst;
  };
  const bool flush_before_dx = side && !tail;
  if (flush_before_dx) GNX_TRY(on_side(h, 0, side, flush_batched));
  for (int t = 0; t < T; ++t)
    GNX_TRY(run_with_image(h, pna_dx_product(P, T, F, pre, post, t, g_post0, a->dP, a->dQ, a->dx), N, ct, im ? im->dx[t] : nullptr,
                           im ? &im->dx_rec[t] : nullptr, a->ws, a->ws_bytes));
  // ---- bond-table gradient chain on side stream 1 (feeds parameter gradients and the shared accumulator only)
  GNX_TRY(on_side(h, 1, side, [&]() -> int32_t {
    if (!fused_bwd) {
      if (!defer) GNX_TRY(gnx_fill(h, a->dTe, (int64_t)R * H, 0.f));
      if (E > 0) GNX_TRY(gnx_key_segment_sum(h, ge, a->code_pos, a->code, E, H, a->dTe));
    }
    if (defer) return GNX_OK;
    for (int t = 0; t < T; ++t) {
      const int k0 = pidx(t, true, 0);
      GNX_TRY(gnx_gemm_wgrad(h, a->dTe + t * F, H, a->EE, F, nullptr, R, F, F, G[k0] + 2 * F, 3 * F, G[k0 + 1]));
      gnx_gemm_seg s = seg(a->dTe + t * F, H, P[k0] + 2 * F, 3 * F, F);
      GNX_TRY(gnx_gemm(h, 1, &s, R, F, nullptr, nullptr, 0, a->dEE, F, t > 0 ? GNX_GEMM_ACCUMULATE : 0, nullptr, 0));
    }
    GNX_TRY(gnx_gemm_wgrad(h, a->dEE, F, a->BE, H, nullptr, R, F, H, G[0], H, G[1]));
    if (a->acc_first) GNX_TRY(gnx_fill(h, a->acc_buf, (int64_t)R * H, 0.f));
    gnx_gemm_seg s = seg(a->dEE, F, P[0], H, F);
    return gnx_gemm(h, 1, &s, R, H, nullptr, nullptr, 0, a->acc_buf, H, GNX_GEMM_ACCUMULATE, nullptr, 0);
  }));
  // ---- the layer's weight gradients in batched launches on side stream 0, then what hangs off dWm
  GNX_TRY(on_side(h, 0, side, [&]() -> int32_t {
    if (!flush_before_dx) GNX_TRY(flush_batched());
    if (!a->merged || defer) return GNX_OK;
    const float* dbm = a->dbm;
    for (int t = 0; t < T; ++t) {
      const int k = pidx(t, false, post - 1);
      const float* Wt = P[k];
      const float* bt = P[k + 1];
      // d lin_w[:, t] += dWm[:, t] W_t^T + dbm b_t^T ; dW_t += lin_w[:, t]^T dWm[:, t] ; db_t += dbm lin_w[:, t]
      gnx_gemm_seg s1 = seg(a->dWm + t * F, H, Wt, F, F);
      GNX_TRY(gnx_gemm(h, 1, &s1, H, F, nullptr, nullptr, 0, G[2] + t * F, H, GNX_GEMM_ACCUMULATE | GNX_GEMM_B_TRANS, nullptr, 0));
      gnx_gemm_seg s2 = seg(dbm, 1, bt, 1, 1);
      GNX_TRY(gnx_gemm(h, 1, &s2, H, F, nullptr, nullptr, 0, G[2] + t * F, H, GNX_GEMM_ACCUMULATE | GNX_GEMM_B_TRANS, nullptr, 0));
      GNX_TRY(gnx_gemm_wgrad(h, lin_w + t * F, H, a->dWm + t * F, H, nullptr, H, F, F, G[k], F, nullptr));
      gnx_gemm_seg s3 = seg(dbm, H, lin_w + t * F, H, H);
      GNX_TRY(gnx_gemm(h, 1, &s3, 1, F, nullptr, nullptr, 0, G[k + 1], F, GNX_GEMM_ACCUMULATE, nullptr, 0));
    }
    return gnx_axpy(h, G[3], dbm, H, 1.0f);
  }));
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// PNA post-layer 0 effective weights per in-degree class d (amp/att depend on d only):
//   Weff[d][o][j] = W[o][F + j] + amp(d) W[o][5F + j] + att(d) W[o][9F + j],   o < F, j < 4F
// and the matching weight gradient:  dW[:, F:5F] += sum_d dWeff[d], [:, 5F:9F] += sum_d amp(d) dWeff[d], ...
// Up to GNX_SMALL_BATCH (layer, tower) pairs per launch (blockIdx.y = pair); gnx_pna_weff(_bwd) is a batch of one.
// ---------------------------------------------------------------------------------------------------------------
struct weff_batch_args {
  const float* W[GNX_SMALL_BATCH];
  float* out[GNX_SMALL_BATCH];
  float avg_log[GNX_SMALL_BATCH];
  int64_t ldw;
  int F, D;
};

// Entry-wise within 4 u (|W1| + amp |W2| + att |W3|) of the exact value (u = 2^-24; tests/test_wgrad_gpu.py): the two
// factors are evaluated in double and rounded once (<= 1 u each; fp32 logf-and-divide is up to 3 u), then each scaled
// term carries its factor's and its product's rounding (2 u of the term) and the two additions one rounding each.  Once
// per block instead of per thread: a block's 256 consecutive elements belong to at most 256 / (4 F^2) + 2 <= 66 classes.
#define WEFF_BLOCK 256
#define WEFF_CLS (WEFF_BLOCK / 4 + 2)
__global__ void __launch_bounds__(WEFF_BLOCK) k_pna_weff_batched(weff_batch_args a) {
  __shared__ float s_amp[WEFF_CLS], s_att[WEFF_CLS];
  const int b = blockIdx.y;
  const int F = a.F;
  const int64_t first = (int64_t)blockIdx.x * WEFF_BLOCK;
  int64_t i = first + threadIdx.x;
  int64_t per = (int64_t)F * 4 * F;
  const int d0 = (int)(first / per);
  if (threadIdx.x < WEFF_CLS) {
    const double dd = (double)(d0 + (int)threadIdx.x), avg = (double)a.avg_log[b];
    s_amp[threadIdx.x] = (float)(log(dd + 1.0) / avg);
    s_att[threadIdx.x] = (float)(avg / log(fmax(dd, 1.0) + 1.0));
  }
  __syncthreads();
  if (i >= per * a.D) return;
  int d = (int)(i / per);
  int o = (int)((i % per) / (4 * F)), j = (int)(i % (4 * F));
  const float amp = s_amp[d - d0], att = s_att[d - d0];
  const float* w = a.W[b] + (int64_t)o * a.ldw;
  a.out[b][i] = w[F + j] + amp * w[5 * F + j] + att * w[9 * F + j];
}

struct weff_bwd_batch_args {
  const float* dWeff[GNX_SMALL_BATCH];
  float* dW[GNX_SMALL_BATCH];
  float avg_log[GNX_SMALL_BATCH];
  int64_t lddw;
  int F, D;
};

__global__ void k_pna_weff_bwd_batched(weff_bwd_batch_args a) {
  const int b = blockIdx.y;
  const int F = a.F;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t per = (int64_t)F * 4 * F;
  if (i >= per) return;
  int o = (int)(i / (4 * F)), j = (int)(i % (4 * F));
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const float avg_log = a.avg_log[b];
  const float* dWeff = a.dWeff[b];
  for (int d = 0; d < a.D; ++d) {
    float dd = (float)d;
    float amp = logf(dd + 1.0f) / avg_log;
    float att = avg_log / logf(fmaxf(dd, 1.0f) + 1.0f);
    float v = dWeff[(int64_t)d * per + i];
    s1 += v;
    s2 += amp * v;
    s3 += att * v;
  }
  float* w = a.dW[b] + (int64_t)o * a.lddw;
  w[F + j] += s1;
  w[5 * F + j] += s2;
  w[9 * F + j] += s3;
}

extern "C" int32_t gnx_pna_weff_bwd_batched(gnx_handle* h, int32_t n, const float* const* dWeff, int32_t F, int32_t D,
                                            const float* avg_deg_log, float* const* dW, int64_t lddw) {
  GNX_CHECK_ARG(h && dWeff && dW && avg_deg_log && n >= 0 && F > 0 && D > 0 && lddw >= 13 * F,
                "gnx_pna_weff_bwd_batched: bad argument");
  const int64_t cnt = (int64_t)F * 4 * F;
  for (int32_t i0 = 0; i0 < n; i0 += GNX_SMALL_BATCH) {
    weff_bwd_batch_args a;
    const int m = n - i0 < GNX_SMALL_BATCH ? n - i0 : GNX_SMALL_BATCH;
    for (int i = 0; i < GNX_SMALL_BATCH; ++i) {
      const int k = i < m ? i0 + i : i0;
      a.dWeff[i] = dWeff[k];
      a.dW[i] = dW[k];
      a.avg_log[i] = avg_deg_log[k];
      GNX_CHECK_ARG(a.dWeff[i] && a.dW[i], "gnx_pna_weff_bwd_batched: NULL pointer at %d", k);
    }
    a.lddw = lddw;
    a.F = F;
    a.D = D;
    hipLaunchKernelGGL(k_pna_weff_bwd_batched, dim3((unsigned)gnx_cdiv(cnt, 256), (unsigned)m), dim3(256), 0, h->stream, a);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

// W[i] / out[i]: HOST arrays of n device pointers (post_nns[t][0].weight [F,13F] -> Weff [D,F,4F]); avg_log: HOST [n]
extern "C" int32_t gnx_pna_weff_batched(gnx_handle* h, int32_t n, const float* const* W, int64_t ldw, int32_t F, int32_t D,
                                        const float* avg_deg_log, float* const* Weff) {
  GNX_CHECK_ARG(h && W && Weff && avg_deg_log && n >= 0 && F > 0 && D > 0 && ldw >= 13 * F, "gnx_pna_weff_batched: bad argument");
  const int64_t cnt = (int64_t)F * 4 * F * D;
  for (int32_t i0 = 0; i0 < n; i0 += GNX_SMALL_BATCH) {
    weff_batch_args a;
    const int m = n - i0 < GNX_SMALL_BATCH ? n - i0 : GNX_SMALL_BATCH;
    for (int i = 0; i < GNX_SMALL_BATCH; ++i) {
      const int k = i < m ? i0 + i : i0;
      a.W[i] = W[k];
      a.out[i] = Weff[k];
      a.avg_log[i] = avg_deg_log[k];
      GNX_CHECK_ARG(a.W[i] && a.out[i], "gnx_pna_weff_batched: NULL pointer at %d", k);
    }
    a.ldw = ldw;
    a.F = F;
    a.D = D;
    hipLaunchKernelGGL(k_pna_weff_batched, dim3((unsigned)gnx_cdiv(cnt, 256), (unsigned)m), dim3(256), 0, h->stream, a);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

extern "C" int32_t gnx_pna_weff(gnx_handle* h, const float* W, int64_t ldw, int32_t F, int32_t D, float avg_deg_log,
                                float* Weff) {
  GNX_CHECK_ARG(h && W && Weff && F > 0 && D > 0 && ldw >= 13 * F, "gnx_pna_weff: bad argument");
  return gnx_pna_weff_batched(h, 1, &W, ldw, F, D, &avg_deg_log, &Weff);
}

extern "C" int32_t gnx_pna_weff_bwd(gnx_handle* h, const float* dWeff, int32_t F, int32_t D, float avg_deg_log,
                                    float* dW, int64_t lddw) {
  GNX_CHECK_ARG(h && dWeff && dW && F > 0 && D > 0 && lddw >= 13 * F, "gnx_pna_weff_bwd: bad argument");
  return gnx_pna_weff_bwd_batched(h, 1, &dWeff, F, D, &avg_deg_log, &dW, lddw);
}

// ---------------------------------------------------------------------------------------------------------------
// Weight-only part of a PNAConv forward (functional._pna_weight_only): EE = BondEmb W_enc^T + b_enc, Te (edge slice of
// pre-layer 0 on the 60-row bond table), Weff(d) per tower, merged lin o last post layer.  5 + 3(T-1) tiny launches.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int32_t gnx_pna_weight_only(gnx_handle* h, const float* BE, int32_t R, int32_t T, int32_t F, int32_t pre_layers,
                                       int32_t post_layers, int32_t D, float avg_deg_log, const float* const* params,
                                       int32_t merged, float* EE, float* Te, float* const* weff, float* Wm, float* bm) {
  GNX_CHECK_ARG(h && BE && params && EE && Te && R > 0 && T >= 1 && T <= GNX_PNA_MAX_TOWERS && F >= 1 && pre_layers >= 1 &&
                    post_layers >= 1, "gnx_pna_weight_only: bad argument");
  const int H = T * F, per = 2 * (pre_layers + post_layers);
  gnx_gemm_seg s = seg(BE, H, params[0], H, H);
  GNX_TRY(gnx_gemm(h, 1, &s, R, F, params[1], nullptr, 0, EE, F, GNX_GEMM_B_TRANS, nullptr, 0));
  for (int t = 0; t < T; ++t) {
    const float* W0 = params[4 + t * per];
    gnx_gemm_seg se = seg(EE, F, W0 + 2 * F, 3 * F, F);
    GNX_TRY(gnx_gemm(h, 1, &se, R, F, params[4 + t * per + 1], nullptr, 0, Te + t * F, H, GNX_GEMM_B_TRANS, nullptr, 0));
    if (D > 0) {
      GNX_CHECK_ARG(weff && weff[t], "gnx_pna_weight_only: weff[%d] is NULL", t);
      GNX_TRY(gnx_pna_weff(h, params[4 + t * per + 2 * pre_layers], 13 * F, F, D, avg_deg_log, weff[t]));
    }
  }
  if (merged) {
    GNX_CHECK_ARG(Wm && bm && post_layers > 1, "gnx_pna_weight_only: merged without Wm / bm");
    const float* lin_w = params[2];
    for (int t = 0; t < T; ++t) {
      const int k = 4 + t * per + 2 * (pre_layers + post_layers - 1);
      gnx_gemm_seg sw = seg(lin_w + t * F, H, params[k], F, F);                        // Wm[:, t] = lin_w[:, t] @ W_last_t
      GNX_TRY(gnx_gemm(h, 1, &sw, H, F, nullptr, nullptr, 0, Wm + t * F, H, 0, nullptr, 0));
      gnx_gemm_seg sb = seg(params[k + 1], F, lin_w + t * F, H, F);                    // bm (+)= b_last_t @ lin_w[:, t]^T
      GNX_TRY(gnx_gemm(h, 1, &sb, 1, H, t == 0 ? params[3] : nullptr, nullptr, 0, bm, H,
                       GNX_GEMM_B_TRANS | (t > 0 ? GNX_GEMM_ACCUMULATE : 0), nullptr, 0));
    }
  }
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Forward launch sequence of one PNAConv (functional.PNAConvFn.forward after the weight-only part): node-level P / Q
// products, message assembly, remaining pre layers, scatter-aggregate, post-layer 0 by degree class, hidden post
// layers, lin (or the merged product).  Every activation the backward needs is written into caller-owned buffers.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int32_t gnx_pna_conv_fwd(gnx_handle* h, const gnx_pna_fwd_args* a) { return gnx_pna_conv_fwd_images(h, a, nullptr); }

extern "C" int32_t gnx_pna_conv_fwd_images(gnx_handle* h, const gnx_pna_fwd_args* a, const gnx_pna_layer_images* im) {
  GNX_CHECK_ARG(h && a, "gnx_pna_conv_fwd: NULL argument");
  const int T = a->T, F = a->F, pre = a->pre_layers, post = a->post_layers, D = a->D;
  const int64_t N = a->N, E = a->E;
  const int H = T * F;
  GNX_CHECK_ARG(T >= 1 && T <= GNX_PNA_MAX_TOWERS && F >= 1 && pre >= 1 && pre <= GNX_PNA_MAX_LAYERS && post >= 1 &&
                    post <= GNX_PNA_MAX_LAYERS && D >= 1, "gnx_pna_conv_fwd: bad layer shape");
  GNX_CHECK_ARG(a->params && a->x && a->Te && a->P && a->Q && a->A && a->out, "gnx_pna_conv_fwd: NULL array");
  const int per = 2 * (pre + post);
  const float* const* W = a->params;
  // post-layer 0's weight images (x part + Weff(d), per tower) come from `im` where gnx_pna_split_all wrote them for this very
  // shape; otherwise the product splits in place
  const class_tiles ct = {a->dperm, a->tiles, a->ntiles, a->max_tiles};
  for (int t = 0; t < T; ++t) {
    const float* W0 = W[4 + t * per];
    gnx_gemm_seg sp = seg(a->x + t * F, H, W0, 3 * F, F), sq = seg(a->x + t * F, H, W0 + F, 3 * F, F);
    GNX_TRY(gnx_gemm(h, 1, &sp, N, F, nullptr, nullptr, 0, a->P + t * F, H, GNX_GEMM_B_TRANS, a->ws, a->ws_bytes));
    GNX_TRY(gnx_gemm(h, 1, &sq, N, F, nullptr, nullptr, 0, a->Q + t * F, H, GNX_GEMM_B_TRANS, a->ws, a->ws_bytes));
  }
  // edge pipeline: message assembly -> pre layers 1.. -> scatter-aggregate.  With two pre layers (the reference's default)
  // it is ONE launch (gnx_pna_edge_fwd: h1 and the messages are written once and never read back, bit-identical results)
  bool fused = pre == 2 && a->etile_info != nullptr && E > 0 && F % 4 == 0 && F <= 128 &&
               a16(a->P) && a16(a->Q) && a16(a->Te) && a16(a->hs[0]) && a16(a->hs[1]) && a16(a->A);
  const float* W1[GNX_PNA_MAX_TOWERS];
  const float* b1[GNX_PNA_MAX_TOWERS];
  for (int t = 0; t < T && fused; ++t) {
    W1[t] = W[4 + t * per + 2];
    b1[t] = W[4 + t * per + 3];
    fused = a16(W1[t]);
  }
  if (fused) {
    GNX_TRY(gnx_pna_edge_fwd(h, a->P, a->Q, a->Te, a->src, a->dst, a->code, a->rowptr, a->etile_info, a->etile_w, N, E, T, F,
                             W1, b1, a->hs[0], a->hs[1], a->A));
  } else {
    GNX_TRY(gnx_edge_combine_fwd(h, a->P, a->Q, a->Te, a->src, a->dst, a->code, E, H, pre > 1 ? 1 : 0, a->hs[0]));
    for (int i = 1; i < pre; ++i)
      for (int t = 0; t < T; ++t) {
        const int k = 4 + t * per + 2 * i;
        gnx_gemm_seg s = seg(a->hs[i - 1] + t * F, H, W[k], F, F);
        GNX_TRY(gnx_gemm(h, 1, &s, E, F, W[k + 1], nullptr, 0, a->hs[i] + t * F, H,
                         GNX_GEMM_B_TRANS | (i < pre - 1 ? GNX_GEMM_RELU : 0), a->ws, a->ws_bytes));
      }
    GNX_TRY(gnx_pna_aggregate_fwd(h, a->hs[pre - 1], a->rowptr, N, E, T, F, a->A));
  }
  for (int t = 0; t < T; ++t)
    GNX_TRY(run_with_image(h, pna_post0_product(W, a->weff[t], T, F, pre, post, D, t, a->x, a->A, a->zs[0], a->tile_rows), N, ct,
                           im ? im->post0[t] : nullptr, im ? &im->post0_rec[t] : nullptr, a->ws, a->ws_bytes));
  const int hidden_end = a->merged ? post - 1 : post;  // hidden layers 1 .. hidden_end-1 are evaluated one by one
  int zi = 0;
  for (int i = 1; i < hidden_end; ++i, ++zi)
    for (int t = 0; t < T; ++t) {
      const int k = 4 + t * per + 2 * (pre + i);
      gnx_gemm_seg s = seg(a->zs[zi] + t * F, H, W[k], F, F);
      GNX_TRY(gnx_gemm(h, 1, &s, N, F, W[k + 1], nullptr, 0, a->zs[zi + 1] + t * F, H,
                       GNX_GEMM_B_TRANS | (i < post - 1 ? GNX_GEMM_RELU : 0), a->ws, a->ws_bytes));
    }
  gnx_gemm_seg sl = a->merged ? seg(a->zs[zi], H, a->Wm, H, H) : seg(a->zs[zi], H, W[2], H, H);
  return gnx_gemm(h, 1, &sl, N, H, a->merged ? a->bm : W[3], nullptr, 0, a->out, H, GNX_GEMM_B_TRANS, a->ws, a->ws_bytes);
}

// ---------------------------------------------------------------------------------------------------------------
// The split weight images of every layer's three tiled products, once per step (behind gnx_pna_weight_only_all: they read
// Weff): planned and laid out by pna_images_layout (gnx_gemm_plan.hpp), written by k_split_weights_batched.
// ---------------------------------------------------------------------------------------------------------------
extern "C" size_t gnx_pna_split_all_bytes(gnx_handle* h, int32_t L, int32_t T, int32_t F, int32_t pre_layers, int32_t post_layers,
                                          int32_t D, int64_t N, int32_t tile_rows) {
  if (h == nullptr || L < 1 || T < 1 || T > GNX_PNA_MAX_TOWERS || F < 1 || pre_layers < 1 || post_layers < 1 || D < 1 || N <= 0) return 0;
  // (only the alignment of a weight enters a plan: every pointer is the aligned stand-in, F % 4 decides the rest)
  const std::vector<const float*> params((size_t)L * (4 + T * 2 * (pre_layers + post_layers)), pna_stand_in());
  const std::vector<const float*> weff((size_t)L * T, pna_stand_in());
  return pna_images_layout(L, T, F, pre_layers, post_layers, D, N, tile_rows, params.data(), weff.data(), h->opt, h->num_cus, nullptr,
                           nullptr, nullptr, nullptr);
}

extern "C" int32_t gnx_pna_split_all(gnx_handle* h, int32_t L, int32_t T, int32_t F, int32_t pre_layers, int32_t post_layers,
                                     int32_t D, int64_t N, int32_t tile_rows, const float* const* params, const float* const* weff,
                                     void* slab, size_t slab_bytes, gnx_pna_layer_images* out) {
  GNX_CHECK_ARG(h && params && weff && out && L >= 1 && T >= 1 && T <= GNX_PNA_MAX_TOWERS && F >= 1 && pre_layers >= 1 &&
                    post_layers >= 1 && D >= 1 && N >= 0, "gnx_pna_split_all: bad argument");
  const size_t np = 4 + (size_t)T * 2 * (pre_layers + post_layers);
  for (size_t i = 0; i < (size_t)L * np; ++i) GNX_CHECK_ARG(params[i], "gnx_pna_split_all: params[%zu] is NULL", i);
  for (size_t i = 0; i < (size_t)L * T; ++i) GNX_CHECK_ARG(weff[i], "gnx_pna_split_all: weff[%zu] is NULL", i);
  std::vector<gemm_split_problem> probs((size_t)3 * L * T);
  int n = 0;
  // first pass without the slab: how much the images of THESE weights need
  const size_t need = pna_images_layout(L, T, F, pre_layers, post_layers, D, N, tile_rows, params, weff, h->opt, h->num_cus, nullptr,
                                        out, nullptr, &n);
  if (n == 0) return GNX_OK;  // (out[] holds no image)
  GNX_CHECK_ARG(slab && (reinterpret_cast<uintptr_t>(slab) & 255) == 0, "gnx_pna_split_all: the slab must be 256-byte aligned");
  if (slab_bytes < need) {
    gnx_set_error("gnx_pna_split_all: slab of %zu bytes, the images need %zu", slab_bytes, need);
    return GNX_E_WORKSPACE;
  }
  pna_images_layout(L, T, F, pre_layers, post_layers, D, N, tile_rows, params, weff, h->opt, h->num_cus, slab, out, probs.data(), &n);
  return gnx_split_weights_batched(h, n, probs.data());
}

// ---------------------------------------------------------------------------------------------------------------
// Model-level batching of the weight-only work.  Everything below depends on weights (and 60-row
// tables) only; issued per layer it was ~14 launches of ~5-10 us each per layer and direction.  Here: all layers at once.
// ---------------------------------------------------------------------------------------------------------------
namespace {
inline gnx_small_prob sprob(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, float* C, int64_t ldc,
                            int M, int N, int K, int flags) {
  gnx_small_prob q;
  q.A = A;
  q.lda = lda;
  q.B = B;
  q.ldb = ldb;
  q.bias = bias;
  q.C = C;
  q.ldc = ldc;
  q.M = M;
  q.N = N;
  q.K = K;
  q.flags = flags;
  return q;
}
}  // namespace

extern "C" int32_t gnx_pna_weight_only_all(gnx_handle* h, int32_t L, const float* BE, int32_t R, int32_t T, int32_t F,
                                           int32_t pre_layers, int32_t post_layers, int32_t D, const float* avg_deg_log,
                                           const float* const* params, int32_t merged, float* const* EE, float* const* Te,
                                           float* const* weff, float* const* Wm, float* const* bm) {
  GNX_CHECK_ARG(h && BE && params && EE && Te && avg_deg_log && L >= 1 && R > 0 && T >= 1 && T <= GNX_PNA_MAX_TOWERS && F >= 1 &&
                    pre_layers >= 1 && post_layers >= 1, "gnx_pna_weight_only_all: bad argument");
  GNX_CHECK_ARG(!merged || (Wm && bm && post_layers > 1), "gnx_pna_weight_only_all: merged without Wm / bm");
  GNX_CHECK_ARG(D <= 0 || weff, "gnx_pna_weight_only_all: weff is NULL");
  const int H = T * F, per = 2 * (pre_layers + post_layers), np = 4 + T * per;
  std::vector<gnx_small_prob> first, second;
  std::vector<std::vector<gnx_small_prob>> later(T > 2 ? T - 2 : 0);  // bm's towers 2.. : one more launch each
  std::vector<const float*> wsrc;
  std::vector<float*> wdst;
  std::vector<float> wavg;
  for (int l = 0; l < L; ++l) {
    const float* const* P = params + (size_t)l * np;
    // EE = BondEmb W_enc^T + b_enc
    first.push_back(sprob(BE, H, P[0], H, P[1], EE[l], F, R, F, H, GNX_SB_B_TRANS));
    for (int t = 0; t < T; ++t) {
      const float* W0 = P[4 + t * per];
      // Te[:, t] = EE W_e^T + b  (the edge slice of pre-layer 0 on the bond table): needs EE -> second launch
      second.push_back(sprob(EE[l], F, W0 + 2 * F, 3 * F, P[4 + t * per + 1], Te[l] + t * F, H, R, F, F, GNX_SB_B_TRANS));
      if (D > 0) {
        wsrc.push_back(P[4 + t * per + 2 * pre_layers]);
        wdst.push_back(weff[(size_t)l * T + t]);
        wavg.push_back(avg_deg_log[l]);
      }
      if (merged) {
        const int k = 4 + t * per + 2 * (pre_layers + post_layers - 1);
        // Wm[:, t] = lin_w[:, t] @ W_last_t ;  bm (+)= b_last_t @ lin_w[:, t]^T (+ lin_b with the first tower)
        first.push_back(sprob(P[2] + t * F, H, P[k], F, nullptr, Wm[l] + t * F, H, H, F, F, 0));
        if (t == 0)
          first.push_back(sprob(P[k + 1], F, P[2], H, P[3], bm[l], H, 1, H, F, GNX_SB_B_TRANS));
        else  // further towers add on top of the previous one's result, one launch later each: a deterministic forward
          (t == 1 ? second : later[t - 2])
              .push_back(sprob(P[k + 1], F, P[2] + t * F, H, nullptr, bm[l], H, 1, H, F, GNX_SB_B_TRANS | GNX_SB_ACCUMULATE));
      }
    }
  }
  GNX_TRY(gnx_gemm_small_batched(h, (int32_t)first.size(), first.data()));
  GNX_TRY(gnx_gemm_small_batched(h, (int32_t)second.size(), second.data()));
  for (auto& v : later) GNX_TRY(gnx_gemm_small_batched(h, (int32_t)v.size(), v.data()));
  if (D > 0)
    GNX_TRY(gnx_pna_weff_batched(h, (int32_t)wsrc.size(), wsrc.data(), 13 * F, F, D, wavg.data(), wdst.data()));
  return GNX_OK;
}

extern "C" int32_t gnx_pna_stack_finish(gnx_handle* h, const gnx_pna_finish_args* a) {
  GNX_CHECK_ARG(h && a, "gnx_pna_stack_finish: NULL argument");
  const int L = a->L, T = a->T, F = a->F, pre = a->pre_layers, post = a->post_layers, R = a->R, D = a->D;
  GNX_CHECK_ARG(L >= 1 && T >= 1 && T <= GNX_PNA_MAX_TOWERS && F >= 1 && pre >= 1 && post >= 1 && R >= 1 && D >= 1,
                "gnx_pna_stack_finish: bad shape");
  GNX_CHECK_ARG(a->BE && a->acc_buf && a->ones && a->avg_deg_log && a->params && a->grads && a->EE && a->dTe && a->dEE &&
                    a->dWeff && (!a->merged || (a->dWm && a->dbm)), "gnx_pna_stack_finish: NULL array");
  const int H = T * F, per = 2 * (pre + post), np = 4 + T * per;
  const bool side = a->use_side_streams != 0;
  // ---- side stream 1: from every layer's dTe (by-code segment sums) to the bond-embedding gradient
  GNX_TRY(on_side(h, 1, side, [&]() -> int32_t {
    std::vector<gnx_small_prob> s1, s2;
    for (int l = 0; l < L; ++l) {
      const float* const* P = a->params + (size_t)l * np;
      float* const* G = a->grads + (size_t)l * np;
      for (int t = 0; t < T; ++t) {
        const int k0 = 4 + t * per;
        const float* dTe = a->dTe[l] + t * F;
        // d W0[:, 2F:3F] += dTe_t^T EE ;  d b0 += column sums of dTe_t ;  dEE += dTe_t W0[:, 2F:3F]
        s1.push_back(sprob(dTe, H, a->EE[l], F, nullptr, G[k0] + 2 * F, 3 * F, F, F, R, GNX_SB_A_TRANS | GNX_SB_ACCUMULATE));
        s1.push_back(sprob(a->ones, R, dTe, H, nullptr, G[k0 + 1], F, 1, F, R, GNX_SB_ACCUMULATE));
        s1.push_back(sprob(dTe, H, P[k0] + 2 * F, 3 * F, nullptr, a->dEE[l], F, R, F, F, GNX_SB_ATOMIC));
      }
      // d W_enc += dEE^T BondEmb ;  d b_enc += column sums of dEE ;  acc += dEE W_enc
      s2.push_back(sprob(a->dEE[l], F, a->BE, H, nullptr, G[0], H, F, H, R, GNX_SB_A_TRANS | GNX_SB_ACCUMULATE));
      s2.push_back(sprob(a->ones, R, a->dEE[l], F, nullptr, G[1], F, 1, F, R, GNX_SB_ACCUMULATE));
      s2.push_back(sprob(a->dEE[l], F, P[0], H, nullptr, a->acc_buf, H, R, H, F, GNX_SB_ATOMIC));
    }
    GNX_TRY(gnx_gemm_small_batched(h, (int32_t)s1.size(), s1.data()));
    return gnx_gemm_small_batched(h, (int32_t)s2.size(), s2.data());
  }));
  // ---- side stream 0, behind the layers' weight gradients: lin / last post layer from dWm, dbm; post-layer 0 from dWeff
  GNX_TRY(on_side(h, 0, side, [&]() -> int32_t {
    std::vector<const float*> dweff;
    std::vector<float*> dwp;
    std::vector<float> avg;
    std::vector<gnx_small_prob> u1, u2;
    for (int l = 0; l < L; ++l) {
      const float* const* P = a->params + (size_t)l * np;
      float* const* G = a->grads + (size_t)l * np;
      for (int t = 0; t < T; ++t) {
        dweff.push_back(a->dWeff[(size_t)l * T + t]);
        dwp.push_back(G[4 + t * per + 2 * pre]);
        avg.push_back(a->avg_deg_log[l]);
        if (!a->merged) continue;
        const int k = 4 + t * per + 2 * (pre + post - 1);
        const float* dWm = a->dWm[l] + t * F;
        const float* lin_w = P[2] + t * F;
        // d lin_w[:, t] += dWm[:, t] W_t^T (+ dbm b_t^T, one launch later: same output) ;  dW_t += lin_w[:, t]^T dWm[:, t] ;
        // db_t += dbm lin_w[:, t]
        u1.push_back(sprob(dWm, H, P[k], F, nullptr, G[2] + t * F, H, H, F, F, GNX_SB_B_TRANS | GNX_SB_ACCUMULATE));
        u2.push_back(sprob(a->dbm[l], 1, P[k + 1], 1, nullptr, G[2] + t * F, H, H, F, 1, GNX_SB_B_TRANS | GNX_SB_ACCUMULATE));
        u1.push_back(sprob(lin_w, H, dWm, H, nullptr, G[k], F, F, F, H, GNX_SB_A_TRANS | GNX_SB_ACCUMULATE));
        u1.push_back(sprob(a->dbm[l], H, lin_w, H, nullptr, G[k + 1], F, 1, F, H, GNX_SB_ACCUMULATE));
      }
      if (a->merged)  // d lin_b += dbm
        u1.push_back(sprob(a->ones, 1, a->dbm[l], H, nullptr, G[3], H, 1, H, 1, GNX_SB_ACCUMULATE));
    }
    GNX_TRY(gnx_pna_weff_bwd_batched(h, (int32_t)dweff.size(), dweff.data(), F, D, avg.data(), dwp.data(), 13 * F));
    GNX_TRY(gnx_gemm_small_batched(h, (int32_t)u1.size(), u1.data()));
    return gnx_gemm_small_batched(h, (int32_t)u2.size(), u2.data());
  }));
  return GNX_OK;
}
