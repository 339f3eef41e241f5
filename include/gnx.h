/*
 * gnx.h — C ABI of libgnnepcsaft_hip.so: the MI355X (gfx950) kernels behind gnnepcsaft's GNN forward/backward.
 *
 * The reference has no FFI for this path: the arithmetic sits in torch_geometric / ogb Python modules that
 * /root/reference/gnnepcsaft/train/models.py only wires together.  Each entry point below therefore cites the
 * reference call site (ref: = /root/reference/gnnepcsaft/...) and the third-party op [3P] it stands in for.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch types.
 *  - every function returns int32 status: 0 = ok, <0 = error (GNX_E_*); text via gnx_last_error() (thread-local).
 *  - the library never allocates or frees tensor memory: all buffers (inputs, outputs, workspaces) are caller-owned
 *    DEVICE pointers (hipMalloc / torch tensors' data_ptr()); workspace sizes are queried with *_workspace_bytes.
 *    (The handle itself owns 4.25 KiB of device memory for the sticky range flag, allocated in gnx_create.)
 *  - all launches go on the handle's stream (gnx_set_stream; default = the NULL stream) and are asynchronous.
 *    Only gnx_check_range (integer input validation read-back) and gnx_prof_end synchronise that stream.
 *  - all float tensors are fp32 row-major; "ld" = leading dimension in elements.  Index tensors handed over by the
 *    caller in the reference's layout are int64; everything the library produces is int32.
 *  - NO gnx_comm_* entry points (SURVEY.md §8b lists gnx_comm_init / gnx_allreduce_f32 as the stand-in for Lightning
 *    DDP's gradient exchange, ref: train/train.py:85-88): the exchange is torch.distributed's "nccl" backend = the RCCL
 *    that PyTorch-ROCm bundles, driven by gnnepcsaft_amd/dp.py on this library's side stream (gnx_side_stream).  A second
 *    RCCL linked into this library would live beside torch's copy in the same process; gnx_scale (below) is the only
 *    arithmetic of the exchange (sum -> average).
 *  - no hidden global state except the opaque gnx_handle (device id, stream, options, profiling events).  The GNX_*
 *    environment variables are read ONCE, in gnx_create, as initial option values; no entry point reads the
 *    environment afterwards (gnx_set_option changes an option at run time).
 */
#ifndef GNX_H_
#define GNX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNX_ABI_VERSION 7

enum {
  GNX_OK = 0,
  GNX_E_INVALID = -1,   /* bad argument (shape, alignment, null pointer) */
  GNX_E_HIP = -2,       /* HIP runtime error; see gnx_last_error() */
  GNX_E_RANGE = -3,     /* integer input out of range (node id >= N, feature >= vocab, unsorted batch) */
  GNX_E_WORKSPACE = -4  /* workspace too small */
};

typedef struct gnx_handle gnx_handle;

/* ---- lifecycle --------------------------------------------------------------------------------------------- */
int32_t gnx_create(gnx_handle** out, int32_t device);
int32_t gnx_destroy(gnx_handle* h);
int32_t gnx_set_stream(gnx_handle* h, void* hip_stream);
const char* gnx_last_error(void);
int32_t gnx_abi_version(void);

/* A/B switches of the handle (kernel selection only; every setting computes the same function).  Initial value = the
 * environment variable of the same name with the GNX_ prefix (e.g. GNX_GEMM_SPLIT=0), read once in gnx_create. */
enum {
  GNX_OPT_GEMM_SPLIT = 0,        /* 1: products with >= 4096 rows as three-bf16-piece split products; 0: fp32 MFMA */
  GNX_OPT_WGRAD_WGS = 1,         /* > 0: target workgroup count of the weight-gradient kernels (default: #CUs) */
  GNX_OPT_EMBED_BWD_MFMA = 2,    /* atom-embedding gradient as a one-hot MFMA product for N >= 256: 1 = scattered bf16 one-hot x three-piece gradient (tables of <= 192 rows), 2 = computed fp32 one-hot on the fp32 matrix pipe, 0 = LDS atomics */
  GNX_OPT_STD_BWD_CENTERED = 3,  /* 1: std gradient divides by the centred two-pass std (see gnx_pna_aggregate_bwd) */
  GNX_OPT_GEMM_PIPE = 4,         /* 1: tiled split products with >= 8 K-tiles per tile take the software-pipelined kernel (bit-identical results) */
  GNX_OPT_WGRAD_PIPE = 5,        /* 1: split weight gradients of 16-byte aligned operands through the software-pipelined kernel */
  GNX_OPT_GEMM_AS = 6,           /* 1: split products with one segment, 96 < K <= 128 and N >= 256 take the activation-stationary kernel (the row tile is split once for all column tiles; bit-identical results) */
  GNX_OPT_GEMM_WS_FAST = 7,      /* the weights-stationary split kernel's predicate-free form (quad-transposed 16-byte stores, exact waits) for N = 128, aligned operands, no accumulate: 2 = as two 4-wave workgroups per CU on 32-row tiles (default), 1 = one 8-wave workgroup per CU on 64-row tiles, 0 = the predicated kernel; bit-identical results */
  GNX_OPT_GEMM_TILE_ROWS = 8,    /* 96 / 128: row-tile height of the pipelined tiled product (0: chosen per launch; bit-identical results) */
  GNX_OPT_GEMM_MID = 9,          /* 1: products with M < 4096 rows and <= 48 tiles of 128 x 128 run on 16 x 16 patches (k_gemm_mid) instead of the latency-bound tiled kernel */
  GNX_OPT_DA_AGG_FUSED = 10,     /* 1: a PNA layer's dA product and scatter-aggregate backward run as one launch per tower where eligible (gnx_pna_da_aggregate_bwd; bit-identical results) */
  GNX_OPT_COUNT = 11
};
int32_t gnx_set_option(gnx_handle* h, int32_t opt, int32_t value);
int32_t gnx_get_option(gnx_handle* h, int32_t opt, int32_t* value);

/* ---- profiling hook (bench.py's live per-kernel timing; HIP events on the handle's stream) ------------------- */
/* kernel ids (groups of kernels with one roofline) */
enum {
  GNX_K_NONE = 0,
  GNX_K_PNA_AGG_FWD = 1,        /* scatter-aggregate forward (the metric's roofline kernel) */
  GNX_K_PNA_AGG_BWD = 2,
  GNX_K_GEMM_WS = 3,            /* weights-stationary products (K, N <= 128) */
  GNX_K_GEMM_WGRAD = 4,         /* single / per-degree-class weight gradients */
  GNX_K_GINE_AGG_FWD = 5,
  GNX_K_GINE_AGG_BWD = 6,
  GNX_K_EDGE_COMBINE_FWD = 7,
  GNX_K_EDGE_COMBINE_BWD = 8,
  GNX_K_BN_FWD = 9,
  GNX_K_BN_BWD = 10,
  GNX_K_GEMM_TILED = 11,        /* tiled multi-segment / degree-class-grouped products (incl. their weight split) */
  GNX_K_GEMM_SMALL = 12,        /* M <= 256 products (60-row bond-table chain, merged H x H weights) */
  GNX_K_GEMM_WGRAD_BATCHED = 13,/* a layer's weight gradients in one launch */
  GNX_K_KEY_SEGMENT_SUM = 14,   /* bond-table gradient through the inverted index */
  GNX_K_EMBED = 15,             /* embedding sums, forward and backward */
  GNX_K_PNA_EDGE_FWD = 16,      /* fused message assembly -> pre-layer 1 -> scatter-aggregate (gnx_pna_edge_fwd) */
  GNX_K_PNA_EDGE_BWD = 17,      /* fused masked input gradient of pre-layer 1 + destination sums + bond-table sums (gnx_pna_edge_bwd) */
  GNX_K_ATTN_FWD = 18,          /* TransformerConv segmented-softmax attention forward (gnx_transformer_attn_fwd) */
  GNX_K_ATTN_BWD = 19,          /* its destination- and source-side backward passes (gnx_transformer_attn_bwd) */
  GNX_K_PCSAFT_RHO = 20,        /* PC-SAFT liquid density at (T, P), fp64 (gnx_pcsaft_density) */
  GNX_K_PCSAFT_VP = 21,         /* PC-SAFT vapour pressure at T, fp64 (gnx_pcsaft_vapor_pressure) */
  GNX_K_PCSAFT_MIX_STATE = 22,  /* mixture PC-SAFT a_res, p, dp/drho at (T, rho, x), fp64 (gnx_pcsaft_mix_state) */
  GNX_K_PCSAFT_MIX_RHO = 23,    /* mixture PC-SAFT liquid density at (T, P, x), fp64 (gnx_pcsaft_mix_density) */
  GNX_K_PCSAFT_MIX_LNPHI_STATE = 24, /* mixture PC-SAFT ln phi_i, Z at (T, rho, x), fp64 (gnx_pcsaft_mix_lnphi_state) */
  GNX_K_PCSAFT_MIX_LNPHI = 25,  /* mixture PC-SAFT ln phi_i at the liquid root of (T, P, x), fp64 (gnx_pcsaft_mix_lnphi) */
  GNX_K_COUNT = 26
};
/* start recording a HIP event pair around every launch of the kernels whose id bit is set in kernel_mask
 * (bit k = GNX_K_* id k).  Events go on the handle's stream, i.e. the stream the kernels run on. */
int32_t gnx_prof_begin(gnx_handle* h, uint32_t kernel_mask);
/* synchronise the stream; #launches of kernel group `kid` seen since gnx_prof_begin, their summed duration (ms), and
 * the sums of what the launches were given to do: ALGORITHMIC bytes (operands read + results written once, fp32 /
 * int32), algorithmic FLOPs (2 M N K of the products) and the bf16-MFMA FLOPs actually executed (6 x the
 * algorithmic ones on the split-operand kernels, 0 on fp32-MFMA kernels).  Any of the three may be NULL. */
int32_t gnx_prof_read(gnx_handle* h, int32_t kid, int64_t* launches, double* total_ms, double* alg_bytes,
                      double* alg_flops, double* mfma_bf16_flops);
/* stop recording and drop the recorded events. */
int32_t gnx_prof_end(gnx_handle* h);

/* ---- input packer: PyG-style COO batch -> dst-sorted CSR (+ by-source index) ------------------------------- */
/* Replaces what PNAConv/GINEConv's MessagePassing.propagate [3P] does implicitly with edge_index on every call
 * (ref: train/models.py:212-214), and utils.degree [3P] (ref: train/models.py:445-457 via DegreeScalerAggregation).
 *   edge_index int64[2,E] (row 0 = source j, row 1 = target i), N nodes.
 *   rowptr  int32[N+1]  CSR by target;  perm int32[E]: CSR position p -> original edge id, STABLE (ascending inside a
 *   row, i.e. the order scatter_add_ visits them);  src int32[E], dst int32[E]: endpoints in CSR order;
 *   colptr int32[N+1], cpos int32[E]: for every source node the ascending list of CSR positions leaving it.
 * Bit-exact integer work.  Out-of-range node ids are clamped and set the handle's sticky range flag (bit 0), which
 * gnx_check_range reports (the only synchronising call), so a training loop can validate once per step.
 * gnx_pack_csr is gnx_pack_batch (below) with no optional part, no edge_attr and no batch: its first 6 launches (5 with
 * E = 0; 17 above gnx_pack_batch_scan_bound() nodes).  ws: gnx_pack_csr_workspace_bytes(N, E), which is
 * gnx_pack_batch_workspace_bytes(N, E, 1, 1) plus room for the bond codes and graph_ptr that those launches also write;
 * a shorter one is GNX_E_WORKSPACE and nothing is launched.  E = 0: the edge arrays may be NULL. */
size_t gnx_pack_csr_workspace_bytes(int64_t N, int64_t E);
int32_t gnx_pack_csr(gnx_handle* h, const int64_t* edge_index, int64_t E, int64_t N, int32_t* rowptr, int32_t* perm,
                     int32_t* src, int32_t* dst, int32_t* colptr, int32_t* cpos, void* ws, size_t ws_bytes);
/* mixed-radix code of the K integer features of every row, gathered through perm (perm may be NULL = identity):
 *   code[p] = ((f[perm[p],0]*dims[1] + f[perm[p],1])*dims[2] + ...) ; dims is a HOST array of K vocab sizes.
 * Used for edge_attr int64[E,3] -> bond code in [0,60) (vocab ref: data/ogb_utils.py:24-33). Range-checked lazily (sticky flag bit 1).
 * ws: unused (may be NULL). */
int32_t gnx_feature_code(gnx_handle* h, const int64_t* feat, int64_t rows, int32_t K, const int32_t* dims,
                         const int32_t* perm, int32_t* code, void* ws, size_t ws_bytes);
/* batch int64[N] (non-decreasing graph id per node, PyG Batch.batch) -> graph_ptr int32[B+1]. Range/sortedness
 * checked lazily (sticky flag bits 2/3). ws: unused (may be NULL). */
int32_t gnx_graph_ptr(gnx_handle* h, const int64_t* batch, int64_t N, int64_t B, int32_t* graph_ptr, void* ws,
                      size_t ws_bytes);
/* PNA degree scalers [3P DegreeScalerAggregation]: amp[n] = log(d+1)/avg_deg_log, att[n] = avg_deg_log/log(max(d,1)+1),
 * d = rowptr[n+1]-rowptr[n]. */
int32_t gnx_degree_scalers(gnx_handle* h, const int32_t* rowptr, int64_t N, float avg_deg_log, float* amp, float* att);

/* ---- on-device batch collation from a device-resident dataset (gnnepcsaft_amd/data/device.py) ------------------
 * Replaces, for training batches, torch_geometric's DataLoader -> Batch.from_data_list [3P] on the host
 * (ref: train/train.py:59-75).  The dataset is stored on the device as the concatenation of its G graphs:
 *   node_ptr / edge_ptr int64[G+1] (offsets of every graph's nodes / edges), x int64[sumN,9],
 *   edge_index int64[2,E_src] holding GRAPH-LOCAL node ids (E_src = sumE), edge_attr int64[E_src,3].
 * A batch is idx int64[B]: slot b takes graph idx[b] (repeats allowed).  An idx[b] outside [0,G) is clamped and sets
 * the sticky range flag (bit 7, gnx_check_range).  Integer copies with plain stores: bit-identical from call to call.
 * gnx_collate_ptr: out_ptr / out_eptr int64[B+1] = exclusive prefix sums of the selected graphs' node / edge counts
 *   (out_ptr = Batch.ptr).  No workspace; 1 launch for B <= 1024, 3 above.  1 <= B < 2^31. */
int32_t gnx_collate_ptr(gnx_handle* h, const int64_t* node_ptr, const int64_t* edge_ptr, int64_t G, const int64_t* idx,
                        int64_t B, int64_t* out_ptr, int64_t* out_eptr);
/* the batch itself from the gnx_collate_ptr offsets: x_out int64[N,9], edge_index_out int64[2,E] (out_ptr[b] added),
 * edge_attr_out int64[E,3], batch_out int64[N] (= b).  N and E are the totals the caller allocated for (it keeps the
 * graph sizes on the host, nothing is read back); a block that would not fit them is cut and sets flag bit 7. */
int32_t gnx_collate_gather(gnx_handle* h, const int64_t* node_ptr, const int64_t* edge_ptr, int64_t G, const int64_t* x,
                           const int64_t* edge_index, const int64_t* edge_attr, int64_t E_src, const int64_t* idx,
                           int64_t B, const int64_t* out_ptr, const int64_t* out_eptr, int64_t N, int64_t E,
                           int64_t* x_out, int64_t* edge_index_out, int64_t* edge_attr_out, int64_t* batch_out);
/* dst[b,:] = src[idx[b],:] for a one-row-per-graph field (para, assoc, ...): src [G,K], dst [B,K], elements of
 * elem_bytes = 4 or 8 bytes moved as raw words (any dtype of that size). */
int32_t gnx_collate_rows(gnx_handle* h, const void* src, int64_t G, const int64_t* idx, int64_t B, int32_t elem_bytes,
                         int32_t K, void* dst);

/* ---- embeddings: AtomEncoder / BondEncoder [3P ogb] (ref: train/models.py:175-176, 205-206) ----------------- */
/* out[n,:] = sum_{k<K} table[offsets[k] + idx[n,k], :], summed left to right in fp32 (bit-exact with the CPU path).
 * idx int64[N,K]; table fp32[R,H] = the K embedding tables stacked; offsets: HOST int32[K+1] (row offsets, last = R).
 * Range-checked lazily: an out-of-range index poisons nothing (it is clamped) and sets the handle's sticky range
 * flag, reported by the next gnx_pack_* / gnx_check_range call. */
int32_t gnx_embed_sum_fwd(gnx_handle* h, const int64_t* idx, int64_t N, int32_t K, const int32_t* offsets,
                          const float* table, int32_t H, float* out);
/* dtable[R,H] += scatter-add of dout[N,H] (embedding_dense_backward): per-workgroup LDS tables (<= 256 rows), then a
 * two-stage fold through the caller's workspace (gnx_table_scatter_workspace_bytes(N, R, H); ws may be NULL = direct
 * atomics, slower: hundreds of workgroups adding into the same few KB serialise at the memory-side atomic units). */
size_t gnx_table_scatter_workspace_bytes(int64_t rows, int32_t R, int32_t H);
int32_t gnx_embed_sum_bwd(gnx_handle* h, const int64_t* idx, int64_t N, int32_t K, const int32_t* offsets,
                          int32_t R, const float* dout, int32_t H, float* dtable, void* ws, size_t ws_bytes);
int32_t gnx_check_range(gnx_handle* h); /* sync; GNX_E_RANGE if any lazy check tripped since the last call */

/* ---- dense contractions on the matrix cores ------------------------------------------------------------------
 * Arithmetic: products with >= 4096 rows evaluate every fp32 operand as an exact sum of three bf16 pieces and the
 * product as six v_mfma_f32_32x32x16_bf16 with fp32 accumulation (fp32-faithful: dropped terms <= 2^-25 |a||b|;
 * DESIGN.md §2); smaller products, row-scaled segments and GNX_OPT_GEMM_SPLIT = 0 use v_mfma_f32_32x32x2_f32. */
/* One A-operand segment of a K-concatenated product.  The product is
 *     C[m,n] (+)= act( sum_s  sum_{k<K_s} (rs_s[m] * A_s[m,k]) * B_s(k,n)  + bias[n] )        m<M, n<N
 *   b_trans = 1 ("NT", forward Linear):   B_s(k,n) = B_s[n*ldb + k]   (weight [out,in] row-major, PyG/torch layout)
 *   b_trans = 0 ("NN", input gradient):   B_s(k,n) = B_s[k*ldb + n]
 * rowscale may be NULL (=1).  Segments let the caller feed torch.cat([...], dim=-1) operands without materialising
 * them: PNAConv's [x_i || x_j || e] pre-layer and the 13F-wide [x || A || amp*A || att*A] post-layer
 * ([3P] PNAConv.message / DegreeScalerAggregation; ref: train/models.py:445-457). */
typedef struct {
  const float* a;        /* [M, k] with leading dimension lda */
  int64_t lda;
  const float* rowscale; /* [M] or NULL */
  const float* b;        /* segment's slice of the weight */
  int64_t ldb;
  int32_t k;
  int32_t _pad;
} gnx_gemm_seg;

enum {
  GNX_GEMM_RELU = 1,       /* C = max(.,0) */
  GNX_GEMM_ACCUMULATE = 2, /* C += (applied before relu; relu+accumulate is rejected) */
  GNX_GEMM_B_TRANS = 4,    /* NT */
  GNX_GEMM_SPLIT_ONLY = 8, /* only write the split weight images this call would use into ws (nothing else is launched; a call that
                              needs no images does nothing): lets the caller run the split ahead of the product, on another stream */
  GNX_GEMM_PRESPLIT = 16   /* ws already holds those images (a GNX_GEMM_SPLIT_ONLY call with the same arguments) */
};
/* mask (optional, may be NULL): multiply the result by (mask[m*ldmask+n] > 0) — ReLU backward fused in dgrad.
 * ws / ws_bytes: caller-owned device scratch for the split weight images of the tiled split-operand kernel, size from
 * gnx_gemm_workspace_bytes with the same arguments (0 = this call needs none).  ws == NULL is allowed: the product
 * then runs on the fp32-MFMA kernel.  A non-NULL workspace that is too small returns GNX_E_WORKSPACE.  The scratch is
 * free for reuse as soon as the launches of this call have run (stream order). */
size_t gnx_gemm_workspace_bytes(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                                int32_t num_classes, int64_t M, int32_t N, const float* mask, int32_t flags,
                                int32_t grouped);
int32_t gnx_gemm(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, int64_t M, int32_t N, const float* bias,
                 const float* mask, int64_t ldmask, float* C, int64_t ldc, int32_t flags, void* ws, size_t ws_bytes);
/* weight gradient ("TN"): dW[n, k] += sum_m dC[m,n] * (rs[m] * A[m,k]),  n<N, k<K.  Split over M across workgroups,
 * fp32 atomics into dW (caller zeroes or accumulates).  dbias (optional) += column sums of dC. */
int32_t gnx_gemm_wgrad(gnx_handle* h, const float* dC, int64_t lddc, const float* A, int64_t lda,
                       const float* rowscale, int64_t M, int32_t N, int32_t K, float* dW, int64_t lddw, float* dbias);

/* several independent weight gradients in ONE launch (a layer's same-shaped dW += dC^T (rs*A) products share the grid:
 * every workgroup gets an nprob x longer row range, so the atomic flush per problem shrinks nprob x).  nprob <= 8;
 * every operand 16-byte aligned with leading dimensions, N and K multiples of 4. */
typedef struct {
  const float* dC;       /* [M, N], ld lddc */
  int64_t lddc;
  const float* A;        /* [M, K], ld lda */
  int64_t lda;
  const float* rowscale; /* [M] or NULL */
  float* dW;             /* [N, K], ld lddw (accumulated) */
  int64_t lddw;
  float* dbias;          /* [N] or NULL (accumulated) */
  int64_t M;
  int32_t N, K;
} gnx_wgrad_prob;
int32_t gnx_gemm_wgrad_batched(gnx_handle* h, int32_t nprob, const gnx_wgrad_prob* probs);

/* several independent SMALL products (M, N <= a few hundred rows: the 60-row bond-table chain, the merged H x H weights
 * and their gradients) in one launch -- for all layers of a model at once instead of ~9 launches of ~8 us per layer:
 *     C (+)= act( op(A) op(B) + bias )     op(A) = A [M,K] or, with GNX_SB_A_TRANS, A stored [K,M] (a TN weight gradient);
 *                                          op(B): GNX_SB_B_TRANS = B stored [N,K] (torch weight layout), else [K,N].
 * GNX_SB_ACCUMULATE: plain read-modify-write (outputs of the launch's problems must then be disjoint);
 * GNX_SB_ATOMIC: fp32 atomic adds (several problems may add into one output; the output must be initialised). */
enum { GNX_SB_A_TRANS = 1, GNX_SB_B_TRANS = 2, GNX_SB_ACCUMULATE = 4, GNX_SB_ATOMIC = 8, GNX_SB_RELU = 16 };
#define GNX_SMALL_BATCH 32
typedef struct {
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  const float* bias; /* [N] or NULL */
  float* C;
  int64_t ldc;
  int32_t M, N, K;
  int32_t flags;
} gnx_small_prob;
int32_t gnx_gemm_small_batched(gnx_handle* h, int32_t nprob, const gnx_small_prob* probs); /* probs: HOST array */

/* ---- in-degree classes: PNA post-layer 0 with one effective weight per degree ------------------------------- */
/* amp/att of [3P] DegreeScalerAggregation depend on the in-degree d only, so
 *     [x | A | amp*A | att*A] W^T  =  x W0^T + A (W1 + amp(d) W2 + att(d) W3)^T  =  x W0^T + A Weff(d)^T
 * with rows grouped by d: 26 N F^2 -> 10 N F^2 FLOPs for the widest product of the layer (ref: train/models.py:445-457).
 * gnx_degree_max: max in-degree (synchronises; the host needs D = max+1 to size buffers; D <= 64 for grouping).
 * gnx_degree_classes: dperm int32[N] = node ids stably sorted by in-degree, cls_ptr int32[D+1] = class boundaries.
 * gnx_class_tiles: tile_info int32[3*(N/tile_rows + D)] = (first position in dperm, #rows, class) per tile, tiles
 * never straddle classes; ntiles int32[1] (device) = number of tiles. */
int32_t gnx_degree_max(gnx_handle* h, const int32_t* rowptr, int64_t N, int32_t* max_degree_host);
size_t gnx_degree_classes_workspace_bytes(int64_t N, int32_t D);
int32_t gnx_degree_classes(gnx_handle* h, const int32_t* rowptr, int64_t N, int32_t D, int32_t* dperm,
                           int32_t* cls_ptr, void* ws, size_t ws_bytes);
int32_t gnx_class_tiles(gnx_handle* h, const int32_t* cls_ptr, int32_t D, int32_t tile_rows, int32_t* tile_info,
                        int32_t* ntiles);
/* gnx_gemm over class tiles: workgroup t handles rows row_index[tile_info[3t] .. +tile_info[3t+1]) (gathered A rows,
 * scattered C rows) and reads segment s's B at b + class * cls_strides[s] (cls_strides: HOST int64[nseg], 0 = shared).
 * num_classes = number of weight sets behind every non-zero stride (class ids in tile_info are < num_classes).
 * Launches max_tiles workgroups; those >= *ntiles exit. */
int32_t gnx_gemm_grouped(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                         int32_t num_classes, int64_t M, int32_t N, const float* bias, const float* mask,
                         int64_t ldmask, float* C, int64_t ldc, int32_t flags, const int32_t* row_index,
                         const int32_t* tile_info, const int32_t* ntiles, int64_t max_tiles, void* ws, size_t ws_bytes);
/* The same over a tile table built with tile_rows = 96 or 128 (gnx_gemm_grouped assumes 128).  gnx_gemm_tile_rows: the
 * height to build it with for M rows x N columns -- 96 where 128-row tiles would leave the last round of the persistent
 * workgroups mostly idle (cfg-2: 640 tiles on 512 workgroup slots), else 128; results are bit-identical either way. */
int32_t gnx_gemm_tile_rows(gnx_handle* h, int64_t M, int32_t N);
int32_t gnx_gemm_grouped_rows(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                              int32_t num_classes, int64_t M, int32_t N, const float* bias, const float* mask,
                              int64_t ldmask, float* C, int64_t ldc, int32_t flags, const int32_t* row_index,
                              const int32_t* tile_info, const int32_t* ntiles, int64_t max_tiles, void* ws,
                              size_t ws_bytes, int32_t tile_rows);
/* Which kernel such a call takes, without launching anything or touching device memory: the arguments of
 * gnx_gemm_grouped_rows (row_index = tile_info = ntiles = NULL: an ungrouped call, as gnx_gemm's; tile_rows = 0: 128-row
 * table, as gnx_gemm_grouped's).  With GNX_GEMM_SPLIT_ONLY `kernel` is the kernel the images are written for, or
 * GNX_GEMM_KERNEL_NONE where the call does nothing. */
enum {
  GNX_GEMM_KERNEL_NONE = 0,          /* nothing is launched (M = 0, or GNX_GEMM_SPLIT_ONLY without images) */
  GNX_GEMM_KERNEL_TILED_VEC = 1,     /* k_gemm, 16-byte loads */
  GNX_GEMM_KERNEL_TILED_GENERIC = 2, /* k_gemm, element-wise loads */
  GNX_GEMM_KERNEL_WS = 3,            /* k_gemm_ws */
  GNX_GEMM_KERNEL_WS3 = 4,           /* k_gemm_ws3, predicated, 8 waves */
  GNX_GEMM_KERNEL_WS3_FAST8 = 5,     /* k_gemm_ws3, predicate-free, 8 waves on 64-row tiles */
  GNX_GEMM_KERNEL_WS3_FAST4 = 6,     /* k_gemm_ws3, predicate-free, 4 waves on 32-row tiles */
  GNX_GEMM_KERNEL_GEMM3 = 7,         /* k_gemm3 */
  GNX_GEMM_KERNEL_GEMM3P_96 = 8,     /* k_gemm3p, 96-row tiles */
  GNX_GEMM_KERNEL_GEMM3P_128 = 9,    /* k_gemm3p, 128-row tiles */
  GNX_GEMM_KERNEL_AS3 = 10,          /* k_gemm_as3 */
  GNX_GEMM_KERNEL_MID = 11,          /* k_gemm_mid */
  GNX_GEMM_KERNEL_SMALL = 12,        /* k_gemm_small_batched */
  GNX_GEMM_KERNEL_COUNT = 13
};
typedef struct {
  int32_t kernel;                  /* GNX_GEMM_KERNEL_* */
  int32_t tile_rows;               /* rows per workgroup tile */
  uint32_t grid_x, grid_y, block;  /* launch dimensions */
  int32_t runs_split;              /* 1: the call launches k_split_weights first */
  size_t image_bytes;              /* = gnx_gemm_workspace_bytes */
} gnx_gemm_plan_info;
int32_t gnx_gemm_plan(gnx_handle* h, int32_t nseg, const gnx_gemm_seg* segs, const int64_t* cls_strides,
                      int32_t num_classes, int64_t M, int32_t N, const float* bias, const float* mask, int64_t ldmask,
                      float* C, int64_t ldc, int32_t flags, const int32_t* row_index, const int32_t* tile_info,
                      const int32_t* ntiles, int64_t max_tiles, void* ws, size_t ws_bytes, int32_t tile_rows,
                      gnx_gemm_plan_info* out);
/* per-class weight gradient: dW_cls[c] (stride dw_cls_stride) += sum over the rows of class c of dC[row]^T A[row]. */
int32_t gnx_gemm_wgrad_grouped(gnx_handle* h, const float* dC, int64_t lddc, const float* A, int64_t lda, int64_t M,
                               int32_t N, int32_t K, float* dW_cls, int64_t lddw, int64_t dw_cls_stride,
                               const int32_t* row_index, const int32_t* chunk_info, const int32_t* nchunks,
                               int64_t max_chunks);
/* Which kernel that call takes and how it shares out the chunk table, without launching anything or touching device
 * memory.  k_gemm_wgrad3p_grouped takes the calls on the split-operand path (M >= 4096, GNX_OPT_GEMM_SPLIT) whose operands
 * are 16-byte aligned with lddc, lda, N, K multiples of 4 and M * ld < 2^32, unless GNX_OPT_WGRAD_PIPE is 0.  Its workgroup
 * (w, n tile, k tile) walks the chunks [w S, (w + 1) S) and merges consecutive chunks of one class into one row range:
 * ranges = max(1, budget / (n tiles * k tiles)), S = ceil(max_chunks / ranges), grid_x = ceil(max_chunks / S); the budget
 * is GNX_OPT_WGRAD_WGS when that is > 0.  The other kernels run one workgroup per chunk (grid_x = max_chunks). */
enum {
  GNX_WGRAD_KERNEL_NONE = 0,            /* nothing is launched (M = 0) */
  GNX_WGRAD_KERNEL_F32_VEC = 1,         /* k_gemm_wgrad<true, true> */
  GNX_WGRAD_KERNEL_F32_GENERIC = 2,     /* k_gemm_wgrad<false, true> */
  GNX_WGRAD_KERNEL_SPLIT3 = 3,          /* k_gemm_wgrad3<true> */
  GNX_WGRAD_KERNEL_SPLIT3P_GROUPED = 4, /* k_gemm_wgrad3p_grouped */
  GNX_WGRAD_KERNEL_COUNT = 5
};
typedef struct {
  int32_t kernel;                          /* GNX_WGRAD_KERNEL_* */
  int32_t ranges, chunks_per_range;        /* as above (whichever kernel is taken) */
  uint32_t grid_x, grid_y, grid_z, block;  /* launch dimensions */
} gnx_wgrad_grouped_plan_info;
int32_t gnx_gemm_wgrad_grouped_plan(gnx_handle* h, int64_t lddc, int64_t lda, const float* dC, const float* A, int64_t M,
                                    int32_t N, int32_t K, int64_t max_chunks, gnx_wgrad_grouped_plan_info* out);
/* Weff[d][o][j] = W[o][F+j] + amp(d) W[o][5F+j] + att(d) W[o][9F+j]  (W = post_nns[t][0].weight [F,13F], ld ldw);
 * gnx_pna_weff_bwd: dW[:,F:5F] += sum_d dWeff[d]; dW[:,5F:9F] += sum_d amp(d) dWeff[d]; dW[:,9F:13F] += sum_d att(d).. */
int32_t gnx_pna_weff(gnx_handle* h, const float* W, int64_t ldw, int32_t F, int32_t D, float avg_deg_log, float* Weff);
int32_t gnx_pna_weff_bwd(gnx_handle* h, const float* dWeff, int32_t F, int32_t D, float avg_deg_log, float* dW,
                         int64_t lddw);
/* gnx_pna_weff for n (layer, tower) pairs in one launch: W / Weff HOST arrays of n device pointers, avg_deg_log HOST [n] */
int32_t gnx_pna_weff_batched(gnx_handle* h, int32_t n, const float* const* W, int64_t ldw, int32_t F, int32_t D,
                             const float* avg_deg_log, float* const* Weff);
int32_t gnx_pna_weff_bwd_batched(gnx_handle* h, int32_t n, const float* const* dWeff, int32_t F, int32_t D,
                                 const float* avg_deg_log, float* const* dW, int64_t lddw);

/* ---- PNA message assembly (first pre-layer folded to node level) ------------------------------------------- */
/* h1[p,:] = relu(P[dst[p],:] + Q[src[p],:] + Te[code[p],:])  for CSR position p;  width = H.
 * ([3P] PNAConv.message: Linear(3F->F) on cat([x_i, x_j, e]) == W_i x_i + W_j x_j + (W_e e + b), then ReLU.) */
int32_t gnx_edge_combine_fwd(gnx_handle* h, const float* P, const float* Q, const float* Te, const int32_t* src,
                             const int32_t* dst, const int32_t* code, int64_t E, int32_t H, int32_t relu, float* h1);
/* given g[E,H] (already masked by relu'):  dP[i,:] = sum_{p in row i} g[p,:] ;  dQ[j,:] = sum_{p in cpos(j)} g[p,:] ;
 * dTe[R,H] += scatter-add by code (LDS-privatised, ws = gnx_table_scatter_workspace_bytes(E, R, H) or NULL).
 * dP/dQ are overwritten. */
int32_t gnx_edge_combine_bwd(gnx_handle* h, const float* g, const int32_t* rowptr, const int32_t* colptr,
                             const int32_t* cpos, const int32_t* code, int64_t N, int64_t E, int32_t H, int32_t R,
                             float* dP, float* dQ, float* dTe, void* ws, size_t ws_bytes);

/* inverted index by a small integer key (bond code): pos int32[E] = item ids stably grouped by key, ptr int32[R+1];
 * ws: gnx_degree_classes_workspace_bytes(E, R); R <= 64.  gnx_key_segment_sum: dtable[r,:] += sum_{items of key r} g[item,:]
 * as a gather-sum over contiguous index runs (no LDS atomics; (#chunks + R) x H global atomics). */
int32_t gnx_group_by_small_key(gnx_handle* h, const int32_t* keys, int64_t E, int32_t R, int32_t* pos, int32_t* ptr,
                               void* ws, size_t ws_bytes);
int32_t gnx_key_segment_sum(gnx_handle* h, const float* g, const int32_t* pos, const int32_t* key, int64_t E, int32_t H,
                            float* dtable);

/* ---- the scatter-aggregate: PNA mean|min|max|std over target nodes  (HBM-bound; the roofline kernel) ------- */
/* [3P] MultiAggregation([Mean,Min,Max,Std], mode='cat') as used by DegreeScalerAggregation
 * (aggregator list ref: train/models.py:443).  m fp32[E, T*F] in CSR order, rowptr int32[N+1].
 * A fp32[N, T, 4F]: per tower [mean || min || max || std].  Empty rows -> 0.  mean = (sequential sum in CSR order)/max(d,1);
 * std = sqrt(max(mean(x*x) - mean^2, 1e-5)) masked to 0 when <= sqrt(1e-5). */
int32_t gnx_pna_aggregate_fwd(gnx_handle* h, const float* m, const int32_t* rowptr, int64_t N, int64_t E, int32_t T,
                              int32_t F, float* A);
/* dm[E,T*F] from dA[N,T,4F]; min/max gradients split evenly over ties (scatter_reduce amin/amax backward);
 * std gradient 0 where the forward masked (the mask decision is the forward's, bit for bit).  Where it is not masked
 * the gradient is dstd (m - mean) / (n std): with GNX_OPT_STD_BWD_CENTERED (default) `std` is re-evaluated as
 * sqrt(sum (m - mean)^2 / n), which is accurate to fp32 rounding, instead of the forward's mean(x^2) - mean(x)^2 whose
 * cancellation error (~ eps mean(x^2) / (2 var) relative, up to 3e-5 just above the mask) the CPU path carries into
 * its gradient; 0 = divide by the forward's value like the CPU path does.  mean / min / max / std are recomputed from
 * the messages with the forward's arithmetic; A (the forward's output) is required but not read. */
int32_t gnx_pna_aggregate_bwd(gnx_handle* h, const float* dA, const float* m, const float* A, const int32_t* rowptr,
                              int64_t N, int64_t E, int32_t T, int32_t F, float* dm);

/* ---- fused PNA edge pipeline: message assembly -> pre-layer 1 -> scatter-aggregate in one kernel ---------------- */
/* [3P] PNAConv.message + DegreeScalerAggregation for pre_layers = 2 (ref: train/models.py:445-457, configs/default.py:44):
 *   h1[p] = relu(P[dst[p]] + Q[src[p]] + Te[code[p]]);  m[p] = h1[p] W1_t^T + b1_t per tower;  A[n] = mean|min|max|std of
 *   the CSR row of n -- the work of gnx_edge_combine_fwd + gnx_gemm + gnx_pna_aggregate_fwd without reading h1 or m back
 *   from HBM; h1, m and A come out bit-identical to that sequence.  h1 / m (fp32[E, T*F]) may be NULL (not kept).
 * Edge tiles: gnx_edge_tiles groups the destination nodes so that tile j = the nodes whose first CSR position lies in
 *   [tile_w j, tile_w (j+1)); tile_info int32[2 (count + 1)] = (first node, first CSR position) per tile, count =
 *   gnx_edge_tiles_count(E, tile_w).  With in-degrees <= maxdeg, tile_w = 65 - maxdeg keeps every tile within the kernel's
 *   64 message rows; a tile that exceeds them (a degree above the bound) drops rows and sets sticky range-flag bit 6
 *   (gnx_check_range).  W1 / b1: HOST arrays of T device pointers ([F,F] row-major [out,in], [F]).  F % 4 == 0, F <= 128,
 *   float operands 16-byte aligned. */
int32_t gnx_edge_tiles_count(int64_t E, int32_t tile_w);
int32_t gnx_edge_tiles(gnx_handle* h, const int32_t* rowptr, int64_t N, int64_t E, int32_t tile_w, int32_t* tile_info);

/* ---- a whole batch's integer structure in one call ---------------------------------------------------------------
 * gnx_pack_batch builds the CSR of gnx_pack_csr and writes what gnx_feature_code (through perm), gnx_graph_ptr,
 * gnx_degree_scalers (once per avg_deg_log), gnx_degree_classes, gnx_class_tiles (once per tile_rows),
 * gnx_group_by_small_key (of code) and gnx_edge_tiles write, bit for bit (clamped values and sticky range-flag bits on bad
 * input included), in 8 launches: 6 for the CSR, codes, graph_ptr and scalers, 2 more with any of the optional parts.
 * Above gnx_pack_batch_scan_bound() nodes the one scan launch becomes 6 per counter array, 19 in all.  No workgroup waits
 * for another, nothing is read back and nothing synchronises: the call captures into a HIP graph.
 *   edge_attr NULL: code = 0.  batch NULL: graph_ptr = [0, N] (B is ignored).
 *   parts: which optional outputs to build; an unbuilt part's pointers may be NULL and its buffers are not touched.
 *     GNX_PACK_CLASSES     dperm, cls_ptr and, per tile_rows[i] > 0, tiles[i] / ntiles[i]; D = max_degree + 1 <= 64 classes
 *     GNX_PACK_CODE_INDEX  code_pos, code_ptr (R <= 64 codes; E > 0)
 *     GNX_PACK_EDGE_TILES  edge_tiles with width edge_tile_w (E > 0, N > 0)
 *     GNX_PACK_TILED_SCAN  use the multi-launch scan whatever N is (tests, measurements)
 *   n_avg <= GNX_PACK_MAX_AVG degree-scaler pairs amp[i] / att[i] fp32[N] for avg_deg_log[i].
 * Buffer sizes are those of the single-purpose entries.  ws: gnx_pack_batch_workspace_bytes(N, E, max_degree + 1, R). */
#define GNX_PACK_MAX_AVG 4
#define GNX_PACK_CLASSES 1u
#define GNX_PACK_CODE_INDEX 2u
#define GNX_PACK_EDGE_TILES 4u
#define GNX_PACK_TILED_SCAN 256u
typedef struct {
  const int64_t* edge_index; /* [2, E] */
  const int64_t* edge_attr;  /* [E, K] or NULL */
  const int64_t* batch;      /* [N] or NULL */
  int64_t N, E, B;
  int32_t K;
  int32_t bond_dims[16];
  int32_t max_degree; /* the caller's bound of the in-degree: D - 1 */
  int32_t R;
  int32_t n_avg;
  float avg_deg_log[GNX_PACK_MAX_AVG];
  int32_t tile_rows[3]; /* 0 = no table */
  int32_t edge_tile_w;
  uint32_t parts;
  int32_t _pad;
  int32_t *rowptr, *perm, *src, *dst, *colptr, *cpos, *code, *graph_ptr;
  float* amp[GNX_PACK_MAX_AVG];
  float* att[GNX_PACK_MAX_AVG];
  int32_t *dperm, *cls_ptr;
  int32_t* tiles[3];
  int32_t* ntiles[3];
  int32_t *code_pos, *code_ptr;
  int32_t* edge_tiles;
  void* ws;
  size_t ws_bytes;
} gnx_pack_batch_args;
size_t gnx_pack_batch_workspace_bytes(int64_t N, int64_t E, int32_t D, int32_t R);
int32_t gnx_pack_batch(gnx_handle* h, const gnx_pack_batch_args* args);
/* gnx_pack_batch scans its counters in tiles of gnx_pack_batch_scan_chunk() and folds the tile offsets into the next
 * launch while a block can scan all tile sums, i.e. up to gnx_pack_batch_scan_bound() nodes */
int64_t gnx_pack_batch_scan_chunk(void);
int64_t gnx_pack_batch_scan_bound(void);
/* backward of the same stage in one pass over the message gradient ge [E, T*F] (CSR order):
 *   gh1[p] = (ge[p] W1_t) * (h1[p] > 0);  dP[n] = sum of gh1 over the CSR row of n;  dTe[c] += sum of gh1 over the positions
 *   with bond code c  (R <= 64 codes; dTe [R, T*F] is ACCUMULATED with one atomic add per (code, column) and workgroup).
 *   gh1 and dP bit-identical to gnx_gemm(mask = h1) + gnx_edge_combine_bwd; dQ stays gnx_edge_combine_bwd(dP = NULL). */
int32_t gnx_pna_edge_bwd(gnx_handle* h, const float* ge, const float* h1, const int32_t* code, const int32_t* rowptr,
                         const int32_t* tile_info, int32_t tile_w, int64_t N, int64_t E, int32_t T, int32_t F, int32_t R,
                         const float* const* W1, float* gh1, float* dP, float* dTe);
int32_t gnx_pna_edge_fwd(gnx_handle* h, const float* P, const float* Q, const float* Te, const int32_t* src,
                         const int32_t* dst, const int32_t* code, const int32_t* rowptr, const int32_t* tile_info,
                         int32_t tile_w, int64_t N, int64_t E, int32_t T, int32_t F, const float* const* W1,
                         const float* const* b1, float* h1, float* m, float* A);

/* ---- GINE message + sum aggregate (fused gather, no materialised messages) --------------------------------- */
/* [3P] GINEConv (ref: train/models.py:529-538): out[i,:] = (1+eps) x[i,:] + sum_{p in row i} relu(x[src[p],:] + Le[code[p],:]) */
int32_t gnx_gine_aggregate_fwd(gnx_handle* h, const float* x, const float* Le, const int32_t* rowptr,
                               const int32_t* src, const int32_t* code, int64_t N, int64_t E, int32_t H, float eps,
                               float* out);
/* dx[j,:] = (1+eps) dout[j,:] + sum_{p in cpos(j)} dout[dst[p],:] * (x[j,:] + Le[code[p],:] > 0);
 * dLe[R,H] (optional) += sum_p [code[p]==r] dout[dst[p],:] * (x[src[p],:] + Le[r,:] > 0); code_pos (optional) =
 * CSR positions stably grouped by code (gnx_group_by_small_key): register sums per key run instead of LDS atomics. */
int32_t gnx_gine_aggregate_bwd(gnx_handle* h, const float* dout, const float* x, const float* Le,
                               const int32_t* colptr, const int32_t* cpos, const int32_t* src, const int32_t* dst,
                               const int32_t* code, const int32_t* code_pos, int64_t N, int64_t E, int32_t H, int32_t R,
                               float eps, float* dx, float* dLe);

/* dLe only (what gnx_gine_aggregate_bwd computes when dLe != NULL), as its own call so that it can run on a side
 * stream beside the dx chain; dLe is ACCUMULATED (+=). */
int32_t gnx_gine_dle(gnx_handle* h, const float* dout, const float* x, const float* Le, const int32_t* src,
                     const int32_t* dst, const int32_t* code, const int32_t* code_pos, int64_t E, int32_t H, int32_t R,
                     float* dLe);

/* ---- TransformerConv attention (segmented softmax over the dst-sorted CSR) ---------------------------------- */
/* [3P] TransformerConv(H, C, heads, concat=True, beta=False, root_weight=True, edge_dim=H) (ref: train/models.py:497-511),
 * H = heads * C.  qkvs [N, 4H] = q | k | v | s (the four node projections, biases included); Le [R, H] = lin_edge of the
 * bond table (edge p = j -> i with bond code c uses Le[c]).  Per head h:
 *   score_p = <q_i, k_j + Le_c> / sqrt(C);  alpha_p = exp(score_p - max_row) / (sum_row exp(. - max_row) + 1e-16);
 *   out_i = concat_h sum_p alpha'_p (v_j + Le_c) + s_i,  alpha'_p = alpha_p keep_p / (1 - p)  (p = 0: alpha' = alpha).
 * keep(p, h) is Philox4x32-10 on element e = p * heads + h (counter (e / 4, offset), key seed; the scheme of gnx_dropout),
 * recomputed by the backward.  Outputs: out [N, H]; alpha [E, heads] in CSR order (before dropout); keep uint8 [E, heads]
 * (may be NULL; 1 = kept).  C % 4 == 0 with C / 4 a power of two up to 64 or C a multiple of 256; H <= 1024; float
 * operands 16-byte aligned.  A node without in-edges gets out_i = s_i.  Any in-degree. */
int32_t gnx_transformer_attn_fwd(gnx_handle* h, const float* qkvs, const float* Le, const int32_t* rowptr,
                                 const int32_t* src, const int32_t* code, int64_t N, int64_t E, int32_t heads,
                                 int32_t C, float p, uint64_t seed, uint64_t offset, float* out, float* alpha,
                                 uint8_t* keep);
/* backward of the same call given dout [N, H] and the saved alpha: dqkv [N, 3H] = dq | dk | dv, deterministic (no
 * floating-point atomics: a destination-side pass per row writes dq and a source-side pass per node over colptr / cpos
 * writes dk, dv).  scratch: caller-owned fp32 [2, E, heads] = dscore_p = alpha_p (dalpha_p - sum_row alpha dalpha) /
 * sqrt(C) and alpha'_p, kept for gnx_transformer_attn_dle.  dLe [R, H] (may be NULL = not computed here) is ACCUMULATED
 * (+=) as gnx_transformer_attn_dle does. */
int32_t gnx_transformer_attn_bwd(gnx_handle* h, const float* dout, const float* qkvs, const float* Le,
                                 const float* alpha, const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                                 const int32_t* code, const int32_t* colptr, const int32_t* cpos,
                                 const int32_t* code_pos, int64_t N, int64_t E, int32_t heads, int32_t C, int32_t R,
                                 float p, uint64_t seed, uint64_t offset, float* dqkv, float* scratch, float* dLe);
/* dLe[c] += sum over the edges with bond code c of dscore_p q_dst + alpha'_p dout_dst, from the scratch of
 * gnx_transformer_attn_bwd, as its own call so that it can run on a side stream; code_pos = CSR positions stably grouped
 * by code (gnx_group_by_small_key, required).  One atomic add per channel and key run. */
int32_t gnx_transformer_attn_dle(gnx_handle* h, const float* dout, const float* qkvs, const float* scratch,
                                 const int32_t* dst, const int32_t* code, const int32_t* code_pos, int64_t E,
                                 int32_t heads, int32_t C, int32_t R, float* dLe);

/* ---- pure-component PC-SAFT (fp64; the exception to "all float tensors are fp32") --------------------------- */
/* [3P] feos 0.8 PC-SAFT (ref: train/utils.py:238-300 rho_batch / vp_batch -> pcsaft/pcsaft_feos.py:349-436
 * pure_den_feos / pure_vp_feos).  params [B, 9] fp64 rows [m, sigma (angstrom), eps/k (K), kappa_ab, eps_ab/k (K),
 * mu (debye), na, nb, mw] (mw unused); point i uses row owner[i] (int64; outside [0, B) -> status 3).  T in K, P in Pa,
 * densities in mol/m^3.  One lane per point, one launch, no atomics (same input, same bits).  status per point:
 * 0 = ok, 1 = no root / not converged within the fixed iteration caps, 2 = T at or above the critical temperature
 * (vapour pressure only), 3 = invalid input (non-finite or non-positive T, P, m, sigma, eps/k; negative others).
 * Every output of a point with status != 0 is exactly 0.0.  DESIGN.md §4b. */
/* rho[i] = the highest-density root of P(rho; T[i]) = P[i] with dP/drho > 0 (feos density_initialization="liquid") */
int32_t gnx_pcsaft_density(gnx_handle* h, const double* params, int64_t B, const int64_t* owner, const double* T,
                           const double* P, int64_t n, double* rho, int32_t* status);
/* psat[i], rho_l[i], rho_v[i]: the saturated state at T[i] (equal pressure and chemical potential; feos
 * PhaseEquilibrium.pure).  rho_l / rho_v may be NULL. */
int32_t gnx_pcsaft_vapor_pressure(gnx_handle* h, const double* params, int64_t B, const int64_t* owner, const double* T,
                                  int64_t n, double* psat, double* rho_l, double* rho_v, int32_t* status);
/* The saturation line at T[i] (ref: pcsaft/pcsaft_feos.py pure_h_lv_feos / pure_s_lv_feos / phase_diagram_feos; feos
 * PhaseEquilibrium.pure and PhaseDiagram.pure with Contributions.Residual): the solve of gnx_pcsaft_vapor_pressure
 * (same psat, rho_l, rho_v and status, bit for bit), then the residual molar enthalpy h = R T (-T a_T + Z - 1) [J/mol]
 * and the residual molar entropy at the same T and V, s = -R (a + T a_T) [J/mol/K], of the liquid and of the vapour.
 * h_v - h_l is the enthalpy of vaporization; s_v - s_l is (h_v - h_l) / T - R ln(rho_l / rho_v), not (h_v - h_l) / T.
 * Each of the seven fp64 outputs may be NULL.  No kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_saturation(gnx_handle* h, const double* params, int64_t B, const int64_t* owner, const double* T,
                              int64_t n, double* psat, double* rho_l, double* rho_v, double* h_l, double* h_v,
                              double* s_l, double* s_v, int32_t* status);
/* Vapour-liquid critical point of every row of params (ref: pcsaft/pcsaft_feos.py critical_points_feos; feos
 * State.critical_point): Tc[b] (K), Pc[b] (Pa), rho_c[b] (mol/m^3) with (dp/drho)_T = (d2p/drho2)_T = 0 on the van der
 * Waals loop that vanishes last as T rises.  One lane per row; the bracket in T is found from above (from 20 eps/k
 * down).  status per row: 0 = ok, 1 = no loop found down to 0.3 eps/k or the polish did not converge, 3 = invalid row;
 * every value is exactly 0.0 where status != 0.  h_c [J/mol] and s_c [J/mol/K], each NULL or [B], are the residual molar
 * enthalpy and entropy of gnx_pcsaft_saturation at (Tc, rho_c): the end point of both branches of a phase diagram.
 * No kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_critical_point(gnx_handle* h, const double* params, int64_t B, double* Tc, double* Pc, double* rho_c,
                                  double* h_c, double* s_c, int32_t* status);

/* ---- mixture PC-SAFT, 1 to 4 components (fp64) ------------------------------------------------------------------ */
/* [3P] feos 0.8 PC-SAFT mixtures (ref: demo/utils_binary.py:116-160 binary_test -> pcsaft/pcsaft_feos.py:311-346
 * mix_den_feos).  params [B, 9] fp64: the pool of component rows (layout as above).  mix_comp [M, nc] int64: the rows of
 * params that make up each mixture, -1 = unused slot (its x is ignored); 1 <= nc <= 4.  mix_kij [M, nc, nc] fp64 or NULL
 * (all zero): binary interaction parameters; mix_eab [M, nc, nc] fp64 or NULL: cross association energies eps_ab,ij/k,
 * a NaN entry (or NULL) = the combining rule (eps_ab,i + eps_ab,j)/2.  Both matrices are read from their upper triangle
 * (entry [min(i,j)][max(i,j)]), which makes them symmetric; their diagonals are ignored.  Point i belongs to mixture
 * owner[i] (int64) and has the composition x[i, 0..nc) (fp64, normalised by its sum; a component with x = 0 contributes
 * exactly nothing and its row is not read).  status per point: 0 = ok, 1 = no root / not converged within the fixed
 * iteration caps, 3 = invalid input (owner outside [0, M), a component index outside [0, B) and not -1, no used slot,
 * negative or non-finite x, zero sum of x, invalid row of a component that is present, non-finite k_ij, non-positive
 * or non-finite T / P / rho, rho at or beyond packing fraction 1).  Every output of a point with status != 0 is exactly
 * 0.0.  One lane per point, one launch, no atomics (same input, same bits).  DESIGN.md §4c. */
/* at the molar density rho[i] (mol/m^3): a_res[i] = reduced residual Helmholtz energy per molecule, p[i] (Pa),
 * dpdrho[i] = dp/drho at constant T, x (Pa m^3/mol) */
int32_t gnx_pcsaft_mix_state(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                             const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                             const double* T, const double* rho, const double* x, int64_t n, double* a_res, double* p,
                             double* dpdrho, int32_t* status);
/* rho[i] (mol/m^3) = the highest-density root of P(rho; T[i], x[i]) = P[i] with dP/drho > 0 */
int32_t gnx_pcsaft_mix_density(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                               const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                               const int64_t* owner, const double* T, const double* P, const double* x, int64_t n,
                               double* rho, int32_t* status);
/* Fugacity coefficients (ref: pcsaft/pcsaft_feos.py mix_ln_fugacity_coefficient, mix_ln_fugacity_coefficient_pure and
 * what builds on them): ln phi_i = mu_i^res/kT - ln Z with mu_i^res/kT = d(N a)/dN_i at fixed T, V, the composition
 * derivatives of a by a first-order forward dual through every term (the site fractions by implicit differentiation).
 * Unlike the two functions above, a used slot with x = 0 stays in the mixture: its ln phi is the value at infinite
 * dilution, and its row is validated.  lnphi [n, nc]: NaN in a -1 slot and in every slot of a point with status != 0.
 * Status codes as above. */
/* at the molar density rho[i]: lnphi[i, :], Z[i] = p/(rho R T).  Z <= 0 (no ln Z): status 1, Z[i] still reported; Z[i] is
 * 0.0 for every other status != 0 */
int32_t gnx_pcsaft_mix_lnphi_state(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                   const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                   const int64_t* owner, const double* T, const double* rho, const double* x, int64_t n,
                                   double* lnphi, double* Z, int32_t* status);
/* at the root gnx_pcsaft_mix_density finds: rho[i] (the same bits; 0.0 with status != 0) and lnphi[i, :] there.
 * lnphi_pure [n, nc] or NULL (skipped): ln phi of each used slot's component alone at its own liquid root at T[i], P[i]
 * (feos ln_phi_pure_liquid); NaN where that component has no liquid root (no stretch with dp/drho <= 0 below its
 * highest root, as above its critical temperature), which leaves status[i] at 0 */
int32_t gnx_pcsaft_mix_lnphi(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                             const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                             const double* T, const double* P, const double* x, int64_t n, double* rho, double* lnphi,
                             double* lnphi_pure, int32_t* status);
/* Bubble point (ref: pcsaft/pcsaft_feos.py mix_vp_feos, the bubble half, and mix_vle_pxy_diagram_feos): at T[i] and the
 * liquid composition x[i, :] the pressure P[i] (Pa) at which a first bubble of vapour forms, that vapour's composition
 * y[i, :] and the molar densities rho_l[i], rho_v[i] of both phases (either may be NULL).  Equal mu_i^res/kT + ln(rho x_i)
 * of every component and equal pressure, by successive substitution from an ideal-vapour start; the equations hold to
 * 1e-10 at the numbers returned.  As in the density entry a used slot with x = 0 is dropped; its y is 0.0, that of a -1
 * slot NaN.  A point with status != 0 has P = 0.0, NaN in its whole y row and densities 0.0; status 1 covers every
 * failure that is not bad input, "no bubble point at this T" (no liquid root at zero pressure: too close to the
 * mixture's critical region, or above it) among them.  The launch has no kernel id (GNX_K_NONE): it is not in the
 * profiling tables. */
int32_t gnx_pcsaft_mix_bubble(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                              const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                              const double* T, const double* x, int64_t n, double* P, double* y, double* rho_l,
                              double* rho_v, int32_t* status);
/* Dew point (ref: pcsaft/pcsaft_feos.py mix_vp_feos, the dew half): the bubble entry with the roles of x and y
 * exchanged.  At T[i] and the vapour composition y[i, :] the pressure P[i] (Pa) at which a first drop of liquid forms,
 * that liquid's composition x[i, :] and the molar densities rho_l[i], rho_v[i] of both phases (either may be NULL).  The
 * same equations, by successive substitution on x from Raoult's law on each component's own liquid at zero pressure (a
 * component without one counts as 100 times as volatile as the most volatile one that has); they hold to 1e-10 at the
 * numbers returned.  A dew point need not be unique (a retrograde vapour has two): the one reported is the one that
 * start leads to.  A used slot with y = 0 is dropped; its x is 0.0, that of a -1 slot NaN.  A point with status != 0 has
 * P = 0.0, NaN in its whole x row and densities 0.0; status 1 covers every failure that is not bad input: no component
 * with a liquid at zero pressure, no root, no end within 400 steps, only the trivial solution.  The launch has no kernel
 * id (GNX_K_NONE). */
int32_t gnx_pcsaft_mix_dew(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                           const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                           const double* T, const double* y, int64_t n, double* P, double* x, double* rho_l,
                           double* rho_v, int32_t* status);
/* Bubble and dew temperatures at given pressure (ref: pcsaft/pcsaft_feos.py mix_vle_diagram_feos; feos
 * PhaseEquilibrium.bubble_point / dew_point at given pressure, PhaseDiagram.binary_vle): the two entries above with P
 * given and T looked for.  At P[i] (Pa) and the liquid composition x[i, :] the temperature T[i] (K) at which a first
 * bubble of vapour forms and that vapour's y[i, :] (gnx_pcsaft_mix_bubble_t); at P[i] and the vapour composition
 * y[i, :] the temperature at which a first drop of liquid forms and that liquid's x[i, :] (gnx_pcsaft_mix_dew_t); the
 * molar densities rho_l[i], rho_v[i] of both phases (either may be NULL).  T0 [n] or NULL: the temperature the solve
 * starts from (feos tp_init); NULL or a NaN entry: the entry's own start, a secant in 1/T on the first pressure estimate
 * of the pressure entry (ideal vapour over the liquid at zero pressure; Raoult's law).  Then successive substitution on
 * the unknown composition with one secant step in 1/T per step; the equations of the pressure entries hold to 1e-10
 * at the numbers returned.  A dew temperature need not be unique: the one reported is the one the start leads to.  A
 * used slot with zero given fraction is dropped (0.0 in the output row), a -1 slot has NaN.  A point with status != 0
 * has T = 0.0, NaN in its whole composition row and densities 0.0.  status 1: no bubble or dew temperature found (no
 * start: the pressure is above what the first estimate reaches, as close to a critical point; a root lost; no end
 * within 400 steps; only the trivial solution); status 3: bad input (P not finite or <= 0, a T0 that is neither NaN nor
 * positive and finite, an invalid mixture as in the other entries).  The launches have no kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_mix_bubble_t(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                const int64_t* owner, const double* P, const double* x, const double* T0, int64_t n,
                                double* T, double* y, double* rho_l, double* rho_v, int32_t* status);
int32_t gnx_pcsaft_mix_dew_t(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                             const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                             const double* P, const double* y, const double* T0, int64_t n, double* T, double* x,
                             double* rho_l, double* rho_v, int32_t* status);
/* Isothermal two-phase flash (ref: pcsaft/pcsaft_feos.py mix_tp_flash_feos): at T[i], P[i] (Pa) the split of the feed
 * z[i, :] (normalised by its sum) into a liquid x[i, :] and a vapour y[i, :], the vapour mole fraction beta[i] in [0, 1]
 * and the molar densities rho_l[i], rho_v[i] of both phases (either may be NULL).  Equal mu_i^res/kT + ln(rho x_i) of
 * every component, both phases at P and z = (1 - beta) x + beta y, by successive substitution on ln K with a
 * Rachford-Rice solve per step, from the bubble entry's ideal-vapour start; the equilibrium equations hold to 1e-10 at
 * the numbers returned.  A used slot with z = 0 is dropped (x = y = 0.0), a -1 slot has NaN in x and y.  status 4 (this
 * entry alone): no vapour-liquid split at (T, P, z): one component, every K on one side of 1, or a converged split with
 * beta outside [0, 1] or with equal phases.  status 3 also covers a non-finite or non-positive P.  A point with
 * status != 0 has beta = 0.0, NaN in its whole x and y rows and densities 0.0.  Liquid-liquid splits are not looked for.
 * The launch has no kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_mix_flash(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                             const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                             const double* T, const double* P, const double* z, int64_t n, double* beta, double* x,
                             double* y, double* rho_l, double* rho_v, int32_t* status);
/* Tangent-plane stability test (ref: pcsaft/pcsaft_feos.py is_stable_feos, called at pcsaft/kij.py:30 on every trial
 * feed before it is flashed): row i is trial trial[i] of the feed z[i, :] (normalised by its sum) at T[i], P[i] (Pa).  A
 * mixture of nc slots has the trials 0 (vapour-like, W = z K), 1 (liquid-like, W = z / K) and 2 + s (rich in slot s, W =
 * 0.1 z + 0.9 e_s), K_i = f_i(z) kT / (z_i P); a caller that wants a verdict runs all nc + 2 as rows of one launch.  Each is
 * successive substitution on the tangent-plane distance D(w) = sum_i w_i (ln f_i(w) - ln f_i(z)), ln f_i = mu_i^res/kT +
 * ln(rho x_i), the state of z and of every w being the one of its liquid and its lowest vapour root at P with the lower
 * sum_i x_i ln f_i.  tpd[i] is 0.0 exactly where the trial fell onto the feed (w[i, :] = z, rho_w = rho_z), the first
 * D < -1e-8 it met (z is unstable, w[i, :] proves it) or D at the stationary point it converged to (residual < 1e-8);
 * rho_w[i], rho_z[i] are the molar densities of w and z (either may be NULL).  A used slot with z = 0 is dropped (w =
 * 0.0), a -1 slot has NaN in w; the trial rich in such a slot and every trial of a single component report the feed.
 * status 1: no end within 400 steps, a non-finite value, or no root of w or z at P.  status 3 also covers a non-finite
 * or non-positive P and a trial outside [0, nc + 2).  A row with status != 0 has tpd = NaN, NaN in its whole w row and
 * densities 0.0.  The launch has no kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_mix_stability(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                 const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                                 const int64_t* trial, const double* T, const double* P, const double* z, int64_t n,
                                 double* tpd, double* w, double* rho_w, double* rho_z, int32_t* status);
/* Liquid-liquid flash started from the stability test (ref: pcsaft/pcsaft_feos.py mix_lle_feos / mix_lle_diagram_feos,
 * and feos's tp_flash after is_stable_feos at pcsaft/kij.py:37, whose caller takes the denser phase): at T[i], P[i] (Pa)
 * the split of the feed z[i, :] (normalised by its sum) into two phases x[i, :] and y[i, :], started from ln K = ln(w0 / z)
 * with w0[i, :] the composition the second phase starts from, in practice the w of gnx_pcsaft_mix_stability with the most
 * negative distance.  Equal mu_i^res/kT + ln(rho x_i) of every component, both phases at P and z = (1 - beta) x + beta y,
 * by successive substitution on ln K with a Rachford-Rice solve per step; the state of each phase is the stability
 * entry's (of its liquid and its lowest vapour root at P the one with the lower sum_i x_i ln f_i), so a feed whose stable
 * split is vapour-liquid comes out as that split.  The equations hold to 1e-10 at the numbers returned.  x is the phase of
 * higher molar density, beta[i] in [0, 1] the mole fraction of the other one, rho_x[i] >= rho_y[i] the molar densities
 * (either may be NULL).  A used slot with z = 0 is dropped (x = y = 0.0), a -1 slot has NaN in x and y, and neither z nor
 * w0 is read there.  status 4: no split: one component, every K on one side of 1 (w0 = z is that), or a converged split
 * with beta outside [0, 1] or with equal phases.  status 3 also covers a non-finite or non-positive P and a w0 that is
 * non-finite or <= 0 in a slot where z > 0.  status 1: no end within 200 steps, a non-finite value, or a phase without a
 * root at P.  A point with status != 0 has beta = 0.0, NaN in its whole x and y rows and densities 0.0.  Three-phase
 * states are not looked for.  The launch has no kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_mix_lle(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                           const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                           const double* T, const double* P, const double* z, const double* w0, int64_t n, double* beta,
                           double* x, double* y, double* rho_x, double* rho_y, int32_t* status);
/* Predicted liquid x_1 of a binary over a list of trial feeds, and its residual against a measurement (ref:
 * pcsaft/kij.py:20-49 _pred_x1_worker and :52-82 _loss_fn): row i is the state T[i], P[i] (Pa) of mixture owner[i] with
 * the measured liquid mole fraction x1_exp[i] of slot 0.  Several candidate k_12 of one system are several mixtures whose
 * mix_comp rows name the same parameter rows and whose mix_kij differ.  nc must be 2 and F >= 1.  Every feed z =
 * (feeds[f], 1 - feeds[f]), f < F, is flashed as gnx_pcsaft_mix_flash flashes it, one wave of 64 lanes per row and one
 * lane per feed, 64 feeds at a time in list order; the row takes the first feed that splits (status 0 of the flash):
 * x1[i] is the bits of that flash's x[.., 0], feed[i] its index in feeds, residual[i] = log((x1 + 1e-6) / (x1_exp + 1e-6))
 * and status[i] = 0.  Where no feed splits x1[i] = NaN, feed[i] = -1, residual[i] = 10.0 (the reference's penalty) and
 * status[i] is 3 where every feed reports bad input (as gnx_pcsaft_mix_flash judges it) or x1_exp[i] is not finite, else 1
 * where a feed ended without convergence, else 4.  Where a feed splits and the residual is not finite (x1_exp[i] not
 * finite or below -1e-6), residual[i] = 10.0 and status[i] = 3 beside the x1 and feed of the split.  Unlike the reference
 * no stability test runs before a flash: a stable feed has no split with beta in [0, 1] and counts as single phase.
 * Liquid-liquid splits are not looked for.  Same input, same bits.  The launch has no kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_kij_x1(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp, const double* mix_kij,
                          const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner, const double* T,
                          const double* P, const double* x1_exp, const double* feeds, int64_t F, int64_t n, double* x1,
                          int32_t* feed, double* residual, int32_t* status);
/* The sums of one Levenberg-Marquardt step in k_12 of S binaries (ref: pcsaft/kij.py:144-188, the least_squares call of
 * optimize_kij with jac="2-point" and the scores after it) over the n rows of a gnx_pcsaft_kij_x1 launch laid out
 * [system][candidate][point]: system s has the points seg[s] .. seg[s + 1], candidate 0 (at k) in the rows 2 seg[s] + j
 * and candidate 1 (at k + hstep) in the rows 2 seg[s] + n_s + j.  A row is penalised where its status != 0.  sums[s, :]:
 * 0 sum r0^2 (penalties included), 1 the number of penalised rows of candidate 0, 2 sum |r0| and 3 sum |x1_0 - x1_exp| /
 * x1_exp over its other rows, 4 sum r1^2, 5 sum J r0, 6 sum J^2, 7 the number of rows with J defined; J = (r1 - r0) /
 * hstep where neither row is penalised and 0 elsewhere (the reference differences the penalty too).  One wave per
 * system, a fixed order of additions: same input, same bits.  A system whose range is not within the n rows has NaN in
 * all eight.  hstep must be finite and not 0.  The launch has no kernel id (GNX_K_NONE). */
int32_t gnx_pcsaft_kij_sums(gnx_handle* h, const double* residual, const double* x1, const double* x1_exp,
                            const int32_t* status, const int64_t* seg, int64_t S, int64_t n, double hstep, double* sums);

/* ---- contiguous segment reduce: global pool (ref: train/models.py:218-225, 587-595) ------------------------ */
enum { GNX_POOL_ADD = 0, GNX_POOL_MEAN = 1, GNX_POOL_MAX = 2 };
int32_t gnx_segment_pool_fwd(gnx_handle* h, const float* x, const int32_t* ptr, int64_t B, int32_t H, int32_t mode,
                             float* out);
int32_t gnx_segment_pool_bwd(gnx_handle* h, const float* dout, const float* x, const float* out, const int32_t* ptr,
                             int64_t B, int32_t H, int32_t mode, float* dx);

/* ---- BatchNorm1d (+ReLU) over rows (ref: train/models.py:184,212-214 and the readout mlp :186-194) ---------- */
size_t gnx_batchnorm_workspace_bytes(int64_t M, int32_t H);
/* training: batch statistics (biased var to normalise, unbiased into running_var, momentum), saves mean/rstd[H].
 * eval (training=0): uses running stats. y = relu?(gamma*(x-mean)*rstd + beta).  num_batches_tracked (device int64[1],
 * may be NULL) is incremented in training mode, as torch.nn.BatchNorm1d does before the call. */
int32_t gnx_batchnorm_fwd(gnx_handle* h, const float* x, int64_t M, int32_t H, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                          float eps, int32_t training, int32_t relu, float* y, float* save_mean, float* save_rstd,
                          void* ws, size_t ws_bytes);
/* dy masked by (y>0) when relu; dgamma/dbeta are ACCUMULATED (+=). */
int32_t gnx_batchnorm_bwd(gnx_handle* h, const float* dy, const float* x, const float* y, int64_t M, int32_t H,
                          const float* gamma, const float* save_mean, const float* save_rstd, int32_t relu,
                          float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes);
/* The same without y: the ReLU mask is recomputed as x * a + b' > 0 with a = rstd * gamma and b' = beta - mean * a, the
 * forward's own expression (one device helper, no contraction), so dx / dgamma / dbeta are bit-identical to
 * gnx_batchnorm_bwd given the y of a training-mode gnx_batchnorm_fwd with the same x, gamma, beta.  Two of the seven
 * [M, H] passes less.  gamma / beta may be NULL (1 / 0).  Same workspace size.  gamma and beta must still hold the
 * forward's values when this runs (the optimizer step comes after the backward). */
int32_t gnx_batchnorm_bwd_x(gnx_handle* h, const float* dy, const float* x, int64_t M, int32_t H, const float* gamma,
                            const float* beta, const float* save_mean, const float* save_rstd, int32_t relu, float* dx,
                            float* dgamma, float* dbeta, void* ws, size_t ws_bytes);

/* ---- dropout (ref: train/models.py:177, 209; p = 0.25 in configs/pna_msigmae_7.py:40) --------------------------- */
/* y[i] = keep(i) ? x[i] / (1 - p) : 0 with keep(i) decided by Philox4x32-10 on the counter (i / 4, offset) under the
 * key `seed` (uniform u in [0,1) from 24 bits; keep iff u >= p).  Stateless: calling it again with the same
 * (seed, offset) on the upstream gradient IS the backward pass (the mask is recomputed, never stored).  In place
 * (y == x) is allowed.  torch's RNG stream cannot be reproduced; parity for p > 0 is statistical. */
int32_t gnx_dropout(gnx_handle* h, const float* x, int64_t n, float p, uint64_t seed, uint64_t offset, float* y);

/* ---- loss: APE-Huber (ref: train/models.py:89-91) + MAPE metric (:92) ---------------------------------------- */
/* out[0] = mean huber((pred-t)/t, delta), out[1] = mean |pred-t|/max(|t|,1.17e-6); dpred (optional) = d out[0]/d pred. */
int32_t gnx_huber_ape(gnx_handle* h, const float* pred, const float* target, int64_t count, float delta, float* out2,
                      float* dpred);

/* ---- optimizer step on device (ref: train/models.py:47-63) ----------------------------------- */
/* torch.optim.AdamW(amsgrad=True) single-tensor arithmetic over flat fp32 buffers of n elements; step counts from 1. */
int32_t gnx_adamw_amsgrad(gnx_handle* h, float* p, const float* g, float* m, float* v, float* vmax, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int64_t step);
/* torch.optim.SGD(momentum=0, weight_decay=0, nesterov=False): p -= lr * g */
int32_t gnx_sgd(gnx_handle* h, float* p, const float* g, int64_t n, float lr);

/* ---- one conv layer's backward as ONE call (native launch sequence) ------------------------------------------- */
/* The backward of PNAConv (ref: train/models.py:445-457 via autograd) is ~35 launches; issued one by one from Python
 * they cost 0.3 ms of host time per layer.  gnx_pna_conv_bwd issues the same launches in the same order on the same
 * streams (bound stream; side stream 0 = weight gradients; side stream 1 = bond-table chain) from one call.  Every
 * pointer is caller-owned device memory except `params` / `grads`, HOST arrays of 4 + T*2*(pre+post) device pointers in
 * the order: edge_encoder.{weight,bias}, lin.{weight,bias}, then per tower pre_nns (w, b) x pre_layers and post_nns
 * (w, b) x post_layers.  All gradients are ACCUMULATED (+=) into `grads` (persistent in-place sinks).  Requires the
 * degree-class form of post-layer 0 (D classes, tables from gnx_degree_classes / gnx_class_tiles with 128-row tiles
 * and the weight-gradient chunks) and the by-code inverted index code_pos (gnx_group_by_small_key). */
#define GNX_PNA_MAX_LAYERS 8
#define GNX_PNA_MAX_TOWERS 8
/* gnx_pna_bwd_args.flags */
enum {
  GNX_PNA_BWD_DEFER_SMALL = 1,   /* dTe / dEE / dWm / dbm / dWeff were ZEROED by the caller and stay alive until
                                    gnx_pna_stack_finish, which runs every layer's 60-row bond-table chain, its lin o last-post
                                    un-merge and its Weff gradient in a few batched launches: gnx_pna_conv_bwd leaves them out */
  GNX_PNA_BWD_LAST_OF_PASS = 2   /* this is the LAST conv backward of the pass: nothing follows on the main stream, so its
                                    batched weight gradients take every CU and go out at the end of the layer */
};
typedef struct {
  int64_t N, E;
  int32_t T, F, pre_layers, post_layers, R, D;
  float avg_deg_log;
  int32_t merged;            /* 1: lin o last post layer was evaluated as one product with Wm (post_layers > 1) */
  int32_t acc_first;         /* 1: this layer's backward is the first of the pass: clear acc_buf before adding */
  int32_t use_side_streams;  /* 0: everything on the bound stream */
  int32_t n_h, n_z;          /* number of saved pre activations hs[] (= pre_layers) and post activations zs[] */
  /* graph structure (gnx_pack_csr, gnx_degree_classes, gnx_class_tiles, gnx_group_by_small_key) */
  const int32_t *rowptr, *colptr, *cpos, *code, *code_pos, *dperm, *tiles, *ntiles, *chunks, *nchunks;
  int64_t max_tiles, max_chunks;
  /* saved by the forward */
  const float *x, *BE, *EE, *A;               /* [N,H], [R,H], [R,F], [N,T*4F] */
  const float* hs[GNX_PNA_MAX_LAYERS];        /* [E,H] each; hs[n_h-1] = the messages */
  const float* zs[GNX_PNA_MAX_LAYERS];        /* [N,H] each */
  const float* weff[GNX_PNA_MAX_TOWERS];      /* [D,F,4F] per tower */
  const float* Wm;                            /* [H,H] merged weight (merged = 1) */
  const float* const* params;                 /* HOST array of device pointers */
  float* const* grads;                        /* HOST array of device pointers (accumulated) */
  const float* dout;                          /* [N,H] upstream gradient */
  /* temporaries, caller-allocated, contents undefined on entry */
  float* gbuf[GNX_PNA_MAX_LAYERS];            /* [N,H] each: post_layers of them (every level of the gradient chain
                                                 keeps its own buffer: queued weight gradients read them later) */
  float* dA;                                  /* [N,T*4F] */
  float* gebuf[GNX_PNA_MAX_LAYERS];           /* [E,H] each: pre_layers of them */
  float *dP, *dQ;                             /* [N,H] */
  float *dTe, *dEE;                           /* [R,H], [R,F] */
  float *dWm, *dbm;                           /* [H,H], [H] (merged = 1) */
  float* dWeff;                               /* [T,D,F,4F] */
  void* ws;                                   /* scratch of the products that split in place: >= gnx_pna_conv_bwd_workspace_bytes */
  size_t ws_bytes;
  float* acc_buf;                             /* [R,H] bond-embedding gradient accumulator shared by the model's layers */
  float* dx;                                  /* [N,H] out: gradient w.r.t. the layer input */
  int32_t flags;                              /* flag word: GNX_PNA_BWD_* (above) */
  int32_t etile_w;                            /* tile width of etile_info */
  const int32_t* etile_info;                  /* gnx_edge_tiles table (NULL: three-launch edge backward); with two pre layers
                                                 the masked input gradient, dP and dTe then come from gnx_pna_edge_bwd */
} gnx_pna_bwd_args;
size_t gnx_pna_conv_bwd_workspace_bytes(int32_t T, int32_t F, int32_t D);
int32_t gnx_pna_conv_bwd(gnx_handle* h, const gnx_pna_bwd_args* args);

/* What gnx_pna_conv_bwd(flags & GNX_PNA_BWD_DEFER_SMALL) left out, for ALL L layers of a model in ~6 launches (instead of ~14 per layer):
 * side stream 1: pre-layer-0 edge-slice / edge_encoder gradients and the bond-embedding gradient (atomic adds into acc_buf,
 * which the caller zeroed) from every layer's dTe; side stream 0 (behind the layers' weight gradients): lin / last-post
 * gradients from dWm / dbm, and post-layer 0's A-block gradients from dWeff.  Pointer arrays are HOST arrays; params /
 * grads hold L x (4 + T 2 (pre + post)) device pointers in gnx_pna_bwd_args' order; ones: device fp32[>= R] of 1.0. */
typedef struct {
  int32_t L, T, F, pre_layers, post_layers, R, D, merged, use_side_streams, _pad;
  const float* BE;
  float* acc_buf;
  const float* ones;
  const float* avg_deg_log;        /* HOST [L] */
  const float* const* params;      /* HOST [L * np] */
  float* const* grads;             /* HOST [L * np] */
  const float* const* EE;          /* HOST [L]: [R,F] */
  float* const* dTe;               /* HOST [L]: [R,H]  (by-code segment sums, complete on side stream 1) */
  float* const* dEE;               /* HOST [L]: [R,F]  zero-initialised */
  const float* const* dWm;         /* HOST [L]: [H,H]  (merged = 1) */
  const float* const* dbm;         /* HOST [L]: [H] */
  const float* const* dWeff;       /* HOST [L * T]: [D,F,4F] */
} gnx_pna_finish_args;
int32_t gnx_pna_stack_finish(gnx_handle* h, const gnx_pna_finish_args* args);
/* gnx_pna_weight_only for all L layers of a model in 3 launches (+ 1 per tower beyond the second): avg_deg_log HOST [L]; params HOST [L * np]; EE / Te / Wm /
 * bm HOST [L]; weff HOST [L * T] (D > 0). */
int32_t gnx_pna_weight_only_all(gnx_handle* h, int32_t L, const float* BE, int32_t R, int32_t T, int32_t F,
                                int32_t pre_layers, int32_t post_layers, int32_t D, const float* avg_deg_log,
                                const float* const* params, int32_t merged, float* const* EE, float* const* Te,
                                float* const* weff, float* const* Wm, float* const* bm);

/* the weight-only part of a PNAConv forward in one call: EE [R,F], Te [R,H], Weff(d) [D,F,4F] per tower (D > 0) and, with
 * merged = 1 (post_layers > 1), Wm [H,H] = lin_w @ blockdiag(W_last_t), bm [H] = lin_w b_last + lin_b.  `params` as in
 * gnx_pna_bwd_args; `weff` a HOST array of T device pointers. */
int32_t gnx_pna_weight_only(gnx_handle* h, const float* BE, int32_t R, int32_t T, int32_t F, int32_t pre_layers,
                            int32_t post_layers, int32_t D, float avg_deg_log, const float* const* params, int32_t merged,
                            float* EE, float* Te, float* const* weff, float* Wm, float* bm);
/* the rest of the forward in one call.  hs[i] ([E,H], pre_layers of them) and zs[i] ([N,H]: post_layers - merged of
 * them) are the activations the backward needs; P, Q [N,H] and A [N,T*4F] likewise caller-owned. */
typedef struct {
  int64_t N, E;
  int32_t T, F, pre_layers, post_layers, D, merged;
  const int32_t *rowptr, *src, *dst, *code, *dperm, *tiles, *ntiles;
  int64_t max_tiles;
  const float *x, *Te;                         /* [N,H], [R,H] */
  const float* weff[GNX_PNA_MAX_TOWERS];
  const float *Wm, *bm;                        /* merged = 1 */
  const float* const* params;                  /* HOST array of device pointers */
  float *P, *Q, *A;
  float* hs[GNX_PNA_MAX_LAYERS];
  float* zs[GNX_PNA_MAX_LAYERS];
  void* ws;                                    /* >= gnx_pna_conv_bwd_workspace_bytes(T, F, D) */
  size_t ws_bytes;
  float* out;                                  /* [N,H] */
  const int32_t* etile_info;                   /* gnx_edge_tiles table (NULL: unfused edge pipeline) */
  int32_t etile_w;                             /* its tile width */
  int32_t tile_rows;                           /* height `tiles` was built with: 96 or 128 (0 = 128); gnx_gemm_tile_rows */
} gnx_pna_fwd_args;
int32_t gnx_pna_conv_fwd(gnx_handle* h, const gnx_pna_fwd_args* args);

/* ---- every PNA layer's split weight images, once per step, in one launch ------------------------------------- */
/* The three tiled products of a PNAConv layer that read split weight images (post-layer 0 by degree class, dA = g Weff(d),
 * the three-segment dx) depend on the parameters and on Weff(d) only, so their images can be written once, behind
 * gnx_pna_weight_only_all, for all L layers and T towers: gnx_pna_split_all plans the three products per (layer, tower)
 * for N rows exactly as the layers will (GNX_GEMM_SPLIT_ONLY), lays the images out in `slab` and writes them with
 * ceil(problems / 32) launches on the bound stream.  A product whose plan reads no images (N < 4096, a single K-tile,
 * GNX_OPT_GEMM_SPLIT = 0, an unaligned weight) takes no room and no part in the launch.  out[l] receives layer l's image
 * pointers (NULL: none) and, per image, the record of what the plan said about it; gnx_pna_conv_fwd_images / _bwd_images
 * take it next to the unchanged argument block.  A layer uses an image only if its own plan of that product now gives an
 * equal record (then GNX_GEMM_PRESPLIT); otherwise it splits in place, as gnx_pna_conv_fwd / _bwd (images = NULL) always
 * do.  The slab stays alive and unchanged until the last layer's backward has run. */
typedef struct {
  uint64_t image_bytes;   /* 0: the product reads no images */
  int32_t classes, Npad, Kpad;
  int32_t koff[5];        /* padded k offset of every segment; koff[nseg..4] = Kpad */
  int32_t frag;           /* 1: fragment-major blocks, 0: tile-major */
  int32_t bt;             /* 1: the weights are [n][k] (GNX_GEMM_B_TRANS) */
} gnx_gemm_image;
typedef struct {
  void* post0[GNX_PNA_MAX_TOWERS];
  void* dA[GNX_PNA_MAX_TOWERS];
  void* dx[GNX_PNA_MAX_TOWERS];
  gnx_gemm_image post0_rec[GNX_PNA_MAX_TOWERS], dA_rec[GNX_PNA_MAX_TOWERS], dx_rec[GNX_PNA_MAX_TOWERS];
} gnx_pna_layer_images;
/* bytes of the slab for L layers (every weight taken as 16-byte aligned: an upper bound); 0: nothing to split.  tile_rows:
 * the height of the forward's degree-class table (gnx_pna_fwd_args.tile_rows). */
size_t gnx_pna_split_all_bytes(gnx_handle* h, int32_t L, int32_t T, int32_t F, int32_t pre_layers, int32_t post_layers,
                               int32_t D, int64_t N, int32_t tile_rows);
/* params HOST [L * np], weff HOST [L * T] (as gnx_pna_weight_only_all's, whose weff this reads: same stream, behind it);
 * out HOST [L]. */
int32_t gnx_pna_split_all(gnx_handle* h, int32_t L, int32_t T, int32_t F, int32_t pre_layers, int32_t post_layers, int32_t D,
                          int64_t N, int32_t tile_rows, const float* const* params, const float* const* weff, void* slab,
                          size_t slab_bytes, gnx_pna_layer_images* out);
/* how many split launches the handle has issued since gnx_create: per_call = k_split_weights (one product's images, directly in
 * front of it: gnx_gemm* without GNX_GEMM_PRESPLIT), batched = k_split_weights_batched (gnx_pna_split_all).  Host counters. */
int32_t gnx_gemm_split_counts(gnx_handle* h, int64_t* per_call, int64_t* batched);
int32_t gnx_pna_conv_fwd_images(gnx_handle* h, const gnx_pna_fwd_args* args, const gnx_pna_layer_images* images);
int32_t gnx_pna_conv_bwd_images(gnx_handle* h, const gnx_pna_bwd_args* args, const gnx_pna_layer_images* images);

/* ---- dA product + scatter-aggregate backward of one tower in one launch --------------------------------------- */
/* ge[:, t F .. (t+1) F) = gnx_pna_aggregate_bwd(dA = g[:, tF..] Weff_t(d))[:, tF..] without writing dA: k_pna_dA_agg_bwd
 * computes the tower's dA tile (k_gemm_as3's product, same MFMAs in the same order) and runs the aggregate backward on the
 * accumulators.  Bit-identical to gnx_gemm_grouped + gnx_pna_aggregate_bwd.  Taken (*fused = 1) only where that product
 * takes k_gemm_as3 from split images with F = 128, m and ge are 16-byte aligned with (T F) % 4 == 0, every offset fits 32
 * bits and GNX_OPT_DA_AGG_FUSED is not 0; otherwise NOTHING is launched, *fused = 0, and the caller runs the two launches.
 * g, m, ge fp32 with row stride T F; dA is looked at for alignment only (never written); dperm / tiles / ntiles /
 * max_tiles: the 96- or 128-row degree-class table (gnx_class_tiles).  image + rec (gnx_pna_split_all) are used under the
 * record-equality rule of gnx_pna_conv_bwd_images, else the weights are split into ws first. */
int32_t gnx_pna_da_aggregate_bwd(gnx_handle* h, const float* weff_t, int32_t T, int32_t F, int32_t D, int32_t t, const float* g,
                                 const float* dA, const float* m, const int32_t* rowptr, int64_t N, int64_t E, float* ge,
                                 const int32_t* dperm, const int32_t* tiles, const int32_t* ntiles, int64_t max_tiles,
                                 void* image, const gnx_gemm_image* rec, void* ws, size_t ws_bytes, int32_t* fused);

/* ---- small elementwise helpers used by the host module ----------------------------------------------------- */
int32_t gnx_fill(gnx_handle* h, float* p, int64_t n, float v);
/* p[i] *= v : the 1/world factor of the gradient average after the all-reduce (sum) of the flat gradient buffer
 * (DDP's averaging; ref: train/train.py:85-88 strategy="auto"). */
int32_t gnx_scale(gnx_handle* h, float* p, int64_t n, float v);
/* y[i] += a * x[i] : bias gradient of ``lin`` from the merged (lin o last post layer) product of PNAConv's backward. */
int32_t gnx_axpy(gnx_handle* h, float* y, const float* x, int64_t n, float a);

/* Second stream for work that is independent of the caller's stream (the weight gradients of a layer's backward;
 * stands in for what the reference gets from autograd's per-op CUDA streams under DDP, ref: train/train.py:85-88).
 * gnx_side_begin: the handle's own side stream waits for everything queued so far on the bound stream, and every
 *   launch until gnx_side_end goes to the side stream.  gnx_side_join: the bound stream waits for the side stream.
 * Buffers touched by side-stream launches must stay allocated until the join (the caller keeps them alive). */
int32_t gnx_side_begin(gnx_handle* h);
/* the side stream itself (created on first use), so that the caller can order OTHER work behind the weight-gradient
 * launches without a host sync: the data-parallel exchange issues a layer's slice of the gradient all-reduce on it
 * (torch.cuda.ExternalStream) while the input-gradient chain of the remaining layers keeps the main stream busy. */
int32_t gnx_side_stream(gnx_handle* h, void** hip_stream);
int32_t gnx_side_end(gnx_handle* h);
int32_t gnx_side_join(gnx_handle* h);
/* the same with an explicit side-stream index (0, 1 or 2 -- no library call forks onto 2; gnx_side_begin / gnx_side_join are index 0).  Stream 1 carries
 * the bond-table gradient chain of a conv layer's backward (by-code segment sum -> 60-row products), which feeds only
 * parameter gradients and the bond-embedding gradient consumed at the very end of backward. */
int32_t gnx_side_stream_n(gnx_handle* h, int32_t which, void** hip_stream);
int32_t gnx_side_begin_n(gnx_handle* h, int32_t which);
int32_t gnx_side_join_n(gnx_handle* h, int32_t which);
/* y[m,:] = clip(x[m,:], lo[:], hi[:]), NaN propagates like Tensor.clip  (pred_with_bounds, ref: train/models.py:246-253) */
int32_t gnx_clip_rows(gnx_handle* h, const float* x, int64_t M, int32_t P, const float* lo, const float* hi, float* y);

#ifdef __cplusplus
}
#endif
#endif /* GNX_H_ */
