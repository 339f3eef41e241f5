// Input packer: PyG-style COO batch (int64) -> dst-sorted CSR + by-source index (int32), bond codes, graph_ptr,
// PNA degree scalers.  Integer work, bit-exact, deterministic (stable inside every row).
#include "gnx_common.hpp"
#include "gnx_pack_dev.hpp"

// ---------------------------------------------------------------------------------------------------------------
// exclusive scan of int32 counts (n elements) -> out[0..n] (out[n] = total). 1024 elements per block.
// ---------------------------------------------------------------------------------------------------------------
#define SCAN_ITEMS 4
#define SCAN_BLOCK 256
#define SCAN_TILE (SCAN_ITEMS * SCAN_BLOCK)

// One tile of SCAN_TILE counts starting at in[tile0], by a block of SCAN_BLOCK threads: out[i] = carry + the exclusive
// prefix inside the tile (in may be out); returns the tile's total.  s: SCAN_BLOCK ints of LDS, free again on return.
__device__ __forceinline__ int pk_scan_tile(const int* in, int* out, int64_t tile0, int64_t n, int carry, int* s) {
  int64_t base = tile0 + (int64_t)threadIdx.x * SCAN_ITEMS;
  int v[SCAN_ITEMS];
  int t = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    v[i] = (base + i < n) ? in[base + i] : 0;
    t += v[i];
  }
  s[threadIdx.x] = t;
  __syncthreads();
  // Hillis-Steele inclusive scan over the 256 thread totals
  for (int off = 1; off < SCAN_BLOCK; off <<= 1) {
    int add = (threadIdx.x >= off) ? s[threadIdx.x - off] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  int excl = carry + s[threadIdx.x] - t;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    if (base + i < n) out[base + i] = excl;
    excl += v[i];
  }
  const int total = s[SCAN_BLOCK - 1];
  __syncthreads();
  return total;
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_tile(const int* __restrict__ in, int* __restrict__ out,
                                                          int* __restrict__ sums, int64_t n) {
  __shared__ int s[SCAN_BLOCK];
  const int total = pk_scan_tile(in, out, (int64_t)blockIdx.x * SCAN_TILE, n, 0, s);
  if (threadIdx.x == SCAN_BLOCK - 1) sums[blockIdx.x] = total;
}

__global__ void k_scan_add(int* __restrict__ out, const int* __restrict__ offs, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x;
  int o = offs[blockIdx.x];
  for (int k = 0; k < SCAN_ITEMS; ++k, i += SCAN_BLOCK)
    if (i < n) out[i] += o;
}

__global__ void k_set_total(int* __restrict__ out, const int* __restrict__ in, int64_t n) {
  // out[n] = out[n-1] + in[n-1]
  if (threadIdx.x == 0 && blockIdx.x == 0) out[n] = (n > 0) ? out[n - 1] + in[n - 1] : 0;
}

// out must hold n+1 ints when write_total, n otherwise.  ws: scan_ws_ints(n) ints.
static int32_t exclusive_scan(gnx_handle* h, const int* in, int* out, int64_t n, int* ws, bool write_total) {
  if (n > 0) {
    int64_t blocks = gnx_cdiv(n, SCAN_TILE);
    hipLaunchKernelGGL(k_scan_tile, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, h->stream, in, out, ws, n);
    GNX_LAUNCH_CHECK();
    if (blocks > 1) {
      int* sums_scanned = ws + blocks + 1;
      // scan the block sums in place into a second array (recursive), then add
      int32_t st = exclusive_scan(h, ws, sums_scanned, blocks, sums_scanned + blocks + 1, false);
      if (st != GNX_OK) return st;
      hipLaunchKernelGGL(k_scan_add, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, h->stream, out, sums_scanned, n);
      GNX_LAUNCH_CHECK();
    }
  }
  if (write_total) {
    hipLaunchKernelGGL(k_set_total, dim3(1), dim3(64), 0, h->stream, out, in, n);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

static size_t scan_ws_ints_total(int64_t n) {
  // recursion above uses, per level, blocks+1 (sums) followed by the next level's arrays
  size_t tot = 0;
  int64_t m = n;
  while (m > 1) {
    int64_t b = gnx_cdiv(m, SCAN_TILE);
    tot += 2 * ((size_t)b + 1);
    m = b;
  }
  return tot + 16;
}

// ---------------------------------------------------------------------------------------------------------------
// endpoints of edge e as int32; an id outside [0, N) clamps BOTH to 0 and sets range-flag bit 0
__device__ __forceinline__ void pk_convert_edge(const int64_t* __restrict__ ei, int64_t e, int64_t E, int64_t N,
                                                int* __restrict__ flag, int& so, int& dO) {
  int64_t s = ei[e], d = ei[E + e];
  bool bad = (s < 0) | (s >= N) | (d < 0) | (d >= N);
  if (bad) {
    atomicOr(flag, 1);
    s = 0;
    d = 0;
  }
  so = (int)s;
  dO = (int)d;
}

// one thread per group: ascending insertion sort of its items (degrees are tiny for molecules; O(d^2) worst case)
__device__ __forceinline__ void pk_sort_group(int* __restrict__ items, int b, int e) {
  for (int a = b + 1; a < e; ++a) {
    int v = items[a];
    int c = a - 1;
    while (c >= b && items[c] > v) {
      items[c + 1] = items[c];
      --c;
    }
    items[c + 1] = v;
  }
}

// N nodes and E edges must leave room in int32; `who`: the entry that was called
static int32_t check_sizes(const char* who, int64_t N, int64_t E) {
  GNX_CHECK_ARG(N >= 0 && E >= 0 && N < (1ll << 31) - 1 && E < (1ll << 31) - 1, "%s: N=%lld E=%lld out of int32 range", who,
                (long long)N, (long long)E);
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
struct dims_t {
  int d[16];
};

// d = the K <= 16 vocabulary sizes dims (HOST), padded with 1; they must be positive and their product fit int32
static int32_t fill_dims(const char* who, int32_t K, const int32_t* dims, dims_t& d) {
  int64_t prod = 1;
  for (int k = 0; k < 16; ++k) d.d[k] = (k < K) ? dims[k] : 1;
  for (int k = 0; k < K; ++k) {
    GNX_CHECK_ARG(dims[k] > 0, "%s: vocabulary size %d <= 0", who, k);
    prod *= dims[k];
    GNX_CHECK_ARG(prod < (1ll << 31), "%s: code space overflows int32", who);
  }
  return GNX_OK;
}

// mixed-radix code of feature row r; a feature outside its vocabulary counts as 0 and sets range-flag bit 1
__device__ __forceinline__ int pk_feature_code(const int64_t* __restrict__ feat, int64_t r, int K, const dims_t& dims,
                                               int* __restrict__ flag) {
  int c = 0;
  bool bad = false;
  for (int k = 0; k < K; ++k) {
    int64_t f = feat[r * K + k];
    if (f < 0 || f >= dims.d[k]) {
      bad = true;
      f = 0;
    }
    c = c * dims.d[k] + (int)f;
  }
  if (bad) atomicOr(flag, 2);
  return c;
}

__global__ void k_feature_code(const int64_t* __restrict__ feat, int64_t rows, int K, dims_t dims,
                               const int* __restrict__ perm, int* __restrict__ code, int* __restrict__ flag) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= rows) return;
  int64_t r = perm ? perm[p] : p;
  code[p] = pk_feature_code(feat, r, K, dims, flag);
}

extern "C" int32_t gnx_feature_code(gnx_handle* h, const int64_t* feat, int64_t rows, int32_t K, const int32_t* dims,
                                    const int32_t* perm, int32_t* code, void* ws, size_t ws_bytes) {
  (void)ws;
  (void)ws_bytes;
  GNX_CHECK_ARG(h && dims && K > 0 && K <= 16 && rows >= 0, "gnx_feature_code: bad argument");
  GNX_CHECK_ARG(rows == 0 || (feat && code), "gnx_feature_code: NULL array with rows>0");
  dims_t d;
  const int32_t st = fill_dims("gnx_feature_code", K, dims, d);
  if (st != GNX_OK) return st;
  if (rows > 0) {
    hipLaunchKernelGGL(k_feature_code, dim3((unsigned)gnx_cdiv(rows, 256)), dim3(256), 0, h->stream, feat, rows, (int)K,
                       d, perm, code, h->d_flag);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// batch (non-decreasing) -> graph_ptr: ptr[g] = first n with batch[n] >= g ; ptr[B] = N
__device__ __forceinline__ void pk_graph_ptr(const int64_t* __restrict__ batch, int64_t n, int64_t N, int64_t B,
                                             int* __restrict__ ptr, int* __restrict__ flag) {
  int64_t prev = (n == 0) ? -1 : batch[n - 1];
  int64_t cur = (n == N) ? B : batch[n];
  if (n < N && (cur < 0 || cur >= B)) {
    atomicOr(flag, 4);
    return;
  }
  if (cur < prev) {
    atomicOr(flag, 8);
    return;
  }
  for (int64_t g = prev + 1; g <= cur; ++g) ptr[g] = (int)n;
}

__global__ void k_graph_ptr(const int64_t* __restrict__ batch, int64_t N, int64_t B, int* __restrict__ ptr,
                            int* __restrict__ flag) {
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n <= N) pk_graph_ptr(batch, n, N, B, ptr, flag);
}

extern "C" int32_t gnx_graph_ptr(gnx_handle* h, const int64_t* batch, int64_t N, int64_t B, int32_t* graph_ptr,
                                 void* ws, size_t ws_bytes) {
  (void)ws;
  (void)ws_bytes;
  GNX_CHECK_ARG(h && graph_ptr && N >= 0 && B >= 0 && (batch || N == 0), "gnx_graph_ptr: bad argument");
  hipLaunchKernelGGL(k_graph_ptr, dim3((unsigned)gnx_cdiv(N + 1, 256)), dim3(256), 0, h->stream, batch, N, B,
                     graph_ptr, h->d_flag);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pk_degree_scalers(int deg, float avg_log, float& amp, float& att) {
  float d = (float)deg;
  amp = logf(d + 1.0f) / avg_log;
  att = avg_log / logf(fmaxf(d, 1.0f) + 1.0f);
}

__global__ void k_degree_scalers(const int* __restrict__ rowptr, int64_t N, float avg_log, float* __restrict__ amp,
                                 float* __restrict__ att) {
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  pk_degree_scalers(rowptr[n + 1] - rowptr[n], avg_log, amp[n], att[n]);
}

extern "C" int32_t gnx_degree_scalers(gnx_handle* h, const int32_t* rowptr, int64_t N, float avg_deg_log, float* amp,
                                      float* att) {
  GNX_CHECK_ARG(h && N >= 0 && (N == 0 || (rowptr && amp && att)), "gnx_degree_scalers: bad argument");
  if (N == 0) return GNX_OK;
  hipLaunchKernelGGL(k_degree_scalers, dim3((unsigned)gnx_cdiv(N, 256)), dim3(256), 0, h->stream, rowptr, N,
                     avg_deg_log, amp, att);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// In-degree classes: nodes stably sorted by in-degree (a deterministic counting sort: per-block histograms -> scan ->
// stable ranks), and tile tables that never straddle two classes.  Lets PNA's post-layer 0 use one effective weight
// W_eff(d) = W1 + amp(d) W2 + att(d) W3 per class instead of the 12F-wide scaled operand (amp/att depend on d only).
// ---------------------------------------------------------------------------------------------------------------
__global__ void k_degree_max(const int* __restrict__ rowptr, int64_t N, int* __restrict__ out) {
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int d = (n < N) ? rowptr[n + 1] - rowptr[n] : 0;
  // wave max, then one atomic per wave
  for (int off = 32; off > 0; off >>= 1) d = max(d, __shfl_xor(d, off));
  if ((threadIdx.x & 63) == 0) atomicMax(out, d);
}

extern "C" int32_t gnx_degree_max(gnx_handle* h, const int32_t* rowptr, int64_t N, int32_t* max_degree_host) {
  GNX_CHECK_ARG(h && max_degree_host && N >= 0 && (N == 0 || rowptr), "gnx_degree_max: bad argument");
  int* d_out = h->d_flag + 8;  // scratch word inside the handle's flag block
  gnx_zero_ints(h, d_out, 1);
  if (N > 0) {
    hipLaunchKernelGGL(k_degree_max, dim3((unsigned)gnx_cdiv(N, 256)), dim3(256), 0, h->stream, rowptr, N, d_out);
    GNX_LAUNCH_CHECK();
  }
  int v = 0;
  GNX_HIP(hipMemcpyAsync(&v, d_out, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  GNX_HIP(hipStreamSynchronize(h->stream));
  *max_degree_host = v;
  return GNX_OK;
}

#define DC_BLOCK 256
#define DC_MAX_CLASSES 64

// blockhist[d * nblocks + b] = #nodes of block b with in-degree d
// keys != NULL: key of item n = keys[n]; else key = in-degree rowptr[n+1]-rowptr[n]
// Block `blk` of DC_BLOCK threads, one item each (d < 0: no item): blockhist[c * nblocks + blk] = #items of key c.
// hist: DC_MAX_CLASSES ints of LDS.  Every thread of the block must call.
__device__ __forceinline__ void pk_block_hist(int d, int D, int nblocks, int blk, int* __restrict__ blockhist,
                                              int* __restrict__ flag, int* hist) {
  if (threadIdx.x < DC_MAX_CLASSES) hist[threadIdx.x] = 0;
  __syncthreads();
  if (d >= 0) {
    if (d >= D) {  // only possible when D came from a caller's hint: reported through the sticky flag (bit 5)
      atomicOr(flag, 32);
      d = D - 1;
    }
    atomicAdd(&hist[d], 1);
  }
  __syncthreads();
  if ((int)threadIdx.x < D) blockhist[threadIdx.x * nblocks + blk] = hist[threadIdx.x];
}

// key of item n clamped to [0, D): keys[n], or the in-degree of node n without keys
__device__ __forceinline__ int pk_dc_key(const int* __restrict__ rowptr, const int* __restrict__ keys, int64_t n) {
  int d = keys ? keys[n] : rowptr[n + 1] - rowptr[n];
  return d < 0 ? 0 : d;
}

__global__ void __launch_bounds__(DC_BLOCK) k_dc_hist(const int* __restrict__ rowptr, const int* __restrict__ keys,
                                                       int64_t N, int D, int nblocks, int* __restrict__ blockhist,
                                                       int* __restrict__ flag) {
  __shared__ int hist[DC_MAX_CLASSES];
  int64_t n = (int64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
  pk_block_hist(n < N ? pk_dc_key(rowptr, keys, n) : -1, D, nblocks, blockIdx.x, blockhist, flag, hist);
}

// stable position of every node: scanned block offset of its (class, block) + rank among earlier same-class threads.
// Block `blk` of DC_BLOCK threads, item n of key d each (d < 0: no item); block 0 also writes the D + 1 class bounds.
// blockoff counts from the start of the whole order, or, with `base` (D ints, LDS), from the start of its class base[d].
// degs: DC_BLOCK ints of LDS.  Every thread of the block must call.
__device__ __forceinline__ void pk_block_fill(int d, int64_t n, int64_t N, int D, int nblocks, int blk,
                                              const int* __restrict__ blockoff, const int* base, int* __restrict__ dperm,
                                              int* __restrict__ cls_ptr, int* degs) {
  if (d >= D) d = D - 1;
  degs[threadIdx.x] = d;
  __syncthreads();
  if (d >= 0) {
    int rank = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) rank += (degs[t] == d) ? 1 : 0;
    dperm[blockoff[d * nblocks + blk] + (base ? base[d] : 0) + rank] = (int)n;
  }
  if (blk == 0 && (int)threadIdx.x <= D)
    cls_ptr[threadIdx.x] = ((int)threadIdx.x == D) ? (int)N
                                                   : blockoff[threadIdx.x * nblocks] + (base ? base[threadIdx.x] : 0);
}

__global__ void __launch_bounds__(DC_BLOCK) k_dc_fill(const int* __restrict__ rowptr, const int* __restrict__ keys,
                                                       int64_t N, int D, int nblocks,
                                                       const int* __restrict__ blockoff, int* __restrict__ dperm,
                                                       int* __restrict__ cls_ptr) {
  __shared__ int degs[DC_BLOCK];
  int64_t n = (int64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
  pk_block_fill(n < N ? pk_dc_key(rowptr, keys, n) : -1, n, N, D, nblocks, blockIdx.x, blockoff, nullptr, dperm, cls_ptr, degs);
}

extern "C" size_t gnx_degree_classes_workspace_bytes(int64_t N, int32_t D) {
  if (N < 0) N = 0;
  int64_t nblocks = gnx_cdiv(N > 0 ? N : 1, DC_BLOCK);
  size_t ints = 2 * (size_t)(D * nblocks + 1) + scan_ws_ints_total(D * nblocks) + 64;
  return ints * sizeof(int);
}

// Stable grouping of n items by a key in [0, D), D <= DC_MAX_CLASSES: the in-degree of node i (rowptr) or keys[i] (rowptr
// NULL).  pos int32[n] = item ids sorted by key, ascending inside a key; bounds int32[D+1].  Per-block histograms -> scan
// -> stable ranks.  ws: gnx_degree_classes_workspace_bytes(n, D); a shorter one is GNX_E_WORKSPACE of the entry `who`.
static int32_t group_small_keys(gnx_handle* h, const char* who, const int* rowptr, const int* keys, int64_t n, int D,
                                int* pos, int* bounds, void* ws, size_t ws_bytes) {
  if (ws_bytes < gnx_degree_classes_workspace_bytes(n, D) || !ws) {
    gnx_set_error("%s: workspace %zu < %zu", who, ws_bytes, gnx_degree_classes_workspace_bytes(n, D));
    return GNX_E_WORKSPACE;
  }
  int nblocks = (int)gnx_cdiv(n > 0 ? n : 1, DC_BLOCK);
  int* blockhist = reinterpret_cast<int*>(ws);
  int* blockoff = blockhist + (size_t)D * nblocks + 1;
  int* scan_ws = blockoff + (size_t)D * nblocks + 1;
  hipLaunchKernelGGL(k_dc_hist, dim3(nblocks), dim3(DC_BLOCK), 0, h->stream, rowptr, keys, n, D, nblocks, blockhist,
                     h->d_flag);
  GNX_LAUNCH_CHECK();
  int32_t st = exclusive_scan(h, blockhist, blockoff, (int64_t)D * nblocks, scan_ws, false);
  if (st != GNX_OK) return st;
  hipLaunchKernelGGL(k_dc_fill, dim3(nblocks), dim3(DC_BLOCK), 0, h->stream, rowptr, keys, n, D, nblocks, blockoff, pos,
                     bounds);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_degree_classes(gnx_handle* h, const int32_t* rowptr, int64_t N, int32_t D, int32_t* dperm,
                                      int32_t* cls_ptr, void* ws, size_t ws_bytes) {
  GNX_CHECK_ARG(h && rowptr && cls_ptr && N >= 0 && D >= 1 && D <= DC_MAX_CLASSES && (N == 0 || dperm),
                "gnx_degree_classes: bad argument (D must be in [1,%d])", DC_MAX_CLASSES);
  return group_small_keys(h, "gnx_degree_classes", rowptr, nullptr, N, D, dperm, cls_ptr, ws, ws_bytes);
}

// Stable grouping of E items by a small integer key (0 <= key < R <= 64): pos int32[E] = item ids sorted by key
// (ascending id inside a key), ptr int32[R+1].  Used for the per-edge bond code: the inverted index lets the bond-table
// gradient be a gather-sum over contiguous index runs instead of 10^7 atomics.  ws: gnx_degree_classes_workspace_bytes(E, R).
extern "C" int32_t gnx_group_by_small_key(gnx_handle* h, const int32_t* keys, int64_t E, int32_t R, int32_t* pos,
                                          int32_t* ptr, void* ws, size_t ws_bytes) {
  GNX_CHECK_ARG(h && ptr && E >= 0 && R >= 1 && R <= DC_MAX_CLASSES && (E == 0 || (keys && pos)),
                "gnx_group_by_small_key: bad argument (R must be in [1,%d])", DC_MAX_CLASSES);
  return group_small_keys(h, "gnx_group_by_small_key", nullptr, keys, E, R, pos, ptr, ws, ws_bytes);
}

// tile table: for class c, ceil(n_c / tile_rows) tiles of (first position in dperm, #rows, class); ntiles[0] = count.
// One thread per tile (grid-stride): the class of tile t is found by walking the D <= 4096 class sizes (a serial loop of one
// thread over ~1000 tiles took 15-28 us inside every step's packing phase).
// block `blk` of `nblk` blocks; cls_ptr may live in LDS
__device__ __forceinline__ void pk_class_tiles(const int* cls_ptr, int D, int tile_rows, int* __restrict__ tile_info,
                                               int* __restrict__ ntiles, int blk, int nblk) {
  int total = 0;
  for (int c = 0; c < D; ++c) total += (cls_ptr[c + 1] - cls_ptr[c] + tile_rows - 1) / tile_rows;
  if (blk == 0 && threadIdx.x == 0) ntiles[0] = total;
  for (int t = blk * blockDim.x + threadIdx.x; t < total; t += nblk * blockDim.x) {
    int first = 0, c = 0;
    for (; c < D; ++c) {
      const int nt = (cls_ptr[c + 1] - cls_ptr[c] + tile_rows - 1) / tile_rows;
      if (t < first + nt) break;
      first += nt;
    }
    const int r = cls_ptr[c] + (t - first) * tile_rows;
    const int rows = cls_ptr[c + 1] - r;
    tile_info[3 * t + 0] = r;
    tile_info[3 * t + 1] = rows < tile_rows ? rows : tile_rows;
    tile_info[3 * t + 2] = c;
  }
}

#define CLASS_TILE_BLOCKS 16
__global__ void __launch_bounds__(256) k_class_tiles(const int* __restrict__ cls_ptr, int D, int tile_rows,
                                                     int* __restrict__ tile_info, int* __restrict__ ntiles) {
  pk_class_tiles(cls_ptr, D, tile_rows, tile_info, ntiles, blockIdx.x, gridDim.x);
}

extern "C" int32_t gnx_class_tiles(gnx_handle* h, const int32_t* cls_ptr, int32_t D, int32_t tile_rows,
                                   int32_t* tile_info, int32_t* ntiles) {
  GNX_CHECK_ARG(h && cls_ptr && tile_info && ntiles && D >= 1 && tile_rows > 0, "gnx_class_tiles: bad argument");
  hipLaunchKernelGGL(k_class_tiles, dim3(CLASS_TILE_BLOCKS), dim3(256), 0, h->stream, cls_ptr, (int)D, (int)tile_rows, tile_info, ntiles);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// gnx_pack_batch: everything above for one batch in 8 launches (include/gnx.h).  The phases are the device functions of
// the single-purpose entries, cut at the points where one phase reads what ANY thread of the previous one wrote; a launch
// boundary is the only ordering between workgroups.  Integer atomics land in any order: the row fill and the column
// fill are sorted per group afterwards, counts and histograms are sums, so no output depends on that order.
//
//   1 zero      one slab: in-degree and out-degree counters, degree totals, code totals
//   2 edges     per edge: int32 endpoints, both degree counts, raw bond code;  per node: graph_ptr
//   3 scan      both counter arrays in tiles of SCAN_TILE: prefix inside the tile, and the tile's sum
//   4 fill      every block scans the <= SCAN_TILE tile sums itself (LDS).  Edge blocks: edge ids into their rows, the
//               in-degree counter counting back down to 0 as the cursor.  Tile blocks: rowptr / colptr = prefix inside
//               the tile + the tile's offset, and the totals
//   5 rows      per node: sort the row, write src / dst / code of its positions, push each position into its source's
//               column group (the out-degree counter as cursor), amp / att, per-block degree histogram
//   6 cols      per node: sort the column group;  per 256 positions: per-block code histogram
//   7 offsets   one workgroup per class / code: its row of per-block counts -> offsets inside the class, and its total
//   8 tables    every block sums the <= 64 totals below its class itself.  dperm and code positions from the offsets
//               (with cls_ptr / code ptr); class tile tables; edge tiles from rowptr
// Above PB_SCAN_MAX_N nodes the tile sums no longer fit one block's scan: launch 3 becomes an exclusive_scan of each
// counter array (three levels of tiles, two adds and the total: 6 launches each) and launch 4 a fill that reads rowptr.
// gnx_pack_csr (at the end of this file) is launches 1 to 6 with no optional part.
//
// A single workgroup per counter array (4096 counts per round, next round's loads in flight) was measured against the
// tiled form and lost at every size: 44 us against 21 us for both arrays at N = 81 920, 171 us against 26 us at 327 680
// (each round pays a load and a store round trip); DESIGN.md §4.
// ---------------------------------------------------------------------------------------------------------------
#define PB_SCAN_MAX_N ((int64_t)SCAN_TILE * SCAN_TILE)

struct pb_args {
  const int64_t *ei, *ea, *batch;
  int64_t N, E, B;
  dims_t dims;
  int K, D, R, n_avg;
  float avg[GNX_PACK_MAX_AVG];
  int tile_rows[3];
  int etile_w, etiles, nb_n, nb_e;
  unsigned parts;
  int *rowptr, *perm, *src, *dst, *colptr, *cpos, *code, *graph_ptr;
  float *amp[GNX_PACK_MAX_AVG], *att[GNX_PACK_MAX_AVG];
  int *dperm, *cls_ptr, *tiles[3], *ntiles[3], *code_pos, *code_ptr, *edge_tiles;
  int *cnt_in, *cnt_out, *deghist, *codehist, *src0, *dst0, *code0, *bh_deg, *bh_code;
  int *lrow, *lcol, *tsum_in, *tsum_out;  // prefix inside each SCAN_TILE of the counters, and the tiles' sums
  int stiles;                             // 0: rowptr / colptr come from exclusive_scan
  int* flag;
};

__global__ void __launch_bounds__(256) k_pb_edges(pb_args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.E) {
    int s, d;
    pk_convert_edge(a.ei, i, a.E, a.N, a.flag, s, d);
    a.src0[i] = s;
    a.dst0[i] = d;
    atomicAdd(&a.cnt_in[d], 1);
    atomicAdd(&a.cnt_out[s], 1);
    a.code0[i] = a.ea ? pk_feature_code(a.ea, i, a.K, a.dims, a.flag) : 0;
  }
  if (a.batch) {
    if (i <= a.N) pk_graph_ptr(a.batch, i, a.N, a.B, a.graph_ptr, a.flag);
  } else if (i == 0) {
    a.graph_ptr[0] = 0;
    a.graph_ptr[1] = (int)a.N;
  }
}

// launch 3: block b < tiles: tile b of the in-degree counters, else tile b - tiles of the out-degree counters
__global__ void __launch_bounds__(SCAN_BLOCK) k_pb_scan_tiles(pb_args a) {
  __shared__ int s[SCAN_BLOCK];
  const bool in = (int)blockIdx.x < a.stiles;
  const int t = in ? blockIdx.x : blockIdx.x - a.stiles;
  const int total = pk_scan_tile(in ? a.cnt_in : a.cnt_out, in ? a.lrow : a.lcol, (int64_t)t * SCAN_TILE, a.N, 0, s);
  if (threadIdx.x == 0) (in ? a.tsum_in : a.tsum_out)[t] = total;
}

// launch 4.  a.stiles == 0: rowptr is final already (exclusive_scan), edge blocks only.
__global__ void __launch_bounds__(SCAN_BLOCK) k_pb_fill(pb_args a, int edge_blocks) {
  __shared__ int s[SCAN_BLOCK];
  __shared__ int off[SCAN_TILE];
  if ((int)blockIdx.x < edge_blocks) {
    if (a.stiles) pk_scan_tile(a.tsum_in, off, 0, a.stiles, 0, s);
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (e >= a.E) return;
    const int d = a.dst0[e];
    const int row = a.stiles ? a.lrow[d] + off[d / SCAN_TILE] : a.rowptr[d];
    a.perm[row + atomicAdd(&a.cnt_in[d], -1) - 1] = (int)e;
    return;
  }
  const int b = blockIdx.x - edge_blocks;
  const bool in = b < a.stiles;
  const int t = in ? b : b - a.stiles;
  const int total = pk_scan_tile(in ? a.tsum_in : a.tsum_out, off, 0, a.stiles, 0, s);
  __syncthreads();
  const int* local = in ? a.lrow : a.lcol;
  int* out = in ? a.rowptr : a.colptr;
  const int o = off[t];
  for (int64_t i = (int64_t)t * SCAN_TILE + threadIdx.x; i < a.N && i < (int64_t)(t + 1) * SCAN_TILE; i += SCAN_BLOCK)
    out[i] = local[i] + o;
  if (t == 0 && threadIdx.x == 0) out[a.N] = total;
}

__global__ void __launch_bounds__(DC_BLOCK) k_pb_rows(pb_args a) {
  __shared__ int hist[DC_MAX_CLASSES];
  const int64_t n = (int64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
  int deg = -1;
  if (n < a.N) {
    const int b = a.rowptr[n], e = a.rowptr[n + 1];
    deg = e - b;
    pk_sort_group(a.perm, b, e);
    for (int p = b; p < e; ++p) {
      const int ed = a.perm[p], s = a.src0[ed];
      a.src[p] = s;
      a.dst[p] = a.dst0[ed];
      a.code[p] = a.code0[ed];
      a.cpos[a.colptr[s] + atomicAdd(&a.cnt_out[s], -1) - 1] = p;
    }
    for (int k = 0; k < a.n_avg; ++k) pk_degree_scalers(deg, a.avg[k], a.amp[k][n], a.att[k][n]);
  }
  if (a.parts & GNX_PACK_CLASSES) pk_block_hist(deg, a.D, a.nb_n, blockIdx.x, a.bh_deg, a.flag, hist);
}

__global__ void __launch_bounds__(DC_BLOCK) k_pb_cols(pb_args a) {
  __shared__ int hist[DC_MAX_CLASSES];
  if ((int)blockIdx.x < a.nb_n) {
    const int64_t n = (int64_t)blockIdx.x * DC_BLOCK + threadIdx.x;
    if (n < a.N) pk_sort_group(a.cpos, a.colptr[n], a.colptr[n + 1]);
    return;
  }
  const int blk = blockIdx.x - a.nb_n;
  const int64_t p = (int64_t)blk * DC_BLOCK + threadIdx.x;
  pk_block_hist(p < a.E ? pk_dc_key(nullptr, a.code, p) : -1, a.R, a.nb_e, blk, a.bh_code, a.flag, hist);
}

// block c < nd: class c of the degree table; block nd + r: code r.  Row of per-block counts -> offsets inside the class,
// in place, and the class's total.
__global__ void __launch_bounds__(SCAN_BLOCK) k_pb_offsets(pb_args a, int nd) {
  __shared__ int s[SCAN_BLOCK];
  const bool deg = (int)blockIdx.x < nd;
  const int c = deg ? blockIdx.x : blockIdx.x - nd;
  const int nb = deg ? a.nb_n : a.nb_e;
  int* row = (deg ? a.bh_deg : a.bh_code) + (int64_t)c * nb;
  int carry = 0;
  for (int64_t t0 = 0; t0 < nb; t0 += SCAN_TILE) carry += pk_scan_tile(row, row, t0, nb, carry, s);
  if (threadIdx.x == 0) (deg ? a.deghist : a.codehist)[c] = carry;
}

// base[c] = sum of total[0..c) for c <= D, by the calling block
__device__ __forceinline__ void pk_class_bases(const int* __restrict__ total, int D, int* base) {
  if ((int)threadIdx.x < D) base[threadIdx.x + 1] = total[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    base[0] = 0;
    for (int c = 1; c <= D; ++c) base[c] += base[c - 1];
  }
  __syncthreads();
}

__global__ void __launch_bounds__(DC_BLOCK) k_pb_tables(pb_args a, int b_pos, int b_tiles, int b_etiles) {
  __shared__ int lds[DC_BLOCK];
  __shared__ int base[DC_MAX_CLASSES + 1];
  int blk = blockIdx.x;
  if (blk < b_pos) {  // dperm, cls_ptr
    pk_class_bases(a.deghist, a.D, base);
    const int64_t n = (int64_t)blk * DC_BLOCK + threadIdx.x;
    pk_block_fill(n < a.N ? pk_dc_key(a.rowptr, nullptr, n) : -1, n, a.N, a.D, a.nb_n, blk, a.bh_deg, base, a.dperm,
                  a.cls_ptr, lds);
  } else if (blk < b_tiles) {  // code positions, code ptr
    pk_class_bases(a.codehist, a.R, base);
    blk -= b_pos;
    const int64_t p = (int64_t)blk * DC_BLOCK + threadIdx.x;
    pk_block_fill(p < a.E ? pk_dc_key(nullptr, a.code, p) : -1, p, a.E, a.R, a.nb_e, blk, a.bh_code, base, a.code_pos,
                  a.code_ptr, lds);
  } else if (blk < b_etiles) {  // class tile tables, from this block's own copy of the class bounds
    blk -= b_tiles;
    const int which = blk / CLASS_TILE_BLOCKS;
    if (a.tile_rows[which] <= 0) return;
    pk_class_bases(a.deghist, a.D, base);  // base[D] = N
    pk_class_tiles(base, a.D, a.tile_rows[which], a.tiles[which], a.ntiles[which], blk % CLASS_TILE_BLOCKS,
                   CLASS_TILE_BLOCKS);
  } else {
    const int j = (blk - b_etiles) * DC_BLOCK + threadIdx.x;
    if (j <= a.etiles) gnx_edge_tile_entry(a.rowptr, a.N, a.E, a.etile_w, a.etiles, j, a.edge_tiles);
  }
}

static inline size_t pb_pad(size_t ints) { return (ints + 3) & ~(size_t)3; }

extern "C" int64_t gnx_pack_batch_scan_chunk(void) { return SCAN_TILE; }
extern "C" int64_t gnx_pack_batch_scan_bound(void) { return PB_SCAN_MAX_N; }

extern "C" size_t gnx_pack_batch_workspace_bytes(int64_t N, int64_t E, int32_t D, int32_t R) {
  if (N < 0) N = 0;
  if (E < 0) E = 0;
  if (D < 1) D = 1;
  if (R < 1) R = 1;
  const size_t nb_n = (size_t)gnx_cdiv(N > 0 ? N : 1, DC_BLOCK), nb_e = (size_t)gnx_cdiv(E > 0 ? E : 1, DC_BLOCK);
  // counters + totals | src0, dst0, code0 | per-block histograms | prefixes inside the tiles | tile sums or scan workspace
  size_t ints = 2 * pb_pad((size_t)N + 1) + 2 * DC_MAX_CLASSES + 3 * pb_pad((size_t)E) + pb_pad((size_t)D * nb_n) +
                pb_pad((size_t)R * nb_e) + 2 * pb_pad((size_t)N + 1) + 2 * SCAN_TILE + scan_ws_ints_total(N) + 64;
  return ints * sizeof(int);
}

extern "C" int32_t gnx_pack_batch(gnx_handle* h, const gnx_pack_batch_args* g) {
  GNX_CHECK_ARG(h && g, "gnx_pack_batch: NULL argument");
  const int64_t N = g->N, E = g->E;
  int32_t st = check_sizes("gnx_pack_batch", N, E);
  if (st != GNX_OK) return st;
  GNX_CHECK_ARG(g->rowptr && g->colptr && g->graph_ptr, "gnx_pack_batch: rowptr/colptr/graph_ptr NULL");
  GNX_CHECK_ARG(E == 0 || (g->edge_index && g->perm && g->src && g->dst && g->cpos && g->code),
                "gnx_pack_batch: NULL edge array with E>0");
  GNX_CHECK_ARG(!g->batch || g->B >= 0, "gnx_pack_batch: B < 0");
  GNX_CHECK_ARG(g->n_avg >= 0 && g->n_avg <= GNX_PACK_MAX_AVG, "gnx_pack_batch: n_avg must be in [0,%d]", GNX_PACK_MAX_AVG);
  const unsigned parts = g->parts;
  const bool classes = parts & GNX_PACK_CLASSES, cindex = parts & GNX_PACK_CODE_INDEX, etiles = parts & GNX_PACK_EDGE_TILES;
  const int D = g->max_degree + 1, R = g->R;
  pb_args a = {};
  if (g->edge_attr) {
    GNX_CHECK_ARG(g->K > 0 && g->K <= 16, "gnx_pack_batch: K must be in [1,16]");
    if ((st = fill_dims("gnx_pack_batch", g->K, g->bond_dims, a.dims)) != GNX_OK) return st;
  }
  for (int k = 0; k < g->n_avg; ++k) {
    GNX_CHECK_ARG(N == 0 || (g->amp[k] && g->att[k]), "gnx_pack_batch: amp/att[%d] NULL", k);
    a.avg[k] = g->avg_deg_log[k];
    a.amp[k] = g->amp[k];
    a.att[k] = g->att[k];
  }
  if (classes) {
    GNX_CHECK_ARG(D >= 1 && D <= DC_MAX_CLASSES && g->cls_ptr && (N == 0 || g->dperm),
                  "gnx_pack_batch: classes need max_degree in [0,%d), cls_ptr and dperm", DC_MAX_CLASSES);
    for (int i = 0; i < 3; ++i) {
      GNX_CHECK_ARG(g->tile_rows[i] <= 0 || (g->tiles[i] && g->ntiles[i]), "gnx_pack_batch: tiles[%d]/ntiles[%d] NULL", i, i);
      a.tile_rows[i] = g->tile_rows[i];
      a.tiles[i] = g->tiles[i];
      a.ntiles[i] = g->ntiles[i];
    }
  }
  if (cindex)
    GNX_CHECK_ARG(R >= 1 && R <= DC_MAX_CLASSES && E > 0 && g->code_pos && g->code_ptr,
                  "gnx_pack_batch: the code index needs R in [1,%d], E > 0, code_pos and code_ptr", DC_MAX_CLASSES);
  if (etiles)
    GNX_CHECK_ARG(g->edge_tile_w >= 1 && g->edge_tile_w <= 64 && E > 0 && N > 0 && g->edge_tiles,
                  "gnx_pack_batch: edge tiles need edge_tile_w in [1,64], E > 0, N > 0 and edge_tiles");
  const size_t need = gnx_pack_batch_workspace_bytes(N, E, classes ? D : 1, cindex ? R : 1);
  if (g->ws_bytes < need || !g->ws) {
    gnx_set_error("gnx_pack_batch: workspace %zu < %zu", g->ws_bytes, need);
    return GNX_E_WORKSPACE;
  }
  a.ei = g->edge_index, a.ea = g->edge_attr, a.batch = g->batch;
  a.N = N, a.E = E, a.B = g->B;
  a.K = g->K, a.D = D, a.R = R, a.n_avg = g->n_avg;
  a.etile_w = g->edge_tile_w, a.etiles = etiles ? gnx_edge_tiles_count(E, g->edge_tile_w) : 0;
  a.nb_n = (int)gnx_cdiv(N > 0 ? N : 1, DC_BLOCK), a.nb_e = (int)gnx_cdiv(E > 0 ? E : 1, DC_BLOCK);
  a.parts = parts;
  a.rowptr = g->rowptr, a.perm = g->perm, a.src = g->src, a.dst = g->dst, a.colptr = g->colptr, a.cpos = g->cpos;
  a.code = g->code, a.graph_ptr = g->graph_ptr, a.dperm = g->dperm, a.cls_ptr = g->cls_ptr;
  a.code_pos = g->code_pos, a.code_ptr = g->code_ptr, a.edge_tiles = g->edge_tiles;
  a.flag = h->d_flag;
  // workspace: the zeroed slab first
  int* w = reinterpret_cast<int*>(g->ws);
  const size_t cnt = pb_pad((size_t)N + 1);
  a.cnt_in = w, a.cnt_out = a.cnt_in + cnt, a.deghist = a.cnt_out + cnt, a.codehist = a.deghist + DC_MAX_CLASSES;
  const size_t slab = 2 * cnt + 2 * DC_MAX_CLASSES;
  a.src0 = w + slab, a.dst0 = a.src0 + pb_pad((size_t)E), a.code0 = a.dst0 + pb_pad((size_t)E);
  a.bh_deg = a.code0 + pb_pad((size_t)E);
  a.bh_code = a.bh_deg + pb_pad(classes ? (size_t)D * a.nb_n : a.nb_n);
  a.lrow = a.bh_code + pb_pad(cindex ? (size_t)R * a.nb_e : a.nb_e), a.lcol = a.lrow + cnt;
  a.tsum_in = a.lcol + cnt, a.tsum_out = a.tsum_in + SCAN_TILE;
  int* scan_ws = a.tsum_out + SCAN_TILE;
  const bool tiled = N <= PB_SCAN_MAX_N && !(parts & GNX_PACK_TILED_SCAN);
  a.stiles = tiled ? (int)gnx_cdiv(N > 0 ? N : 1, SCAN_TILE) : 0;

  gnx_zero_ints(h, w, (int64_t)slab);
  GNX_LAUNCH_CHECK();
  const int64_t work = E > N + 1 ? E : N + 1;
  hipLaunchKernelGGL(k_pb_edges, dim3((unsigned)gnx_cdiv(work, 256)), dim3(256), 0, h->stream, a);
  GNX_LAUNCH_CHECK();
  if (tiled) {
    hipLaunchKernelGGL(k_pb_scan_tiles, dim3(2 * a.stiles), dim3(SCAN_BLOCK), 0, h->stream, a);
    GNX_LAUNCH_CHECK();
  } else {
    int32_t st = exclusive_scan(h, a.cnt_in, a.rowptr, N, scan_ws, true);
    if (st == GNX_OK) st = exclusive_scan(h, a.cnt_out, a.colptr, N, scan_ws, true);
    if (st != GNX_OK) return st;
  }
  const int edge_blocks = (int)gnx_cdiv(E, SCAN_BLOCK);
  if (edge_blocks + 2 * a.stiles > 0) {
    hipLaunchKernelGGL(k_pb_fill, dim3(edge_blocks + 2 * a.stiles), dim3(SCAN_BLOCK), 0, h->stream, a, edge_blocks);
    GNX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pb_rows, dim3(a.nb_n), dim3(DC_BLOCK), 0, h->stream, a);
  GNX_LAUNCH_CHECK();
  if (E > 0) {
    hipLaunchKernelGGL(k_pb_cols, dim3(a.nb_n + (cindex ? a.nb_e : 0)), dim3(DC_BLOCK), 0, h->stream, a);
    GNX_LAUNCH_CHECK();
  }
  const int nd = classes ? D : 0, nr = cindex ? R : 0;
  if (nd + nr > 0) {
    hipLaunchKernelGGL(k_pb_offsets, dim3(nd + nr), dim3(SCAN_BLOCK), 0, h->stream, a, nd);
    GNX_LAUNCH_CHECK();
  }
  const int b_pos = classes ? a.nb_n : 0, b_tiles = b_pos + (cindex ? a.nb_e : 0);
  const int b_etiles = b_tiles + (classes ? 3 * CLASS_TILE_BLOCKS : 0);
  const int b_end = b_etiles + (etiles ? (int)gnx_cdiv(a.etiles + 1, DC_BLOCK) : 0);
  if (b_end > 0) {
    hipLaunchKernelGGL(k_pb_tables, dim3(b_end), dim3(DC_BLOCK), 0, h->stream, a, b_pos, b_tiles, b_etiles);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// gnx_pack_csr: the CSR alone, by launches 1 to 6 of gnx_pack_batch.  The bond codes (all 0) and graph_ptr = [0, N] that
// those launches write anyway go behind the batch workspace.
// ---------------------------------------------------------------------------------------------------------------
extern "C" size_t gnx_pack_csr_workspace_bytes(int64_t N, int64_t E) {
  if (E < 0) E = 0;
  return gnx_pack_batch_workspace_bytes(N, E, 1, 1) + (pb_pad((size_t)E) + 2) * sizeof(int);
}

extern "C" int32_t gnx_pack_csr(gnx_handle* h, const int64_t* edge_index, int64_t E, int64_t N, int32_t* rowptr,
                                int32_t* perm, int32_t* src, int32_t* dst, int32_t* colptr, int32_t* cpos, void* ws,
                                size_t ws_bytes) {
  GNX_CHECK_ARG(h != nullptr, "gnx_pack_csr: handle is NULL");
  const int32_t st = check_sizes("gnx_pack_csr", N, E);
  if (st != GNX_OK) return st;
  GNX_CHECK_ARG(rowptr && colptr, "gnx_pack_csr: rowptr/colptr NULL");
  GNX_CHECK_ARG(E == 0 || (edge_index && perm && src && dst && cpos), "gnx_pack_csr: NULL edge array with E>0");
  if (ws_bytes < gnx_pack_csr_workspace_bytes(N, E) || (!ws && ws_bytes)) {
    gnx_set_error("gnx_pack_csr: workspace %zu < %zu", ws_bytes, gnx_pack_csr_workspace_bytes(N, E));
    return GNX_E_WORKSPACE;
  }
  GNX_CHECK_ARG(ws != nullptr, "gnx_pack_csr: workspace is NULL");
  gnx_pack_batch_args a = {};
  a.edge_index = edge_index, a.N = N, a.E = E;
  a.rowptr = rowptr, a.perm = perm, a.src = src, a.dst = dst, a.colptr = colptr, a.cpos = cpos;
  a.ws = ws, a.ws_bytes = gnx_pack_batch_workspace_bytes(N, E, 1, 1);
  a.code = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + a.ws_bytes);
  a.graph_ptr = a.code + pb_pad((size_t)E);
  return gnx_pack_batch(h, &a);
}
