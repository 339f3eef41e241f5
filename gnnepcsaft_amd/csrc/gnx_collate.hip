// On-device batch collation from a device-resident dataset (gnnepcsaft_amd/data/device.py): the integer work of
// Batch.from_data_list as two small scans and one block-copy kernel.  The dataset is stored as the concatenation of its
// graphs (x int64[sumN,9], edge_index int64[2,sumE] with graph-local node ids, edge_attr int64[sumE,3]) plus the two
// offset arrays node_ptr / edge_ptr int64[G+1]; batch slot b takes graph idx[b].  Everything a graph contributes is a
// contiguous block, so a batch is B block copies.  Plain vector stores only: bit-identical from call to call.
#include "gnx_common.hpp"

#define CL_ITEMS 4
#define CL_BLOCK 256
#define CL_TILE (CL_ITEMS * CL_BLOCK)
#define CL_FLAG_IDX 128  // sticky range-flag bit 7: a batch index outside [0,G) (or totals that do not fit the outputs)

__device__ __forceinline__ int64_t cl_graph(const int64_t* __restrict__ idx, int64_t b, int64_t G, int* __restrict__ flag) {
  int64_t g = idx[b];
  if (g < 0 || g >= G) {
    atomicOr(flag, CL_FLAG_IDX);
    g = g < 0 ? 0 : G - 1;
  }
  return g;
}

// ---------------------------------------------------------------------------------------------------------------
// Exclusive prefix sums of the selected graphs' node and edge counts, without a workspace: every 1024-slot tile is
// scanned on its own and parks its total in its first output element (whose local value, 0, carries no information);
// one workgroup then turns the parked totals into the tiles' offsets in place (which are those elements' final values)
// and a third launch adds each tile's offset to the rest of the tile.  B <= 1024 is the first launch alone.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CL_BLOCK) k_collate_scan_tile(const int64_t* __restrict__ node_ptr,
                                                                const int64_t* __restrict__ edge_ptr, int64_t G,
                                                                const int64_t* __restrict__ idx, int64_t B,
                                                                int64_t* __restrict__ out_ptr,
                                                                int64_t* __restrict__ out_eptr, int* __restrict__ flag) {
  __shared__ int64_t sn[CL_BLOCK], se[CL_BLOCK];
  const int64_t tile0 = (int64_t)blockIdx.x * CL_TILE;
  const int64_t base = tile0 + (int64_t)threadIdx.x * CL_ITEMS;
  int64_t vn[CL_ITEMS], ve[CL_ITEMS];
  int64_t tn = 0, te = 0;
#pragma unroll
  for (int i = 0; i < CL_ITEMS; ++i) {
    vn[i] = ve[i] = 0;
    if (base + i < B) {
      const int64_t g = cl_graph(idx, base + i, G, flag);
      vn[i] = node_ptr[g + 1] - node_ptr[g];
      ve[i] = edge_ptr[g + 1] - edge_ptr[g];
    }
    tn += vn[i];
    te += ve[i];
  }
  sn[threadIdx.x] = tn;
  se[threadIdx.x] = te;
  __syncthreads();
  for (int off = 1; off < CL_BLOCK; off <<= 1) {  // Hillis-Steele inclusive scan over the 256 thread totals
    const int64_t an = (threadIdx.x >= off) ? sn[threadIdx.x - off] : 0;
    const int64_t ae = (threadIdx.x >= off) ? se[threadIdx.x - off] : 0;
    __syncthreads();
    sn[threadIdx.x] += an;
    se[threadIdx.x] += ae;
    __syncthreads();
  }
  int64_t en = sn[threadIdx.x] - tn, ee = se[threadIdx.x] - te;
  const bool single = gridDim.x == 1;
#pragma unroll
  for (int i = 0; i < CL_ITEMS; ++i) {
    if (base + i < B && (single || base + i != tile0)) {
      out_ptr[base + i] = en;
      out_eptr[base + i] = ee;
    }
    en += vn[i];
    ee += ve[i];
  }
  if (threadIdx.x == CL_BLOCK - 1) {
    const int64_t at = single ? B : tile0;
    out_ptr[at] = sn[CL_BLOCK - 1];
    out_eptr[at] = se[CL_BLOCK - 1];
  }
}

// one workgroup: out[t * 1024] (tile totals) -> exclusive prefix over the tiles, out[B] = grand total
__global__ void __launch_bounds__(CL_BLOCK) k_collate_scan_offsets(int64_t B, int64_t tiles, int64_t* __restrict__ out_ptr,
                                                                   int64_t* __restrict__ out_eptr) {
  __shared__ int64_t sn[CL_BLOCK], se[CL_BLOCK];
  int64_t carry_n = 0, carry_e = 0;
  for (int64_t t0 = 0; t0 < tiles; t0 += CL_BLOCK) {
    const int64_t t = t0 + threadIdx.x;
    const int64_t vn = t < tiles ? out_ptr[t * CL_TILE] : 0, ve = t < tiles ? out_eptr[t * CL_TILE] : 0;
    sn[threadIdx.x] = vn;
    se[threadIdx.x] = ve;
    __syncthreads();
    for (int off = 1; off < CL_BLOCK; off <<= 1) {
      const int64_t an = (threadIdx.x >= off) ? sn[threadIdx.x - off] : 0;
      const int64_t ae = (threadIdx.x >= off) ? se[threadIdx.x - off] : 0;
      __syncthreads();
      sn[threadIdx.x] += an;
      se[threadIdx.x] += ae;
      __syncthreads();
    }
    if (t < tiles) {
      out_ptr[t * CL_TILE] = carry_n + sn[threadIdx.x] - vn;
      out_eptr[t * CL_TILE] = carry_e + se[threadIdx.x] - ve;
    }
    carry_n += sn[CL_BLOCK - 1];
    carry_e += se[CL_BLOCK - 1];
    __syncthreads();  // sn / se are rewritten by the next round
  }
  if (threadIdx.x == 0) {
    out_ptr[B] = carry_n;
    out_eptr[B] = carry_e;
  }
}

__global__ void __launch_bounds__(CL_BLOCK) k_collate_scan_add(int64_t B, int64_t* __restrict__ out_ptr,
                                                               int64_t* __restrict__ out_eptr) {
  const int64_t tile0 = (int64_t)blockIdx.x * CL_TILE;
  const int64_t on = out_ptr[tile0], oe = out_eptr[tile0];
  for (int k = 0; k < CL_ITEMS; ++k) {
    const int64_t i = tile0 + (int64_t)k * CL_BLOCK + threadIdx.x;
    if (i < B && i != tile0) {
      out_ptr[i] += on;
      out_eptr[i] += oe;
    }
  }
}

extern "C" int32_t gnx_collate_ptr(gnx_handle* h, const int64_t* node_ptr, const int64_t* edge_ptr, int64_t G,
                                   const int64_t* idx, int64_t B, int64_t* out_ptr, int64_t* out_eptr) {
  GNX_CHECK_ARG(h != nullptr, "gnx_collate_ptr: handle is NULL");
  GNX_CHECK_ARG(G >= 1 && B >= 1 && B < (1ll << 31), "gnx_collate_ptr: G=%lld B=%lld (need G >= 1, 1 <= B < 2^31)",
                (long long)G, (long long)B);
  GNX_CHECK_ARG(node_ptr && edge_ptr && idx && out_ptr && out_eptr, "gnx_collate_ptr: NULL array");
  const int64_t tiles = gnx_cdiv(B, CL_TILE);
  hipLaunchKernelGGL(k_collate_scan_tile, dim3((unsigned)tiles), dim3(CL_BLOCK), 0, h->stream, node_ptr, edge_ptr, G, idx,
                     B, out_ptr, out_eptr, h->d_flag);
  GNX_LAUNCH_CHECK();
  if (tiles > 1) {
    hipLaunchKernelGGL(k_collate_scan_offsets, dim3(1), dim3(CL_BLOCK), 0, h->stream, B, tiles, out_ptr, out_eptr);
    GNX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_collate_scan_add, dim3((unsigned)tiles), dim3(CL_BLOCK), 0, h->stream, B, out_ptr, out_eptr);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The gather: one wave per batch slot, the lanes striding over each of the slot's contiguous blocks (so a 98-atom star
// costs 14 rounds of one 512-byte wave access, not 882 steps of one lane).  An x block starts at node_ptr * 72 bytes:
// only 8-byte alignment is guaranteed on either side, hence int64 accesses.  Four loads are issued before their stores.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cl_copy(int64_t* __restrict__ dst, const int64_t* __restrict__ src, int64_t n, int lane,
                                        int64_t add) {
  for (int64_t i = lane; i < n; i += 4 * 64) {
    int64_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + 64 * k < n) v[k] = src[i + 64 * k];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + 64 * k < n) dst[i + 64 * k] = v[k] + add;
  }
}

struct collate_args {
  const int64_t *node_ptr, *edge_ptr, *x, *edge_index, *edge_attr, *idx, *out_ptr, *out_eptr;
  int64_t *x_out, *ei_out, *ea_out, *batch_out;
  int64_t G, E_src, B, N, E;
  int* flag;
};

__global__ void __launch_bounds__(CL_BLOCK) k_collate_gather(collate_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (CL_BLOCK / 64) + (threadIdx.x >> 6);
  if (b >= a.B) return;
  int64_t g = a.idx[b];
  if (g < 0 || g >= a.G) g = g < 0 ? 0 : a.G - 1;  // flagged by gnx_collate_ptr's pass over idx
  const int64_t n0 = a.node_ptr[g], e0 = a.edge_ptr[g];
  int64_t n = a.node_ptr[g + 1] - n0, e = a.edge_ptr[g + 1] - e0;
  const int64_t o = a.out_ptr[b], oe = a.out_eptr[b];
  // the caller sized the outputs from its own copy of the graph sizes: a block that does not fit them is cut, never written
  // past the end
  if (o < 0 || oe < 0 || n < 0 || e < 0 || o + n > a.N || oe + e > a.E) {
    if (lane == 0) atomicOr(a.flag, CL_FLAG_IDX);
    n = (o < 0 || n < 0) ? 0 : (o + n > a.N ? (a.N > o ? a.N - o : 0) : n);
    e = (oe < 0 || e < 0) ? 0 : (oe + e > a.E ? (a.E > oe ? a.E - oe : 0) : e);
  }
  cl_copy(a.x_out + o * 9, a.x + n0 * 9, n * 9, lane, 0);
  for (int64_t i = lane; i < n; i += 64) a.batch_out[o + i] = b;
  cl_copy(a.ei_out + oe, a.edge_index + e0, e, lane, o);
  cl_copy(a.ei_out + a.E + oe, a.edge_index + a.E_src + e0, e, lane, o);
  cl_copy(a.ea_out + oe * 3, a.edge_attr + e0 * 3, e * 3, lane, 0);
}

extern "C" int32_t gnx_collate_gather(gnx_handle* h, const int64_t* node_ptr, const int64_t* edge_ptr, int64_t G,
                                      const int64_t* x, const int64_t* edge_index, const int64_t* edge_attr,
                                      int64_t E_src, const int64_t* idx, int64_t B, const int64_t* out_ptr,
                                      const int64_t* out_eptr, int64_t N, int64_t E, int64_t* x_out,
                                      int64_t* edge_index_out, int64_t* edge_attr_out, int64_t* batch_out) {
  GNX_CHECK_ARG(h != nullptr, "gnx_collate_gather: handle is NULL");
  GNX_CHECK_ARG(G >= 1 && B >= 1 && B < (1ll << 31) && N >= 0 && E >= 0 && E_src >= 0,
                "gnx_collate_gather: G=%lld B=%lld N=%lld E=%lld E_src=%lld", (long long)G, (long long)B, (long long)N,
                (long long)E, (long long)E_src);
  GNX_CHECK_ARG(node_ptr && edge_ptr && idx && out_ptr && out_eptr, "gnx_collate_gather: NULL index array");
  GNX_CHECK_ARG(N == 0 || (x && x_out && batch_out), "gnx_collate_gather: NULL node array with N>0");
  GNX_CHECK_ARG(E == 0 || (edge_index && edge_attr && edge_index_out && edge_attr_out),
                "gnx_collate_gather: NULL edge array with E>0");
  collate_args a;
  a.node_ptr = node_ptr, a.edge_ptr = edge_ptr, a.x = x, a.edge_index = edge_index, a.edge_attr = edge_attr;
  a.idx = idx, a.out_ptr = out_ptr, a.out_eptr = out_eptr;
  a.x_out = x_out, a.ei_out = edge_index_out, a.ea_out = edge_attr_out, a.batch_out = batch_out;
  a.G = G, a.E_src = E_src, a.B = B, a.N = N, a.E = E;
  a.flag = h->d_flag;
  hipLaunchKernelGGL(k_collate_gather, dim3((unsigned)gnx_cdiv(B, CL_BLOCK / 64)), dim3(CL_BLOCK), 0, h->stream, a);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// dst[b, :] = src[idx[b], :] for one-row-per-graph label fields of 4- or 8-byte elements (moved as raw words)
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void k_collate_rows(const T* __restrict__ src, int64_t G, const int64_t* __restrict__ idx, int64_t B, int K,
                               T* __restrict__ dst, int* __restrict__ flag) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * K) return;
  const int64_t b = t / K;
  const int k = (int)(t - b * K);
  dst[t] = src[cl_graph(idx, b, G, flag) * K + k];
}

extern "C" int32_t gnx_collate_rows(gnx_handle* h, const void* src, int64_t G, const int64_t* idx, int64_t B,
                                    int32_t elem_bytes, int32_t K, void* dst) {
  GNX_CHECK_ARG(h != nullptr, "gnx_collate_rows: handle is NULL");
  GNX_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "gnx_collate_rows: elem_bytes=%d (4 or 8)", elem_bytes);
  GNX_CHECK_ARG(G >= 1 && B >= 1 && K >= 0 && B * (int64_t)K < (1ll << 38), "gnx_collate_rows: G=%lld B=%lld K=%d",
                (long long)G, (long long)B, K);
  GNX_CHECK_ARG(idx && (K == 0 || (src && dst)), "gnx_collate_rows: NULL array");
  if (K == 0) return GNX_OK;
  const dim3 grid((unsigned)gnx_cdiv(B * K, 256));
  if (elem_bytes == 4)
    hipLaunchKernelGGL(k_collate_rows<uint32_t>, grid, dim3(256), 0, h->stream, (const uint32_t*)src, G, idx, B, (int)K,
                       (uint32_t*)dst, h->d_flag);
  else
    hipLaunchKernelGGL(k_collate_rows<uint64_t>, grid, dim3(256), 0, h->stream, (const uint64_t*)src, G, idx, B, (int)K,
                       (uint64_t*)dst, h->d_flag);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}
