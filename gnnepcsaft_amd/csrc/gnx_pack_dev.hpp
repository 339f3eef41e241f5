// Device code of the packer that more than one translation unit launches.
#pragma once
#include <cstdint>

// Entry j of the edge-tile table (gnx_edge_tiles; layout in gnx_fused.hip): (first node, first CSR position) of tile j,
// j <= ntiles; entry ntiles is the end marker (N, E).
__device__ __forceinline__ void gnx_edge_tile_entry(const int* __restrict__ rowptr, int64_t N, int64_t E, int W, int ntiles,
                                                    int j, int* __restrict__ info) {
  if (j == ntiles) {
    info[2 * j] = (int)N;
    info[2 * j + 1] = (int)E;
    return;
  }
  const int64_t target = (int64_t)W * j;  // <= E by the choice of ntiles
  int lo = 0, hi = (int)N;                // first n in [0, N] with rowptr[n] >= target (rowptr[N] = E)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] >= target) hi = mid;
    else lo = mid + 1;
  }
  info[2 * j] = lo;
  info[2 * j + 1] = rowptr[lo];
}
