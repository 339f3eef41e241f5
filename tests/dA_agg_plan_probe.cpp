// Stand-alone probe of pna_dA_agg_plan_of (gnnepcsaft_amd/csrc/gnx_gemm_plan.hpp) for tests/test_dA_agg_plan_cpu.py: host
// C++ only, no device.  One query per line of stdin:
//   N E T F D max_tiles off_g off_dA off_m off_ge off_w have_ws FUSED SPLIT AS grouped
// (off_*: bytes from 16-byte alignment; have_ws 0: no workspace, so no images; FUSED / SPLIT / AS: GNX_OPT_DA_AGG_FUSED /
// _GEMM_SPLIT / _GEMM_AS; grouped 0: the product as an ungrouped call), one answer per line:
//   fused product_kernel grid_x lds
#include <cstdio>

#include "gnx_gemm_plan.hpp"

int main() {
  long long N, E, T, F, D, max_tiles, off_g, off_dA, off_m, off_ge, off_w, have_ws, fused, split, as, grouped;
  while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &N, &E, &T, &F, &D, &max_tiles,
               &off_g, &off_dA, &off_m, &off_ge, &off_w, &have_ws, &fused, &split, &as, &grouped) == 16) {
    int opt[GNX_OPT_COUNT] = {};
    opt[GNX_OPT_GEMM_SPLIT] = (int)split;
    opt[GNX_OPT_GEMM_AS] = (int)as;
    opt[GNX_OPT_GEMM_PIPE] = 1;
    opt[GNX_OPT_GEMM_MID] = 1;
    opt[GNX_OPT_DA_AGG_FUSED] = (int)fused;
    // fake device addresses, never dereferenced
    const float* g = reinterpret_cast<const float*>(0x10000000 + off_g);
    float* dA = reinterpret_cast<float*>(0x20000000 + off_dA);
    const float* m = reinterpret_cast<const float*>(0x30000000 + off_m);
    const float* ge = reinterpret_cast<const float*>(0x40000000 + off_ge);
    const float* w = reinterpret_cast<const float*>(0x50000000 + off_w);
    pna_product q = pna_dA_product(w, (int)T, (int)F, (int)D, 0, g, dA);
    q.grouped = grouped != 0;
    const pna_dA_agg_plan p = pna_dA_agg_plan_of(q, N, E, T * F, m, ge, 0, have_ws ? reinterpret_cast<const void*>(0x60000000) : nullptr,
                                                 max_tiles, opt, 256);
    printf("%d %d %u %zu\n", p.fused ? 1 : 0, p.product.kernel, p.grid_x, p.lds);
  }
  return 0;
}
