// Stand-alone probe of gnnepcsaft_amd/csrc/gnx_wgrad_plan.hpp for tests/test_wgrad_grouped_plan_cpu.py: host C++ only, no
// device.  One query per line of stdin:  M N K budget max_chunks off_dC off_A lddc lda SPLIT PIPE  (off_*: bytes from
// 16-byte alignment; lddc / lda 0 = N / K; budget = GNX_OPT_WGRAD_WGS), one answer per line:  kernel ranges S grid_x
#include <cstdio>

#include "gnx_wgrad_plan.hpp"

int main() {
  long long M, N, K, budget, max_chunks, off_x, off_a, lddc, lda, split, pipe;
  while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &M, &N, &K, &budget, &max_chunks, &off_x, &off_a, &lddc,
               &lda, &split, &pipe) == 11) {
    int opt[GNX_OPT_COUNT] = {};
    opt[GNX_OPT_GEMM_SPLIT] = (int)split;
    opt[GNX_OPT_WGRAD_PIPE] = (int)pipe;
    opt[GNX_OPT_WGRAD_WGS] = (int)budget;
    // fake device addresses, never dereferenced
    const wgrad_grouped_plan p = wgrad_grouped_plan_of(reinterpret_cast<const float*>(0x10000000 + off_x), lddc ? lddc : N,
                                                       reinterpret_cast<const float*>(0x20000000 + off_a), lda ? lda : K, M,
                                                       (int32_t)N, (int32_t)K, max_chunks, opt);
    printf("%d %d %d %u\n", p.kernel, p.ranges, p.chunks_per_range, p.grid_x);
  }
  return 0;
}
