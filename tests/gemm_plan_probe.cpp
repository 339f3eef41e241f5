// Stand-alone probe of gnnepcsaft_amd/csrc/gnx_gemm_plan.hpp for tests/test_gemm_plan_cpu.py: host C++ only, no device.
// Reads one query per line from stdin, "key=value" tokens in any order, and prints one answer line per query.
//   op=plan (default): a gemm call.  Keys (defaults): nseg (1), k (128: every segment), k0..k3, M (8192), N (128), bt (1),
//     relu, acc, mask, bias, split_only, presplit, grouped (all 0), max_tiles (0), classes (1), cls_stride (0), tile_rows (0),
//     ws (1: the call brings a workspace), rowscale (0), lda / ldb / ldc / ldmask (0 = the tight value), cus (256), and byte
//     offsets from 16-byte alignment a_off, b_off, c_off, mask_off, bias_off (0); options SPLIT (1), PIPE (1), AS (1),
//     WS_FAST (2), TILE_ROWS (0), MID (1): the defaults of gnx_create.  a_off, b_off, rowscale, lda, ldb apply to segment 0.
//     Answer: kernel grid_x grid_y block tile_rows image_bytes lds run_split stop_after_split frag Kpad
//   op=tile_rows  M N forced cus            -> gemm_plan_tile_rows
//   op=image_bytes classes N kpad           -> gemm_plan_image_bytes
//   op=kpad k                               -> plan_kpad
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

#include "gnx_gemm_plan.hpp"

int main() {
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::map<std::string, long long> kv;
    std::string op = "plan";
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "bad token %s\n", tok.c_str());
        return 2;
      }
      if (tok.substr(0, eq) == "op")
        op = tok.substr(eq + 1);
      else
        kv[tok.substr(0, eq)] = atoll(tok.c_str() + eq + 1);
    }
    if (kv.empty() && op == "plan") continue;
    auto get = [&](const char* key, long long def) {
      const auto it = kv.find(key);
      if (it == kv.end()) return def;
      const long long v = it->second;
      kv.erase(it);
      return v;
    };
    if (op == "tile_rows") {
      const long long M = get("M", 0), N = get("N", 128), forced = get("forced", 0), cus = get("cus", 256);
      printf("%d\n", gemm_plan_tile_rows(M, (int32_t)N, (int)forced, (int)cus));
    } else if (op == "image_bytes") {
      const long long c = get("classes", 1), N = get("N", 128), kpad = get("kpad", 128);
      printf("%zu\n", gemm_plan_image_bytes(c, N, kpad));
    } else if (op == "kpad") {
      printf("%d\n", plan_kpad(get("k", 0)));
    } else {
      // fake device addresses: 16-byte aligned bases, never dereferenced
      const uintptr_t A = 0x10000000, B = 0x20000000, Cb = 0x30000000, MASK = 0x40000000, BIAS = 0x50000000, WS = 0x60000000,
                      RS = 0x70000000, TILES = 0x80000000;
      const int nseg = (int)get("nseg", 1);
      const long long M = get("M", 8192), N = get("N", 128), kall = get("k", 128);
      const bool bt = get("bt", 1) != 0;
      gnx_gemm_seg segs[PLAN_MAX_SEGS];
      int64_t strides[PLAN_MAX_SEGS];
      const long long cls_stride = get("cls_stride", 0);
      for (int s = 0; s < PLAN_MAX_SEGS; ++s) {
        const std::string ks = "k" + std::to_string(s);
        const long long k = get(ks.c_str(), kall);
        segs[s] = gnx_gemm_seg{reinterpret_cast<const float*>(A + 0x1000000 * s), k, nullptr,
                               reinterpret_cast<const float*>(B + 0x1000000 * s), bt ? k : N, (int32_t)k, 0};
        strides[s] = cls_stride;
      }
      segs[0].a = reinterpret_cast<const float*>(A + get("a_off", 0));
      segs[0].b = reinterpret_cast<const float*>(B + get("b_off", 0));
      if (get("rowscale", 0)) segs[0].rowscale = reinterpret_cast<const float*>(RS);
      if (const long long v = get("lda", 0)) segs[0].lda = v;
      if (const long long v = get("ldb", 0)) segs[0].ldb = v;
      const bool grouped = get("grouped", 0) != 0;
      const long long ldc = get("ldc", 0), ldmask = get("ldmask", 0);
      const float* mask = get("mask", 0) ? reinterpret_cast<const float*>(MASK + get("mask_off", 0)) : nullptr;
      const float* bias = get("bias", 0) ? reinterpret_cast<const float*>(BIAS + get("bias_off", 0)) : nullptr;
      const int32_t flags = (get("relu", 0) ? GNX_GEMM_RELU : 0) | (get("acc", 0) ? GNX_GEMM_ACCUMULATE : 0) |
                            (bt ? GNX_GEMM_B_TRANS : 0) | (get("split_only", 0) ? GNX_GEMM_SPLIT_ONLY : 0) |
                            (get("presplit", 0) ? GNX_GEMM_PRESPLIT : 0);
      int opt[GNX_OPT_COUNT] = {};
      opt[GNX_OPT_EMBED_BWD_MFMA] = opt[GNX_OPT_STD_BWD_CENTERED] = opt[GNX_OPT_WGRAD_PIPE] = 1;
      opt[GNX_OPT_GEMM_SPLIT] = (int)get("SPLIT", 1);
      opt[GNX_OPT_GEMM_PIPE] = (int)get("PIPE", 1);
      opt[GNX_OPT_GEMM_AS] = (int)get("AS", 1);
      opt[GNX_OPT_GEMM_WS_FAST] = (int)get("WS_FAST", 2);
      opt[GNX_OPT_GEMM_TILE_ROWS] = (int)get("TILE_ROWS", 0);
      opt[GNX_OPT_GEMM_MID] = (int)get("MID", 1);
      const gemm_plan p = gemm_plan_of(
          nseg, segs, grouped ? strides : nullptr, (int32_t)get("classes", 1), M, (int32_t)N, bias, mask, ldmask ? ldmask : N,
          reinterpret_cast<const float*>(Cb + get("c_off", 0)), ldc ? ldc : N, flags,
          grouped ? reinterpret_cast<const int32_t*>(TILES) : nullptr, get("max_tiles", 0),
          get("ws", 1) ? reinterpret_cast<const void*>(WS) : nullptr, (int32_t)get("tile_rows", 0), opt, (int)get("cus", 256));
      printf("%d %u %u %u %d %zu %zu %d %d %d %d\n", p.kernel, p.grid_x, p.grid_y, p.block, p.tile_rows, p.image_bytes, p.lds,
             (int)p.run_split, (int)p.stop_after_split, p.frag, p.Kpad);
    }
    if (!kv.empty()) {
      fprintf(stderr, "unknown key %s\n", kv.begin()->first.c_str());
      return 2;
    }
  }
  return 0;
}
