// Stand-alone probe of the split-image part of gnnepcsaft_amd/csrc/gnx_gemm_plan.hpp for tests/test_split_all_cpu.py: host
// C++ only, no device.  Reads one query per line from stdin, "key=value" tokens in any order, and prints one answer line.
//   Keys (defaults): L (1), T (1), F (128), pre (2), post (2), D (5), N (4096: rows), tile_rows (128), SPLIT (1), PIPE (1), AS (1),
//     cus (256), w_off (0: byte offset of every post-layer-0 weight from 16-byte alignment).
//   Answer: total problems, then per (layer, tower) "| post0_off post0_bytes dA_off dA_bytes dx_off dx_bytes" (offset -1: no image),
//     then "| rec" and the post0 / dA / dx records of layer 0, tower 0, each as
//     image_bytes classes Npad Kpad koff0..koff4 frag bt.
//   op=equal: two shapes a_KEY / b_KEY (same keys, prefixed); answer: three 0/1 flags, whether the post0 / dA / dx records of
//     layer 0, tower 0 are equal (gemm_image_equal).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "gnx_gemm_plan.hpp"

namespace {
struct shape {
  int L, T, F, pre, post, D, tile_rows, cus;
  long long N, w_off;
  int opt[GNX_OPT_COUNT];
};

shape read_shape(std::map<std::string, long long>& kv, const std::string& prefix) {
  auto get = [&](const char* key, long long def) {
    const auto it = kv.find(prefix + key);
    if (it == kv.end()) return def;
    const long long v = it->second;
    kv.erase(it);
    return v;
  };
  shape s = {};
  s.L = (int)get("L", 1);
  s.T = (int)get("T", 1);
  s.F = (int)get("F", 128);
  s.pre = (int)get("pre", 2);
  s.post = (int)get("post", 2);
  s.D = (int)get("D", 5);
  s.N = get("N", 4096);
  s.tile_rows = (int)get("tile_rows", 128);
  s.cus = (int)get("cus", 256);
  s.w_off = get("w_off", 0);
  s.opt[GNX_OPT_EMBED_BWD_MFMA] = s.opt[GNX_OPT_STD_BWD_CENTERED] = s.opt[GNX_OPT_WGRAD_PIPE] = 1;
  s.opt[GNX_OPT_GEMM_SPLIT] = (int)get("SPLIT", 1);
  s.opt[GNX_OPT_GEMM_PIPE] = (int)get("PIPE", 1);
  s.opt[GNX_OPT_GEMM_AS] = (int)get("AS", 1);
  s.opt[GNX_OPT_GEMM_WS_FAST] = 2;
  s.opt[GNX_OPT_GEMM_MID] = 1;
  return s;
}

// fake device addresses, never dereferenced: every parameter 1 MB apart
size_t layout(const shape& s, std::vector<gnx_pna_layer_images>& out, int& nprobs) {
  const int per = 2 * (s.pre + s.post), np = 4 + s.T * per;
  std::vector<const float*> params((size_t)s.L * np), weff((size_t)s.L * s.T);
  uintptr_t next = 0x10000000;
  for (auto& p : params) p = reinterpret_cast<const float*>(next += 0x100000);
  for (auto& p : weff) p = reinterpret_cast<const float*>(next += 0x100000);
  for (int l = 0; l < s.L; ++l)
    for (int t = 0; t < s.T; ++t) {
      const float*& w = params[(size_t)l * np + 4 + t * per + 2 * s.pre];
      w = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(w) + (uintptr_t)s.w_off);
    }
  out.assign(s.L, gnx_pna_layer_images{});
  std::vector<gemm_split_problem> probs((size_t)3 * s.L * s.T);
  return pna_images_layout(s.L, s.T, s.F, s.pre, s.post, s.D, s.N, s.tile_rows, params.data(), weff.data(), s.opt, s.cus, nullptr,
                           out.data(), probs.data(), &nprobs);
}

void print_rec(const gnx_gemm_image& r) {
  printf(" %llu %d %d %d %d %d %d %d %d %d %d", (unsigned long long)r.image_bytes, r.classes, r.Npad, r.Kpad, r.koff[0], r.koff[1],
         r.koff[2], r.koff[3], r.koff[4], r.frag, r.bt);
}
}  // namespace

int main() {
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::map<std::string, long long> kv;
    std::string op = "layout";
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
    std::vector<gnx_pna_layer_images> a, b;
    int na = 0, nb = 0;
    if (op == "equal") {
      const shape sa = read_shape(kv, "a_"), sb = read_shape(kv, "b_");
      layout(sa, a, na);
      layout(sb, b, nb);
      printf("%d %d %d\n", (int)gemm_image_equal(a[0].post0_rec[0], b[0].post0_rec[0]),
             (int)gemm_image_equal(a[0].dA_rec[0], b[0].dA_rec[0]), (int)gemm_image_equal(a[0].dx_rec[0], b[0].dx_rec[0]));
    } else {
      const shape s = read_shape(kv, "");
      const size_t total = layout(s, a, na);
      printf("%zu %d", total, na);
      // (the layout ran without a slab: an image's pointer IS its offset; a record without bytes means no image)
      auto off = [](const void* p, const gnx_gemm_image& r) { return r.image_bytes ? (long long)reinterpret_cast<uintptr_t>(p) : -1LL; };
      for (int l = 0; l < s.L; ++l)
        for (int t = 0; t < s.T; ++t) {
          const gnx_pna_layer_images& li = a[l];
          printf(" | %lld %llu %lld %llu %lld %llu", off(li.post0[t], li.post0_rec[t]), (unsigned long long)li.post0_rec[t].image_bytes,
                 off(li.dA[t], li.dA_rec[t]), (unsigned long long)li.dA_rec[t].image_bytes, off(li.dx[t], li.dx_rec[t]),
                 (unsigned long long)li.dx_rec[t].image_bytes);
        }
      printf(" | rec");
      print_rec(a[0].post0_rec[0]);
      print_rec(a[0].dA_rec[0]);
      print_rec(a[0].dx_rec[0]);
      printf("\n");
    }
    if (!kv.empty()) {
      fprintf(stderr, "unknown key %s\n", kv.begin()->first.c_str());
      return 2;
    }
  }
  return 0;
}
