// AtomEncoder / BondEncoder [3P ogb]: sum of K embedding rows, and the embedding_dense_backward scatter-add into
// tiny tables (174 / 13 / 60 rows) done in LDS-privatised form instead of 10^5 contending global atomics, or for large
// batches as a one-hot x gradient product on the matrix cores.
#include "gnx_split.hpp"

struct offs_t {
  int o[18];
};

template <int VEC>
__global__ void __launch_bounds__(256) k_embed_fwd(const int64_t* __restrict__ idx, int64_t N, int K, offs_t offs,
                                                   const float* __restrict__ table, int H, float* __restrict__ out,
                                                   int* __restrict__ flag) {
  const int G = H / VEC;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * G) return;
  int64_t n = t / G;
  int c = (int)(t % G) * VEC;
  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
  // four features at a time: their indices, then their table rows, are loaded together (one dependent index -> row pair
  // per feature was 18 serial round trips for the 9 atom features); summed in feature order as before
  for (int k0 = 0; k0 < K; k0 += 4) {
    int64_t f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = idx[n * K + (k0 + j < K ? k0 + j : K - 1)];
    const float* row[4];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + j < K ? k0 + j : K - 1;
      const int rows = offs.o[k + 1] - offs.o[k];
      if (f[j] < 0 || f[j] >= rows) {
        bad = bad || (k0 + j < K);
        f[j] = 0;
      }
      row[j] = table + (int64_t)(offs.o[k] + (int)f[j]) * H + c;
    }
    if (bad && c == 0) atomicOr(flag, 16);
    if constexpr (VEC == 4) {
      f32x4 r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = *reinterpret_cast<const f32x4*>(row[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k0 + j < K) {
          acc[0] += r[j].x;
          acc[1] += r[j].y;
          acc[2] += r[j].z;
          acc[3] += r[j].w;
        }
    } else {
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = row[j][0];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k0 + j < K) acc[0] += r[j];
    }
  }
  float* o = out + n * H + c;
  if constexpr (VEC == 4) {
    f32x4 r = {acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(o) = r;
  } else {
    o[0] = acc[0];
  }
}

extern "C" int32_t gnx_embed_sum_fwd(gnx_handle* h, const int64_t* idx, int64_t N, int32_t K, const int32_t* offsets,
                                     const float* table, int32_t H, float* out) {
  GNX_CHECK_ARG(h && offsets && table && K > 0 && K <= 16 && H > 0 && N >= 0, "gnx_embed_sum_fwd: bad argument");
  GNX_CHECK_ARG(N == 0 || (idx && out), "gnx_embed_sum_fwd: NULL array with N>0");
  if (N == 0) return GNX_OK;
  gnx_prof_scope prof(h, GNX_K_EMBED, 8.0 * N * K + 4.0 * N * H);
  offs_t o;
  for (int k = 0; k <= 17; ++k) o.o[k] = offsets[k <= K ? k : K];
  if (H % 4 == 0) {
    int64_t threads = N * (H / 4);
    hipLaunchKernelGGL(k_embed_fwd<4>, dim3((unsigned)gnx_cdiv(threads, 256)), dim3(256), 0, h->stream, idx, N, (int)K,
                       o, table, (int)H, out, h->d_flag);
  } else {
    int64_t threads = N * H;
    hipLaunchKernelGGL(k_embed_fwd<1>, dim3((unsigned)gnx_cdiv(threads, 256)), dim3(256), 0, h->stream, idx, N, (int)K,
                       o, table, (int)H, out, h->d_flag);
  }
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// dtable[R, H] += sum over rows n, features k of dout[n, :] at row offs[k]+idx[n,k].
// grid = (row chunks, column slabs of CW).  Block: 256 threads = (256/CW) row lanes x CW columns.
// LDS table R x CW accumulated with ds_add_f32, flushed with one global atomic per touched element.
// ---------------------------------------------------------------------------------------------------------------
template <typename IdxT, int VEC>
__global__ void __launch_bounds__(256) k_table_scatter_add(const IdxT* __restrict__ idx, int64_t N, int K, offs_t offs,
                                                           int R, const float* __restrict__ dout, int H, int CW,
                                                           int64_t rows_per_block, float* __restrict__ dtable,
                                                           float* __restrict__ part) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  for (int i = tid; i < R * CW; i += 256) lds[i] = 0.f;
  __syncthreads();
  const int G = CW / VEC;        // threads per row
  const int cg = tid % G;
  const int rl = tid / G;
  const int RL = 256 / G;        // rows in flight per pass
  const int c = cg * VEC;        // column inside the slab
  const int col = blockIdx.y * CW + c;
  int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > N) r1 = N;
  if (col < H && r0 < r1) {
    // four rows in flight per thread; every load is unconditional (clamped row) and issued before any use, so one
    // round trip serves 4 rows x (1 gradient quad + 1 index) instead of a dependent chain per row
    constexpr int UN = (VEC == 1) ? 8 : 4;
    for (int64_t n = r0 + rl; n < r1; n += UN * RL) {
      int64_t nn[UN];
      bool ok[UN];
      float g[UN][VEC];
#pragma unroll
      for (int j = 0; j < UN; ++j) {
        const int64_t row = n + (int64_t)j * RL;
        ok[j] = row < r1;
        nn[j] = ok[j] ? row : r0;
      }
#pragma unroll
      for (int j = 0; j < UN; ++j) {
        if constexpr (VEC == 4) {
          f32x4 v = *reinterpret_cast<const f32x4*>(dout + nn[j] * H + col);
          g[j][0] = v.x;
          g[j][1] = v.y;
          g[j][2] = v.z;
          g[j][3] = v.w;
        } else {
          g[j][0] = dout[nn[j] * H + col];
        }
      }
      for (int k = 0; k < K; ++k) {
        const int rows = offs.o[k + 1] - offs.o[k];
        int64_t f[UN];
#pragma unroll
        for (int j = 0; j < UN; ++j) f[j] = (int64_t)idx[nn[j] * K + k];
#pragma unroll
        for (int j = 0; j < UN; ++j) {
          if (ok[j] && f[j] >= 0 && f[j] < rows) {  // out-of-range indices were flagged in forward
            float* d = &lds[(offs.o[k] + (int)f[j]) * CW + c];
#pragma unroll
            for (int v = 0; v < VEC; ++v) atomicAdd(d + v, g[j][v]);
          }
        }
      }
    }
  }
  __syncthreads();
  if (part != nullptr) {
    // two-stage reduction: every block stores its private table; k_table_reduce folds them.  (Hundreds of blocks
    // atomically adding into the same few KB serialise at the memory-side atomic units: 100+ us for a 60-row table.)
    float* dst = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (int64_t)R * CW;
    for (int i = tid; i < R * CW; i += 256) dst[i] = lds[i];
    return;
  }
  for (int i = tid; i < R * CW; i += 256) {
    int r = i / CW, cc = blockIdx.y * CW + (i % CW);
    float v = lds[i];
    if (cc < H && v != 0.f) atomicAdd(&dtable[(int64_t)r * H + cc], v);
  }
}

// dtable[r, col] += sum over chunks of part[chunk][slab][r][c]; grid = (elements / 256, chunk groups); each thread folds
// its chunk group in order and issues one atomic (<= 16 per address in total).
__global__ void __launch_bounds__(256) k_table_reduce(const float* __restrict__ part, int nchunks, int slabs, int R,
                                                      int CW, int H, int chunks_per_group, float* __restrict__ dtable) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // element of the [R, slabs*CW] padded table
  const int W = slabs * CW;
  if (e >= (int64_t)R * W) return;
  const int r = (int)(e / W), col = (int)(e % W);
  if (col >= H) return;
  const int slab = col / CW, c = col % CW;
  int c0 = blockIdx.y * chunks_per_group, c1 = c0 + chunks_per_group;
  if (c1 > nchunks) c1 = nchunks;
  float acc = 0.f;
  for (int ch = c0; ch < c1; ++ch) acc += part[(((int64_t)ch * slabs + slab) * R + r) * CW + c];
  if (acc != 0.f) atomicAdd(&dtable[(int64_t)r * H + col], acc);
}

static void table_scatter_geometry(int64_t N, int R, int H, int* CW, int* slabs, int64_t* rows_per_block,
                                   int64_t* chunks) {
  int cw = 64;
  while ((size_t)R * cw * sizeof(float) > 64 * 1024 && cw > 8) cw >>= 1;
  *CW = cw;
  *slabs = (int)gnx_cdiv(H, cw);
  // ~768 blocks (3 per CU) in total; at least 256 rows each so the per-block table traffic stays a small fraction
  int64_t rpb = gnx_cdiv(N, gnx_cdiv(768, *slabs));
  if (rpb < 256) rpb = 256;
  *rows_per_block = rpb;
  *chunks = gnx_cdiv(N, rpb);
}

size_t gnx_table_scatter_ws_bytes(int64_t N, int R, int H) {
  if (N <= 0) return 0;
  int CW, slabs;
  int64_t rpb, chunks;
  table_scatter_geometry(N, R, H, &CW, &slabs, &rpb, &chunks);
  return sizeof(float) * (size_t)chunks * slabs * R * CW;
}

template <typename IdxT>
static int32_t launch_table_scatter_add(gnx_handle* h, const IdxT* idx, int64_t N, int K, const int32_t* offsets, int R,
                                        const float* dout, int H, float* dtable, void* ws, size_t ws_bytes) {
  offs_t o;
  for (int k = 0; k <= 17; ++k) o.o[k] = offsets[k <= K ? k : K];
  int CW, slabs;
  int64_t rows_per_block, chunks;
  table_scatter_geometry(N, R, H, &CW, &slabs, &rows_per_block, &chunks);
  GNX_CHECK_ARG((size_t)R * CW * sizeof(float) <= 64 * 1024, "table scatter-add: %d rows do not fit the LDS tile", R);
  float* part = nullptr;
  if (ws != nullptr && chunks > 8) {
    if (ws_bytes < gnx_table_scatter_ws_bytes(N, R, H)) {
      gnx_set_error("table scatter-add: workspace %zu < %zu", ws_bytes, gnx_table_scatter_ws_bytes(N, R, H));
      return GNX_E_WORKSPACE;
    }
    part = reinterpret_cast<float*>(ws);
  }
  // One column per lane: a wave's ds_add_f32 then touches 64 consecutive floats (2 lanes per bank, the minimum).  The
  // float4-per-thread layout put every lane of an instruction on 8 banks (8-way conflict on the LDS atomic unit:
  // 106 us for a 163840 x 128 gradient instead of ~25 us), so it is not used even when H % 4 == 0.
  if (false)
    hipLaunchKernelGGL((k_table_scatter_add<IdxT, 4>), dim3((unsigned)chunks, (unsigned)slabs), dim3(256),
                       (size_t)R * CW * sizeof(float), h->stream, idx, N, K, o, R, dout, H, CW, rows_per_block, dtable,
                       part);
  else
    hipLaunchKernelGGL((k_table_scatter_add<IdxT, 1>), dim3((unsigned)chunks, (unsigned)slabs), dim3(256),
                       (size_t)R * CW * sizeof(float), h->stream, idx, N, K, o, R, dout, H, CW, rows_per_block, dtable,
                       part);
  GNX_LAUNCH_CHECK();
  if (part != nullptr) {
    const int groups = (int)(chunks < 16 ? chunks : 16);
    const int cpg = (int)gnx_cdiv(chunks, groups);
    hipLaunchKernelGGL(k_table_reduce, dim3((unsigned)gnx_cdiv((int64_t)R * slabs * CW, 256), (unsigned)groups),
                       dim3(256), 0, h->stream, part, (int)chunks, slabs, R, CW, H, cpg, dtable);
    GNX_LAUNCH_CHECK();
  }
  return GNX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Embedding backward on the matrix cores: dTable[r, :] += sum_n onehot[n, r] * dOut[n, :], where onehot[n, r] counts the
// features k with offs[k] + idx[n,k] == r ([3P] embedding_dense_backward summed over the K tables of an ogb encoder).
// It is the weight-gradient contraction over rows with a left operand GENERATED from the integer features (exact: the
// products are by 0/1), so the 10^8 LDS atomic lane-ops of the table-scatter kernel (~2 clk each) become ~5 GFLOP of MFMA.
// grid = (row chunks, R tiles of 128, H tiles of 128).
// ---------------------------------------------------------------------------------------------------------------
#define EMB_MAX_K 12
struct embed_bwd_args {
  const int64_t* idx;  // [N, K]
  int offs[EMB_MAX_K + 1];
  int K;
  const float* Y;  // dOut [N, H]
  int64_t ldy;
  int64_t N;
  int R, H;
  float* dT;  // [R, H]
  int64_t rows_per_block;
};

__global__ void __launch_bounds__(256, 2) k_embed_bwd_mfma(embed_bwd_args g) {
  __shared__ __attribute__((aligned(16))) float Xs[BK * LDN];
  __shared__ __attribute__((aligned(16))) float Ys[BK * LDN];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * BN;  // table-row tile
  const int c0 = blockIdx.z * BN;  // channel tile
  const int64_t r_begin = (int64_t)blockIdx.x * g.rows_per_block;
  int64_t r_end = r_begin + g.rows_per_block;
  if (r_end > g.N) r_end = g.N;
  if (r_begin >= r_end) return;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int br = tid >> 5;
  const int bc = (tid & 31) * 4;
  const int yk = c0 + bc;
  const bool y_ok = yk < g.H;
  const int yc = y_ok ? yk : 0;
  f32x4 ry[4];
  int fr[4][EMB_MAX_K];  // table rows hit by the 4 batch rows this thread stages (raw loads, used at LDS-store time)
  int okmask = 0;

  auto load_tile = [&](int64_t r0) {
    okmask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t pos = r0 + br + 8 * i;
      const bool rv = pos < r_end;
      const int64_t row = rv ? pos : r_begin;
      ry[i] = *reinterpret_cast<const f32x4*>(g.Y + row * g.ldy + yc);
#pragma unroll
      for (int k = 0; k < EMB_MAX_K; ++k) fr[i][k] = (int)g.idx[row * g.K + (k < g.K ? k : 0)];  // unconditional
      okmask |= rv ? (1 << i) : 0;
    }
  };

  int64_t r0 = r_begin;
  load_tile(r0);
  while (r0 < r_end) {
    __syncthreads();
    {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool rv = (okmask >> i) & 1;
        f32x4 x = z;
#pragma unroll
        for (int k = 0; k < EMB_MAX_K; ++k) {
          const int span = g.offs[k + 1 <= g.K ? k + 1 : g.K] - g.offs[k < g.K ? k : g.K];
          const int f = fr[i][k];
          const int r = g.offs[k < g.K ? k : 0] + f - (n0 + bc);  // position relative to this thread's 4 table rows
          const bool hit = rv && k < g.K && f >= 0 && f < span;
          x.x += (hit && r == 0) ? 1.f : 0.f;
          x.y += (hit && r == 1) ? 1.f : 0.f;
          x.z += (hit && r == 2) ? 1.f : 0.f;
          x.w += (hit && r == 3) ? 1.f : 0.f;
        }
        const int kr = br + 8 * i;
        *reinterpret_cast<f32x4*>(&Xs[kr * LDN + bc]) = x;
        *reinterpret_cast<f32x4*>(&Ys[kr * LDN + bc]) = (rv && y_ok) ? ry[i] : z;
      }
    }
    __syncthreads();
    r0 += BK;
    if (r0 < r_end) load_tile(r0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      f32x4 a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const float* p = &Xs[(kk * 8 + 4 * lh) * LDN + wm * 64 + mi * 32 + li];
        a[mi].x = p[0];
        a[mi].y = p[LDN];
        a[mi].z = p[2 * LDN];
        a[mi].w = p[3 * LDN];
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const float* p = &Ys[(kk * 8 + 4 * lh) * LDN + wn * 64 + ni * 32 + li];
        b[ni].x = p[0];
        b[ni].y = p[LDN];
        b[ni].z = p[2 * LDN];
        b[ni].w = p[3 * LDN];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][t], b[ni][t], acc[mi][ni], 0, 0, 0);
    }
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int gc = c0 + wn * 64 + ni * 32 + li;
      if (gc >= g.H) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gr = n0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gr >= g.R) continue;
        const float v = acc[mi][ni][r];
        if (v != 0.f) atomicAdd(g.dT + (int64_t)gr * g.H + gc, v);
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same gradient on the bf16 matrix pipe (R <= 192 table rows, e.g. the 174 rows of the nine atom-feature tables):
// the one-hot operand is EXACT in bf16 and is not computed but SCATTERED -- its [table row][batch row] LDS image stays
// zero except for the K ones per batch row, which the thread that set them clears again after the multiply --, the
// gradient goes through the three-piece split like every other product (three bf16 MFMAs per slab instead of eight
// fp32 ones at a sixteenth of the rate: the fp32 kernel above spends 34 of its 107 us in the matrix pipe and most of the
// rest building the one-hot operand with K x 4 compares per element).  A workgroup owns ALL table rows (six 32-row
// blocks) x 128 channels (wave w: channels 32 w ..) of a row chunk; 32 batch rows per step; fp32 atomics at the end.
// ---------------------------------------------------------------------------------------------------------------
#define EB_R 192
#define EB_LDX 80   // bytes per image row: 32 batch rows of bf16 + 16 (odd number of 16-byte slots)
#define EB_X_BYTES (EB_R * EB_LDX)
#define EB_Y_BYTES (128 * EB_LDX)
__global__ void __launch_bounds__(256, 2) k_embed_bwd_bf16(embed_bwd_args g) {
  __shared__ __attribute__((aligned(16))) unsigned char Xs[EB_X_BYTES];       // one-hot  [table row][32 batch rows]
  __shared__ __attribute__((aligned(16))) unsigned char Ys[3 * EB_Y_BYTES];   // gradient [piece][channel][32 batch rows]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int c0 = blockIdx.y * 128;
  const int64_t r_begin = (int64_t)blockIdx.x * g.rows_per_block;
  int64_t r_end = r_begin + g.rows_per_block;
  if (r_end > g.N) r_end = g.N;
  if (r_begin >= r_end) return;

  for (int i = tid; i < EB_X_BYTES / 16; i += 256) reinterpret_cast<f32x4*>(Xs)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();  // (the first step's ones are set by other threads than the ones that zeroed their words)

  f32x16 acc[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // gradient loader: thread = (channel, 16 batch rows): 4-byte loads, 256 contiguous bytes per wave instruction
  const int yc = tid & 127, yh = tid >> 7;
  const bool y_ok = c0 + yc < g.H;
  // one-hot setter: work item = (batch row, feature): K <= 12 -> at most 384 items, two per thread at most
  const int nitems = 32 * g.K;
  int xpos[2] = {-1, -1};

  for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
    float yv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int64_t row = r0 + 16 * yh + j;
      yv[j] = (y_ok && row < r_end) ? g.Y[row * g.ldy + c0 + yc] : 0.f;
    }
    int fi[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int it = tid + 256 * q;
      const int m = it / g.K, k = it - m * g.K;
      const int64_t row = r0 + m;
      fi[q] = -1;
      if (it < nitems && row < r_end) {
        const int f = (int)g.idx[row * g.K + k];
        const int span = g.offs[k + 1] - g.offs[k];
        if (f >= 0 && f < span) fi[q] = (g.offs[k] + f) * EB_LDX + m * 2;  // byte offset of X[table row][m]
      }
    }
    {
      bf16x8 pc[2][3];
      float x8[8];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x8[j] = yv[8 * hf + j];
        split3(x8, pc[hf][0], pc[hf][1], pc[hf][2]);
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        unsigned char* q = Ys + p * EB_Y_BYTES + yc * EB_LDX + 32 * yh;
        *reinterpret_cast<bf16x8*>(q) = pc[0][p];
        *reinterpret_cast<bf16x8*>(q + 16) = pc[1][p];
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      xpos[q] = fi[q];
      if (fi[q] >= 0) *reinterpret_cast<unsigned short*>(Xs + fi[q]) = 0x3F80;  // bf16 1.0
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      bf16x8 b[3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
        b[p] = *reinterpret_cast<const bf16x8*>(Ys + p * EB_Y_BYTES + (wave * 32 + li) * EB_LDX + 32 * sl + 16 * lh);
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(Xs + (i * 32 + li) * EB_LDX + 32 * sl + 16 * lh);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[2], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[1], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[0], acc[i], 0, 0, 0);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (xpos[q] >= 0) *reinterpret_cast<unsigned short*>(Xs + xpos[q]) = 0;  // (same thread that set it)
  }
  const int gc = c0 + wave * 32 + li;
  if (gc < g.H) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gr = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float v = acc[i][r];
        if (gr < g.R && v != 0.f) atomicAdd(g.dT + (int64_t)gr * g.H + gc, v);
      }
  }
}

// returns GNX_OK after launching, or 1 if the shape is not eligible (caller falls back to the LDS-atomic kernel)
static int32_t gnx_embed_bwd_mfma(gnx_handle* h, const int64_t* idx, int64_t N, int K, const int32_t* offsets, int R,
                                  const float* dout, int H, float* dtable) {
  if (K > EMB_MAX_K || (H % 4) != 0 || !aligned16(dout) || N < 256) return 1;  // (below 4096 rows the LDS-atomic kernel
  // is contention-bound: 76 us for a 32-graph batch's 640 atoms, whose feature values repeat in every row)
  if (h->opt[GNX_OPT_EMBED_BWD_MFMA] == 0) return 1;
  embed_bwd_args g;
  g.idx = idx;
  for (int k = 0; k <= EMB_MAX_K; ++k) g.offs[k] = offsets[k <= K ? k : K];
  g.K = K;
  g.Y = dout;
  g.ldy = H;
  g.N = N;
  g.R = R;
  g.H = H;
  g.dT = dtable;
  if (h->opt[GNX_OPT_EMBED_BWD_MFMA] == 1 && R <= EB_R) {  // (2 = the fp32-MFMA kernel below)
    // ~256 workgroups; at least 128 rows each; small batches: ONE chunk per channel tile (one adder per element: deterministic)
    int64_t rows = gnx_cdiv(gnx_cdiv(N, (int64_t)(N < 4096 ? 1 : 256)), 32) * 32;
    if (rows < 128) rows = 128;
    g.rows_per_block = rows;
    dim3 grid((unsigned)gnx_cdiv(N, rows), (unsigned)gnx_cdiv(H, 128));
    hipLaunchKernelGGL(k_embed_bwd_bf16, grid, dim3(256), 0, h->stream, g);
    GNX_LAUNCH_CHECK();
    return GNX_OK;
  }
  const int64_t tiles = gnx_cdiv(R, BN) * gnx_cdiv(H, BN);
  int64_t chunks = gnx_cdiv(512, tiles);
  int64_t rows = gnx_cdiv(gnx_cdiv(N, chunks), BK) * BK;
  if (rows < 128) rows = 128;
  if (N < 4096) rows = gnx_cdiv(N, (int64_t)BK) * BK;  // small batches: ONE row chunk per output tile, i.e. one adder per
                                                       // table element -> a deterministic sum (and 20 K-steps at most)
  g.rows_per_block = rows;
  dim3 grid((unsigned)gnx_cdiv(N, rows), (unsigned)gnx_cdiv(R, BN), (unsigned)gnx_cdiv(H, BN));
  hipLaunchKernelGGL(k_embed_bwd_mfma, grid, dim3(256), 0, h->stream, g);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" size_t gnx_table_scatter_workspace_bytes(int64_t rows, int32_t R, int32_t H) {
  return gnx_table_scatter_ws_bytes(rows, R, H);
}

extern "C" int32_t gnx_embed_sum_bwd(gnx_handle* h, const int64_t* idx, int64_t N, int32_t K, const int32_t* offsets,
                                     int32_t R, const float* dout, int32_t H, float* dtable, void* ws, size_t ws_bytes) {
  GNX_CHECK_ARG(h && offsets && dtable && K > 0 && K <= 16 && H > 0 && R > 0 && N >= 0, "gnx_embed_sum_bwd: bad argument");
  GNX_CHECK_ARG(N == 0 || (idx && dout), "gnx_embed_sum_bwd: NULL array with N>0");
  GNX_CHECK_ARG(offsets[K] == R, "gnx_embed_sum_bwd: offsets[K]=%d != R=%d", offsets[K], R);
  if (N == 0) return GNX_OK;
  gnx_prof_scope prof(h, GNX_K_EMBED, 8.0 * N * K + 4.0 * N * H);
  {
    // large batches: the one-hot x gradient product on the MFMA (exact); small ones: LDS-privatised table adds
    const int32_t st = gnx_embed_bwd_mfma(h, idx, N, K, offsets, R, dout, H, dtable);
    if (st <= 0) return st;
  }
  return launch_table_scatter_add<int64_t>(h, idx, N, K, offsets, R, dout, H, dtable, ws, ws_bytes);
}

// used by gnx_edge_combine_bwd / gnx_gine_aggregate_bwd (int32 codes, one table)
int32_t gnx_code_scatter_add(gnx_handle* h, const int32_t* code, int64_t E, int R, const float* g, int H,
                             float* dtable, void* ws, size_t ws_bytes) {
  if (E == 0) return GNX_OK;
  int32_t offs[2] = {0, R};
  return launch_table_scatter_add<int32_t>(h, code, E, 1, offs, R, g, H, dtable, ws, ws_bytes);
}
