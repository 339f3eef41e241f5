// The two kernels of the k_ij fit of binary mixtures (ref: pcsaft/kij.py _pred_x1_worker, _loss_fn and the
// least_squares call of optimize_kij).  DESIGN.md §4c.
//
// gnx_pcsaft_kij_x1: a row is one (state, mixture) pair, a measured (T, P, x1_exp) under one candidate k_12; the
// candidates of a system are mixtures that share their component rows and differ in mix_kij.  One wave per row.  Lane l
// of chunk c flashes the feed z = (feeds[64 c + l], 1 - feeds[64 c + l]) with the solve of gnx_pcsaft_mix_flash.hpp; the
// lanes past F vote "no split".  __ballot(status == ST_OK) and its lowest set bit pick the first feed, in list order,
// that splits, __shfl brings its liquid x_1 to every lane, and the loop over the chunks ends, for the whole wave, at the
// first chunk with a hit.  Lane 0 writes the row:
//   x1, feed (its index in feeds), residual = log((x1 + 1e-6) / (x1_exp + 1e-6)), status 0;
//   without a split x1 = NaN, feed = -1, residual = 10.0 (the reference's penalty) and the status ST_BAD_INPUT where every
//   feed reports it or x1_exp is not finite, else ST_NO_CONV where a feed ended without convergence, else
//   ST_SINGLE_PHASE.
// A residual that is not finite although a feed split (x1_exp not finite or below -1e-6) is the penalty as well, as the
// reference counts it, with status ST_BAD_INPUT beside the x1 and feed of the split.
// No stability test runs before a flash, unlike the reference: a stable feed has no split with beta in [0, 1] and the flash
// reports it as single phase.  Liquid-liquid splits are not looked for.
//
// gnx_pcsaft_kij_sums: the eight sums per system that one Levenberg-Marquardt step needs, over the rows
// [system][candidate][point] of a kij_x1 launch, candidate 0 at k and candidate 1 at k + h.  One wave per system; lane l
// adds the points j = l, l + 64, ... in ascending order, then a __shfl_xor butterfly with fixed offsets 32 .. 1.
//
// No shared memory, no atomics, no cross-lane operation under a divergent branch: same input, same bits.  Neither launch
// has a kernel id (GNX_K_NONE); time them with events around the calls (tools/pcsaft_bench.py --kij).
#include "gnx_pcsaft_mix_flash.hpp"

namespace {

constexpr int kWave = 64;
constexpr double kKijPenalty = 10.0;  // residual of a row without a predicted x1 (pcsaft/kij.py _loss_fn)
constexpr double kKijShift = 1e-6;    // log((x1 + shift) / (x1_exp + shift))

// lane i % 64 of row i / 64: k_pcsaft_mix's n is 64 x rows, so a wave is whole or absent
struct KijX1Point {
  const double *T, *P, *x1_exp, *feeds;
  int64_t F;
  double *x1, *residual;
  int32_t *feed, *status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    const int64_t row = i / kWave;
    const int lane = (int)(i % kWave);
    const MixRef m = mix_of(set, row);
    const double t = T[row], p = P[row];
    bool all_bad = true, any_noconv = false;
    double found = NAN;
    int64_t at = -1;
    for (int64_t base = 0; base < F; base += kWave) {  // base, F and the exit below are the same in every lane
      const int64_t f = base + lane;
      int32_t st = ST_SINGLE_PHASE;  // a lane past F: no split, and no say in the status
      double xl = 0.0;
      if (f < F) {
        const double z1 = feeds[f];
        const double zr[2] = {z1, 1.0 - z1};
        double bt, rl, rv, xv[NC_MAX], yv[NC_MAX];
        st = mix_flash_solve(m, t, p, zr, bt, xv, yv, rl, rv);
        xl = xv[0];
      }
      const unsigned long long hit = __ballot(st == ST_OK);
      const unsigned long long fine = __ballot(f < F && st != ST_BAD_INPUT);
      const unsigned long long open = __ballot(f < F && st == ST_NO_CONV);
      all_bad = all_bad && fine == 0ull;
      any_noconv = any_noconv || open != 0ull;
      if (hit != 0ull) {
        const int src = __ffsll(hit) - 1;
        found = __shfl(xl, src, kWave);
        at = base + src;
        break;
      }
    }
    if (lane == 0) {  // nothing crosses lanes from here on
      const double xe = x1_exp[row];
      int32_t st = ST_OK;
      double r = kKijPenalty;
      if (at >= 0) {
        r = ::log((found + kKijShift) / (xe + kKijShift));
        if (!isfinite(r)) {
          r = kKijPenalty;
          st = ST_BAD_INPUT;
        }
      } else {
        st = (all_bad || !isfinite(xe)) ? ST_BAD_INPUT : any_noconv ? ST_NO_CONV : ST_SINGLE_PHASE;
      }
      x1[row] = found;
      feed[row] = (int32_t)at;
      residual[row] = r;
      status[row] = st;
    }
  }
};

// sums[s, 0 .. 8) of system s: rows 2 seg[s] + j (candidate 0) and 2 seg[s] + n_s + j (candidate 1), j < n_s = seg[s + 1] -
// seg[s].  A system whose range does not lie in the n rows gets NaN in every slot.
__global__ void __launch_bounds__(256) k_pcsaft_kij_sums(const double* residual, const double* x1, const double* x1_exp,
                                                         const int32_t* status, const int64_t* seg, int64_t S, int64_t n,
                                                         double hstep, double* sums) {
  const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x % kWave;
  const bool active = s < S;  // the same in every lane of a wave; a wave past S adds nothing and writes nothing
  const int64_t lo = active ? seg[s] : 0, hi = active ? seg[s + 1] : 0;
  const bool valid = lo >= 0 && hi >= lo && hi <= n / 2;
  const int64_t ns = valid ? hi - lo : 0;
  double v[8];
  for (int k = 0; k < 8; ++k) v[k] = 0.0;
  for (int64_t j = lane; j < ns; j += kWave) {
    const int64_t a = 2 * lo + j, b = a + ns;
    const double r0 = residual[a], r1 = residual[b];
    const bool p0 = status[a] != ST_OK, p1 = status[b] != ST_OK;
    v[0] += r0 * r0;
    v[4] += r1 * r1;
    if (p0) {
      v[1] += 1.0;
    } else {
      const double xe = x1_exp[a];
      v[2] += ::fabs(r0);
      v[3] += ::fabs((x1[a] - xe) / xe);
      if (!p1) {
        const double jac = (r1 - r0) / hstep;
        v[5] += jac * r0;
        v[6] += jac * jac;
        v[7] += 1.0;
      }
    }
  }
  for (int off = kWave / 2; off >= 1; off >>= 1)
    for (int k = 0; k < 8; ++k) v[k] += __shfl_xor(v[k], off, kWave);
  if (active && lane == 0)
    for (int k = 0; k < 8; ++k) sums[s * 8 + k] = valid ? v[k] : NAN;
}

}  // namespace

extern "C" int32_t gnx_pcsaft_kij_x1(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                     const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                     const int64_t* owner, const double* T, const double* P, const double* x1_exp,
                                     const double* feeds, int64_t F, int64_t n, double* x1, int32_t* feed,
                                     double* residual, int32_t* status) {
  GNX_CHECK_ARG(nc == 2 && F >= 1 && n >= 0 && n <= ((int64_t)1 << 31),
                "gnx_pcsaft_kij_x1: bad argument (nc == 2, F >= 1, n <= 2^31)");
  // no kernel id of its own: under GNX_K_NONE the scope stays off and the launch is a plain one
  return mix_launch(h, "gnx_pcsaft_kij_x1", GNX_K_NONE, (44.0 + 8.0 * F) / kWave,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, 2, owner}, n * kWave,
                    T && P && x1_exp && feeds && x1 && feed && residual && status,
                    KijX1Point{T, P, x1_exp, feeds, F, x1, residual, feed, status});
}

extern "C" int32_t gnx_pcsaft_kij_sums(gnx_handle* h, const double* residual, const double* x1, const double* x1_exp,
                                       const int32_t* status, const int64_t* seg, int64_t S, int64_t n, double hstep,
                                       double* sums) {
  GNX_CHECK_ARG(h && S >= 0 && n >= 0 && S <= ((int64_t)1 << 31) && hstep != 0.0 && std::isfinite(hstep),
                "gnx_pcsaft_kij_sums: bad argument (S, n >= 0, h finite and not 0)");
  if (S == 0) return GNX_OK;
  GNX_CHECK_ARG(residual && x1 && x1_exp && status && seg && sums, "gnx_pcsaft_kij_sums: NULL argument");
  gnx_prof_scope prof(h, GNX_K_NONE, 0.0, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_kij_sums, dim3((unsigned)gnx_cdiv(S * kWave, 256)), dim3(256), 0, h->stream, residual,
                   x1, x1_exp, status, seg, S, n, hstep, sums);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}
