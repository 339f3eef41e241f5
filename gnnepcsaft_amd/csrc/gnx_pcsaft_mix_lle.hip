// Mixture PC-SAFT liquid-liquid flash in fp64: at (T, P) the split of the feed z into two phases x and y started from a
// composition w0 of the second phase, in practice the w with the most negative tangent-plane distance of the stability
// test (gnx_pcsaft_mix_stab.hip).  (ref: pcsaft/pcsaft_feos.py mix_lle_feos / mix_lle_diagram_feos, and pcsaft/kij.py:37
// _pred_x1_worker, which runs feos's tp_flash after is_stable_feos and takes the denser phase because that flash also
// returns liquid-liquid pairs; [3P] feos 0.8 PhaseEquilibrium.tp_flash).  DESIGN.md §4c.
//
// Equations, in the flash kernel's form without ln Z: with ln f_i = mu_i^res/kT + ln(rho x_i),
//   ln f_i(T, rho_x, x) = ln f_i(T, rho_y, y),  p(T, rho_x, x) = p(T, rho_y, y) = P,  z_i = (1 - beta) x_i + beta y_i.
// The state of a phase is the stability test's (stab_state, gnx_pcsaft_mix_state.hpp): of its highest liquid root and its
// lowest vapour root at P the one with the lower g = sum_i x_i ln f_i, the only root where there is one, the liquid root
// on a tie.  So w0 and the split agree about what a phase is, and a feed whose stable split is vapour-liquid comes out as
// that split, the tie line gnx_pcsaft_mix_flash.hip finds.
//
// Successive substitution on ln K over the components present.  Start: ln K_i = ln(w0_i / z_i), both normalised over the
// present slots.  Step: Rachford-Rice for beta on the negative-flash window, x = z / (1 + beta (K - 1)), y = K x, the
// state of both, ln K_i += ln f_i(x) - ln f_i(y).  It ends when max_i |ln f_i(x) - ln f_i(y)| < 1e-10 at the densities
// that are reported.  No split (ST_SINGLE_PHASE): one component, an empty window (w0 = z is one: it ends at once),
// convergence with beta outside [0, 1], or onto equal phases (max_i |ln(y_i / x_i)| and |rho_y / rho_x - 1| below 1e-4,
// the stability test's rule for a trial on the feed).  On output x is the phase of higher molar density and beta the
// mole fraction of the other one.
//
// As in the flash and the stability test, once a step has moved ln K by less than 0.05 the next one looks for each root
// within 5 % of the previous one first, takes a root that was not there to be still missing, and scans only where a
// bracket does not hold.  A point that ends on roots found this way evaluates that step again from the scans, and goes
// on with scans alone if it does not end there: every number reported comes from the highest liquid root and the lowest
// vapour root of both phases.
//
// One lane per point, no shared memory, no atomics, every loop with a fixed trip cap: same input, same bits, wherever the
// row stands in the launch.  No kernel id (GNX_K_NONE); time it with events around the call (tools/pcsaft_bench.py
// --lle).
#include "gnx_pcsaft_mix_state.hpp"

namespace {

// The oracle ends the eight liquid-liquid test points at 1e-8 in 19 to 25 steps and the three vapour-liquid ones in 5 to
// 9, the residual falling by 0.35 to 0.42 a step: 1e-10 is some 5 steps further.  A feed near a plait point loses far
// less per step.
constexpr int kLleIters = 200;
constexpr int kLleSplitIters = 100;     // safeguarded Newton of the Rachford-Rice equation
constexpr double kLleNearMove = 0.05;   // largest step in ln K after which the next roots are sought near the previous
constexpr double kLleSame = 1e-4;       // ln(y_i / x_i) and rho_y / rho_x - 1 within this: both phases are the same fluid

enum : int { RR_OK = 0, RR_EMPTY = 1, RR_FAIL = 2 };

// root beta of g(beta) = sum_k z_k (K_k - 1) / (1 + beta (K_k - 1)) over the n components present, on the negative-flash
// window (1 / (1 - K_max), 1 / (1 - K_min)).  RR_EMPTY: no K above 1 or none below.  The flash has the same function in
// its own unit (flash_split), which is left as it is.
__device__ int lle_split(const double* z, const double* K, int n, double& beta) {
  double kmax = K[0], kmin = K[0];
  for (int k = 1; k < n; ++k) {
    kmax = ::fmax(kmax, K[k]);
    kmin = ::fmin(kmin, K[k]);
  }
  if (!(kmax > 1.0) || !(kmin < 1.0)) return (kmax == kmax && kmin == kmin) ? RR_EMPTY : RR_FAIL;
  double lo = 1.0 / (1.0 - kmax), hi = 1.0 / (1.0 - kmin), b = 0.5;
  for (int it = 0; it < kLleSplitIters; ++it) {
    double g = 0.0, dg = 0.0;
    for (int k = 0; k < n; ++k) {
      const double r = (K[k] - 1.0) / (1.0 + b * (K[k] - 1.0));
      g += z[k] * r;
      dg += z[k] * r * r;
    }
    if (!isfinite(g)) return RR_FAIL;
    if (g == 0.0) break;
    if (g > 0.0)
      lo = b;
    else
      hi = b;
    double bn = b + g / dg;
    if (!(bn > lo && bn < hi)) bn = 0.5 * (lo + hi);
    if (!(bn > lo && bn < hi)) break;  // the bracket has closed on b
    const bool done = ::fabs(bn - b) <= 1e-16 * ::fmax(1.0, ::fabs(b));
    b = bn;
    if (done) break;
  }
  beta = b;
  return RR_OK;
}

// split of point i at (T, P, z) started from w0
struct MixLlePoint {
  const double *T, *P, *z, *w0;
  double *beta, *x, *y, *rho_x, *rho_y;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix c;
    const MixRef m = mix_of(set, i);
    const double t = T[i], p = P[i];
    int32_t st = ST_BAD_INPUT;
    double bt = 0.0, rx = 0.0, ry = 0.0, xv[NC_MAX], yv[NC_MAX];
    for (int s = 0; s < NC_MAX; ++s) xv[s] = yv[s] = 0.0;
    if (isfinite(p) && p > 0.0 && load_mix(m, z, i, t, c)) {
      const double *zin = z + i * m.nc, *win = w0 + i * m.nc;
      int64_t cm[NC_MAX];
      const MixRef mp = mix_present(m, zin, cm);  // both phases have the feed's components and no others
      const int nc = m.nc;
      const int n = c.n;
      const double pt = p / c.kT_pa;
      double zc[NC_MAX], xc[NC_MAX], yc[NC_MAX], lnk[NC_MAX], lnkp[NC_MAX], kv[NC_MAX], lnf[2][NC_MAX];
      double sum = 0.0, wsum = 0.0;
      int slot[NC_MAX];
      bool ok = true;  // every start value in a present slot is a positive number
      for (int s = 0; s < nc; ++s)
        if (cm[s] != -1) {
          sum += zin[s];
          wsum += win[s];
          ok = ok && isfinite(win[s]) && win[s] > 0.0;
        }
      ok = ok && isfinite(wsum);
      if (ok) {
        st = ST_NO_CONV;
        for (int s = 0, k = 0; s < nc; ++s)
          if (cm[s] != -1) {
            slot[k] = s;
            zc[k] = zin[s] / sum;
            lnk[k] = lnkp[k] = ::log(win[s] / wsum / zc[k]);
            ok = ok && isfinite(lnk[k]);
            ++k;
          }
        bool conv = false, single = n == 1, scans_only = false;
        int damp = 0;
        double prev[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, step = 1.0;  // the roots of both phases and the move of ln K, last step
        for (int it = 0; ok && !single && it < kLleIters; ++it) {
          for (int k = 0; k < n; ++k) kv[k] = ::exp(lnk[k]);
          const int sp = lle_split(zc, kv, n, bt);
          single = sp == RR_EMPTY;
          ok = sp == RR_OK;
          if (!ok) break;
          for (int k = 0; k < n; ++k) {
            xv[slot[k]] = xc[k] = zc[k] / (1.0 + bt * (kv[k] - 1.0));
            yv[slot[k]] = yc[k] = kv[k] * xc[k];
            ok = ok && xc[k] > 0.0 && yc[k] > 0.0 && isfinite(xc[k]) && isfinite(yc[k]);
          }
          if (!ok) break;
          const bool try_near = !scans_only && step < kLleNearMove;
          bool near[2] = {try_near, try_near}, has = true;
          double rr[2] = {0.0, 0.0};
#pragma unroll 1
          for (int ph = 0; has && ph < 2; ++ph)
            has = stab_state(mp, ph ? yv : xv, ph ? yc : xc, n, t, pt, c, rr[ph], lnf[ph], prev[ph], near[ph]);
          rx = rr[0];
          ry = rr[1];
          if (!has && try_near) {
            scans_only = true;  // this step again, ln K as it is, from the scans
            continue;
          }
          if (!has) {
            if (++damp > kVleMixDamp) break;
            for (int k = 0; k < n; ++k) lnk[k] = 0.5 * (lnk[k] + lnkp[k]);  // no root of a phase: half the step back
            step = 1.0;
            continue;
          }
          damp = 0;
          double res = 0.0;
          for (int k = 0; k < n; ++k) {
            const double d = lnf[0][k] - lnf[1][k];
            res = ::fmax(res, ::fabs(d));
            ok = ok && isfinite(d);
          }
          if (!ok) break;
          conv = res < kVleMixTol;
          if (conv && (near[0] || near[1])) {
            // what is reported is the state of the highest liquid root and the lowest vapour root: only the scans say so
            scans_only = true;
            conv = false;
            continue;
          }
          if (conv) break;
          step = res;
          for (int k = 0; k < n; ++k) {
            lnkp[k] = lnk[k];
            lnk[k] += lnf[0][k] - lnf[1][k];
          }
        }
        if (single) {
          st = ST_SINGLE_PHASE;
        } else if (ok && conv) {
          double same = ::fabs(ry / rx - 1.0);
          for (int k = 0; k < n; ++k) same = ::fmax(same, ::fabs(::log(yc[k] / xc[k])));
          if (!isfinite(same))
            st = ST_NO_CONV;
          else
            st = (same < kLleSame || !(bt >= 0.0 && bt <= 1.0)) ? ST_SINGLE_PHASE : ST_OK;
          if (st == ST_OK && ry > rx) {  // x is the denser phase, beta the share of the other one
            bt = 1.0 - bt;
            const double r = rx;
            rx = ry;
            ry = r;
            for (int k = 0; k < n; ++k) {
              xv[slot[k]] = yc[k];
              yv[slot[k]] = xc[k];
            }
          }
        }
      }
    }
    const bool good = st == ST_OK;
    beta[i] = good ? bt : 0.0;
    if (rho_x) rho_x[i] = good ? rx : 0.0;
    if (rho_y) rho_y[i] = good ? ry : 0.0;
    store_row(x, i, m, good, xv);
    store_row(y, i, m, good, yv);
    status[i] = st;
  }
};

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_lle(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                      const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                      const int64_t* owner, const double* T, const double* P, const double* z,
                                      const double* w0, int64_t n, double* beta, double* x, double* y, double* rho_x,
                                      double* rho_y, int32_t* status) {
  // no kernel id of its own: under GNX_K_NONE the scope stays off and the launch is a plain one
  return mix_launch(h, "gnx_pcsaft_mix_lle", GNX_K_NONE, 52.0 + 32.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n,
                    T && P && z && w0 && beta && x && y && status,
                    MixLlePoint{T, P, z, w0, beta, x, y, rho_x, rho_y, status});
}
