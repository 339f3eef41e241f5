// Mixture PC-SAFT dew point in fp64: at (T, y) the pressure P at which the vapour y is in equilibrium with a first drop
// of liquid, that liquid's composition x and both densities, on the model of gnx_pcsaft_mix.hpp (ref:
// pcsaft/pcsaft_feos.py mix_vp_feos, the dew half; [3P] feos 0.8 PhaseEquilibrium.dew_point).  DESIGN.md §4c.
//
// The equations are the bubble point's (gnx_pcsaft_mix_vle.hip), in the form without ln Z:
//   ln f_i^L(T, rho_L, x) = ln f_i^V(T, rho_V, y) for every component present,  p(T, rho_L, x) = p(T, rho_V, y) = P,
// with the roles of x and y exchanged: y is given, x is looked for.
//
// Successive substitution.  Start: Raoult's law on each component's own liquid at zero pressure, k_i = f_i^L of
// component i alone there (times kT a pressure; 100 x the largest k found for a component without such a liquid),
// P = 1 / sum_i (y_i / k_i), x_i = y_i / k_i normalised.  A start from x = y collapses onto the trivial solution for a
// vapour rich in a light gas; this one does not.  Step: liquid root of x and vapour root of y at P, x_i K_i^-1 =
// x_i f_i^V / f_i^L, s = sum of them, x <- that / s, P <- P / s; it ends when max(|ln s|, max_i |d ln x_i|) < 1e-10, and
// what is reported is the state at which the fugacities were evaluated.  The vapour's mixture is folded once, the
// liquid's from x at every step.  The substitution converges linearly, slowly where the liquid is far from ideal, so
// every few steps one step is stretched by 1 / (1 - lambda), lambda the dominant eigenvalue read from two consecutive
// steps (167 -> 23 steps on ethanol + water in the oracle's arithmetic); what a step ends on is judged
// by the same residual.  A dew point need not be unique (retrograde vapours have two): the one reported is the
// one this start leads to.
//
// This file is a translation unit of its own so that the bubble kernel compiles to the instructions it had before.
// One lane per point, no shared memory, no atomics, every loop with a fixed trip cap: same input, same bits.  The
// launch carries no kernel id (GNX_K_NONE); time it with events around the call (tools/pcsaft_bench.py --dew).
#include "gnx_pcsaft_mix_vle.hpp"

namespace {

// Substitution steps.  The liquid's composition moves by the ratio of the K values per step, which is slow where the
// liquid is far from ideal: the oracle takes 166 steps on ethanol + water at 350 K, the most of the test cases; the cap
// is a little more than twice that.  kVleMixIters = 200 of the bubble loop would lose that point.
constexpr int kDewMixIters = 400;
constexpr double kDewNoLiquid = 100.0;  // k of a component without a liquid of its own, in units of the largest k found
// Extrapolation of the substitution (below): after this many plain steps in a row, once the residual is below the gate
// (the map is close to linear there) and only for a dominant eigenvalue in (0, kDewAccelMax): a step is at most 20 d.
constexpr int kDewAccelAfter = 3;
constexpr double kDewAccelGate = 1e-2;
constexpr double kDewAccelMax = 0.95;

// dew point of point i at (T, y); dew_raoult, the start, is in gnx_pcsaft_mix_vle.hpp
struct MixDewPoint {
  const double *T, *y;
  double *P, *x, *rho_l, *rho_v;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix cl, cv;
    const MixRef m = mix_of(set, i);
    const double t = T[i];
    int32_t st = ST_BAD_INPUT;
    double pt = 0.0, rl = 0.0, rv = 0.0, xv[NC_MAX];
    for (int s = 0; s < NC_MAX; ++s) xv[s] = 0.0;
    if (load_mix(m, y, i, t, cv)) {  // the vapour: folded once, y does not change
      st = ST_NO_CONV;
      const double* yin = y + i * m.nc;
      int64_t cm[NC_MAX];
      const MixRef mp = mix_present(m, yin, cm);  // the liquid has the vapour's components and no others
      const int nc = m.nc;
      const int n = cv.n;
      // the start: Raoult's law on each component's own liquid at zero pressure
      double kr[NC_MAX], kmax = 0.0, ysum = 0.0;
      for (int q = 0; q < nc; ++q) {
        kr[q] = 0.0;
        if (cm[q] == -1) continue;
        ysum += yin[q];
        kr[q] = dew_raoult(mp, q, t, cl);
        kmax = ::fmax(kmax, kr[q]);
      }
      bool ok = kmax > 0.0, conv = false;
      if (ok) {
        double s = 0.0;
        for (int q = 0; q < nc; ++q)
          if (cm[q] != -1) {
            xv[q] = yin[q] / ysum / (kr[q] > 0.0 ? kr[q] : kDewNoLiquid * kmax);
            s += xv[q];
          }
        ok = s > 0.0 && isfinite(s);
        pt = 1.0 / s;
        for (int q = 0; q < nc; ++q)
          if (cm[q] != -1) {
            xv[q] /= s;
            ok = ok && xv[q] > 0.0;
          }
        ok = ok && pt > 0.0 && isfinite(pt);
      }
      double pprev = 0.0, lnf[2][NC_MAX], dprev[NC_MAX];
      int damp = 0, plain = 0;  // plain: substitution steps since the start, a halving or an extrapolation
      bool prev = false;        // dprev holds the d of the step before this one
      for (int it = 0; ok && !conv && it < kDewMixIters; ++it) {
        double el, ev;
        ok = cl.init(mp, xv, t) && cl.n == n && density_root(cl, pt, el) == ST_OK;
        if (!ok) break;
        const int vr = vapour_root(cv, pt, ev);
        if (vr == VR_NONE && ++damp <= kVleMixDamp) {
          pt = 0.5 * (pt + pprev);  // no vapour of y at this pressure: half the step back
          prev = false;
          plain = 0;
          continue;
        }
        ok = vr == VR_OK;
        if (!ok) break;
        damp = 0;
        // at the densities reported, converted as the state forms convert them
        rl = molar_density(el, cl.c3);
        rv = molar_density(ev, cv.c3);
        for (int ph = 0; ok && ph < 2; ++ph)
          ok = mix_lnf_at(mp, ph ? yin : xv, t, number_density(ph ? rv : rl), ph ? cv : cl, lnf[ph]);
        if (!ok) break;
        double xk[NC_MAX], s = 0.0;  // x_i / K_i = x_i f_i^V / f_i^L
        for (int q = 0, k = 0; q < nc; ++q)
          if (cm[q] != -1) {
            xk[k] = xv[q] * ::exp(lnf[1][k] - lnf[0][k]);
            s += xk[k++];
          }
        ok = s > 0.0 && isfinite(s);
        if (!ok) break;
        const double ls = ::log(s);
        double res = ::fabs(ls);
        for (int k = 0; k < n; ++k) res = ::fmax(res, ::fabs(lnf[1][k] - lnf[0][k] - ls));
        ok = res == res;
        conv = res < kVleMixTol;
        if (conv || !ok) break;
        // Dominant-eigenvalue extrapolation.  In l_i = ln(x_i / P) a step is l <- l + d, d_i = ln f_i^V - ln f_i^L, and near
        // the solution d shrinks by the factor lambda of the map's dominant eigenvalue per step: the steps still to come
        // sum to d / (1 - lambda).  lambda is read from this step's d and the one before it.
        bool acc = false;
        if (prev && plain >= kDewAccelAfter && res < kDewAccelGate) {
          double dd = 0.0, pp = 0.0;
          for (int j = 0; j < n; ++j) {
            dd += (lnf[1][j] - lnf[0][j]) * dprev[j];
            pp += dprev[j] * dprev[j];
          }
          const double lambda = dd / pp;
          acc = lambda > 0.0 && lambda < kDewAccelMax;
          if (acc) {
            s = 0.0;
            for (int q = 0, j = 0; q < nc; ++q)
              if (cm[q] != -1) {
                xk[j] = xv[q] * ::exp((lnf[1][j] - lnf[0][j]) / (1.0 - lambda));
                s += xk[j++];
              }
            ok = s > 0.0 && isfinite(s);
            if (!ok) break;
          }
        }
        prev = !acc;  // the step after an extrapolation is no continuation of the one before it
        plain = acc ? 0 : plain + 1;
        for (int j = 0; j < n; ++j) dprev[j] = lnf[1][j] - lnf[0][j];
        int k = 0;
        for (int q = 0; q < nc; ++q)
          if (cm[q] != -1) {
            xv[q] = xk[k++] / s;
            ok = ok && xv[q] > 0.0;
          }
        pprev = pt;
        pt = pt / s;
        ok = ok && pt > 0.0 && isfinite(pt);
      }
      // equal densities: the trivial solution, both phases the same fluid
      if (ok && conv && rv > 0.0 && rl - rv > kVleTrivial * rl) st = ST_OK;
    }
    const bool good = st == ST_OK;
    P[i] = good ? pt * cv.kT_pa : 0.0;
    if (rho_l) rho_l[i] = good ? rl : 0.0;
    if (rho_v) rho_v[i] = good ? rv : 0.0;
    store_row(x, i, m, good, xv);
    status[i] = st;
  }
};

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_dew(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                      const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                      const int64_t* owner, const double* T, const double* y, int64_t n, double* P,
                                      double* x, double* rho_l, double* rho_v, int32_t* status) {
  // no kernel id of its own: under GNX_K_NONE the scope stays off and the launch is a plain one
  return mix_launch(h, "gnx_pcsaft_mix_dew", GNX_K_NONE, 44.0 + 16.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n, T && y && P && x && status,
                    MixDewPoint{T, y, P, x, rho_l, rho_v, status});
}
