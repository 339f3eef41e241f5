// The (T, P) flash of one feed as a device function, shared by gnx_pcsaft_mix_flash.hip (one lane per point) and
// gnx_pcsaft_kij.hip (one lane per trial feed of a row).  Equations, start, step and end: the head of
// gnx_pcsaft_mix_flash.hip; DESIGN.md §4c.
#pragma once

#include "gnx_pcsaft_mix_vle.hpp"

namespace {

constexpr int kFlashSplitIters = 100;  // safeguarded Newton of the Rachford-Rice equation
constexpr double kFlashNear = 0.05;    // half width, relative, of the bracket around the previous step's root
constexpr double kFlashNearRes = 0.05; // largest step in ln K after which the next roots are sought near the previous
constexpr double kFlashSame = 1e-9;    // relative agreement of a root found near the previous one with the scan's

enum : int { RR_OK = 0, RR_EMPTY = 1, RR_FAIL = 2 };

// root beta of g(beta) = sum_k z_k (K_k - 1) / (1 + beta (K_k - 1)) over the n components present.  g falls from +inf to
// -inf on (1 / (1 - K_max), 1 / (1 - K_min)), on which every x and y stays positive.  RR_EMPTY: no K above 1 or none
// below, g has no root.  Newton from 0.5 (always inside), bisection where a step leaves the bracket.
__device__ int flash_split(const double* z, const double* K, int n, double& beta) {
  double kmax = K[0], kmin = K[0];
  for (int k = 1; k < n; ++k) {
    kmax = ::fmax(kmax, K[k]);
    kmin = ::fmin(kmin, K[k]);
  }
  if (!(kmax > 1.0) || !(kmin < 1.0)) return (kmax == kmax && kmin == kmin) ? RR_EMPTY : RR_FAIL;
  double lo = 1.0 / (1.0 - kmax), hi = 1.0 / (1.0 - kmin), b = 0.5;
  for (int it = 0; it < kFlashSplitIters; ++it) {
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

// root of p~(eta) = pt with dp/deta > 0 within kFlashNear of e0, the root of the previous step.  false: the bracket does
// not hold it with a rising p~ at both ends, or the root solve failed; the caller scans.
__device__ bool root_near(Mix& c, double pt, double e0, double& out) {
  const double lo = e0 * (1.0 - kFlashNear), hi = ::fmin(e0 * (1.0 + kFlashNear), kEtaMax);
  if (!(lo > 0.0) || !(hi > lo)) return false;
  const Mix::Eval a = c.eval(lo), b = c.eval(hi);
  if (!a.ok || !b.ok || !(a.p <= pt) || !(b.p > pt) || !(a.dp > 0.0) || !(b.dp > 0.0)) return false;
  double xr;
  if (!pcsaft_root(c, pt, lo, hi, e0, xr) || !(xr > 0.0)) return false;
  const Mix::Eval r = c.eval(xr);
  if (!r.ok || !(r.dp > 0.0)) return false;
  out = xr;
  return true;
}

// Flash of the feed zin[0 .. m.nc) of mixture m at (t, p) -> status.  bt, xv, yv, rl, rv: the state the fugacities were
// last evaluated at, the result where the status is ST_OK and without meaning elsewhere; the caller writes what its entry
// documents for a failed point.  xv and yv have NC_MAX slots, 0.0 in those the solve does not use.
__device__ int32_t mix_flash_solve(const MixRef& m, double t, double p, const double* zin, double& bt, double* xv,
                                   double* yv, double& rl, double& rv) {
  Mix cl, cv;
  int32_t st = ST_BAD_INPUT;
  bt = rl = rv = 0.0;
  for (int s = 0; s < NC_MAX; ++s) xv[s] = yv[s] = 0.0;
  if (isfinite(p) && p > 0.0 && m.comp && cl.init(m, zin, t)) {
    st = ST_NO_CONV;
    int64_t cm[NC_MAX];
    const MixRef mp = mix_present(m, zin, cm);  // both phases have the feed's components and no others
    const int nc = m.nc;
    const int n = cl.n;
    const double pt = p / cl.kT_pa;
    double zc[NC_MAX], lnk[NC_MAX], lnkp[NC_MAX], kv[NC_MAX], lnf[2][NC_MAX], sum = 0.0;
    for (int s = 0; s < nc; ++s)
      if (cm[s] != -1) sum += zin[s];
    for (int s = 0, k = 0; s < nc; ++s)
      if (cm[s] != -1) zc[k++] = zin[s] / sum;
    bool ok = true, conv = false, single = n == 1;  // one component has no split away from its vapour pressure
    if (!single) {
      // the start: the liquid z at zero pressure under an ideal vapour; without one, the highest root of z at P
      double el;
      ok = density_root(cl, 0.0, el) == ST_OK && el >= kEtaMax / kScanDensity;
      if (!ok) ok = density_root(cl, pt, el) == ST_OK;
      ok = ok && mix_lnf_at(mp, zin, t, number_density(molar_density(el, cl.c3)), cl, lnf[0]);
      for (int k = 0; ok && k < n; ++k) {
        lnk[k] = lnkp[k] = lnf[0][k] - ::log(zc[k] * pt);
        ok = isfinite(lnk[k]);
      }
    }
    int damp = 0;
    double el0 = 0.0, ev0 = 0.0, step = 1.0;  // the roots and the step in ln K of the last full step
    bool scans_only = false;
    for (int it = 0; ok && !single && it < kVleMixIters; ++it) {
      for (int k = 0; k < n; ++k) kv[k] = ::exp(lnk[k]);
      const int sp = flash_split(zc, kv, n, bt);
      single = sp == RR_EMPTY;
      ok = sp == RR_OK;
      if (!ok) break;
      for (int s = 0, k = 0; s < nc; ++s)
        if (cm[s] != -1) {
          xv[s] = zc[k] / (1.0 + bt * (kv[k] - 1.0));
          yv[s] = kv[k] * xv[s];
          ok = ok && xv[s] > 0.0 && yv[s] > 0.0 && isfinite(xv[s]) && isfinite(yv[s]);
          ++k;
        }
      ok = ok && cl.init(mp, xv, t) && cl.n == n && cv.init(mp, yv, t) && cv.n == n;
      if (!ok) break;
      double el, ev = 0.0;
      const bool near = !scans_only && el0 > 0.0 && step < kFlashNearRes && root_near(cl, pt, el0, el) &&
                        root_near(cv, pt, ev0, ev);
      if (!near) {
        const bool liquid = density_root(cl, pt, el) == ST_OK;
        const int vr = liquid ? vapour_root(cv, pt, ev) : VR_NONE;
        if ((!liquid || vr == VR_NONE) && ++damp <= kVleMixDamp) {
          for (int k = 0; k < n; ++k) lnk[k] = 0.5 * (lnk[k] + lnkp[k]);  // no root of a phase: half the step back
          continue;
        }
        ok = liquid && vr == VR_OK;
        if (!ok) break;
      }
      damp = 0;
      // at the densities reported, converted as the state forms convert them
      rl = molar_density(el, cl.c3);
      rv = molar_density(ev, cv.c3);
      for (int ph = 0; ok && ph < 2; ++ph)
        ok = mix_lnf_at(mp, ph ? yv : xv, t, number_density(ph ? rv : rl), ph ? cv : cl, lnf[ph]);
      if (!ok) break;
      double res = 0.0;
      for (int k = 0; k < n; ++k) res = ::fmax(res, ::fabs(lnf[0][k] - lnf[1][k]));
      for (int k = 0; k < n; ++k) ok = ok && isfinite(lnf[0][k] - lnf[1][k]);
      conv = ok && res < kVleMixTol;
      if (conv && near) {
        // the liquid root is the highest and the vapour root the lowest only if the scans find them too
        double es, vs;
        conv = density_root(cl, pt, es) == ST_OK && vapour_root(cv, pt, vs) == VR_OK &&
               ::fabs(es - el) <= kFlashSame * el && ::fabs(vs - ev) <= kFlashSame * ev;
        if (!conv) {
          scans_only = true;  // this step again, ln K as it is, from the scans
          continue;
        }
      }
      if (conv || !ok) break;
      el0 = el;
      ev0 = ev;
      step = res;
      for (int k = 0; k < n; ++k) {
        lnkp[k] = lnk[k];
        lnk[k] += lnf[0][k] - lnf[1][k];
      }
    }
    if (single)
      st = ST_SINGLE_PHASE;
    else if (ok && conv)  // equal densities: the trivial solution; beta outside [0, 1]: the feed is off the tie line
      st = (rv > 0.0 && rl - rv > kVleTrivial * rl && bt >= 0.0 && bt <= 1.0) ? ST_OK : ST_SINGLE_PHASE;
  }
  return st;
}

}  // namespace
