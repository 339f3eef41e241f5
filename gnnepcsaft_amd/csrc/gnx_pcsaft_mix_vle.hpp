// What the two-phase kernels of a mixture share: gnx_pcsaft_mix_vle.hip (bubble point) and gnx_pcsaft_mix_flash.hip
// ((T, P) flash).  Both need the lowest root of p~(eta) = pt of a vapour and ln f_i = mu_i^res/kT + ln(rho x_i) of a
// phase at a given composition, and both end on the same bounds.  DESIGN.md §4c.
#pragma once

#include "gnx_pcsaft_mix_grad.hpp"

namespace {

constexpr int kVleScanLog = 64;       // vapour scan: 64 log-spaced points in [1e-10, 1e-2) ...
constexpr int kVleScanLin = 512;      // ... then 512 linear points in (1e-2, kEtaMax]
constexpr int kVleMixIters = 200;     // successive substitution steps
constexpr int kVleMixDamp = 20;       // halvings of a pressure step in a row that finds no vapour root
// the liquid's mu^res moves by (dp/drho)/(RT) ~ 1e2 .. 1e3 per relative change of rho and a root ends at 1e-14: the
// residual's rounding floor is about 1e-11
constexpr double kVleMixTol = 1e-10;
constexpr double kVleTrivial = 1e-3;  // rho_l - rho_v <= this * rho_l: both phases are the same fluid

__device__ __forceinline__ double vapour_grid(int k) {
  return k < kVleScanLog ? 1e-10 * ::pow(1e8, (double)k / kVleScanLog)
                         : 1e-2 + (kEtaMax - 1e-2) * (double)(k - kVleScanLog + 1) / kVleScanLin;
}

enum : int { VR_OK = 0, VR_NONE = 1, VR_FAIL = 2 };

// packing fraction of the lowest root of p~(eta) = pt with dp/deta > 0.  VR_NONE: p~ turns over (dp/deta <= 0) below
// pt, the mixture has no vapour at this pressure; VR_FAIL: an evaluation failed.
__device__ int vapour_root(Mix& c, double pt, double& out) {
  double lo = 0.0;
  for (int k = 0; k < kVleScanLog + kVleScanLin; ++k) {
    const double eta = vapour_grid(k);
    const Mix::Eval e = c.eval(eta);
    if (!e.ok || !isfinite(e.p) || !isfinite(e.dp)) return VR_FAIL;
    if (e.p >= pt) {
      double xr;
      if (!pcsaft_root(c, pt, lo, eta, pt * c.c3, xr) || !(xr > 0.0)) return VR_FAIL;
      const Mix::Eval r = c.eval(xr);
      if (!r.ok) return VR_FAIL;
      if (!(r.dp > 0.0)) return VR_NONE;
      out = xr;
      return VR_OK;
    }
    if (!(e.dp > 0.0)) return VR_NONE;
    lo = eta;
  }
  return VR_NONE;
}

// ln f_i = mu_i^res/kT + ln(rn x_i) of the components present, in their compact order, at (T, number density rn, x).  c
// is mixture m in real arithmetic, initialised from the same arguments; every used slot of m must have x > 0.  The
// sibling of gnx_pcsaft_mix_phi.hip's mix_lnphi_at without the ln Z:
//   mu_i^res/kT = a + (Z - 1) + a_xi - sum_j x_j a_xj,  a_xi = da/dx_i at fixed T, rho, the x independent
// The two are the same up to their last statements.  Sharing that part is deferred, not done: with the common part in
// one function (results through a struct, through references) the bubble kernel ran 1.0 % and the fugacity state kernel
// 1.9 % slower (profiles/pcsaft_mix_set_ab.json).  A further entry calls one of the two; it does not copy them again.
__device__ bool mix_lnf_at(const MixRef& m, const double* xin, double T, double rn, Mix& c, double* lnf) {
  if (!(rn > 0.0) || !(rn * c.c3 < 1.0)) return false;
  const Mix::Eval e = c.eval_rho(rn);  // Z from the second-order dual in rho; leaves the converged X_A in c.xa
  if (!e.ok || !isfinite(e.a) || !isfinite(e.z)) return false;
  MixT<GX> g;
  if (!g.init(m, xin, T)) return false;
  GX xaG[NC_MAX];
  for (int i = 0; i < NC_MAX; ++i) xaG[i] = GX(1.0);
  if (c.assoc && !mix_sites_grad(c, g, rn, xaG)) return false;
  const GX a = g.a_res(GX(rn), xaG);
  double sum = 0.0;
  for (int s = 0; s < m.nc; ++s)
    if (m.comp[s] != -1) sum += xin[s];
  double xs = 0.0;
  int k = 0;
  for (int s = 0; s < m.nc; ++s)
    if (m.comp[s] != -1) xs += xin[s] / sum * a.g[k++];
  const double base = a.v + (e.z - 1.0) - xs;
  k = 0;
  bool fin = true;
  for (int s = 0; s < m.nc; ++s)
    if (m.comp[s] != -1) {
      lnf[k] = base + a.g[k] + ::log(rn * (xin[s] / sum));
      fin = fin && isfinite(lnf[k]);
      ++k;
    }
  return fin;
}

// f = rho exp(mu^res/kT) [1/angstrom^3] of the component in slot s of m alone at its liquid root at zero pressure; 0.0
// where it has none (the acceptance test of the bubble start: a root below the lowest step of the density scan is the
// dilute gas).  c is scratch.  One component: mu^res/kT = a + Z - 1.  The Raoult's-law start of the dew kernels
// (gnx_pcsaft_mix_dew.hip at given T, gnx_pcsaft_mix_tvle.hip at given P).
__device__ double dew_raoult(const MixRef& m, int s, double T, Mix& c) {
  const double one = 1.0;
  if (!c.init(MixRef{m.params, m.B, m.comp + s, nullptr, nullptr, 1}, &one, T)) return 0.0;
  double el;
  if (density_root(c, 0.0, el) != ST_OK || !(el >= kEtaMax / kScanDensity)) return 0.0;
  const double rn = number_density(molar_density(el, c.c3));
  const Mix::Eval e = c.eval_rho(rn);
  const double f = rn * ::exp(e.a + e.z - 1.0);
  return e.ok && isfinite(f) && f > 0.0 ? f : 0.0;
}

}  // namespace
