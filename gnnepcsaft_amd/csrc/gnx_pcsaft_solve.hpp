// The solver core shared by the pure kernels (gnx_pcsaft.hip) and the mixture kernels (gnx_pcsaft_mix.hpp): status codes,
// solver constants, the density unit changes and the safeguarded Newton root of p~(eta) = pt; for the mixture kernels
// also the check of a parameter row and the liquid-density solve, which the pure kernels write out.
//
// A model M (Pure, MixT<double>) offers `M::Eval eval(double eta)` with the members p (p / kT, 1/angstrom^3), dp
// (d(p/kT)/d eta) and ok (false: the evaluation itself failed; a constant true for a model that cannot).
#pragma once

#include "gnx_common.hpp"
#include "gnx_pcsaft_consts.hpp"

#include <cmath>

namespace {

using namespace gnx_pcsaft;

constexpr double kPi = 3.14159265358979323846;
constexpr int kScanDensity = 512;   // downward eta scan of the density solve (step kEtaMax / 512)
constexpr int kRootIters = 200;     // safeguarded Newton of one density at a given pressure
constexpr double kRootTol = 1e-14;  // relative step / bracket width that ends a root solve

// ST_SUPERCRITICAL is reported by the vapour pressure alone; no mixture entry gives it.  ST_SINGLE_PHASE is the flash's:
// no vapour-liquid split at (T, P, z)
enum : int32_t { ST_OK = 0, ST_NO_CONV = 1, ST_SUPERCRITICAL = 2, ST_BAD_INPUT = 3, ST_SINGLE_PHASE = 4 };

// a parameter row [m, sigma, eps/k, kappa_ab, eps_ab/k, mu, na, nb, mw]: m, sigma, eps > 0, the rest >= 0, all finite
__device__ __forceinline__ bool valid_row(const double* __restrict__ row) {
  const double m = row[0], sigma = row[1], eps = row[2], kab = row[3], eab = row[4], mu = row[5], na = row[6], nb = row[7];
  return !(!(m > 0.0) || !(sigma > 0.0) || !(eps > 0.0) || !(kab >= 0.0) || !(eab >= 0.0) || !(mu >= 0.0) ||
           !(na >= 0.0) || !(nb >= 0.0) || !isfinite(m) || !isfinite(sigma) || !isfinite(eps) || !isfinite(kab) ||
           !isfinite(eab) || !isfinite(mu) || !isfinite(na) || !isfinite(nb));
}

// packing fraction -> molar density [mol/m^3], eta_per_rho = eta / rho in angstrom^3; molar -> number density
// [1/angstrom^3].  The order of the operations is part of the results' bits.
__device__ __forceinline__ double molar_density(double eta, double eta_per_rho) {
  return eta / eta_per_rho * 1e30 / kAvogadro;
}
__device__ __forceinline__ double number_density(double rho_molar) { return rho_molar * (kAvogadro * 1e-30); }

// root of p~(eta) = pt in [lo, hi] with p~(lo) <= pt < p~(hi), by Newton from x safeguarded by bisection
template <typename M>
__device__ bool pcsaft_root(M& c, double pt, double lo, double hi, double x, double& out) {
  if (!(x > lo && x < hi)) x = 0.5 * (lo + hi);
  for (int it = 0; it < kRootIters; ++it) {
    const typename M::Eval e = c.eval(x);
    const double f = e.p - pt;
    if (!e.ok || !isfinite(f)) return false;
    if (f > 0.0)
      hi = x;
    else
      lo = x;
    if (f == 0.0) {
      out = x;
      return true;
    }
    double xn = x - f / e.dp;
    if (!(e.dp > 0.0) || !(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
    if (::fabs(xn - x) <= kRootTol * x || hi - lo <= kRootTol * hi) {
      out = xn;
      return true;
    }
    x = xn;
  }
  return false;
}

// packing fraction of the highest-density root of p~(eta) = pt with dp/deta > 0; ST_OK or ST_NO_CONV
template <typename M>
__device__ int32_t density_root(M& c, double pt, double& out) {
  // p~(kEtaMax) > pt, then scan down to the first eta with p~ <= pt: the bracket of the highest crossing
  double hi = kEtaMax, lo = 0.0;
  typename M::Eval e = c.eval(hi);
  bool ok = e.ok && e.p - pt > 0.0;
  for (int k = kScanDensity - 1; ok && k >= 1; --k) {
    const double eta = kEtaMax * k / kScanDensity;
    e = c.eval(eta);
    ok = e.ok;
    if (e.p - pt <= 0.0) {
      lo = eta;
      break;
    }
    hi = eta;
  }
  double xr;
  if (ok && pcsaft_root(c, pt, lo, hi, hi, xr) && xr > 0.0) {
    e = c.eval(xr);
    if (e.ok && e.dp > 0.0) {
      out = xr;
      return ST_OK;
    }
  }
  return ST_NO_CONV;
}

}  // namespace
