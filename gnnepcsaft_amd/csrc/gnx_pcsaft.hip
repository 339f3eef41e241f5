// Pure-component PC-SAFT liquid density and vapour pressure in fp64 (ref: train/utils.py:238-300 rho_batch / vp_batch
// -> pcsaft/pcsaft_feos.py:349-436 pure_den_feos / pure_vp_feos; [3P] feos 0.8 State(..., density_initialization=
// "liquid") and PhaseEquilibrium.pure), the residual enthalpy and entropy of both saturated phases and the critical
// point (ref: pcsaft/pcsaft_feos.py pure_h_lv_feos / pure_s_lv_feos / critical_points_feos / phase_diagram_feos).
//
// Model.  Reduced residual Helmholtz energy per molecule a(T, rho), rho in 1/angstrom^3, of a parameter
// row [m, sigma, eps/k, kappa_ab, eps_ab/k, mu, na, nb, mw]:
//   hard chain   m (4 eta - 3 eta^2) / (1 - eta)^2 - (m - 1) ln g_hs      (BMCSL for one component = Carnahan-Starling)
//   dispersion   -2 pi rho I1 m^2 (eps/kT) sigma^3 - pi rho m C1 I2 m^2 (eps/kT)^2 sigma^3      (Gross & Sadowski 2001)
//   association  na (ln XA - XA/2 + 1/2) + nb (ln XB - XB/2 + 1/2), A-B bonding only, XA/XB in closed form (Wertheim)
//   dipole       A2 / (1 - A3 / A2)                                                               (Gross & Vrabec 2006)
// with d = sigma (1 - 0.12 exp(-3 eps/kT)) and eta = (pi/6) rho m d^3.
//
// a is written once, as a template over its number type, and evaluated on a second-order forward dual in rho
// (value, d/drho, d2/drho2): Z = 1 + rho a', p/kT = rho Z, d(p/kT)/drho = 1 + 2 rho a' + rho^2 a''.  Both solvers work
// in the packing fraction eta (rho = eta / (pi/6 m d^3)) and in the reduced pressure p~ = p / kT (1/angstrom^3).  The
// root of p~(eta) = p~, the status codes, the solver constants and the unit changes are gnx_pcsaft_solve.hpp's, shared
// with the mixture kernels.  The temperature derivative a_T comes from the same template on a first-order dual seeded in
// T (PureT<DG<1>>), p_rho and p_rhorho of the critical-point conditions from a third-order dual in rho (D3).
//
// One lane per state point; a lane loads its parameter row through owner[i].  Every loop has a fixed trip cap; a point
// that runs into one reports a status != 0 and the value 0.0.  No atomics: same input, same bits.
#include "gnx_common.hpp"
#include "gnx_pcsaft_consts.hpp"
#include "gnx_pcsaft_dual.hpp"
#include "gnx_pcsaft_solve.hpp"

#include <cmath>

namespace {

constexpr int kScanLog = 64;        // spinodal scan: 64 log-spaced points in [1e-10, 1e-2] ...
constexpr int kScanLin = 512;       // ... then 512 linear points in (1e-2, kEtaMax]
constexpr int kBisectIters = 60;    // spinodal refinement
constexpr int kSuccIters = 100;     // successive substitution p <- p phi_L / phi_V
constexpr int kNewtonIters = 50;    // Newton on (eta_L, eta_V)
// relative Newton step that ends the VLE solve: quadratic convergence leaves an error far below it after that step,
// while a tighter bound can sit under the rounding noise of g_L for long chains (m ~ 10: |dg| ~ 1e-13)
constexpr double kVleTol = 1e-10;

// ---- one component at one temperature: everything that does not depend on rho --------------------------------------
// S is the number type of T and of every coefficient that depends on it: double in the solvers (Pure), DG<1> seeded in T
// where d/dT of a_res at constant rho is wanted (a_res then takes rho as a constant DG<1>).
template <typename S>
struct PureT {
  double m, sig3, na, nb;
  S eps_t;
  S eta_per_rho;                // pi/6 m d^3
  double ai[7], bi[7];          // a_i(m), b_i(m) of the dispersion integrals
  S m2es3, m2e2s3;              // m^2 (eps/kT) sigma^3, m^2 (eps/kT)^2 sigma^3
  bool assoc, polar;
  S delta0;                     // sigma^3 kappa_ab (exp(eps_ab/kT) - 1): Delta = delta0 g_hs
  S j2[5];                      // a_n + b_n eps/kT of the dipole integrals (m capped at 2)
  double j3[5];                 // c_n of the dipole integrals
  S a2c, a3c;                   // A2 = a2c rho J2, A3 = a3c rho^2 J3
  double kT_pa;                 // p [Pa] = p~ [1/angstrom^3] * kT_pa

  __device__ bool init(const double* __restrict__ row, S Ts) {
    const double T = value_of(Ts);
    m = row[0];
    const double sigma = row[1], eps = row[2], kab = row[3], eab = row[4], mu = row[5];
    na = row[6];
    nb = row[7];
    // valid_row's tests with T's among them, written out: behind a helper the chain compiles to other code
    if (!(T > 0.0) || !(m > 0.0) || !(sigma > 0.0) || !(eps > 0.0) || !(kab >= 0.0) || !(eab >= 0.0) ||
        !(mu >= 0.0) || !(na >= 0.0) || !(nb >= 0.0) || !isfinite(T) || !isfinite(m) || !isfinite(sigma) ||
        !isfinite(eps) || !isfinite(kab) || !isfinite(eab) || !isfinite(mu) || !isfinite(na) || !isfinite(nb))
      return false;
    eps_t = eps / Ts;
    const S d = sigma * (1.0 - 0.12 * exp(-3.0 * eps_t));
    sig3 = sigma * sigma * sigma;
    eta_per_rho = kPi / 6.0 * m * d * d * d;
    const double f1 = (m - 1.0) / m, f2 = f1 * (m - 2.0) / m;
    for (int i = 0; i < 7; ++i) {
      ai[i] = kDispA[0][i] + f1 * kDispA[1][i] + f2 * kDispA[2][i];
      bi[i] = kDispB[0][i] + f1 * kDispB[1][i] + f2 * kDispB[2][i];
    }
    m2es3 = m * m * eps_t * sig3;
    m2e2s3 = m2es3 * eps_t;
    assoc = na * nb > 0.0 && kab > 0.0;
    delta0 = sig3 * kab * expm1(eab / Ts);
    polar = mu > 0.0;
    const double mc = m < 2.0 ? m : 2.0;
    const double g1 = (mc - 1.0) / mc, g2 = g1 * (mc - 2.0) / mc;
    for (int n = 0; n < 5; ++n) {
      j2[n] = kDipA[0][n] + g1 * kDipA[1][n] + g2 * kDipA[2][n] +
              (kDipB[0][n] + g1 * kDipB[1][n] + g2 * kDipB[2][n]) * eps_t;
      j3[n] = kDipC[0][n] + g1 * kDipC[1][n] + g2 * kDipC[2][n];
    }
    const double mu2 = mu * mu / (m * eps * sig3) * kDipoleFactor;  // mu*^2
    a2c = -kPi * eps_t * eps_t * sig3 * mu2 * mu2;
    a3c = -4.0 / 3.0 * kPi * kPi * eps_t * eps_t * eps_t * sig3 * sig3 * mu2 * mu2 * mu2;
    kT_pa = kBoltzmann * T * 1e30;
    return true;
  }

  // reduced residual Helmholtz energy per molecule at number density rho [1/angstrom^3]
  template <typename R>
  __device__ R a_res(R rho) const {
    const R eta = rho * eta_per_rho;
    const R om = 1.0 - eta;
    const R om2 = om * om;
    const R ghs = 1.0 / om + 1.5 * eta / om2 + 0.5 * eta * eta / (om2 * om);
    const R ahc = m * (eta * (4.0 - 3.0 * eta)) / om2 - (m - 1.0) * log(ghs);
    R i1 = ai[6] + 0.0 * eta, i2 = bi[6] + 0.0 * eta;
    for (int i = 5; i >= 0; --i) {
      i1 = i1 * eta + ai[i];
      i2 = i2 * eta + bi[i];
    }
    const R eta2 = eta * eta;
    const R tw = om * (2.0 - eta);
    const R c1 = 1.0 / (1.0 + m * (8.0 * eta - 2.0 * eta2) / (om2 * om2) +
                        (1.0 - m) * (20.0 * eta - 27.0 * eta2 + 12.0 * eta2 * eta - 2.0 * eta2 * eta2) / (tw * tw));
    R a = ahc - 2.0 * kPi * m2es3 * (rho * i1) - kPi * m * m2e2s3 * (rho * c1 * i2);
    if (assoc) {
      const R x = rho * delta0 * ghs;  // rho Delta
      const R xa = site_fraction(1.0 + (nb - na) * x, na * x);
      const R xb = site_fraction(1.0 + (na - nb) * x, nb * x);
      a = a + na * (log(xa) - 0.5 * xa + 0.5) + nb * (log(xb) - 0.5 * xb + 0.5);
    }
    if (polar) {
      R jj2 = j2[4] + 0.0 * eta, jj3 = j3[4] + 0.0 * eta;
      for (int n = 3; n >= 0; --n) {
        jj2 = jj2 * eta + j2[n];
        jj3 = jj3 * eta + j3[n];
      }
      const R A2 = a2c * rho * jj2;
      const R A3 = a3c * rho * rho * jj3;
      a = a + A2 / (1.0 - A3 / A2);
    }
    return a;
  }

  struct Eval {
    double p;      // p / kT [1/angstrom^3]
    double dp;     // d(p/kT)/d eta
    double g;      // mu / kT up to a function of T: ln rho + a + Z - 1 (= ln phi + ln p~)
    static constexpr bool ok = true;  // closed-form site fractions: the evaluation cannot fail
  };
  __device__ Eval eval(double eta) const {
    const double rho = eta / eta_per_rho;
    const D2 a = a_res(D2{rho, 1.0, 0.0});
    const double z = 1.0 + rho * a.d;
    Eval e;
    e.p = rho * z;
    e.dp = (1.0 + 2.0 * rho * a.d + rho * rho * a.dd) / eta_per_rho;
    e.g = ::log(rho) + a.v + z - 1.0;
    return e;
  }
};
using Pure = PureT<double>;

__device__ __forceinline__ bool load_row(const double* __restrict__ params, int64_t B, const int64_t* __restrict__ owner,
                                         int64_t i, double T, Pure& c) {
  const int64_t o = owner[i];
  if (o < 0 || o >= B) return false;
  double row[9];
  for (int k = 0; k < 9; ++k) row[k] = params[o * 9 + k];
  return c.init(row, T);
}

// density at (T, P): the highest-density root of p(eta) = P with dp/deta > 0
__global__ void __launch_bounds__(256) k_pcsaft_density(const double* __restrict__ params, int64_t B,
                                                        const int64_t* __restrict__ owner, const double* __restrict__ T,
                                                        const double* __restrict__ P, int64_t n,
                                                        double* __restrict__ rho, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Pure c;
  const double t = T[i], p = P[i];
  int32_t st = ST_BAD_INPUT;
  double out = 0.0;
  if (load_row(params, B, owner, i, t, c) && p > 0.0 && isfinite(p)) {
    st = ST_NO_CONV;
    const double pt = p / c.kT_pa;
    // p~(kEtaMax) > pt, then scan down to the first eta with p~ <= pt: the bracket of the highest crossing.  This is
    // density_root written out: through it the kernel compiled to other, slower code
    double hi = kEtaMax, lo = 0.0;
    if (c.eval(hi).p - pt > 0.0) {
      for (int k = kScanDensity - 1; k >= 1; --k) {
        const double eta = kEtaMax * k / kScanDensity;
        if (c.eval(eta).p - pt <= 0.0) {
          lo = eta;
          break;
        }
        hi = eta;
      }
      double x;
      if (pcsaft_root(c, pt, lo, hi, hi, x) && x > 0.0 && c.eval(x).dp > 0.0) {
        st = ST_OK;
        out = molar_density(x, c.eta_per_rho);
      }
    }
  }
  rho[i] = st == ST_OK ? out : 0.0;
  status[i] = st;
}

__device__ __forceinline__ double spinodal_grid(int k) {
  return k < kScanLog ? 1e-10 * ::pow(1e8, (double)k / kScanLog)
                      : 1e-2 + (kEtaMax - 1e-2) * (double)(k - kScanLog + 1) / kScanLin;
}

// first zero of dp/deta in (a, b] where the sign goes from `from_pos` to its opposite, by bisection
__device__ double bisect_spinodal(const Pure& c, double a, double b, bool from_pos) {
  for (int it = 0; it < kBisectIters; ++it) {
    const double mid = 0.5 * (a + b);
    if ((c.eval(mid).dp > 0.0) == from_pos)
      a = mid;
    else
      b = mid;
  }
  return from_pos ? a : b;  // the end on the stable side
}

// the van der Waals loop of c on the scan: the first grid point kv where dp/deta is <= 0 (vapour spinodal in the cell
// before it), then the first kl where it is > 0 again (liquid spinodal in the cell before it); false if there is none
__device__ __forceinline__ bool spinodal_scan(const Pure& c, int& kv, int& kl) {
  kv = -1;
  kl = -1;
  const int ngrid = kScanLog + kScanLin;
  for (int k = 0; k < ngrid; ++k) {
    const bool pos = c.eval(spinodal_grid(k)).dp > 0.0;
    if (kv < 0 && !pos && k > 0) {
      kv = k;
    } else if (kv >= 0 && pos) {
      kl = k;
      break;
    }
  }
  return kv > 0 && kl > 0;
}

// the phase equilibrium of the component c at its temperature: spinodal scan, successive substitution, Newton.  Returns
// the status of the vapour-pressure entry; on ST_OK ps is p_sat [Pa], el / ev the molar densities [mol/m^3] and xl / xv
// the packing fractions of liquid and vapour.  The one solve of k_pcsaft_vapor_pressure and k_pcsaft_saturation.
__device__ __forceinline__ int32_t saturation_solve(const Pure& c, double& ps, double& el, double& ev, double& xl,
                                                    double& xv) {
  int32_t st;
  {  // the solve as it stood in the kernel, line for line at its old depth
    double evs = 0.0, els = 0.0;
    int kv, kl;
    st = ST_SUPERCRITICAL;
    if (spinodal_scan(c, kv, kl)) {
      st = ST_NO_CONV;
      evs = bisect_spinodal(c, spinodal_grid(kv - 1), spinodal_grid(kv), true);
      els = bisect_spinodal(c, spinodal_grid(kl - 1), spinodal_grid(kl), false);
      const double pvs = c.eval(evs).p, pls = c.eval(els).p;
      const double plo = pls > 0.0 ? pls : 0.0;
      bool ok = pvs > plo && c.eval(kEtaMax).p > pvs;
      // successive substitution from a pressure between the spinodal pressures
      double p = plo > 0.0 ? 0.5 * (plo + pvs) : 0.5 * pvs;
      xl = kEtaMax;
      xv = 0.0;
      for (int it = 0; ok && it < kSuccIters; ++it) {
        ok = pcsaft_root(c, p, els, kEtaMax, xl, xl) &&
             pcsaft_root(c, p, 0.0, evs, xv > 0.0 ? xv : p * c.eta_per_rho, xv);
        if (!ok) break;
        // ln phi_L - ln phi_V at equal pressure = g_L - g_V: the form without ln Z, which is lost to rounding in a
        // liquid far below its normal boiling point (Z_L ~ 1e-19 next to terms of size 1)
        const double step = c.eval(xl).g - c.eval(xv).g;
        if (!isfinite(step)) {
          ok = false;
          break;
        }
        double pn = p * ::exp(step);
        if (pn >= pvs) pn = 0.5 * (p + pvs);
        if (pn <= plo) pn = 0.5 * (p + plo);
        p = pn;
        if (::fabs(step) < 1e-8) break;
      }
      // Newton on (eta_L, eta_V): p~_L = p~_V and g_L = g_V
      bool conv = false;
      if (ok) {
        ok = pcsaft_root(c, p, els, kEtaMax, xl, xl) && pcsaft_root(c, p, 0.0, evs, xv, xv);
      }
      for (int it = 0; ok && it < kNewtonIters; ++it) {
        const Pure::Eval L = c.eval(xl), V = c.eval(xv);
        const double rl = xl / c.eta_per_rho, rv = xv / c.eta_per_rho;
        const double f1 = L.p - V.p, f2 = L.g - V.g;
        const double j11 = L.dp, j12 = -V.dp, j21 = L.dp / rl, j22 = -V.dp / rv;
        const double det = j11 * j22 - j12 * j21;
        if (!isfinite(f1) || !isfinite(f2) || !(det != 0.0) || !isfinite(det)) {
          ok = false;
          break;
        }
        const double dl = -(j22 * f1 - j12 * f2) / det, dv = -(j11 * f2 - j21 * f1) / det;
        double s = 1.0;
        int h = 0;
        while (h < 30 && !(xl + s * dl > els && xl + s * dl < kEtaMax && xv + s * dv > 0.0 && xv + s * dv < evs)) {
          s *= 0.5;
          ++h;
        }
        if (h == 30) {
          ok = false;
          break;
        }
        xl += s * dl;
        xv += s * dv;
        if (s == 1.0 && ::fabs(dl) <= kVleTol * xl && ::fabs(dv) <= kVleTol * xv) {
          conv = true;
          break;
        }
      }
      if (ok && conv) {
        const double pv = c.eval(xv).p;
        if (pv > 0.0 && isfinite(pv)) {
          st = ST_OK;
          ps = pv * c.kT_pa;
          el = molar_density(xl, c.eta_per_rho);
          ev = molar_density(xv, c.eta_per_rho);
        }
      }
    }
  }
  return st;
}

// vapour pressure at T: p_sat with equal p and mu of liquid and vapour
__global__ void __launch_bounds__(256) k_pcsaft_vapor_pressure(const double* __restrict__ params, int64_t B,
                                                               const int64_t* __restrict__ owner,
                                                               const double* __restrict__ T, int64_t n,
                                                               double* __restrict__ psat, double* __restrict__ rho_l,
                                                               double* __restrict__ rho_v, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Pure c;
  const double t = T[i];
  int32_t st = ST_BAD_INPUT;
  double ps = 0.0, el = 0.0, ev = 0.0, xl, xv;
  if (load_row(params, B, owner, i, t, c)) st = saturation_solve(c, ps, el, ev, xl, xv);
  const bool good = st == ST_OK;
  psat[i] = good ? ps : 0.0;
  if (rho_l) rho_l[i] = good ? el : 0.0;
  if (rho_v) rho_v[i] = good ? ev : 0.0;
  status[i] = st;
}

constexpr double kGasConstant = kAvogadro * kBoltzmann;  // J/mol/K

// residual molar enthalpy [J/mol] and entropy [J/mol/K] (at the same T and V) of the phase at packing fraction eta:
// h = R T (-T a_T + Z - 1), s = -R (a + T a_T).  a and a_T come from one evaluation of a_res on the dual seeded in T at
// constant rho (ct), Z from the double model's eval (c); both at the same temperature t.
__device__ void phase_h_s(const Pure& c, const PureT<DG<1>>& ct, double t, double eta, double& h, double& s) {
  const double rho = eta / c.eta_per_rho;
  const DG<1> a = ct.a_res(DG<1>(rho));
  const double z = c.eval(eta).p / rho;
  const double t_at = t * a.g[0];
  h = kGasConstant * t * (z - 1.0 - t_at);
  s = -kGasConstant * (a.v + t_at);
}

// the saturation line at T: the vapour-pressure solve, then h and s of both phases.  Every fp64 output may be NULL.
__global__ void __launch_bounds__(256) k_pcsaft_saturation(const double* __restrict__ params, int64_t B,
                                                           const int64_t* __restrict__ owner,
                                                           const double* __restrict__ T, int64_t n,
                                                           double* __restrict__ psat, double* __restrict__ rho_l,
                                                           double* __restrict__ rho_v, double* __restrict__ h_l,
                                                           double* __restrict__ h_v, double* __restrict__ s_l,
                                                           double* __restrict__ s_v, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double t = T[i];
  const int64_t o = owner[i];
  int32_t st = ST_BAD_INPUT;
  double ps = 0.0, el = 0.0, ev = 0.0, hl = 0.0, hv = 0.0, sl = 0.0, sv = 0.0;
  if (o >= 0 && o < B) {
    double row[9];
    for (int k = 0; k < 9; ++k) row[k] = params[o * 9 + k];
    Pure c;
    if (c.init(row, t)) {
      double xl, xv;
      st = saturation_solve(c, ps, el, ev, xl, xv);
      if (st == ST_OK) {
        PureT<DG<1>> ct;
        ct.init(row, DG<1>::seed(t, 0));
        phase_h_s(c, ct, t, xl, hl, sl);
        phase_h_s(c, ct, t, xv, hv, sv);
        if (!(isfinite(hl) && isfinite(hv) && isfinite(sl) && isfinite(sv))) st = ST_NO_CONV;
      }
    }
  }
  const bool good = st == ST_OK;
  if (psat) psat[i] = good ? ps : 0.0;
  if (rho_l) rho_l[i] = good ? el : 0.0;
  if (rho_v) rho_v[i] = good ? ev : 0.0;
  if (h_l) h_l[i] = good ? hl : 0.0;
  if (h_v) h_v[i] = good ? hv : 0.0;
  if (s_l) s_l[i] = good ? sl : 0.0;
  if (s_v) s_v[i] = good ? sv : 0.0;
  status[i] = st;
}

// ---- critical point ---------------------------------------------------------------------------------------------------
constexpr double kCritStart = 20.0;   // first temperature tried, in eps/k: no fixture or generator row has a loop there
constexpr double kCritStep = 0.9;     // geometric step down until the scan finds a loop ...
constexpr int kCritSteps = 40;        // ... at most this often: down to 20 * 0.9^40 = 0.30 eps/k
constexpr int kCritBisect = 24;       // bisection of T on "the scan finds a loop": bracket 0.1 * 2^-24 wide, relative
constexpr int kCritInner = 40;        // secant in eta on p_rhorho = 0
constexpr int kCritOuter = 30;        // secant in T on p_rho = 0 at that eta
constexpr double kCritTol = 1e-12;    // relative secant step in eta and in T that ends the polish

// d(p/kT)/drho = 1 + 2 rho a' + rho^2 a'' (f1) and rho d2(p/kT)/drho2 = rho (2 a' + 4 rho a'' + rho^2 a''') (f2) at
// packing fraction eta: both dimensionless, both zero at the critical point
__device__ void crit_funcs(const Pure& c, double eta, double& f1, double& f2) {
  const double rho = eta / c.eta_per_rho;
  const D3 a = c.a_res(D3{rho, 1.0, 0.0, 0.0});
  f1 = 1.0 + 2.0 * rho * a.d + rho * rho * a.dd;
  f2 = rho * (2.0 * a.d + 4.0 * rho * a.dd + rho * rho * a.d3);
}

// the inflection of p(eta) at the temperature of c next to x: secant on f2 from x and x (1 + 1e-4).  On success x is the
// root and f1 the slope there.
__device__ bool crit_inflection(const Pure& c, double& x, double& f1) {
  double x0 = x, x1 = x * (1.0 + 1e-4), g0, g1, unused;
  crit_funcs(c, x0, unused, g0);
  crit_funcs(c, x1, f1, g1);
  for (int it = 0; it < kCritInner; ++it) {
    if (!isfinite(g0) || !isfinite(g1)) return false;
    if (g1 == 0.0) {
      x = x1;
      return true;
    }
    if (g1 == g0) return false;
    const double xn = x1 - g1 * (x1 - x0) / (g1 - g0);
    if (!(xn > 0.0 && xn < kEtaMax)) return false;
    const bool done = ::fabs(xn - x1) <= kCritTol * x1;
    x0 = x1;
    g0 = g1;
    x1 = xn;
    crit_funcs(c, x1, f1, g1);
    if (done) {
      x = x1;
      return isfinite(f1);
    }
  }
  return false;
}

// critical point of every parameter row: (dp/drho)_T = (d2p/drho2)_T = 0 on the loop that vanishes last as T rises.
// The bracket comes from above: from kCritStart eps/k, where the scan finds no loop, down in steps of kCritStep until it
// finds one, then bisection of T on "a loop exists".  From the midpoint of the two spinodals at the lower end, nested
// secants: eta on p_rhorho = 0 inside, T on p_rho = 0 outside.
__global__ void __launch_bounds__(256) k_pcsaft_critical_point(const double* __restrict__ params, int64_t B,
                                                               double* __restrict__ Tc, double* __restrict__ Pc,
                                                               double* __restrict__ rho_c, double* __restrict__ h_c,
                                                               double* __restrict__ s_c, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double row[9];
  for (int k = 0; k < 9; ++k) row[k] = params[i * 9 + k];
  int32_t st = ST_BAD_INPUT;
  double tc = 0.0, pc = 0.0, rc = 0.0, hc = 0.0, sc = 0.0;
  Pure c;
  double t_hi = kCritStart * row[2];
  if (c.init(row, t_hi)) {
    st = ST_NO_CONV;
    int kv, kl;
    bool found = false;
    double t_lo = t_hi;
    if (!spinodal_scan(c, kv, kl)) {
      for (int k = 0; k < kCritSteps; ++k) {
        t_lo = t_hi * kCritStep;
        c.init(row, t_lo);
        if (spinodal_scan(c, kv, kl)) {
          found = true;
          break;
        }
        t_hi = t_lo;
      }
    }
    if (found) {
      for (int it = 0; it < kCritBisect; ++it) {
        const double mid = 0.5 * (t_lo + t_hi);
        c.init(row, mid);
        if (spinodal_scan(c, kv, kl))
          t_lo = mid;
        else
          t_hi = mid;
      }
      c.init(row, t_lo);
      found = spinodal_scan(c, kv, kl);
    }
    if (found) {
      const double evs = bisect_spinodal(c, spinodal_grid(kv - 1), spinodal_grid(kv), true);
      const double els = bisect_spinodal(c, spinodal_grid(kl - 1), spinodal_grid(kl), false);
      double x = 0.5 * (evs + els);
      double t0 = t_lo, t1 = t_lo * (1.0 + 1e-4), f0, f1;
      bool ok = crit_inflection(c, x, f0);
      if (ok) {
        c.init(row, t1);
        ok = crit_inflection(c, x, f1);
      }
      bool conv = false;
      for (int it = 0; ok && !conv && it < kCritOuter; ++it) {
        if (f1 == f0) break;
        const double tn = f1 == 0.0 ? t1 : t1 - f1 * (t1 - t0) / (f1 - f0);
        if (!(tn > 0.5 * t_lo && tn < 2.0 * t_lo)) break;  // the bracket is 1e-5 from Tc: a step out of here is lost
        conv = ::fabs(tn - t1) <= kCritTol * t1;
        t0 = t1;
        f0 = f1;
        t1 = tn;
        c.init(row, t1);
        ok = crit_inflection(c, x, f1);
      }
      if (ok && conv) {
        const double p = c.eval(x).p * c.kT_pa;
        const double r = molar_density(x, c.eta_per_rho);
        if (h_c || s_c) {
          PureT<DG<1>> ct;
          ct.init(row, DG<1>::seed(t1, 0));
          phase_h_s(c, ct, t1, x, hc, sc);
        }
        if (p > 0.0 && isfinite(p) && r > 0.0 && isfinite(r) && isfinite(hc) && isfinite(sc)) {
          st = ST_OK;
          tc = t1;
          pc = p;
          rc = r;
        }
      }
    }
  }
  Tc[i] = tc;
  Pc[i] = pc;
  rho_c[i] = rc;
  if (h_c) h_c[i] = st == ST_OK ? hc : 0.0;
  if (s_c) s_c[i] = st == ST_OK ? sc : 0.0;
  status[i] = st;
}

}  // namespace

extern "C" int32_t gnx_pcsaft_density(gnx_handle* h, const double* params, int64_t B, const int64_t* owner,
                                      const double* T, const double* P, int64_t n, double* rho, int32_t* status) {
  GNX_CHECK_ARG(h && n >= 0 && B >= 0, "gnx_pcsaft_density: bad argument");
  if (n == 0) return GNX_OK;
  GNX_CHECK_ARG(params && owner && T && P && rho && status, "gnx_pcsaft_density: NULL argument");
  gnx_prof_scope prof(h, GNX_K_PCSAFT_RHO, 36.0 * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_density, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, params, B, owner,
                   T, P, n, rho, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_pcsaft_vapor_pressure(gnx_handle* h, const double* params, int64_t B, const int64_t* owner,
                                             const double* T, int64_t n, double* psat, double* rho_l, double* rho_v,
                                             int32_t* status) {
  GNX_CHECK_ARG(h && n >= 0 && B >= 0, "gnx_pcsaft_vapor_pressure: bad argument");
  if (n == 0) return GNX_OK;
  GNX_CHECK_ARG(params && owner && T && psat && status, "gnx_pcsaft_vapor_pressure: NULL argument");
  gnx_prof_scope prof(h, GNX_K_PCSAFT_VP, 44.0 * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_vapor_pressure, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, params, B,
                   owner, T, n, psat, rho_l, rho_v, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_pcsaft_saturation(gnx_handle* h, const double* params, int64_t B, const int64_t* owner,
                                         const double* T, int64_t n, double* psat, double* rho_l, double* rho_v,
                                         double* h_l, double* h_v, double* s_l, double* s_v, int32_t* status) {
  GNX_CHECK_ARG(h && n >= 0 && B >= 0, "gnx_pcsaft_saturation: bad argument");
  if (n == 0) return GNX_OK;
  GNX_CHECK_ARG(params && owner && T && status, "gnx_pcsaft_saturation: NULL argument");
  gnx_prof_scope prof(h, GNX_K_NONE, 76.0 * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_saturation, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, params, B, owner,
                   T, n, psat, rho_l, rho_v, h_l, h_v, s_l, s_v, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_pcsaft_critical_point(gnx_handle* h, const double* params, int64_t B, double* Tc, double* Pc,
                                             double* rho_c, double* h_c, double* s_c, int32_t* status) {
  GNX_CHECK_ARG(h && B >= 0, "gnx_pcsaft_critical_point: bad argument");
  if (B == 0) return GNX_OK;
  GNX_CHECK_ARG(params && Tc && Pc && rho_c && status, "gnx_pcsaft_critical_point: NULL argument");
  gnx_prof_scope prof(h, GNX_K_NONE, 100.0 * B, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_critical_point, dim3((unsigned)gnx_cdiv(B, 256)), dim3(256), 0, h->stream, params, B, Tc,
                   Pc, rho_c, h_c, s_c, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}
