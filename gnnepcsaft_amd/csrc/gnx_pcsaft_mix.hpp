// Mixture PC-SAFT for 1 to 4 components in fp64: the model, shared by gnx_pcsaft_mix.hip (state at (T, rho, x), liquid
// density at (T, P, x)) and gnx_pcsaft_mix_phi.hip (fugacity coefficients).  The root and density solve on it are the
// pure code's, from gnx_pcsaft_solve.hpp.
// (ref: demo/utils_binary.py:116-160 binary_test -> pcsaft/pcsaft_feos.py:311-346 mix_den_feos; [3P] feos 0.8
// State(..., molefracs=x, density_initialization="liquid")).
//
// Model.  Reduced residual Helmholtz energy per molecule a(T, rho, x), rho in 1/angstrom^3, of the
// component rows [m, sigma, eps/k, kappa_ab, eps_ab/k, mu, na, nb, mw] of one mixture, with zeta_n = pi/6 rho
// sum_i x_i m_i d_i^n, eta = zeta_3, mbar = sum_i x_i m_i and the pure code's d_i:
//   hard chain   mbar a_hs(BMCSL) - sum_i x_i (m_i - 1) ln g_ii,  g_ij = 1/(1-z3) + d_ij 3 z2/(1-z3)^2 + d_ij^2 2 z2^2/
//                (1-z3)^3,  d_ij = d_i d_j / (d_i + d_j)
//   dispersion   -2 pi rho I1(eta, mbar) sum_ij x_i x_j m_i m_j (eps_ij/T) sigma_ij^3
//                - pi rho mbar C1(eta, mbar) I2(eta, mbar) sum_ij x_i x_j m_i m_j (eps_ij/T)^2 sigma_ij^3,
//                sigma_ij = (sigma_i + sigma_j)/2, eps_ij = sqrt(eps_i eps_j) (1 - k_ij)          (Gross & Sadowski 2001)
//   association  sum_i x_i [na_i (ln XA_i - XA_i/2 + 1/2) + nb_i (ln XB_i - XB_i/2 + 1/2)], A-B bonding only,
//                XA_i = 1 / (1 + rho sum_j x_j nb_j XB_j Delta_ij), XB_i likewise with na_j XA_j,
//                Delta_ij = g_ij sigma_ij^3 kappa_ij (exp(eps_ab,ij/T) - 1)
//   dipole       A2 / (1 - A3 / A2), A2 the double and A3 the triple sum over components       (Gross & Vrabec 2006)
// With one component every term is the pure code's.
//
// Everything that does not depend on rho is folded once per point into a handful of coefficients (Mix::init); a is then
// written once, as a template over its number type, and evaluated on the second-order forward dual in rho of
// gnx_pcsaft_dual.hpp: Z = 1 + rho a', p/kT = rho Z, d(p/kT)/drho = 1 + 2 rho a' + rho^2 a''.  The site fractions have no
// closed form in a mixture.  X_B is eliminated, F(X_A) = X_A - G(X_A) = 0 is solved by Newton's method in real
// arithmetic (damped substitution where a Newton step leaves (0, 1]), and three further Newton steps carried on the dual
// type with the converged Jacobian give dX_A/drho and d2X_A/drho2 exactly (implicit differentiation).
//
// Plumbing, shared by the four translation units of the mixture entries.  An entry packs its eight leading arguments
// into a MixSet and gives mix_launch the functor of its point: one kernel template, k_pcsaft_mix<Point>, one lane per
// state point.  mix_of(set, i) is the one place that goes owner -> mix_comp / mix_kij / mix_eab; everything below the
// kernel takes the MixRef it returns.  The fields of both structs and the arrays of the point functors carry no
// __restrict__, on purpose: state, density, bubble and flash kernels run at the parent's time without it; the two
// fugacity points of gnx_pcsaft_mix_phi.hip keep it with the rest of their old body.
// Components with x_i = 0 (unless init<KEEP>) and slots marked -1 are dropped before anything is computed.  Every loop
// has a fixed trip cap; a point that runs into one reports a status != 0 and the value 0.0.  No atomics, no shared
// memory: same input, same bits.  The fp64 arrays indexed at run time live in scratch; the solve is latency-bound per
// point.
#pragma once

#include "gnx_common.hpp"
#include "gnx_pcsaft_consts.hpp"
#include "gnx_pcsaft_dual.hpp"
#include "gnx_pcsaft_solve.hpp"

#include <cmath>

namespace {

constexpr int NC_MAX = 4;            // components per mixture: every array below has this extent
constexpr int kSiteIters = 100;      // Newton / damped substitution of the site fractions
constexpr double kSiteTol = 1e-12;   // largest Newton step that ends the site-fraction solve (the dual steps polish it)

// The mixtures of one call, as every entry receives them (include/gnx.h): built once in the entry, passed by value to
// the kernel.
struct MixSet {
  const double* params;  // [B, 9] pool of component rows
  int64_t B;
  const int64_t* comp;   // [M, nc] rows of each mixture, -1 = unused slot
  const double* kij;     // [M, nc, nc] or NULL
  const double* eab;     // [M, nc, nc] or NULL
  int64_t M;
  int nc;
  const int64_t* owner;  // [n] mixture of each point
};

// One mixture of the set: comp, kij and eab are its own slices.  comp is NULL where the set has no such mixture.
struct MixRef {
  const double* params;
  int64_t B;
  const int64_t* comp;
  const double* kij;
  const double* eab;
  int nc;
};

// the mixture of point i: the one place that checks owner[i] and slices the set's tables
__device__ __forceinline__ MixRef mix_of(const MixSet& set, int64_t i) {
  const int64_t o = set.owner[i];
  const int nc = set.nc;
  MixRef m{set.params, set.B, nullptr, nullptr, nullptr, nc};
  if (o >= 0 && o < set.M) {
    const int64_t sq = o * nc * nc;
    m.comp = set.comp + o * nc;
    m.kij = set.kij ? set.kij + sq : nullptr;
    m.eab = set.eab ? set.eab + sq : nullptr;
  }
  return m;
}

// J y = r for up to NC_MAX unknowns and NR right-hand sides, by elimination with partial pivoting; r is overwritten by y
template <int NR>
__device__ bool solve_small(double J[NC_MAX][NC_MAX], double r[NC_MAX][NR], int n) {
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int i = c + 1; i < n; ++i)
      if (::fabs(J[i][c]) > ::fabs(J[piv][c])) piv = i;
    if (!(::fabs(J[piv][c]) > 0.0)) return false;
    if (piv != c) {
      for (int k = 0; k < n; ++k) {
        const double t = J[c][k];
        J[c][k] = J[piv][k];
        J[piv][k] = t;
      }
      for (int k = 0; k < NR; ++k) {
        const double t = r[c][k];
        r[c][k] = r[piv][k];
        r[piv][k] = t;
      }
    }
    for (int i = c + 1; i < n; ++i) {
      const double f = J[i][c] / J[c][c];
      for (int k = c; k < n; ++k) J[i][k] -= f * J[c][k];
      for (int k = 0; k < NR; ++k) r[i][k] -= f * r[c][k];
    }
  }
  for (int c = n - 1; c >= 0; --c)
    for (int k = 0; k < NR; ++k) {
      double s = r[c][k];
      for (int j = c + 1; j < n; ++j) s -= J[c][j] * r[j][k];
      r[c][k] = s / J[c][c];
    }
  return true;
}

// ---- one mixture at one temperature and composition: everything that does not depend on rho ------------------------
// X is the number type of everything that depends on the composition: double for the state and density kernels, the
// gradient dual GX (the x_i as independent variables) for the fugacity kernels.  The density-dependent member templates
// take their own number type R: double or D2 beside X = double, GX beside X = GX.
using GX = DG<NC_MAX>;
template <typename X>
struct MixVar {
  __device__ static X at(double v, int) { return v; }
};
template <>
struct MixVar<GX> {
  __device__ static GX at(double v, int k) { return GX::seed(v, k); }
};

template <typename X>
struct MixT {
  int n;                                  // components present (used slot, x > 0 unless KEEP), compacted to 0 .. n-1
  X xm1[NC_MAX];                          // x_i (m_i - 1)
  X xna[NC_MAX], xnb[NC_MAX];             // x_i na_i, x_i nb_i
  X mbar, c0, c1, c2, c3;                 // zeta_n = c_n rho
  X ai[7], bi[7];                         // a_i(mbar), b_i(mbar) of the dispersion integrals
  X s1, s2;                               // 2 pi sum m^2 eps sigma^3, pi mbar sum m^2 eps^2 sigma^3
  double dij[NC_MAX][NC_MAX];             // d_i d_j / (d_i + d_j)
  bool assoc, polar;
  double delta0[NC_MAX][NC_MAX];          // sigma_ij^3 kappa_ij (exp(eps_ab,ij/T) - 1): Delta_ij = delta0_ij g_ij
  X q2[5], q3[5];                         // A2 = rho sum_n q2_n eta^n, A3 = rho^2 sum_n q3_n eta^n
  double kT_pa;                           // p [Pa] = p~ [1/angstrom^3] * kT_pa
  double xa[NC_MAX];                      // site fractions X_A of the last solve: the start of the next one

  // mr: this point's mixture, its kij / eab read from the upper triangle; xin: the composition of its nc slots.
  // KEEP: a used slot with x = 0 stays in the mixture (infinite dilution) instead of being dropped.
  template <bool KEEP = false>
  __device__ bool init(const MixRef& mr, const double* __restrict__ xin, double T) {
    const int nc = mr.nc;
    if (!(T > 0.0) || !isfinite(T)) return false;
    double sum = 0.0;
    int used = 0;
    for (int s = 0; s < nc; ++s) {
      const int64_t c = mr.comp[s];
      if (c == -1) continue;
      const double xs = xin[s];
      if (c < 0 || c >= mr.B || !(xs >= 0.0) || !isfinite(xs)) return false;
      sum += xs;
      ++used;
    }
    if (used == 0 || !(sum > 0.0) || !isfinite(sum)) return false;
    X x[NC_MAX];
    double m[NC_MAX], sigma[NC_MAX], eps[NC_MAX], kab[NC_MAX], eabv[NC_MAX], mu2[NC_MAX], d[NC_MAX];
    int slot[NC_MAX];
    n = 0;
    for (int s = 0; s < nc; ++s) {
      const int64_t c = mr.comp[s];
      if (c == -1 || (!KEEP && !(xin[s] > 0.0))) continue;
      const double* row = mr.params + c * 9;
      const double mm = row[0], sg = row[1], ep = row[2], ka = row[3], ea = row[4], mu = row[5], a = row[6], b = row[7];
      if (!valid_row(row)) return false;
      const int i = n++;
      slot[i] = s;
      x[i] = MixVar<X>::at(xin[s] / sum, i);
      m[i] = mm;
      sigma[i] = sg;
      eps[i] = ep;
      eabv[i] = ea;
      kab[i] = (ka > 0.0 && a + b > 0.0) ? ka : 0.0;  // kappa = 0 or no sites: does not associate
      mu2[i] = mu * mu / (mm * ep * sg * sg * sg) * kDipoleFactor;  // mu*^2
      d[i] = sg * (1.0 - 0.12 * ::exp(-3.0 * ep / T));
      xm1[i] = x[i] * (mm - 1.0);
      xna[i] = x[i] * a;
      xnb[i] = x[i] * b;
      xa[i] = 1.0;
    }
    mbar = c0 = c1 = c2 = c3 = 0.0;
    for (int i = 0; i < n; ++i) {
      const X xm = x[i] * m[i];
      mbar += xm;
      c1 += xm * d[i];
      c2 += xm * d[i] * d[i];
      c3 += xm * d[i] * d[i] * d[i];
    }
    c0 = kPi / 6.0 * mbar;
    c1 *= kPi / 6.0;
    c2 *= kPi / 6.0;
    c3 *= kPi / 6.0;
    const X f1 = (mbar - 1.0) / mbar, f2 = f1 * (mbar - 2.0) / mbar;
    for (int k = 0; k < 7; ++k) {
      ai[k] = kDispA[0][k] + f1 * kDispA[1][k] + f2 * kDispA[2][k];
      bi[k] = kDispB[0][k] + f1 * kDispB[1][k] + f2 * kDispB[2][k];
    }
    s1 = s2 = 0.0;
    assoc = polar = false;
    for (int k = 0; k < 5; ++k) q2[k] = q3[k] = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const int lo = slot[i] < slot[j] ? slot[i] : slot[j], hi = slot[i] < slot[j] ? slot[j] : slot[i];
        const double k_ij = (mr.kij && i != j) ? mr.kij[lo * nc + hi] : 0.0;
        if (!isfinite(k_ij)) return false;
        const double sij = 0.5 * (sigma[i] + sigma[j]), sij3 = sij * sij * sij;
        const double et = ::sqrt(eps[i] * eps[j]) * (1.0 - k_ij) / T;  // eps_ij / T
        const X w = x[i] * m[i] * x[j] * m[j] * sij3;
        s1 += w * et;
        s2 += w * et * et;
        dij[i][j] = d[i] * d[j] / (d[i] + d[j]);
        delta0[i][j] = 0.0;
        if (kab[i] > 0.0 && kab[j] > 0.0) {
          double e_ab = 0.5 * (eabv[i] + eabv[j]);
          if (mr.eab && i != j) {
            const double given = mr.eab[lo * nc + hi];
            if (given == given) e_ab = given;  // NaN: the combining rule
          }
          if (!isfinite(e_ab)) return false;
          const double r = ::sqrt(sigma[i] * sigma[j]) / sij;
          delta0[i][j] = sij3 * ::sqrt(kab[i] * kab[j]) * r * r * r * ::expm1(e_ab / T);
          assoc = true;
        }
        if (mu2[i] > 0.0 && mu2[j] > 0.0) {
          polar = true;
          const double si3 = sigma[i] * sigma[i] * sigma[i], sj3 = sigma[j] * sigma[j] * sigma[j];
          const double eti = eps[i] / T, etj = eps[j] / T;
          const X w2 = x[i] * x[j] * eti * etj * si3 * sj3 / sij3 * mu2[i] * mu2[j];
          double mc = ::sqrt(m[i] * m[j]);
          mc = mc < 2.0 ? mc : 2.0;
          const double g1 = (mc - 1.0) / mc, g2 = g1 * (mc - 2.0) / mc;
          for (int k = 0; k < 5; ++k)
            q2[k] += w2 * (kDipA[0][k] + g1 * kDipA[1][k] + g2 * kDipA[2][k] +
                           (kDipB[0][k] + g1 * kDipB[1][k] + g2 * kDipB[2][k]) * et);
          for (int l = 0; l < n; ++l) {
            if (!(mu2[l] > 0.0)) continue;
            const double sl3 = sigma[l] * sigma[l] * sigma[l];
            const double sil = 0.5 * (sigma[i] + sigma[l]), sjl = 0.5 * (sigma[j] + sigma[l]);
            const X w3 = x[i] * x[j] * x[l] * eti * etj * (eps[l] / T) * si3 * sj3 * sl3 / (sij * sil * sjl) *
                              mu2[i] * mu2[j] * mu2[l];
            double m3 = ::cbrt(m[i] * m[j] * m[l]);
            m3 = m3 < 2.0 ? m3 : 2.0;
            const double h1 = (m3 - 1.0) / m3, h2 = h1 * (m3 - 2.0) / m3;
            for (int k = 0; k < 5; ++k) q3[k] += w3 * (kDipC[0][k] + h1 * kDipC[1][k] + h2 * kDipC[2][k]);
          }
        }
      }
    s1 *= 2.0 * kPi;
    s2 *= kPi * mbar;
    for (int k = 0; k < 5; ++k) {
      q2[k] *= -kPi;
      q3[k] *= -4.0 / 3.0 * kPi * kPi;
    }
    kT_pa = kBoltzmann * T * 1e30;
    if (KEEP && polar) {
      // A2 and A3 are of second and third order in the x of the polar components: with none of them present both
      // vanish with their gradients, and A2 / (1 - A3 / A2) must not be formed
      polar = false;
      for (int i = 0; i < n; ++i) polar = polar || (mu2[i] > 0.0 && value_of(x[i]) > 0.0);
    }
    return true;
  }

  // the three density-dependent pieces of g_ij = g0 + d_ij g1 + d_ij^2 g2
  template <typename R>
  __device__ void contact(R rho, R& g0, R& g1, R& g2) const {
    const R z2 = rho * c2;
    const R om = 1.0 - rho * c3;
    const R om2 = om * om;
    g0 = 1.0 / om;
    g1 = 3.0 * z2 / om2;
    g2 = 2.0 * z2 * z2 / (om2 * om);
  }

  // X_B of every component from X_A (the eliminated half of the mass-action equations)
  template <typename R>
  __device__ void xb_of(R rho, R g0, R g1, R g2, const R* xaR, R* xbR) const {
    for (int i = 0; i < n; ++i) {
      R s = 0.0 * rho;
      for (int k = 0; k < n; ++k)
        if (delta0[i][k] != 0.0 && !is_zero(xna[k]))
          s = s + (xna[k] * delta0[i][k]) * (g0 + dij[i][k] * g1 + (dij[i][k] * dij[i][k]) * g2) * xaR[k];
      xbR[i] = 1.0 / (1.0 + rho * s);
    }
  }

  // G_i(X_A) = 1 / (1 + rho sum_j x_j nb_j Delta_ij X_B,j(X_A))
  template <typename R>
  __device__ void g_of(R rho, R g0, R g1, R g2, const R* xbR, R* gR) const {
    for (int i = 0; i < n; ++i) {
      R s = 0.0 * rho;
      for (int j = 0; j < n; ++j)
        if (delta0[i][j] != 0.0 && !is_zero(xnb[j]))
          s = s + (xnb[j] * delta0[i][j]) * (g0 + dij[i][j] * g1 + (dij[i][j] * dij[i][j]) * g2) * xbR[j];
      gR[i] = 1.0 / (1.0 + rho * s);
    }
  }

  // site fractions X_A at rho with their first and second rho-derivatives; false if the value iteration hits its cap
  __device__ bool sites(double rho, D2* xaD) {
    double g0, g1, g2, xb[NC_MAX], G[NC_MAX], J[NC_MAX][NC_MAX];
    contact(rho, g0, g1, g2);
    bool conv = false;
    for (int it = 0; it < kSiteIters && !conv; ++it) {
      xb_of(rho, g0, g1, g2, xa, xb);
      g_of(rho, g0, g1, g2, xb, G);
      jacobian(rho, g0, g1, g2, xb, G, J);
      double r[NC_MAX][1];
      for (int i = 0; i < n; ++i) r[i][0] = xa[i] - G[i];
      bool newton = solve_small<1>(J, r, n);
      for (int i = 0; newton && i < n; ++i) {
        const double c = xa[i] - r[i][0];
        newton = c > 0.0 && c <= 1.0;
      }
      double step = 0.0;
      for (int i = 0; i < n; ++i) {
        const double c = newton ? xa[i] - r[i][0] : 0.5 * (xa[i] + G[i]);
        step = ::fmax(step, ::fabs(c - xa[i]));
        xa[i] = c;
      }
      if (!(step == step)) return false;
      conv = step <= kSiteTol;
    }
    if (!conv) return false;
    // Newton steps on the dual type with the Jacobian at the solution: the first makes dX/drho exact, the second
    // d2X/drho2; a third takes out what the rounding of a nearly singular Jacobian (strong association) leaves behind
    xb_of(rho, g0, g1, g2, xa, xb);
    g_of(rho, g0, g1, g2, xb, G);
    for (int i = 0; i < n; ++i) xaD[i] = D2{xa[i], 0.0, 0.0};
    const D2 rhoD{rho, 1.0, 0.0};
    D2 h0, h1, h2, xbD[NC_MAX], GD[NC_MAX];
    contact(rhoD, h0, h1, h2);
    for (int pass = 0; pass < 3; ++pass) {
      jacobian(rho, g0, g1, g2, xb, G, J);
      xb_of(rhoD, h0, h1, h2, xaD, xbD);
      g_of(rhoD, h0, h1, h2, xbD, GD);
      double r[NC_MAX][3];
      for (int i = 0; i < n; ++i) {
        const D2 f = xaD[i] - GD[i];
        r[i][0] = f.v;
        r[i][1] = f.d;
        r[i][2] = f.dd;
      }
      if (!solve_small<3>(J, r, n)) return false;
      for (int i = 0; i < n; ++i) xaD[i] = xaD[i] - D2{r[i][0], r[i][1], r[i][2]};
    }
    for (int i = 0; i < n; ++i) {
      if (!(xaD[i].v > 0.0) || !isfinite(xaD[i].d) || !isfinite(xaD[i].dd)) return false;
      xa[i] = xaD[i].v <= 1.0 ? xaD[i].v : 1.0;
    }
    return true;
  }

  // J_ik = delta_ik - dG_i/dXA_k = delta_ik - G_i^2 rho x_k na_k sum_j rho x_j nb_j Delta_ij XB_j^2 Delta_jk
  __device__ void jacobian(double rho, double g0, double g1, double g2, const double* xb, const double* G,
                           double J[NC_MAX][NC_MAX]) const {
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < n; ++k) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) {
          const double dl_ij = delta0[i][j] * (g0 + dij[i][j] * g1 + dij[i][j] * dij[i][j] * g2);
          const double dl_jk = delta0[j][k] * (g0 + dij[j][k] * g1 + dij[j][k] * dij[j][k] * g2);
          s += rho * xnb[j] * dl_ij * xb[j] * xb[j] * dl_jk;
        }
        J[i][k] = (i == k ? 1.0 : 0.0) - G[i] * G[i] * rho * xna[k] * s;
      }
  }

  // reduced residual Helmholtz energy per molecule at number density rho [1/angstrom^3]; xaR: the site fractions X_A
  template <typename R>
  __device__ R a_res(R rho, const R* xaR) const {
    const R eta = rho * c3;
    const R om = 1.0 - eta;
    const R om2 = om * om;
    R g0, g1, g2;
    contact(rho, g0, g1, g2);
    // BMCSL with the zeta ratios written through c_n: zeta_2^3/zeta_3 = rho^2 c2^3/c3, zeta_2^3/zeta_3^2 = rho c2^3/c3^2
    const X c23 = c2 * c2 * c2;
    const R ahs = (3.0 * c1 * c2 / c0) * (rho / om) + (c23 / (c3 * c0)) * (rho / om2) +
                  (c23 / (c3 * c3 * c0) - 1.0) * log(om);
    R a = mbar * ahs;
    for (int i = 0; i < n; ++i)
      if (!is_zero(xm1[i])) a = a - xm1[i] * log(g0 + dij[i][i] * g1 + (dij[i][i] * dij[i][i]) * g2);
    R i1 = ai[6] + 0.0 * eta, i2 = bi[6] + 0.0 * eta;
    for (int i = 5; i >= 0; --i) {
      i1 = i1 * eta + ai[i];
      i2 = i2 * eta + bi[i];
    }
    const R eta2 = eta * eta;
    const R tw = om * (2.0 - eta);
    const R cc1 = 1.0 / (1.0 + mbar * (8.0 * eta - 2.0 * eta2) / (om2 * om2) +
                         (1.0 - mbar) * (20.0 * eta - 27.0 * eta2 + 12.0 * eta2 * eta - 2.0 * eta2 * eta2) / (tw * tw));
    a = a - s1 * (rho * i1) - s2 * (rho * cc1 * i2);
    if (assoc) {
      R xbR[NC_MAX];
      xb_of(rho, g0, g1, g2, xaR, xbR);
      for (int i = 0; i < n; ++i) {
        if (!is_zero(xna[i])) a = a + xna[i] * (log(xaR[i]) - 0.5 * xaR[i] + 0.5);
        if (!is_zero(xnb[i])) a = a + xnb[i] * (log(xbR[i]) - 0.5 * xbR[i] + 0.5);
      }
    }
    if (polar) {
      R jj2 = q2[4] + 0.0 * eta, jj3 = q3[4] + 0.0 * eta;
      for (int k = 3; k >= 0; --k) {
        jj2 = jj2 * eta + q2[k];
        jj3 = jj3 * eta + q3[k];
      }
      const R A2 = rho * jj2;
      const R A3 = rho * rho * jj3;
      a = a + A2 / (1.0 - A3 / A2);
    }
    return a;
  }

  struct Eval {
    double a;      // a_res
    double z;      // compressibility factor
    double p;      // p / kT [1/angstrom^3]
    double dp;     // d(p/kT)/d rho
    bool ok;       // false: the site fractions did not converge
  };
  __device__ Eval eval_rho(double rho) {
    D2 xaD[NC_MAX];
    for (int i = 0; i < NC_MAX; ++i) xaD[i] = D2{1.0, 0.0, 0.0};
    Eval e;
    e.ok = !assoc || sites(rho, xaD);
    const D2 a = a_res(D2{rho, 1.0, 0.0}, xaD);
    e.a = a.v;
    e.z = 1.0 + rho * a.d;
    e.p = rho * e.z;
    e.dp = 1.0 + 2.0 * rho * a.d + rho * rho * a.dd;
    return e;
  }
  // in the packing fraction: dp becomes d(p/kT)/d eta
  __device__ Eval eval(double eta) {
    Eval e = eval_rho(eta / c3);
    e.dp /= c3;
    return e;
  }
};
using Mix = MixT<double>;

// the mixture of point i folded at (T, row i of x); false: no such mixture, or bad input as init judges it
__device__ __forceinline__ bool load_mix(const MixRef& m, const double* __restrict__ x, int64_t i, double T, Mix& c) {
  return m.comp && c.init(m, x + i * m.nc, T);
}

// m with the slots that are absent (x <= 0) marked unused: cm receives the slots, the result reads them from there
__device__ __forceinline__ MixRef mix_present(const MixRef& m, const double* __restrict__ x, int64_t* cm) {
  for (int s = 0; s < NC_MAX; ++s) cm[s] = (s < m.nc && m.comp[s] != -1 && x[s] > 0.0) ? m.comp[s] : -1;
  MixRef r = m;
  r.comp = cm;
  return r;
}

// row i of an [n, nc] output: v in the used slots of m, NaN in its -1 slots and in the whole row of a point that failed
__device__ __forceinline__ void store_row(double* __restrict__ out, int64_t i, const MixRef& m, bool good,
                                          const double* v) {
  for (int s = 0; s < m.nc; ++s) out[i * m.nc + s] = (good && m.comp[s] != -1) ? v[s] : NAN;
}

// One lane per point: Point holds the arrays of one entry and computes point i of the set in operator()(set, i).
template <typename Point>
__global__ void __launch_bounds__(256) k_pcsaft_mix(MixSet set, int64_t n, Point point) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) point(set, i);
}

// The host path of every mixture entry: argument checks, profiling scope under kernel id `kid` (GNX_K_NONE: none) and
// the launch.  arrays: the entry's own required arrays are all there.
template <typename Point>
int32_t mix_launch(gnx_handle* h, const char* name, int kid, double bytes_per_point, const MixSet& set, int64_t n,
                   bool arrays, const Point& point) {
  GNX_CHECK_ARG(h && n >= 0 && set.B >= 0 && set.M >= 0 && set.nc >= 1 && set.nc <= NC_MAX,
                "%s: bad argument (1 <= nc <= 4)", name);
  if (n == 0) return GNX_OK;
  GNX_CHECK_ARG(arrays && set.owner && (set.params || set.B == 0) && (set.comp || set.M == 0), "%s: NULL argument",
                name);
  gnx_prof_scope prof(h, kid, bytes_per_point * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_mix<Point>, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, set, n, point);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

}  // namespace
