// Mixture PC-SAFT bubble and dew temperatures in fp64: at (P, x) the temperature T at which the liquid x starts to boil
// and the vapour y that forms, at (P, y) the temperature at which the vapour y starts to condense and the liquid x that
// forms, with both densities, on the model of gnx_pcsaft_mix.hpp (ref: pcsaft/pcsaft_feos.py mix_vle_diagram_feos;
// [3P] feos 0.8 PhaseEquilibrium.bubble_point / dew_point at given pressure, PhaseDiagram.binary_vle).  DESIGN.md §4c.
//
// The equations are those of the pressure kernels (gnx_pcsaft_mix_vle.hip, gnx_pcsaft_mix_dew.hip), in the form
// without ln Z:
//   ln f_i^L(T, rho_L, x) = ln f_i^V(T, rho_V, y) for every component present,  p(T, rho_L, x) = p(T, rho_V, y) = P,
// with P given and T looked for.  z is the given composition (x of the bubble, y of the dew point), w the one looked for.
//
// Start, where the caller gives no T0: T = 0.7 sum_i z_i eps_i (0.85 + 0.42 m_i), then a secant in u = 1/T on
// g = ln(P_est(T) / P) until |g| < 1e-2.  P_est is the start of the pressure kernel: kT sum_i f_i of the liquid z at
// zero pressure under an ideal vapour (bubble), 1 / sum_i (y_i / k_i) from Raoult's law on each component's own liquid
// at zero pressure (dew, dew_raoult).  ln P is close to linear in 1/T (Clausius-Clapeyron); the first slope is
// dg/du = -10 T (Trouton's rule), a secant slope is taken only where it lies in -[0.25, 40] T, a step is held to
// u_new / u in [0.8, 1.25], and without a liquid at zero pressure at the trial T the search restarts from 0.85 T.  The
// estimate at the last T is also the first w.  With a T0 the estimate is taken there (at 0.85^k T0 where T0 has no such
// liquid) for its w alone.
//
// Loop, at (T, P): liquid root of x and vapour root of y, both mixtures folded again since T moves; d_i = ln f_i^L -
// ln f_i^V (bubble; the dew point the other way round), w'_i = w_i exp(d_i), s = sum_i w'_i; it ends when
// max(|ln s|, max_i |d_i - ln s|) < 1e-10, and what is reported is the state at which the fugacities were evaluated.
// Else w <- w' / s and one secant step in u on ln s, which is ln(P_bubble(T) / P) (bubble) or ln(P / P_dew(T)) (dew) to
// first order: first slope -+10 T, secant slopes only within -+[0.25, 40] T, a step held to u_new / u in [0.9, 1.1].
// Without a vapour root of y at (T, P) the step is halved back towards the u before it.  A dew point need not be
// unique: the one reported is the one the start leads to.
//
// This file is a translation unit of its own so that the pressure kernels compile to the instructions they had before.
// One lane per point, no shared memory, no atomics, every loop with a fixed trip cap: same input, same bits.  The
// launches carry no kernel id (GNX_K_NONE); time them with events around the call (tools/pcsaft_bench.py --bubble-t,
// --dew-t).
#include "gnx_pcsaft_mix_vle.hpp"

namespace {

constexpr int kTvleStartEvals = 40;     // estimates of the start, restarts included (the oracle needs at most 7)
constexpr double kTvleStartTol = 1e-2;  // |ln(P_est / P)| that ends the start
constexpr int kTvleIters = 400;         // steps of the loop (the oracle: 168 on the dew point of ethanol + water)
constexpr double kTvleTrouton = 10.0;   // |d ln P / d(1/T)| / T of the first step
constexpr double kTvleSlopeMin = 0.25, kTvleSlopeMax = 40.0;  // a secant slope is believed within these, in units of T

// a secant slope sec = dg/du of the sign sgn and a believable size at T
__device__ __forceinline__ bool tvle_slope_ok(double sec, double sgn, double T) {
  const double r = sgn * sec / T;
  return r >= kTvleSlopeMin && r <= kTvleSlopeMax;
}

// P_est / kT [1/angstrom^3] of the given composition zin of mp at T and the first w (slots of mp, normalised) that goes
// with it; false: no liquid at zero pressure at this T.  c is scratch.
template <bool DEW>
__device__ bool tvle_estimate(const MixRef& mp, const double* zin, double T, Mix& c, double& pe, double* w) {
  const int nc = mp.nc;
  double s = 0.0;
  if (DEW) {
    double kr[NC_MAX], kmax = 0.0, zsum = 0.0;
    for (int q = 0; q < nc; ++q) {
      kr[q] = 0.0;
      if (mp.comp[q] == -1) continue;
      zsum += zin[q];
      kr[q] = dew_raoult(mp, q, T, c);
      kmax = ::fmax(kmax, kr[q]);
    }
    if (!(kmax > 0.0)) return false;
    for (int q = 0; q < nc; ++q)
      if (mp.comp[q] != -1) {
        w[q] = zin[q] / zsum / (kr[q] > 0.0 ? kr[q] : 100.0 * kmax);
        s += w[q];
      }
    pe = 1.0 / s;
  } else {
    double el, lnf[NC_MAX];
    if (!c.init(mp, zin, T) || density_root(c, 0.0, el) != ST_OK || !(el >= kEtaMax / kScanDensity)) return false;
    if (!mix_lnf_at(mp, zin, T, number_density(molar_density(el, c.c3)), c, lnf)) return false;
    for (int q = 0, k = 0; q < nc; ++q)
      if (mp.comp[q] != -1) {
        w[q] = ::exp(lnf[k++]);
        s += w[q];
      }
    pe = s;
  }
  if (!(s > 0.0) || !isfinite(s) || !(pe > 0.0) || !isfinite(pe)) return false;
  bool ok = true;
  for (int q = 0; q < nc; ++q)
    if (mp.comp[q] != -1) {
      w[q] /= s;
      ok = ok && w[q] > 0.0;
    }
  return ok;
}

// bubble (DEW false: z = x, w = y) or dew (DEW true: z = y, w = x) temperature of point i at (P, z)
template <bool DEW>
struct MixTvlePoint {
  const double *P, *z, *T0;
  double *T, *w, *rho_l, *rho_v;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix cl, cv;
    const MixRef m = mix_of(set, i);
    const int nc = m.nc;
    const double p = P[i], t0 = T0 ? T0[i] : NAN;
    const bool given = t0 == t0;
    int32_t st = ST_BAD_INPUT;
    double t = 0.0, rl = 0.0, rv = 0.0, wv[NC_MAX];
    for (int s = 0; s < NC_MAX; ++s) wv[s] = 0.0;
    const double* zin = z + i * nc;
    // the first guess; the rows are read only where the slot names one, and load_mix checks them afterwards
    bool in = m.comp && p > 0.0 && isfinite(p) && (!given || (t0 > 0.0 && isfinite(t0)));
    if (in) {
      double tg = 0.0, zs = 0.0;
      for (int s = 0; s < nc; ++s) {
        const int64_t c = m.comp[s];
        if (c == -1) continue;
        if (c < 0 || c >= m.B) {
          in = false;
          break;
        }
        if (zin[s] > 0.0) {
          const double* row = m.params + c * 9;
          tg += zin[s] * row[2] * (0.85 + 0.42 * row[0]);
          zs += zin[s];
        }
      }
      t = given ? t0 : 0.7 * tg / zs;
      in = in && t > 0.0 && isfinite(t);
    }
    if (in && load_mix(m, z, i, t, cl)) {
      st = ST_NO_CONV;
      int64_t cm[NC_MAX];
      const MixRef mp = mix_present(m, zin, cm);  // both phases have the given one's components and no others
      const int n = cl.n;
      const double sgn = DEW ? 1.0 : -1.0;  // the sign of d ln s / d(1/T) of the loop; the start's is negative
      // ---- the start: T where the estimate meets P, and the w that goes with it
      bool ok = false;
      {
        double te = t, slope = 0.0, uprev = 0.0, gprev = 0.0;
        bool prev = false;
        for (int ev = 0; ev < kTvleStartEvals; ++ev) {
          double pe;
          if (!tvle_estimate<DEW>(mp, zin, te, cl, pe, wv)) {
            te *= 0.85;
            prev = false;
            ok = te > 0.0;
            if (!ok) break;
            ok = false;
            continue;
          }
          if (given) {
            ok = true;
            break;
          }
          const double g = ::log(pe * (kBoltzmann * te * 1e30) / p);
          if (!(g == g)) break;
          if (::fabs(g) < kTvleStartTol) {
            t = te;
            ok = true;
            break;
          }
          const double u = 1.0 / te;
          if (!prev) {
            slope = -kTvleTrouton * te;
          } else {
            const double sec = (g - gprev) / (u - uprev);
            if (tvle_slope_ok(sec, -1.0, te)) slope = sec;
          }
          const double un = ::fmin(::fmax(u - g / slope, 0.8 * u), 1.25 * u);
          uprev = u;
          gprev = g;
          prev = true;
          te = 1.0 / un;
        }
      }
      // ---- the loop
      double u = 1.0 / t, uprev = 0.0, lsprev = 0.0, slope = 0.0, lnf[2][NC_MAX];
      int damp = 0;
      bool prev = false, conv = false;
      for (int it = 0; ok && !conv && it < kTvleIters; ++it) {
        t = 1.0 / u;
        const double* xl = DEW ? wv : zin;
        const double* yv = DEW ? zin : wv;
        double el, ev;
        ok = cl.init(mp, xl, t) && cl.n == n && cv.init(mp, yv, t) && cv.n == n;
        if (!ok) break;
        const double pt = p / cl.kT_pa;
        ok = density_root(cl, pt, el) == ST_OK;
        if (!ok) break;
        const int vr = vapour_root(cv, pt, ev);
        if (vr == VR_NONE && prev && ++damp <= kVleMixDamp) {
          u = 0.5 * (u + uprev);  // no vapour of y at this temperature: half the step back
          continue;
        }
        ok = vr == VR_OK;
        if (!ok) break;
        damp = 0;
        // at the densities reported, converted as the state forms convert them
        rl = molar_density(el, cl.c3);
        rv = molar_density(ev, cv.c3);
        for (int ph = 0; ok && ph < 2; ++ph)
          ok = mix_lnf_at(mp, ph ? yv : xl, t, number_density(ph ? rv : rl), ph ? cv : cl, lnf[ph]);
        if (!ok) break;
        double d[NC_MAX], wk[NC_MAX], s = 0.0;
        for (int q = 0, k = 0; q < nc; ++q)
          if (cm[q] != -1) {
            d[k] = DEW ? lnf[1][k] - lnf[0][k] : lnf[0][k] - lnf[1][k];
            wk[k] = wv[q] * ::exp(d[k]);
            s += wk[k++];
          }
        ok = s > 0.0 && isfinite(s);
        if (!ok) break;
        const double ls = ::log(s);
        double res = ::fabs(ls);
        for (int k = 0; k < n; ++k) res = ::fmax(res, ::fabs(d[k] - ls));
        ok = res == res;
        conv = res < kVleMixTol;
        if (conv || !ok) break;
        if (!prev) {
          slope = sgn * kTvleTrouton * t;
        } else {
          const double sec = (ls - lsprev) / (u - uprev);
          if (tvle_slope_ok(sec, sgn, t)) slope = sec;
        }
        int k = 0;
        for (int q = 0; q < nc; ++q)
          if (cm[q] != -1) {
            wv[q] = wk[k++] / s;
            ok = ok && wv[q] > 0.0;
          }
        uprev = u;
        lsprev = ls;
        prev = true;
        u = ::fmin(::fmax(u - ls / slope, 0.9 * u), 1.1 * u);
        ok = ok && u > 0.0 && isfinite(u);
      }
      // equal densities: the trivial solution, both phases the same fluid
      if (ok && conv && rv > 0.0 && rl - rv > kVleTrivial * rl) st = ST_OK;
    }
    const bool good = st == ST_OK;
    T[i] = good ? t : 0.0;
    if (rho_l) rho_l[i] = good ? rl : 0.0;
    if (rho_v) rho_v[i] = good ? rv : 0.0;
    if (m.comp)
      store_row(w, i, m, good, wv);
    else
      for (int s = 0; s < nc; ++s) w[i * nc + s] = NAN;
    status[i] = st;
  }
};

template <bool DEW>
int32_t tvle_entry(const char* name, gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                   const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc, const int64_t* owner,
                   const double* P, const double* z, const double* T0, int64_t n, double* T, double* w, double* rho_l,
                   double* rho_v, int32_t* status) {
  // no kernel id of its own: under GNX_K_NONE the scope stays off and the launch is a plain one
  return mix_launch(h, name, GNX_K_NONE, 52.0 + 16.0 * nc, MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner},
                    n, P && z && T && w && status, MixTvlePoint<DEW>{P, z, T0, T, w, rho_l, rho_v, status});
}

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_bubble_t(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                           const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                           const int64_t* owner, const double* P, const double* x, const double* T0,
                                           int64_t n, double* T, double* y, double* rho_l, double* rho_v,
                                           int32_t* status) {
  return tvle_entry<false>("gnx_pcsaft_mix_bubble_t", h, params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, P, x, T0, n,
                           T, y, rho_l, rho_v, status);
}

extern "C" int32_t gnx_pcsaft_mix_dew_t(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                        const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                        const int64_t* owner, const double* P, const double* y, const double* T0,
                                        int64_t n, double* T, double* x, double* rho_l, double* rho_v,
                                        int32_t* status) {
  return tvle_entry<true>("gnx_pcsaft_mix_dew_t", h, params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, P, y, T0, n, T,
                          x, rho_l, rho_v, status);
}
