// Mixture PC-SAFT isothermal two-phase flash in fp64: at (T, P) the split of the feed z into a liquid x and a vapour y,
// the vapour mole fraction beta and both densities, on the model of gnx_pcsaft_mix.hpp (ref: pcsaft/pcsaft_feos.py
// mix_tp_flash_feos, and what pcsaft/kij.py and pcsaft/phase_equilibria.py loop over it; [3P] feos 0.8
// PhaseEquilibrium.tp_flash).  DESIGN.md §4c.
//
// Equations, in the bubble kernel's form without ln Z (gnx_pcsaft_mix_vle.hip): with ln f_i = mu_i^res/kT + ln(rho x_i),
//   ln f_i^L(T, rho_L, x) = ln f_i^V(T, rho_V, y),  p(T, rho_L, x) = p(T, rho_V, y) = P,  z_i = (1 - beta) x_i + beta y_i.
//
// Successive substitution on ln K.  Start: the liquid root of z at zero pressure under an ideal vapour, K_i = f_i^L kT /
// (z_i P) (the bubble kernel's start); where z has no liquid at zero pressure, its highest root at P instead.  Step:
// Rachford-Rice for beta on the negative-flash window (1 / (1 - K_max), 1 / (1 - K_min)), x = z / (1 + beta (K - 1)), y = K
// x, liquid root of x and lowest vapour root of y at P, ln K_i += ln f_i^L - ln f_i^V.  It ends when max_i |ln f_i^L -
// ln f_i^V| < 1e-10, and what is reported is the state at which the fugacities were evaluated: the equations hold to
// that bound at the numbers returned, and the material balance by construction.  No split (ST_SINGLE_PHASE): one
// component, an empty window (no K above 1 or none below), convergence with beta outside [0, 1], or onto equal phases.
//
// The two scans of a step cost some 600 to 1100 evaluations of the pressure, the roots themselves about ten.  Once a step
// has moved ln K by less than 0.05, the next one looks for both roots within 5 % of the previous ones first and scans only
// if a bracket there does not hold; a point that converges on such roots is accepted only after the scans have found
// the same roots at that state, and goes on with scans alone otherwise.
//
// One lane per point, no shared memory, no atomics, every loop with a fixed trip cap: same input, same bits.  Like the
// bubble launch this one carries no kernel id (GNX_K_NONE); time it with events around the call
// (tools/pcsaft_bench.py --flash).
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

// flash of point i at (T, P, z)
struct MixFlashPoint {
  const double *T, *P, *z;
  double *beta, *x, *y, *rho_l, *rho_v;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix cl, cv;
    const MixRef m = mix_of(set, i);
    const double t = T[i], p = P[i];
    int32_t st = ST_BAD_INPUT;
    double bt = 0.0, rl = 0.0, rv = 0.0, xv[NC_MAX], yv[NC_MAX];
    for (int s = 0; s < NC_MAX; ++s) xv[s] = yv[s] = 0.0;
    if (isfinite(p) && p > 0.0 && load_mix(m, z, i, t, cl)) {
      st = ST_NO_CONV;
      const double* zin = z + i * m.nc;
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
    const bool good = st == ST_OK;
    beta[i] = good ? bt : 0.0;
    if (rho_l) rho_l[i] = good ? rl : 0.0;
    if (rho_v) rho_v[i] = good ? rv : 0.0;
    store_row(x, i, m, good, xv);
    store_row(y, i, m, good, yv);
    status[i] = st;
  }
};

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_flash(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                        const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                        const int64_t* owner, const double* T, const double* P, const double* z, int64_t n,
                                        double* beta, double* x, double* y, double* rho_l, double* rho_v,
                                        int32_t* status) {
  // no kernel id of its own: under GNX_K_NONE the scope stays off and the launch is a plain one
  return mix_launch(h, "gnx_pcsaft_mix_flash", GNX_K_NONE, 52.0 + 24.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n,
                    T && P && z && beta && x && y && status, MixFlashPoint{T, P, z, beta, x, y, rho_l, rho_v, status});
}
