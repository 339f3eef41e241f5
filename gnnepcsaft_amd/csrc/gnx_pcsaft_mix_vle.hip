// Mixture PC-SAFT bubble point in fp64: at (T, x) the pressure P at which the liquid x is in equilibrium with a first
// bubble of vapour, that vapour's composition y and both densities, on the model of gnx_pcsaft_mix.hpp (ref:
// pcsaft/pcsaft_feos.py mix_vp_feos, the bubble half, and mix_vle_pxy_diagram_feos; [3P] feos 0.8
// PhaseEquilibrium.bubble_point / PhaseDiagram.binary_vle).  DESIGN.md §4c.
//
// Equilibrium in the form without ln Z: with ln f_i = mu_i^res/kT + ln(rho x_i), rho the number density of the phase,
//   ln f_i^L(T, rho_L, x) = ln f_i^V(T, rho_V, y) for every component,  p(T, rho_L, x) = p(T, rho_V, y) = P.
// ln phi_i = ln f_i - ln(x_i p/kT) carries -ln Z, and Z of a liquid at 0.4 Pa is 1e-11: written through ln phi the
// equations would lose six digits there.
//
// Successive substitution.  Start: the liquid root at zero pressure, P = kT sum_i f_i^L, y_i = f_i^L kT / P (an ideal
// vapour).  Step: liquid root of x and vapour root of y at P, K_i = (f_i^L/x_i)/(f_i^V/y_i), s = sum_i x_i K_i,
// y <- x K / s, P <- P s; it ends when max(|ln s|, max_i |d ln y_i|) < 1e-10, and what is reported is the state at which
// the fugacities were evaluated, so that the equations hold to that bound at the numbers returned.  The liquid root is
// density_root (the highest root with dp/drho > 0), the vapour root the lowest one, from an upward scan.
//
// One lane per point, no shared memory, no atomics, every loop with a fixed trip cap: same input, same bits.  The
// launch carries no kernel id (GNX_K_NONE): the profiling tables keep their 26 entries and the profiler hook of the
// launch scope is off; time it with events around the call (tools/pcsaft_bench.py --bubble).
#include "gnx_pcsaft_mix_vle.hpp"

namespace {

// bubble point of point i at (T, x)
struct MixBubblePoint {
  const double *T, *x;
  double *P, *y, *rho_l, *rho_v;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix cl, cv;
    const MixRef m = mix_of(set, i);
    const double t = T[i];
    int32_t st = ST_BAD_INPUT;
    double pt = 0.0, rl = 0.0, rv = 0.0, yv[NC_MAX];
    for (int s = 0; s < NC_MAX; ++s) yv[s] = 0.0;
    if (load_mix(m, x, i, t, cl)) {
      st = ST_NO_CONV;
      const double* xin = x + i * m.nc;
      int64_t cm[NC_MAX];
      const MixRef mp = mix_present(m, xin, cm);  // the vapour has the liquid's components and no others
      const int nc = m.nc;
      const int n = cl.n;
      double pprev = 0.0, lnf[2][NC_MAX];
      int damp = 0;
      bool ok = true, conv = false;
      // it = -1 is the start: the liquid at zero pressure under an ideal vapour
      for (int it = -1; ok && !conv && it < kVleMixIters; ++it) {
        const bool start = it < 0;
        double el, ev = 0.0;
        ok = density_root(cl, start ? 0.0 : pt, el) == ST_OK;
        // without a liquid at zero pressure the scan runs out at its lowest step and the root is the dilute gas: the
        // point is too close to the mixture's critical region for this method
        if (ok && start) ok = el >= kEtaMax / kScanDensity;
        if (!ok) break;
        if (!start) {
          ok = cv.init(mp, yv, t) && cv.n == n;
          if (!ok) break;
          const int vr = vapour_root(cv, pt, ev);
          if (vr == VR_NONE && ++damp <= kVleMixDamp) {
            pt = 0.5 * (pt + pprev);  // no vapour of y at this pressure: half the step back
            continue;
          }
          ok = vr == VR_OK;
          if (!ok) break;
          damp = 0;
        }
        // at the densities reported, converted as the state forms convert them
        rl = molar_density(el, cl.c3);
        rv = start ? 0.0 : molar_density(ev, cv.c3);
        for (int ph = 0; ok && ph < (start ? 1 : 2); ++ph)
          ok = mix_lnf_at(mp, ph ? yv : xin, t, number_density(ph ? rv : rl), ph ? cv : cl, lnf[ph]);
        if (!ok) break;
        double xk[NC_MAX], s = 0.0;  // x_i K_i = y_i f_i^L / f_i^V; at the start f_i^L itself
        for (int q = 0, k = 0; q < nc; ++q)
          if (cm[q] != -1) {
            xk[k] = start ? ::exp(lnf[0][k]) : yv[q] * ::exp(lnf[0][k] - lnf[1][k]);
            s += xk[k++];
          }
        ok = s > 0.0 && isfinite(s);
        if (!ok) break;
        if (!start) {
          const double ls = ::log(s);
          double res = ::fabs(ls);
          for (int k = 0; k < n; ++k) res = ::fmax(res, ::fabs(lnf[0][k] - lnf[1][k] - ls));
          ok = res == res;
          conv = res < kVleMixTol;
          if (conv || !ok) break;
        }
        int k = 0;
        for (int q = 0; q < nc; ++q)
          if (cm[q] != -1) {
            yv[q] = xk[k++] / s;
            ok = ok && yv[q] > 0.0;
          }
        pprev = start ? 0.0 : pt;
        pt = start ? s : pt * s;
        ok = ok && pt > 0.0 && isfinite(pt);
      }
      // equal densities: the trivial solution, both phases the same fluid
      if (ok && conv && rv > 0.0 && rl - rv > kVleTrivial * rl) st = ST_OK;
    }
    const bool good = st == ST_OK;
    P[i] = good ? pt * cl.kT_pa : 0.0;
    if (rho_l) rho_l[i] = good ? rl : 0.0;
    if (rho_v) rho_v[i] = good ? rv : 0.0;
    store_row(y, i, m, good, yv);
    status[i] = st;
  }
};

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_bubble(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                         const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                         const int64_t* owner, const double* T, const double* x, int64_t n, double* P,
                                         double* y, double* rho_l, double* rho_v, int32_t* status) {
  // no kernel id of its own: under GNX_K_NONE the scope stays off and the launch is a plain one
  return mix_launch(h, "gnx_pcsaft_mix_bubble", GNX_K_NONE, 44.0 + 16.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n, T && x && P && y && status,
                    MixBubblePoint{T, x, P, y, rho_l, rho_v, status});
}
