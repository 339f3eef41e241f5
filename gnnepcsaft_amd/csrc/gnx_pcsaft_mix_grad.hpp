// Composition derivatives of the mixture site fractions on the gradient dual, shared by gnx_pcsaft_mix_phi.hip
// (fugacity coefficients) and gnx_pcsaft_mix_vle.hip (bubble point): both need d a / d x_i at fixed T and rho, and with
// association that needs d X_A / d x_k.
#pragma once

#include "gnx_pcsaft_mix.hpp"

namespace {

// Composition derivatives of the site fractions at number density rho: r holds the converged real solution (r.xa, after
// r.eval_rho(rho)), g the same mixture on the gradient dual.  Newton steps on the dual type with the real Jacobian of the
// solution: the first makes dX_A/dx_k exact, the second takes out what the rounding of a nearly singular Jacobian leaves.
__device__ bool mix_sites_grad(const Mix& r, const MixT<GX>& g, double rho, GX* xaG) {
  const int n = r.n;
  double g0, g1, g2, xb[NC_MAX], G[NC_MAX], J[NC_MAX][NC_MAX];
  r.contact(rho, g0, g1, g2);
  r.xb_of(rho, g0, g1, g2, r.xa, xb);
  r.g_of(rho, g0, g1, g2, xb, G);
  for (int i = 0; i < n; ++i) xaG[i] = GX(r.xa[i]);
  const GX rhoG(rho);
  GX h0, h1, h2, xbG[NC_MAX], GG[NC_MAX];
  g.contact(rhoG, h0, h1, h2);
  for (int pass = 0; pass < 2; ++pass) {
    r.jacobian(rho, g0, g1, g2, xb, G, J);
    g.xb_of(rhoG, h0, h1, h2, xaG, xbG);
    g.g_of(rhoG, h0, h1, h2, xbG, GG);
    double rr[NC_MAX][1 + NC_MAX];
    for (int i = 0; i < n; ++i) {
      const GX f = xaG[i] - GG[i];
      rr[i][0] = f.v;
      for (int k = 0; k < NC_MAX; ++k) rr[i][1 + k] = f.g[k];
    }
    if (!solve_small<1 + NC_MAX>(J, rr, n)) return false;
    for (int i = 0; i < n; ++i) {
      xaG[i].v -= rr[i][0];
      for (int k = 0; k < NC_MAX; ++k) xaG[i].g[k] -= rr[i][1 + k];
    }
  }
  for (int i = 0; i < n; ++i) {
    if (!(xaG[i].v > 0.0)) return false;
    for (int k = 0; k < NC_MAX; ++k)
      if (!isfinite(xaG[i].g[k])) return false;
  }
  return true;
}

}  // namespace
