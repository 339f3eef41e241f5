// The state of a composition at (T, P) by the rule of the tangent-plane stability test (gnx_pcsaft_mix_stab.hip, feos's
// density_initialization=None): of its highest liquid root and its lowest vapour root the one with the lower g = sum_i
// x_i ln f_i.  For the units that must agree with that test about what a phase is: the liquid-liquid flash
// (gnx_pcsaft_mix_lle.hip) starts from the test's w and splits the feed into two such states.  DESIGN.md §4c.
#pragma once

#include "gnx_pcsaft_mix_vle.hpp"

namespace {

constexpr double kStabNear = 0.05;  // half width, relative, of the bracket around the previous step's root

// root of p~(eta) = pt with dp/deta > 0 within kStabNear of e0, the root of the previous step; false: the bracket does
// not hold it with a rising p~ at both ends, or the root solve failed, and the caller scans.
__device__ bool stab_root_near(Mix& c, double pt, double e0, double& out) {
  const double lo = e0 * (1.0 - kStabNear), hi = ::fmin(e0 * (1.0 + kStabNear), kEtaMax);
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

// The state at (T, pt) of the composition xin (one value per slot of mp, every used slot > 0; xc: the same, normalised,
// in compact order): c folded at xin, then of the liquid root and the lowest vapour root the one with the lower g = sum
// x ln f.  rho: its molar density, lnf: its ln f in compact order.  false: no root, or an evaluation failed.
// prev: the packing fractions of both roots at the last call, 0.0 for one that was not there; updated.  near (in): take
// the roots to be where they were, each within kStabNear of its place and none where none was, and scan only if one of
// those brackets does not hold; (out): the roots were found that way, and no scan has confirmed them.
__device__ bool stab_state(const MixRef& mp, const double* xin, const double* xc, int n, double T, double pt, Mix& c,
                           double& rho, double* lnf, double* prev, bool& near) {
  if (!c.init(mp, xin, T) || c.n != n) return false;
  double eta[2] = {0.0, 0.0}, best = 0.0;
  bool has[2] = {prev[0] > 0.0, prev[1] > 0.0}, found = false;
  for (int ph = 0; near && ph < 2; ++ph) near = !has[ph] || stab_root_near(c, pt, prev[ph], eta[ph]);
  if (!near) {
    has[0] = density_root(c, pt, eta[0]) == ST_OK;
    const int vr = vapour_root(c, pt, eta[1]);
    if (vr == VR_FAIL) return false;
    has[1] = vr == VR_OK;
  }
  for (int ph = 0; ph < 2; ++ph) prev[ph] = has[ph] ? eta[ph] : 0.0;
  for (int ph = 0; ph < 2; ++ph) {  // the liquid root first: it stays on a tie
    if (!has[ph]) continue;
    double l[NC_MAX], g = 0.0;
    const double r = molar_density(eta[ph], c.c3);
    if (!mix_lnf_at(mp, xin, T, number_density(r), c, l)) continue;
    for (int k = 0; k < n; ++k) g += xc[k] * l[k];
    if (found && !(g < best)) continue;
    found = true;
    best = g;
    rho = r;
    for (int k = 0; k < n; ++k) lnf[k] = l[k];
  }
  return found;
}

}  // namespace
