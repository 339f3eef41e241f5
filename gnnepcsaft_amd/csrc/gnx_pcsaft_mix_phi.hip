// Mixture PC-SAFT fugacity coefficients in fp64: ln phi_i at (T, rho, x) and at the liquid root of (T, P, x), on the model
// of gnx_pcsaft_mix.hpp (ref: pcsaft/pcsaft_feos.py mix_ln_fugacity_coefficient, mix_ln_fugacity_coefficient_pure; [3P]
// feos 0.8 State.ln_phi / ln_phi_pure_liquid).  DESIGN.md §4c.
//
//   ln phi_i = mu_i^res/kT - ln Z,  mu_i^res/kT = d(N a)/dN_i at fixed T, V = a + (Z - 1) + a_xi - sum_j x_j a_xj
//
// a_xi = da/dx_i at fixed T and rho with the x as independent variables.  The mixture is folded a second time on the
// first-order gradient dual DG<NC_MAX> (MixT<GX>: the x_i seeded as the variables), and a_res, the code the density solve
// evaluates on D2, is evaluated once on it.  The site fractions are converged in real arithmetic by the density code and
// their composition derivatives follow from Newton steps on the dual type with the converged Jacobian.  Z and the root
// come from the density code as it is.  This file is a translation unit of its own so that the state and density
// kernels of gnx_pcsaft_mix.hip compile to the instructions they had before it existed.
//
// One lane per state point, no shared memory, no atomics, every loop with a fixed trip cap: same input, same bits.
#include "gnx_pcsaft_mix_grad.hpp"

namespace {

// ln phi of every slot of mixture m at (T, number density rn, x), NaN in the -1 slots, and Z.  A used slot with x = 0
// stays in the mixture: its ln phi is the value at infinite dilution.  c is scratch: the mixture in real arithmetic.
// Up to its last statements this is mix_lnf_at of gnx_pcsaft_mix_vle.hpp.  Sharing that part is deferred, not done: the
// two forms tried (results through a struct, through references) cost the bubble kernel 1.0 % and the state kernel
// here 1.9 % (profiles/pcsaft_mix_set_ab.json).  A further entry that needs mu_i^res/kT calls one of the two; it does
// not copy them a third time.
//   ln phi_i = a + (Z - 1) + a_xi - sum_j x_j a_xj - ln Z,  a_xi = da/dx_i at fixed T, rho, the x independent
__device__ int32_t mix_lnphi_at(const MixRef& m, const double* __restrict__ xin, double T, double rn, Mix& c,
                                double* lnphi, double& z) {
  if (!c.init<true>(m, xin, T)) return ST_BAD_INPUT;
  if (!(rn * c.c3 < 1.0)) return ST_BAD_INPUT;
  const Mix::Eval e = c.eval_rho(rn);  // Z from the second-order dual in rho; leaves the converged X_A in c.xa
  if (!e.ok || !isfinite(e.a) || !isfinite(e.z)) return ST_NO_CONV;
  z = e.z;
  if (!(e.z > 0.0)) return ST_NO_CONV;  // no ln Z at a negative pressure
  MixT<GX> g;
  if (!g.init<true>(m, xin, T)) return ST_BAD_INPUT;
  GX xaG[NC_MAX];
  for (int i = 0; i < NC_MAX; ++i) xaG[i] = GX(1.0);
  if (c.assoc && !mix_sites_grad(c, g, rn, xaG)) return ST_NO_CONV;
  const GX a = g.a_res(GX(rn), xaG);
  double sum = 0.0;
  for (int s = 0; s < m.nc; ++s)
    if (m.comp[s] != -1) sum += xin[s];
  double xs = 0.0;
  int k = 0;
  for (int s = 0; s < m.nc; ++s)
    if (m.comp[s] != -1) xs += xin[s] / sum * a.g[k++];
  const double base = a.v + (e.z - 1.0) - xs - ::log(e.z);
  bool fin = isfinite(base);
  for (int j = 0; j < k; ++j) fin = fin && isfinite(a.g[j]);
  if (!fin) return ST_NO_CONV;
  k = 0;
  for (int s = 0; s < m.nc; ++s) lnphi[s] = m.comp[s] != -1 ? base + a.g[k++] : NAN;
  return ST_OK;
}

// ln phi of the component in slot s of m alone at its own liquid root at (T, P): a + Z - 1 - ln Z there.  NaN where it
// has none: the highest root with dp/drho > 0 counts as liquid only if p(rho) has a mechanically unstable stretch
// (dp/drho <= 0) below it, looked for on the grid of the density scan; above the critical temperature there is none.
__device__ double mix_lnphi_pure(const MixRef& m, int s, double T, double p, Mix& c) {
  const double one = 1.0;
  if (!c.init(MixRef{m.params, m.B, m.comp + s, nullptr, nullptr, 1}, &one, T)) return NAN;
  double xr;
  if (density_root(c, p / c.kT_pa, xr) != ST_OK) return NAN;
  bool liquid = false;
  for (int k = kScanDensity - 1; k >= 1 && !liquid; --k) {
    const double eta = kEtaMax * k / kScanDensity;
    if (!(eta < xr)) continue;
    const Mix::Eval e = c.eval(eta);
    if (!e.ok) break;
    liquid = e.dp <= 0.0;
  }
  if (!liquid) return NAN;
  // at the density a one-component call would report, converted as the state form converts it
  const Mix::Eval e = c.eval_rho(number_density(molar_density(xr, c.c3)));
  const double v = e.a + e.z - 1.0 - ::log(e.z);
  return e.ok && isfinite(v) ? v : NAN;
}

// The two points below keep the body of their kernels as it was before the plumbing was folded: the arrays
// __restrict__, the mixture's slices taken where they are used instead of held across the density solve, mix_lnphi_at
// writing the NaN of a -1 slot itself and every row stored in its own loop, lnphi_pure slot by slot, instead of through
// store_row.  With the folded body the root form ran 0.5 % to 0.7 % slower than the parent at 10^6 points, with this one
// at the parent's time (profiles/pcsaft_mix_set_ab.json).

// ln phi and Z of point i at (T, rho, x)
struct MixLnphiStatePoint {
  const double *__restrict__ T, *__restrict__ rho, *__restrict__ x;
  double *__restrict__ lnphi, *__restrict__ Z;
  int32_t* __restrict__ status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix c;
    const MixRef m = mix_of(set, i);
    const double t = T[i], r = rho[i];
    int32_t st = ST_BAD_INPUT;
    double row[NC_MAX], z = 0.0;
    if (m.comp && r > 0.0 && isfinite(r)) st = mix_lnphi_at(m, x + i * m.nc, t, number_density(r), c, row, z);
    for (int s = 0; s < m.nc; ++s) lnphi[i * m.nc + s] = st == ST_OK ? row[s] : NAN;
    Z[i] = z;
    status[i] = st;
  }
};

// liquid density of point i at (T, P, x) as MixDensityPoint finds it, ln phi there and, if asked for, ln phi of every
// used slot's component alone at (T, P)
struct MixLnphiPoint {
  const double *__restrict__ T, *__restrict__ P, *__restrict__ x;
  double *__restrict__ rho, *__restrict__ lnphi, *__restrict__ lnphi_pure;
  int32_t* __restrict__ status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix c;
    const double t = T[i], p = P[i];
    int32_t st = ST_BAD_INPUT;
    double out = 0.0, row[NC_MAX], z = 0.0;
    if (load_mix(mix_of(set, i), x, i, t, c) && p > 0.0 && isfinite(p)) {
      double xr;
      st = density_root(c, p / c.kT_pa, xr);
      if (st == ST_OK) {
        out = molar_density(xr, c.c3);
        // at the density reported, converted as the state form converts it: the two forms then agree bit for bit
        st = mix_lnphi_at(mix_of(set, i), x + i * set.nc, t, number_density(out), c, row, z);
      }
    }
    const MixRef m = mix_of(set, i);
    const bool good = st == ST_OK;
    rho[i] = good ? out : 0.0;
    for (int s = 0; s < m.nc; ++s) lnphi[i * m.nc + s] = good ? row[s] : NAN;
    if (lnphi_pure)
      for (int s = 0; s < m.nc; ++s)
        lnphi_pure[i * m.nc + s] = (good && m.comp[s] != -1) ? mix_lnphi_pure(m, s, t, p, c) : NAN;
    status[i] = st;
  }
};

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_lnphi_state(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                              const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                              const int64_t* owner, const double* T, const double* rho, const double* x,
                                              int64_t n, double* lnphi, double* Z, int32_t* status) {
  return mix_launch(h, "gnx_pcsaft_mix_lnphi_state", GNX_K_PCSAFT_MIX_LNPHI_STATE, 36.0 + 16.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n,
                    T && rho && x && lnphi && Z && status, MixLnphiStatePoint{T, rho, x, lnphi, Z, status});
}

extern "C" int32_t gnx_pcsaft_mix_lnphi(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                        const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                        const int64_t* owner, const double* T, const double* P, const double* x,
                                        int64_t n, double* rho, double* lnphi, double* lnphi_pure, int32_t* status) {
  return mix_launch(h, "gnx_pcsaft_mix_lnphi", GNX_K_PCSAFT_MIX_LNPHI, 36.0 + (lnphi_pure ? 24.0 : 16.0) * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n,
                    T && P && x && rho && lnphi && status, MixLnphiPoint{T, P, x, rho, lnphi, lnphi_pure, status});
}
