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

// ln phi of every slot of one mixture at (T, number density rn, x), NaN in the -1 slots, and Z.  A used slot with x = 0
// stays in the mixture: its ln phi is the value at infinite dilution.  c is scratch: the mixture in real arithmetic.
//   ln phi_i = a + (Z - 1) + a_xi - sum_j x_j a_xj - ln Z,  a_xi = da/dx_i at fixed T, rho, the x independent
__device__ int32_t mix_lnphi_at(const double* __restrict__ params, int64_t B, const int64_t* __restrict__ comp,
                                const double* __restrict__ kij, const double* __restrict__ eab, int nc,
                                const double* __restrict__ xin, double T, double rn, Mix& c, double* lnphi, double& z) {
  if (!c.init<true>(params, B, comp, kij, eab, nc, xin, T)) return ST_BAD_INPUT;
  if (!(rn * c.c3 < 1.0)) return ST_BAD_INPUT;
  const Mix::Eval e = c.eval_rho(rn);  // Z from the second-order dual in rho; leaves the converged X_A in c.xa
  if (!e.ok || !isfinite(e.a) || !isfinite(e.z)) return ST_NO_CONV;
  z = e.z;
  if (!(e.z > 0.0)) return ST_NO_CONV;  // no ln Z at a negative pressure
  MixT<GX> g;
  if (!g.init<true>(params, B, comp, kij, eab, nc, xin, T)) return ST_BAD_INPUT;
  GX xaG[NC_MAX];
  for (int i = 0; i < NC_MAX; ++i) xaG[i] = GX(1.0);
  if (c.assoc && !mix_sites_grad(c, g, rn, xaG)) return ST_NO_CONV;
  const GX a = g.a_res(GX(rn), xaG);
  double sum = 0.0;
  for (int s = 0; s < nc; ++s)
    if (comp[s] != -1) sum += xin[s];
  double xs = 0.0;
  int k = 0;
  for (int s = 0; s < nc; ++s)
    if (comp[s] != -1) xs += xin[s] / sum * a.g[k++];
  const double base = a.v + (e.z - 1.0) - xs - ::log(e.z);
  bool fin = isfinite(base);
  for (int j = 0; j < k; ++j) fin = fin && isfinite(a.g[j]);
  if (!fin) return ST_NO_CONV;
  k = 0;
  for (int s = 0; s < nc; ++s) lnphi[s] = comp[s] != -1 ? base + a.g[k++] : NAN;
  return ST_OK;
}

// ln phi of component row `comp` alone at its own liquid root at (T, P): a + Z - 1 - ln Z there.  NaN where it has none:
// the highest root with dp/drho > 0 counts as liquid only if p(rho) has a mechanically unstable stretch (dp/drho <= 0)
// below it, looked for on the grid of the density scan; above the critical temperature there is none.
__device__ double mix_lnphi_pure(const double* __restrict__ params, int64_t B, const int64_t* __restrict__ comp,
                                 double T, double p, Mix& c) {
  const double one = 1.0;
  if (!c.init(params, B, comp, nullptr, nullptr, 1, &one, T)) return NAN;
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

// ln phi and Z of point i at (T, rho, x)
__device__ void mix_lnphi_state_point(const double* __restrict__ params, int64_t B,
                                      const int64_t* __restrict__ mix_comp, const double* __restrict__ mix_kij,
                                      const double* __restrict__ mix_eab, int64_t M, int nc,
                                      const int64_t* __restrict__ owner, const double* __restrict__ T,
                                      const double* __restrict__ rho, const double* __restrict__ x, int64_t i,
                                      double* __restrict__ lnphi, double* __restrict__ Z, int32_t* __restrict__ status) {
  Mix c;
  const double t = T[i], r = rho[i];
  const int64_t o = owner[i];
  int32_t st = ST_BAD_INPUT;
  double row[NC_MAX], z = 0.0;
  if (o >= 0 && o < M && r > 0.0 && isfinite(r))
    st = mix_lnphi_at(params, B, mix_comp + o * nc, mix_kij ? mix_kij + o * nc * nc : nullptr,
                      mix_eab ? mix_eab + o * nc * nc : nullptr, nc, x + i * nc, t, number_density(r), c, row, z);
  for (int s = 0; s < nc; ++s) lnphi[i * nc + s] = st == ST_OK ? row[s] : NAN;
  Z[i] = z;
  status[i] = st;
}

// liquid density of point i at (T, P, x) as mix_density_point finds it, ln phi there and, if asked for, ln phi of every
// used slot's component alone at (T, P)
__device__ void mix_lnphi_point(const double* __restrict__ params, int64_t B, const int64_t* __restrict__ mix_comp,
                                const double* __restrict__ mix_kij, const double* __restrict__ mix_eab, int64_t M, int nc,
                                const int64_t* __restrict__ owner, const double* __restrict__ T,
                                const double* __restrict__ P, const double* __restrict__ x, int64_t i,
                                double* __restrict__ rho, double* __restrict__ lnphi, double* __restrict__ lnphi_pure,
                                int32_t* __restrict__ status) {
  Mix c;
  const double t = T[i], p = P[i];
  int32_t st = ST_BAD_INPUT;
  double out = 0.0, row[NC_MAX], z = 0.0;
  if (load_mix(params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, x, i, t, c) && p > 0.0 && isfinite(p)) {
    double xr;
    st = density_root(c, p / c.kT_pa, xr);
    if (st == ST_OK) {
      out = molar_density(xr, c.c3);
      // at the density reported, converted as the state form converts it: the two forms then agree bit for bit
      const int64_t o = owner[i];
      st = mix_lnphi_at(params, B, mix_comp + o * nc, mix_kij ? mix_kij + o * nc * nc : nullptr,
                        mix_eab ? mix_eab + o * nc * nc : nullptr, nc, x + i * nc, t, number_density(out), c, row, z);
    }
  }
  rho[i] = st == ST_OK ? out : 0.0;
  for (int s = 0; s < nc; ++s) lnphi[i * nc + s] = st == ST_OK ? row[s] : NAN;
  if (lnphi_pure) {
    const int64_t* comp = st == ST_OK ? mix_comp + owner[i] * nc : nullptr;
    for (int s = 0; s < nc; ++s)
      lnphi_pure[i * nc + s] = (comp && comp[s] != -1) ? mix_lnphi_pure(params, B, comp + s, t, p, c) : NAN;
  }
  status[i] = st;
}

__global__ void __launch_bounds__(256) k_pcsaft_mix_lnphi_state(const double* __restrict__ params, int64_t B,
                                                                const int64_t* __restrict__ mix_comp,
                                                                const double* __restrict__ mix_kij,
                                                                const double* __restrict__ mix_eab, int64_t M, int nc,
                                                                const int64_t* __restrict__ owner,
                                                                const double* __restrict__ T,
                                                                const double* __restrict__ rho,
                                                                const double* __restrict__ x, int64_t n,
                                                                double* __restrict__ lnphi, double* __restrict__ Z,
                                                                int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mix_lnphi_state_point(params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, T, rho, x, i, lnphi, Z, status);
}

__global__ void __launch_bounds__(256) k_pcsaft_mix_lnphi(const double* __restrict__ params, int64_t B,
                                                          const int64_t* __restrict__ mix_comp,
                                                          const double* __restrict__ mix_kij,
                                                          const double* __restrict__ mix_eab, int64_t M, int nc,
                                                          const int64_t* __restrict__ owner, const double* __restrict__ T,
                                                          const double* __restrict__ P, const double* __restrict__ x,
                                                          int64_t n, double* __restrict__ rho,
                                                          double* __restrict__ lnphi, double* __restrict__ lnphi_pure,
                                                          int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    mix_lnphi_point(params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, T, P, x, i, rho, lnphi, lnphi_pure, status);
}

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_lnphi_state(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                              const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                              const int64_t* owner, const double* T, const double* rho, const double* x,
                                              int64_t n, double* lnphi, double* Z, int32_t* status) {
  GNX_MIX_CHECK("gnx_pcsaft_mix_lnphi_state")
  GNX_CHECK_ARG(owner && T && rho && x && lnphi && Z && status && (params || B == 0) && (mix_comp || M == 0),
                "gnx_pcsaft_mix_lnphi_state: NULL argument");
  gnx_prof_scope prof(h, GNX_K_PCSAFT_MIX_LNPHI_STATE, (36.0 + 16.0 * nc) * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_mix_lnphi_state, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, params, B,
                   mix_comp, mix_kij, mix_eab, M, (int)nc, owner, T, rho, x, n, lnphi, Z, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_pcsaft_mix_lnphi(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                        const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                        const int64_t* owner, const double* T, const double* P, const double* x,
                                        int64_t n, double* rho, double* lnphi, double* lnphi_pure, int32_t* status) {
  GNX_MIX_CHECK("gnx_pcsaft_mix_lnphi")
  GNX_CHECK_ARG(owner && T && P && x && rho && lnphi && status && (params || B == 0) && (mix_comp || M == 0),
                "gnx_pcsaft_mix_lnphi: NULL argument");
  gnx_prof_scope prof(h, GNX_K_PCSAFT_MIX_LNPHI, (36.0 + (lnphi_pure ? 24.0 : 16.0) * nc) * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_mix_lnphi, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, params, B,
                   mix_comp, mix_kij, mix_eab, M, (int)nc, owner, T, P, x, n, rho, lnphi, lnphi_pure, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}
