// Mixture PC-SAFT kernels in fp64: state evaluation at (T, rho, x) and liquid density at (T, P, x), on the model of
// gnx_pcsaft_mix.hpp.  One lane per state point.
#include "gnx_pcsaft_mix.hpp"

namespace {

// a_res, p and dp/drho of point i at (T, rho, x)
__device__ void mix_state_point(const double* __restrict__ params, int64_t B, const int64_t* __restrict__ mix_comp,
                                const double* __restrict__ mix_kij, const double* __restrict__ mix_eab, int64_t M,
                                int nc, const int64_t* __restrict__ owner, const double* __restrict__ T,
                                const double* __restrict__ rho, const double* __restrict__ x, int64_t i,
                                double* __restrict__ a_res, double* __restrict__ p, double* __restrict__ dpdrho,
                                int32_t* __restrict__ status) {
  Mix c;
  const double t = T[i], r = rho[i];
  int32_t st = ST_BAD_INPUT;
  double oa = 0.0, op = 0.0, od = 0.0;
  if (load_mix(params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, x, i, t, c) && r > 0.0 && isfinite(r)) {
    const double rn = number_density(r);  // 1/angstrom^3
    if (rn * c.c3 < 1.0) {
      st = ST_NO_CONV;
      const Mix::Eval e = c.eval_rho(rn);
      if (e.ok && isfinite(e.a) && isfinite(e.p) && isfinite(e.dp)) {
        st = ST_OK;
        oa = e.a;
        op = e.p * c.kT_pa;
        od = e.dp * (kBoltzmann * kAvogadro * t);
      }
    }
  }
  a_res[i] = oa;
  p[i] = op;
  dpdrho[i] = od;
  status[i] = st;
}

// density of point i at (T, P, x): the highest-density root of p(eta) = P with dp/deta > 0
__device__ void mix_density_point(const double* __restrict__ params, int64_t B, const int64_t* __restrict__ mix_comp,
                                  const double* __restrict__ mix_kij, const double* __restrict__ mix_eab, int64_t M,
                                  int nc, const int64_t* __restrict__ owner, const double* __restrict__ T,
                                  const double* __restrict__ P, const double* __restrict__ x, int64_t i,
                                  double* __restrict__ rho, int32_t* __restrict__ status) {
  Mix c;
  const double t = T[i], p = P[i];
  int32_t st = ST_BAD_INPUT;
  double out = 0.0;
  if (load_mix(params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, x, i, t, c) && p > 0.0 && isfinite(p)) {
    double xr;
    st = density_root(c, p / c.kT_pa, xr);
    if (st == ST_OK) out = molar_density(xr, c.c3);
  }
  rho[i] = st == ST_OK ? out : 0.0;
  status[i] = st;
}

__global__ void __launch_bounds__(256) k_pcsaft_mix_state(const double* __restrict__ params, int64_t B,
                                                          const int64_t* __restrict__ mix_comp,
                                                          const double* __restrict__ mix_kij,
                                                          const double* __restrict__ mix_eab, int64_t M, int nc,
                                                          const int64_t* __restrict__ owner, const double* __restrict__ T,
                                                          const double* __restrict__ rho, const double* __restrict__ x,
                                                          int64_t n, double* __restrict__ a_res, double* __restrict__ p,
                                                          double* __restrict__ dpdrho, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mix_state_point(params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, T, rho, x, i, a_res, p, dpdrho, status);
}

__global__ void __launch_bounds__(256) k_pcsaft_mix_density(const double* __restrict__ params, int64_t B,
                                                            const int64_t* __restrict__ mix_comp,
                                                            const double* __restrict__ mix_kij,
                                                            const double* __restrict__ mix_eab, int64_t M, int nc,
                                                            const int64_t* __restrict__ owner,
                                                            const double* __restrict__ T, const double* __restrict__ P,
                                                            const double* __restrict__ x, int64_t n,
                                                            double* __restrict__ rho, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mix_density_point(params, B, mix_comp, mix_kij, mix_eab, M, nc, owner, T, P, x, i, rho, status);
}

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_state(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                        const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                        const int64_t* owner, const double* T, const double* rho, const double* x,
                                        int64_t n, double* a_res, double* p, double* dpdrho, int32_t* status) {
  GNX_MIX_CHECK("gnx_pcsaft_mix_state")
  GNX_CHECK_ARG(owner && T && rho && x && a_res && p && dpdrho && status && (params || B == 0) && (mix_comp || M == 0),
                "gnx_pcsaft_mix_state: NULL argument");
  gnx_prof_scope prof(h, GNX_K_PCSAFT_MIX_STATE, (52.0 + 8.0 * nc) * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_mix_state, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, params, B,
                   mix_comp, mix_kij, mix_eab, M, (int)nc, owner, T, rho, x, n, a_res, p, dpdrho, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}

extern "C" int32_t gnx_pcsaft_mix_density(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                          const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                          const int64_t* owner, const double* T, const double* P, const double* x,
                                          int64_t n, double* rho, int32_t* status) {
  GNX_MIX_CHECK("gnx_pcsaft_mix_density")
  GNX_CHECK_ARG(owner && T && P && x && rho && status && (params || B == 0) && (mix_comp || M == 0),
                "gnx_pcsaft_mix_density: NULL argument");
  gnx_prof_scope prof(h, GNX_K_PCSAFT_MIX_RHO, (36.0 + 8.0 * nc) * n, 0.0, 0.0, true);
  GNX_LAUNCH_TIMED(prof, k_pcsaft_mix_density, dim3((unsigned)gnx_cdiv(n, 256)), dim3(256), 0, h->stream, params, B,
                   mix_comp, mix_kij, mix_eab, M, (int)nc, owner, T, P, x, n, rho, status);
  GNX_LAUNCH_CHECK();
  return GNX_OK;
}
