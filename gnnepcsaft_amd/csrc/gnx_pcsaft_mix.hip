// Mixture PC-SAFT kernels in fp64: state evaluation at (T, rho, x) and liquid density at (T, P, x), on the model of
// gnx_pcsaft_mix.hpp.  One lane per state point: k_pcsaft_mix over the two point functors below.
#include "gnx_pcsaft_mix.hpp"

namespace {

// a_res, p and dp/drho of point i at (T, rho, x)
struct MixStatePoint {
  const double *T, *rho, *x;
  double *a_res, *p, *dpdrho;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix c;
    const double t = T[i], r = rho[i];
    int32_t st = ST_BAD_INPUT;
    double oa = 0.0, op = 0.0, od = 0.0;
    if (load_mix(mix_of(set, i), x, i, t, c) && r > 0.0 && isfinite(r)) {
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
};

// density of point i at (T, P, x): the highest-density root of p(eta) = P with dp/deta > 0
struct MixDensityPoint {
  const double *T, *P, *x;
  double* rho;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix c;
    const double t = T[i], p = P[i];
    int32_t st = ST_BAD_INPUT;
    double out = 0.0;
    if (load_mix(mix_of(set, i), x, i, t, c) && p > 0.0 && isfinite(p)) {
      double xr;
      st = density_root(c, p / c.kT_pa, xr);
      if (st == ST_OK) out = molar_density(xr, c.c3);
    }
    rho[i] = st == ST_OK ? out : 0.0;
    status[i] = st;
  }
};

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_state(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                        const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                        const int64_t* owner, const double* T, const double* rho, const double* x,
                                        int64_t n, double* a_res, double* p, double* dpdrho, int32_t* status) {
  return mix_launch(h, "gnx_pcsaft_mix_state", GNX_K_PCSAFT_MIX_STATE, 52.0 + 8.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n,
                    T && rho && x && a_res && p && dpdrho && status, MixStatePoint{T, rho, x, a_res, p, dpdrho, status});
}

extern "C" int32_t gnx_pcsaft_mix_density(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                          const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                          const int64_t* owner, const double* T, const double* P, const double* x,
                                          int64_t n, double* rho, int32_t* status) {
  return mix_launch(h, "gnx_pcsaft_mix_density", GNX_K_PCSAFT_MIX_RHO, 36.0 + 8.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n, T && P && x && rho && status,
                    MixDensityPoint{T, P, x, rho, status});
}
