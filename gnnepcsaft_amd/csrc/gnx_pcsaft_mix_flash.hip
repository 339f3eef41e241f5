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
#include "gnx_pcsaft_mix_flash.hpp"

namespace {

// flash of point i at (T, P, z): the load, the solve of gnx_pcsaft_mix_flash.hpp, the stores
struct MixFlashPoint {
  const double *T, *P, *z;
  double *beta, *x, *y, *rho_l, *rho_v;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    const MixRef m = mix_of(set, i);
    double bt, rl, rv, xv[NC_MAX], yv[NC_MAX];
    const int32_t st = mix_flash_solve(m, T[i], P[i], z + i * m.nc, bt, xv, yv, rl, rv);
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
