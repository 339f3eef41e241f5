// Mixture PC-SAFT tangent-plane stability test in fp64 (Michelsen 1982): is the feed z one stable phase at (T, P), and if
// not, which composition w proves it.  (ref: pcsaft/pcsaft_feos.py is_stable_feos, which pcsaft/kij.py:30
// _pred_x1_worker and pcsaft/phase_equilibria.py call on every trial feed before they flash it; [3P] feos 0.8
// State.is_stable with density_initialization=None).  DESIGN.md §4c.
//
// Equations, in the bubble and flash kernels' form without ln Z: with ln f_i = mu_i^res/kT + ln(rho x_i) and d_i =
// ln f_i(z), the tangent-plane distance of a normalised trial composition w is
//   D(w) = sum_i w_i (ln f_i(w) - d_i),
// and z is stable iff D >= 0 for every w.  The state of a composition at (T, P) is the one of its liquid root
// (density_root) and its lowest vapour root (vapour_root) with the lower g = sum_i x_i ln f_i; the only root where there
// is one, the liquid root on a tie.
//
// A row is one (point, trial) pair: the trials of a point stand in rows of their own, not in a loop of one lane.  A
// mixture of nc slots has nc + 2 trials, started from unnormalised mole numbers W, K_i = f_i(z) kT / (z_i P):
//   trial 0      W = z K        the ideal vapour over the feed
//   trial 1      W = z / K      liquid-like
//   trial 2 + s  W = 0.1 z + 0.9 e_s   rich in slot s
// One step of successive substitution: S = sum W, w = W / S, the state of w, r_i = ln S + ln f_i(w) - d_i, D(w), next
// W_i = w_i exp(d_i - ln f_i(w)).  A trial ends, tested in this order at every step,
//   trivial     max_i |ln(w_i / z_i)| < 1e-4 and |rho_w / rho_z - 1| < 1e-4: it fell onto the feed; tpd = 0.0, w = z
//   negative    D < -1e-8: a certificate that z is unstable, converged or not; this D and this w
//   stationary  max_i |r_i| < 1e-8: a stationary point of the distance; D and w
// and with status 1 after kStabIters steps, on a non-finite value, or where w (or z) has no root at P.  The trial rich
// in a slot that is unused (-1) or dropped (z = 0) is trivial, as is every trial of a single component.
//
// The two scans of a step cost some 600 to 1100 evaluations of the pressure.  As in the flash, once a step has moved ln w
// by less than 0.05 the next one looks for each root within 5 % of the previous one first, takes a root that was not
// there to be still missing, and scans only where a bracket does not hold.  A trial that ends on roots found this way
// evaluates that step again from the scans, and goes on with scans alone if it does not end there: every number
// reported comes from the highest liquid root and the lowest vapour root.
//
// One lane per row, no shared memory, no atomics, every loop with a fixed trip cap: same input, same bits, wherever the
// row stands in the launch.  Like the bubble and flash launches this one carries no kernel id (GNX_K_NONE); time it with
// events around the call (tools/pcsaft_bench.py --stability).
#include "gnx_pcsaft_mix_state.hpp"

namespace {

constexpr int kStabIters = 400;          // successive substitution steps of one trial
constexpr double kStabTol = 1e-8;        // max_i |r_i| below which a trial is stationary
constexpr double kStabNegative = -1e-8;  // D below this: unstable.  Above the 4.6e-9 the oracle's two steps disagree by
constexpr double kStabTrivial = 1e-4;    // ln(w_i / z_i) and rho_w / rho_z - 1 within this: the trial is the feed
constexpr double kStabRich = 0.9;        // share of the slot a "rich in slot s" trial starts from; the rest is z
constexpr double kStabNearMove = 0.05;   // largest step in ln w after which the next roots are sought near the previous

// trial trial[i] of the feed z[i, :] at (T[i], P[i])
struct MixStabPoint {
  const int64_t* trial;
  const double *T, *P, *z;
  double *tpd, *w, *rho_w, *rho_z;
  int32_t* status;
  __device__ void operator()(const MixSet& set, int64_t i) const {
    Mix c;
    const MixRef m = mix_of(set, i);
    const double t = T[i], p = P[i];
    const int64_t tr = trial[i];
    int32_t st = ST_BAD_INPUT;
    double dist = 0.0, rw = 0.0, rz = 0.0, wv[NC_MAX];
    for (int s = 0; s < NC_MAX; ++s) wv[s] = 0.0;
    if (isfinite(p) && p > 0.0 && tr >= 0 && tr < m.nc + 2 && load_mix(m, z, i, t, c)) {
      st = ST_NO_CONV;
      const double* zin = z + i * m.nc;
      int64_t cm[NC_MAX];
      const MixRef mp = mix_present(m, zin, cm);  // a trial phase has the feed's components and no others
      const int nc = m.nc;
      const int n = c.n;
      const double pt = p / c.kT_pa;
      double zc[NC_MAX], d[NC_MAX], W[NC_MAX], wc[NC_MAX], lnf[NC_MAX], sum = 0.0, lnS = 0.0;
      int slot[NC_MAX];
      for (int s = 0; s < nc; ++s)
        if (cm[s] != -1) sum += zin[s];
      int rich = -1;  // the compact index of the slot that trial 2 + s is rich in; -1: that slot is not in the mixture
      for (int s = 0, k = 0; s < nc; ++s)
        if (cm[s] != -1) {
          if (tr == 2 + s) rich = k;
          slot[k] = s;
          zc[k++] = zin[s] / sum;
        }
      for (int k = 0; k < n; ++k) wv[slot[k]] = wc[k] = zc[k];
      bool ok = true, trivial = false, done = false, scans_only = false;
      double prev[2] = {0.0, 0.0}, move = 1.0;  // the roots of the last step, and how far it moved ln w
      for (int it = 0; it <= kStabIters; ++it) {  // pass 0 is the feed itself: d_i = ln f_i(z) and rho_z
        bool near = !scans_only && move < kStabNearMove;
        ok = stab_state(mp, wv, wc, n, t, pt, c, rw, lnf, prev, near);
        if (!ok && near) {
          scans_only = true;  // this step again, w as it is, from the scans
          continue;
        }
        if (!ok) break;
        if (it == 0) {
          rz = rw;
          trivial = n == 1 || (tr >= 2 && rich < 0);
          for (int k = 0; k < n; ++k) {
            d[k] = lnf[k];
            const double lnk = d[k] - ::log(zc[k] * pt);
            W[k] = tr == 0   ? zc[k] * ::exp(lnk)
                   : tr == 1 ? zc[k] * ::exp(-lnk)
                             : (1.0 - kStabRich) * zc[k] + (k == rich ? kStabRich : 0.0);
          }
        } else {
          double near = ::fabs(rw / rz - 1.0), res = 0.0;
          dist = 0.0;
          for (int k = 0; k < n; ++k) {
            const double dl = lnf[k] - d[k];
            near = ::fmax(near, ::fabs(::log(wc[k] / zc[k])));
            res = ::fmax(res, ::fabs(lnS + dl));
            dist += wc[k] * dl;
            ok = ok && isfinite(dl);
            W[k] = wc[k] * ::exp(-dl);
          }
          ok = ok && isfinite(near);
          trivial = near < kStabTrivial;
          done = !trivial && (dist < kStabNegative || res < kStabTol);
        }
        if (ok && (trivial || done) && near) {
          // what is reported is the state of the highest liquid root and the lowest vapour root: only the scans say so
          scans_only = true;
          trivial = done = false;
          continue;
        }
        if (!ok || trivial || done) break;
        double S = 0.0;
        for (int k = 0; k < n; ++k) S += W[k];
        lnS = ::log(S);
        ok = isfinite(S) && S > 0.0 && isfinite(lnS);
        move = 0.0;
        for (int k = 0; ok && k < n; ++k) {
          const double wn = W[k] / S;
          move = ::fmax(move, ::fabs(::log(wn / wc[k])));
          wv[slot[k]] = wc[k] = wn;
          ok = wc[k] > 0.0 && isfinite(wc[k]) && isfinite(move);
        }
        if (!ok) break;
      }
      if (ok && trivial) {
        // on the feed: the distance is 0 there by definition, not by rounding
        dist = 0.0;
        rw = rz;
        for (int k = 0; k < n; ++k) wv[slot[k]] = zc[k];
      }
      if (ok && (trivial || done)) st = ST_OK;
    }
    const bool good = st == ST_OK;
    tpd[i] = good ? dist : NAN;
    if (rho_w) rho_w[i] = good ? rw : 0.0;
    if (rho_z) rho_z[i] = good ? rz : 0.0;
    store_row(w, i, m, good, wv);
    status[i] = st;
  }
};

}  // namespace

extern "C" int32_t gnx_pcsaft_mix_stability(gnx_handle* h, const double* params, int64_t B, const int64_t* mix_comp,
                                            const double* mix_kij, const double* mix_eab, int64_t M, int32_t nc,
                                            const int64_t* owner, const int64_t* trial, const double* T, const double* P,
                                            const double* z, int64_t n, double* tpd, double* w, double* rho_w,
                                            double* rho_z, int32_t* status) {
  // no kernel id of its own: under GNX_K_NONE the scope stays off and the launch is a plain one
  return mix_launch(h, "gnx_pcsaft_mix_stability", GNX_K_NONE, 60.0 + 16.0 * nc,
                    MixSet{params, B, mix_comp, mix_kij, mix_eab, M, (int)nc, owner}, n,
                    trial && T && P && z && tpd && w && status, MixStabPoint{trial, T, P, z, tpd, w, rho_w, rho_z, status});
}
