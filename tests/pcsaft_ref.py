"""Test-only fp64 NumPy restatement of the pure-component PC-SAFT of csrc/gnx_pcsaft.hip.

It shares no mechanism with the kernel: the pressure comes from a complex-step derivative of ``a_res`` in rho (the
kernel uses forward duals), dP/drho from a central difference of that pressure, the hard-sphere term from the general
BMCSL expression, densities from a dense packing-fraction scan followed by Brent's method, and the phase equilibrium
from ``scipy.optimize.root`` on (ln eta_L, ln eta_V) started from the spinodals of a scan.  The constant tables are
typed here a second time (tests/test_pcsaft_cpu.py compares them with the kernel's header).

Rows are ``[m, sigma (Å), eps/k (K), kappa_ab, eps_ab/k (K), mu (D), na, nb, mw]``; T in K, P in Pa, rho in mol/m³.
"""
from __future__ import annotations

import numpy as np
from scipy import optimize

NA = 6.02214076e23
KB = 1.380649e-23
RGAS = NA * KB
DIPOLE_FACTOR = 7242.702976750923
ETA_MAX = 0.7405
TO_A3 = NA * 1e-30  # mol/m^3 -> 1/Å^3

# Gross & Sadowski 2001, Table 1: rows (a0, a1, a2) / (b0, b1, b2), i = 0..6
DISP_A = np.array([[0.9105631445, 0.6361281449, 2.6861347891, -26.547362491, 97.759208784, -159.59154087, 91.297774084],
                   [-0.3084016918, 0.1860531159, -2.5030047259, 21.419793629, -65.255885330, 83.318680481, -33.746922930],
                   [-0.0906148351, 0.4527842806, 0.5962700728, -1.7241829131, -4.1302112531, 13.776631870, -8.6728470368]])
DISP_B = np.array([[0.7240946941, 2.2382791861, -4.0025849485, -21.003576815, 26.855641363, 206.55133841, -355.60235612],
                   [-0.5755498075, 0.6995095521, 3.8925673390, -17.215471648, 192.67226447, -161.82646165, -165.20769346],
                   [0.0976883116, -0.2557574982, -9.1558561530, 20.642075974, -38.804430052, 93.626774077, -29.666905585]])
# Gross & Vrabec 2006, Table 1: n = 0..4
DIP_A = np.array([[0.3043504, -0.1358588, 1.4493329, 0.3556977, -2.0653308],
                  [0.9534641, -1.8396383, 2.0131180, -7.3724958, 8.2374135],
                  [-1.1610080, 4.5258607, 0.9751222, -12.281038, 5.9397575]])
DIP_B = np.array([[0.2187939, -1.1896431, 1.1626889, 0.0, 0.0],
                  [-0.5873164, 1.2489132, -0.5085280, 0.0, 0.0],
                  [3.4869576, -14.915974, 15.372022, 0.0, 0.0]])
DIP_C = np.array([[-0.0646774, 0.1975882, -0.8087562, 0.6902849, 0.0],
                  [-0.9520876, 2.9924258, -2.3802636, -0.2701261, 0.0],
                  [-0.6260979, 1.2924686, 1.6542783, -3.4396744, 0.0]])


def _interp(table, m):
    return table[0] + (m - 1.0) / m * table[1] + (m - 1.0) / m * (m - 2.0) / m * table[2]


def _poly(coef, x):
    return sum(c * x ** i for i, c in enumerate(coef))


def seg_diameter(row, T):
    return row[1] * (1.0 - 0.12 * np.exp(-3.0 * row[2] / T))


def eta_per_rho(row, T):
    """packing fraction per number density (Å^3)"""
    return np.pi / 6.0 * row[0] * seg_diameter(row, T) ** 3


def assoc_fractions(na, nb, x):
    """closed-form (X_A, X_B) of X_A = 1 / (1 + nb x X_B), X_B = 1 / (1 + na x X_A), x = rho Delta"""
    def root(u, q):  # positive root of q X^2 + u X - 1, the branch without cancellation
        s = np.sqrt(u * u + 4.0 * q)
        with np.errstate(all="ignore"):
            return np.where(np.real(u) >= 0, 2.0 / (u + s), (s - u) / (2.0 * q))
    return root(1.0 + (nb - na) * x, na * x), root(1.0 + (na - nb) * x, nb * x)


def assoc_fractions_iterated(na, nb, x, steps=500):
    xa = xb = 1.0
    for _ in range(steps):
        xa, xb = 0.5 * (xa + 1.0 / (1.0 + nb * x * xb)), 0.5 * (xb + 1.0 / (1.0 + na * x * xa))
    return xa, xb


def a_terms(row, T, rho):
    """(hard chain, dispersion, association, dipole) reduced residual Helmholtz energies at rho [1/Å^3] (real or
    complex, scalar or array)."""
    m, sigma, eps, kab, eab, mu, na, nb = (float(v) for v in row[:8])
    d = seg_diameter(row, T)
    z0, z1, z2, z3 = (np.pi / 6.0 * rho * m * d ** k for k in range(4))
    ahs = (3.0 * z1 * z2 / (1.0 - z3) + z2 ** 3 / (z3 * (1.0 - z3) ** 2) + (z2 ** 3 / z3 ** 2 - z0) * np.log(1.0 - z3)) / z0
    ghs = 1.0 / (1.0 - z3) + d / 2.0 * 3.0 * z2 / (1.0 - z3) ** 2 + (d / 2.0) ** 2 * 2.0 * z2 ** 2 / (1.0 - z3) ** 3
    a_hc = m * ahs - (m - 1.0) * np.log(ghs)
    eta = z3
    i1, i2 = _poly(_interp(DISP_A, m), eta), _poly(_interp(DISP_B, m), eta)
    c1 = 1.0 / (1.0 + m * (8 * eta - 2 * eta ** 2) / (1 - eta) ** 4
                + (1 - m) * (20 * eta - 27 * eta ** 2 + 12 * eta ** 3 - 2 * eta ** 4) / ((1 - eta) * (2 - eta)) ** 2)
    et, s3 = eps / T, sigma ** 3
    a_disp = -2.0 * np.pi * rho * i1 * m * m * et * s3 - np.pi * rho * m * c1 * i2 * m * m * et * et * s3
    a_assoc = 0.0 * rho
    if na * nb > 0 and kab > 0:
        xa, xb = assoc_fractions(na, nb, rho * s3 * kab * np.expm1(eab / T) * ghs)
        a_assoc = na * (np.log(xa) - xa / 2.0 + 0.5) + nb * (np.log(xb) - xb / 2.0 + 0.5)
    a_dip = 0.0 * rho
    if mu > 0:
        mc = min(m, 2.0)
        mu2 = mu * mu / (m * eps * s3) * DIPOLE_FACTOR
        j2 = _poly(_interp(DIP_A, mc) + _interp(DIP_B, mc) * et, eta)
        j3 = _poly(_interp(DIP_C, mc), eta)
        A2 = -np.pi * rho * et ** 2 * s3 * mu2 ** 2 * j2
        A3 = -4.0 / 3.0 * np.pi ** 2 * rho ** 2 * et ** 3 * s3 ** 2 * mu2 ** 3 * j3
        a_dip = A2 / (1.0 - A3 / A2)
    return a_hc, a_disp, a_assoc, a_dip


def a_res(row, T, rho):
    return sum(a_terms(row, T, rho))


def _da(row, T, rho):
    """d a_res / d rho by complex step"""
    h = rho * 1e-20
    return np.imag(a_res(row, T, rho + 1j * h)) / h


def compressibility(row, T, rho):
    return 1.0 + rho * _da(row, T, rho)


def pressure_eta(row, T, eta):
    """P [Pa] at packing fraction eta"""
    rho = eta / eta_per_rho(row, T)
    return rho / TO_A3 * RGAS * T * compressibility(row, T, rho)


def pressure(row, T, rho_mol):
    return pressure_eta(row, T, rho_mol * TO_A3 * eta_per_rho(row, T))


def dpdeta(row, T, eta, rel=1e-6):
    h = eta * rel
    return (pressure_eta(row, T, eta + h) - pressure_eta(row, T, eta - h)) / (2.0 * h)


def chem_pot(row, T, eta):
    """mu / kT up to a function of T: ln rho + a + Z - 1"""
    rho = eta / eta_per_rho(row, T)
    return np.log(rho) + a_res(row, T, rho) + compressibility(row, T, rho) - 1.0


def ln_phi(row, T, rho_mol):
    rho = rho_mol * TO_A3
    z = compressibility(row, T, rho)
    return a_res(row, T, rho) + z - 1.0 - np.log(z)


_GRID = np.concatenate([np.geomspace(1e-12, 1e-2, 400, endpoint=False), np.linspace(1e-2, ETA_MAX, 6000)])


def _brent(f, lo, hi):
    return optimize.brentq(f, lo, hi, xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=1000)


def density(row, T, P):
    """highest-density root of P(rho) = P with dP/drho > 0, mol/m³; None if there is none"""
    f = pressure_eta(row, T, _GRID) - P
    if not np.all(np.isfinite(f)) or f[-1] <= 0:
        return None
    below = np.nonzero(f <= 0)[0]
    lo, hi = (0.0, _GRID[0]) if below.size == 0 else (_GRID[below[-1]], _GRID[below[-1] + 1])
    if lo == 0.0 and pressure_eta(row, T, hi) <= P:
        return None
    eta = _brent(lambda e: pressure_eta(row, T, e) - P, lo, hi) if lo > 0 else \
        _brent(lambda e: pressure_eta(row, T, e) - P if e > 0 else -P, lo, hi)
    if not dpdeta(row, T, eta) > 0:
        return None
    return eta / eta_per_rho(row, T) / TO_A3


def spinodals(row, T):
    """(eta_vapour_spinodal, eta_liquid_spinodal) from the sign changes of dP/deta on the scan, None above Tc"""
    pos = dpdeta(row, T, _GRID) > 0
    neg = np.nonzero(~pos)[0]
    if neg.size == 0 or neg[0] == 0:
        return None
    after = np.nonzero(pos[neg[0]:])[0]
    if after.size == 0:
        return None
    kl = neg[0] + after[0]
    fv = lambda e: dpdeta(row, T, e)  # noqa: E731
    return _brent(fv, _GRID[neg[0] - 1], _GRID[neg[0]]), _brent(fv, _GRID[kl - 1], _GRID[kl])


def unstable_regions(row, T):
    """number of separate eta intervals of the scan with dP/deta <= 0 (1 = one van der Waals loop; more = the phase
    equilibrium between the first two spinodals is not the only one)"""
    neg = (dpdeta(row, T, _GRID) <= 0).astype(int)
    return int(neg[0] + np.count_nonzero(np.diff(neg) == 1))


def vle(row, T):
    """(p_sat Pa, rho_L, rho_V mol/m³) of the pure component at T, or None at/above Tc or without convergence"""
    sp = spinodals(row, T)
    if sp is None:
        return None
    evs, els = sp
    pvs, pls = pressure_eta(row, T, evs), pressure_eta(row, T, els)
    if not pressure_eta(row, T, ETA_MAX) > pvs:  # no liquid branch above the vapour spinodal pressure
        return None
    p0 = 0.5 * (max(pls, 0.0) + pvs)
    try:
        el = _brent(lambda e: pressure_eta(row, T, e) - p0, els, ETA_MAX)
        ev = _brent(lambda e: pressure_eta(row, T, e) - p0 if e > 0 else -p0, 0.0, evs)
    except ValueError:  # P not monotone on a branch: no liquid / vapour root pair
        return None
    c = eta_per_rho(row, T)

    def eqs(x):
        xl, xv = np.exp(x)
        rl = xl / c / TO_A3  # P_L is a difference of terms of size rho_L R T: its rounding sets the scale
        return [(pressure_eta(row, T, xl) - pressure_eta(row, T, xv)) / (rl * RGAS * T),
                chem_pot(row, T, xl) - chem_pot(row, T, xv)]

    def solve(el, ev):
        with np.errstate(all="ignore"):
            sol = optimize.root(eqs, np.log([el, ev]), method="hybr", options={"xtol": 1e-15, "maxfev": 2000})
            xl, xv = np.exp(sol.x)
            if not (np.all(np.isfinite(sol.x)) and els < xl < ETA_MAX and 0 < xv < evs):
                return None
            res = eqs(sol.x)
        if abs(res[0]) > 1e-12 or abs(res[1]) > 1e-12:
            return None
        return pressure_eta(row, T, xv), xl / c / TO_A3, xv / c / TO_A3

    out = solve(el, ev)
    if out is None:
        # far from p0 (p_sat many decades below the spinodal pressure): a coarse bracketed search in ln p for
        # mu_L(p) = mu_V(p) gives the starting densities
        def roots(lnp):
            p = np.exp(lnp)
            return (_brent(lambda e: pressure_eta(row, T, e) - p, els, ETA_MAX),
                    _brent(lambda e: pressure_eta(row, T, e) - p if e > 0 else -p, 0.0, evs))

        def dmu(lnp):
            xl, xv = roots(lnp)
            return chem_pot(row, T, xl) - chem_pot(row, T, xv)

        lo = np.log(pls * (1 + 1e-12)) if pls > 0 else np.log(pvs) - 250.0
        try:
            lnp = optimize.brentq(dmu, lo, np.log(pvs * (1 - 1e-9)), xtol=1e-3)
        except ValueError:
            return None
        out = solve(*roots(lnp))
    return out


def critical_temperature(row, t_lo=None, t_hi=5000.0, tol=1e-3):
    """highest T (K) at which the two spinodals still exist, by bisection on T (from 0.2 eps/k up)"""
    t_lo = 0.2 * row[2] if t_lo is None else t_lo
    if spinodals(row, t_lo) is None:
        return t_lo
    if spinodals(row, t_hi) is not None:
        return t_hi
    while t_hi - t_lo > tol:
        mid = 0.5 * (t_lo + t_hi)
        if spinodals(row, mid) is None:
            t_hi = mid
        else:
            t_lo = mid
    return t_lo
