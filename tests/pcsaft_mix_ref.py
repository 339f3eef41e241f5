"""Test-only fp64 NumPy restatement of the mixture PC-SAFT of csrc/gnx_pcsaft_mix.hip, for 1 to 4
components.  The constant tables come from tests/pcsaft_ref.py.

It shares no mechanism with the kernel: every term is written from the general mixture sums at each call (the kernel
folds everything that does not depend on rho into coefficients once per point), the pressure comes from a complex step
on ``a_res`` in rho (the kernel uses second-order forward duals), dP/drho from a central difference of that pressure,
the site fractions from a fixed number of damped substitutions followed by a fixed number of Newton steps on the full
(X_A, X_B) system in its product form (a damped substitution instead wherever a Newton step leaves (0, 1]), all in
complex arithmetic so that the step carries through, and a point whose fractions then miss the mass-action equations by
more than 1e-12 counts as not solved (the kernel
eliminates X_B, solves the X_A system in real arithmetic and differentiates it implicitly), and the density from a
dense packing-fraction scan followed by Brent's method.

Rows are ``[m, sigma (Å), eps/k (K), kappa_ab, eps_ab/k (K), mu (D), na, nb, mw]``; T in K, P in Pa, rho in mol/m³.
``kij`` / ``eab`` are [nc, nc] matrices read from their upper triangle (diagonal ignored); a NaN in ``eab`` means the
combining rule.
"""
from __future__ import annotations

import numpy as np
from scipy import optimize

from tests.pcsaft_ref import (DIP_A, DIP_B, DIP_C, DIPOLE_FACTOR, DISP_A, DISP_B, ETA_MAX, RGAS, TO_A3, _interp,
                              _poly)

SUBSTITUTIONS, NEWTON_STEPS, RESIDUAL = 40, 100, 1e-12


class Mixture:
    """rows [nc, 9], composition x [nc] (normalised here by its sum), optional kij / eab [nc, nc]"""

    def __init__(self, rows, x, kij=None, eab=None):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
        x = np.asarray(x, dtype=np.float64)
        assert rows.shape[0] == x.shape[0] and np.all(x >= 0) and x.sum() > 0
        self.nc = nc = rows.shape[0]
        self.x = x / x.sum()
        self.m, self.sigma, self.eps, self.kab, self.eab, self.mu, self.na, self.nb = rows[:, :8].T
        up = lambda a: np.triu(np.asarray(a, dtype=np.float64), 1) + np.triu(np.asarray(a, dtype=np.float64), 1).T
        self.kij = np.zeros((nc, nc)) if kij is None else up(kij)
        rule = 0.5 * (self.eab[:, None] + self.eab[None, :])
        self.eab_ij = rule
        if eab is not None:
            given = up(np.where(np.isnan(np.asarray(eab, dtype=np.float64)), np.inf, eab))
            self.eab_ij = np.where(np.isfinite(given) & ~np.eye(nc, dtype=bool), given, rule)
        self.mbar = float(self.x @ self.m)

    def diameters(self, T):
        return self.sigma * (1.0 - 0.12 * np.exp(-3.0 * self.eps / T))

    def eta_per_rho(self, T):
        """packing fraction per number density (Å^3)"""
        return np.pi / 6.0 * float(self.x @ (self.m * self.diameters(T) ** 3))


def _contact(mix, T, rho):
    """(zeta_0..3 [G], g_ij [G, nc, nc])"""
    d = mix.diameters(T)
    z = [np.pi / 6.0 * rho * float(mix.x @ (mix.m * d ** k)) for k in range(4)]
    dij = d[:, None] * d[None, :] / (d[:, None] + d[None, :])
    om = (1.0 - z[3])[:, None, None]
    z2 = z[2][:, None, None]
    g = 1.0 / om + dij * 3.0 * z2 / om ** 2 + dij ** 2 * 2.0 * z2 ** 2 / om ** 3
    return z, g


def _delta0(mix, T):
    """sigma_ij^3 kappa_ij (exp(eps_ab,ij / T) - 1), zero where either component does not associate"""
    sij = 0.5 * (mix.sigma[:, None] + mix.sigma[None, :])
    active = (mix.kab > 0) & (mix.na + mix.nb > 0)
    kap = np.sqrt(np.outer(mix.kab, mix.kab)) * (np.sqrt(np.outer(mix.sigma, mix.sigma)) / sij) ** 3
    return np.where(np.outer(active, active), sij ** 3 * kap * np.expm1(mix.eab_ij / T), 0.0)


def site_fractions(mix, T, rho):
    """(X_A, X_B, Delta), each [G, nc(, nc)], at number densities rho [G] (real or complex)"""
    rho = np.atleast_1d(rho)
    _, g = _contact(mix, T, rho)
    delta = g * _delta0(mix, T)
    G, nc = rho.shape[0], mix.nc
    wa, wb = mix.x * mix.na, mix.x * mix.nb
    r = rho[:, None]
    xa = np.ones((G, nc), dtype=delta.dtype)
    xb = np.ones((G, nc), dtype=delta.dtype)
    for _ in range(SUBSTITUTIONS):
        na_ = 1.0 / (1.0 + r * np.einsum("gij,gj->gi", delta, wb * xb))
        nb_ = 1.0 / (1.0 + r * np.einsum("gij,gj->gi", delta, wa * xa))
        xa, xb = 0.5 * (xa + na_), 0.5 * (xb + nb_)
    eye = np.eye(nc)

    def inside(v):
        with np.errstate(invalid="ignore"):
            return np.all((np.real(v) > 0) & (np.real(v) <= 1), axis=1)

    settled = 0
    for _ in range(NEWTON_STEPS):  # the cap; it ends early three steps after every point has stopped moving
        sa = r * np.einsum("gij,gj->gi", delta, wb * xb)
        sb = r * np.einsum("gij,gj->gi", delta, wa * xa)
        f = np.concatenate([xa * (1.0 + sa) - 1.0, xb * (1.0 + sb) - 1.0], axis=1)
        jac = np.zeros((G, 2 * nc, 2 * nc), dtype=delta.dtype)
        jac[:, :nc, :nc] = eye * (1.0 + sa)[:, :, None]
        jac[:, :nc, nc:] = xa[:, :, None] * r[:, :, None] * delta * wb
        jac[:, nc:, :nc] = xb[:, :, None] * r[:, :, None] * delta * wa
        jac[:, nc:, nc:] = eye * (1.0 + sb)[:, :, None]
        try:
            step = np.linalg.solve(jac, f[:, :, None])[:, :, 0]
        except np.linalg.LinAlgError:  # strong association: the X_A - X_B direction carries no weight in fp64
            step = (np.linalg.pinv(jac) @ f[:, :, None])[:, :, 0]
        ya, yb = xa - step[:, :nc], xb - step[:, nc:]
        good = (inside(ya) & inside(yb))[:, None]  # elsewhere one more damped substitution
        xa, xb = np.where(good, ya, 0.5 * (xa + 1.0 / (1.0 + sa))), np.where(good, yb, 0.5 * (xb + 1.0 / (1.0 + sb)))
        settled = settled + 1 if np.all(good) and np.max(np.abs(np.real(step))) <= 1e-15 else 0
        if settled == 3:
            break
    # a point whose fractions do not satisfy the mass-action equations to 1e-12 has no answer here: NaN
    sa = r * np.einsum("gij,gj->gi", delta, wb * xb)
    sb = r * np.einsum("gij,gj->gi", delta, wa * xa)
    res = np.maximum(np.abs(xa * (1.0 + sa) - 1.0).max(axis=1), np.abs(xb * (1.0 + sb) - 1.0).max(axis=1))
    with np.errstate(invalid="ignore"):
        solved = (inside(xa) & inside(xb) & (res <= RESIDUAL))[:, None]
    xa, xb = np.where(solved, xa, np.nan), np.where(solved, xb, np.nan)
    return xa, xb, delta


def a_terms(mix, T, rho):
    """(hard chain, dispersion, association, dipole) reduced residual Helmholtz energies per molecule at number density
    rho [1/Å^3] (real or complex, scalar or 1-D array)"""
    scalar = np.ndim(rho) == 0
    rho = np.atleast_1d(rho)
    x, m, nc = mix.x, mix.m, mix.nc
    z, g = _contact(mix, T, rho)
    z0, z1, z2, z3 = z
    ahs = (3.0 * z1 * z2 / (1.0 - z3) + z2 ** 3 / (z3 * (1.0 - z3) ** 2) + (z2 ** 3 / z3 ** 2 - z0) * np.log(1.0 - z3)) / z0
    a_hc = mix.mbar * ahs
    for i in range(nc):
        a_hc = a_hc - x[i] * (m[i] - 1.0) * np.log(g[:, i, i])
    eta, mb = z3, mix.mbar
    sij = 0.5 * (mix.sigma[:, None] + mix.sigma[None, :])
    eij = np.sqrt(np.outer(mix.eps, mix.eps)) * (1.0 - mix.kij)
    xxmm = np.outer(x * m, x * m)
    s1, s2 = np.sum(xxmm * (eij / T) * sij ** 3), np.sum(xxmm * (eij / T) ** 2 * sij ** 3)
    i1, i2 = _poly(_interp(DISP_A, mb), eta), _poly(_interp(DISP_B, mb), eta)
    c1 = 1.0 / (1.0 + mb * (8 * eta - 2 * eta ** 2) / (1 - eta) ** 4
                + (1 - mb) * (20 * eta - 27 * eta ** 2 + 12 * eta ** 3 - 2 * eta ** 4) / ((1 - eta) * (2 - eta)) ** 2)
    a_disp = -2.0 * np.pi * rho * i1 * s1 - np.pi * rho * mb * c1 * i2 * s2
    a_assoc = 0.0 * rho
    if np.any(_delta0(mix, T) != 0.0):
        xa, xb, _ = site_fractions(mix, T, rho)
        for i in range(nc):
            if x[i] > 0:  # ln X of an absent species carries no weight
                a_assoc = a_assoc + x[i] * (mix.na[i] * (np.log(xa[:, i]) - xa[:, i] / 2.0 + 0.5)
                                            + mix.nb[i] * (np.log(xb[:, i]) - xb[:, i] / 2.0 + 0.5))
    a_dip = 0.0 * rho
    polar = [i for i in range(nc) if mix.mu[i] > 0 and x[i] > 0]
    if polar:
        et, s3 = mix.eps / T, mix.sigma ** 3
        mu2 = mix.mu ** 2 / (m * mix.eps * s3) * DIPOLE_FACTOR
        A2, A3 = 0.0 * rho, 0.0 * rho
        for i in polar:
            for j in polar:
                mij = min(np.sqrt(m[i] * m[j]), 2.0)
                j2 = _poly(_interp(DIP_A, mij) + _interp(DIP_B, mij) * eij[i, j] / T, eta)
                A2 = A2 + x[i] * x[j] * et[i] * et[j] * s3[i] * s3[j] / sij[i, j] ** 3 * mu2[i] * mu2[j] * j2
                for k in polar:
                    mijk = min(np.cbrt(m[i] * m[j] * m[k]), 2.0)
                    j3 = _poly(_interp(DIP_C, mijk), eta)
                    A3 = A3 + (x[i] * x[j] * x[k] * et[i] * et[j] * et[k] * s3[i] * s3[j] * s3[k]
                               / (sij[i, j] * sij[i, k] * sij[j, k]) * mu2[i] * mu2[j] * mu2[k] * j3)
        A2 = -np.pi * rho * A2
        A3 = -4.0 / 3.0 * np.pi ** 2 * rho ** 2 * A3
        a_dip = A2 / (1.0 - A3 / A2)
    out = (a_hc, a_disp, a_assoc, a_dip)
    return tuple(t[0] for t in out) if scalar else out


def a_res(mix, T, rho):
    return sum(a_terms(mix, T, rho))


def compressibility(mix, T, rho):
    """Z = 1 + rho da/drho, the derivative by complex step; rho in 1/Å^3"""
    h = rho * 1e-20
    return 1.0 + rho * np.imag(a_res(mix, T, rho + 1j * h)) / h


def pressure_eta(mix, T, eta):
    """P [Pa] at packing fraction eta"""
    rho = eta / mix.eta_per_rho(T)
    return rho / TO_A3 * RGAS * T * compressibility(mix, T, rho)


def pressure(mix, T, rho_mol):
    return pressure_eta(mix, T, rho_mol * TO_A3 * mix.eta_per_rho(T))


def dpdrho(mix, T, rho_mol, rel=1e-6):
    """dP/drho [Pa m³/mol] by central difference of the complex-step pressure"""
    h = rho_mol * rel
    return (pressure(mix, T, rho_mol + h) - pressure(mix, T, rho_mol - h)) / (2.0 * h)


_GRID = np.concatenate([np.geomspace(1e-10, 1e-2, 100, endpoint=False), np.linspace(1e-2, ETA_MAX, 1500)])


def _brent(f, lo, hi):
    return optimize.brentq(f, lo, hi, xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=1000)


def density(mix, T, P):
    """highest-density root of P(rho) = P with dP/drho > 0, mol/m³; None if there is none"""
    with np.errstate(all="ignore"):
        f = pressure_eta(mix, T, _GRID) - P
        below = np.nonzero(f <= 0)[0]
        if below.size == 0 or not np.all(np.isfinite(f[below[-1]:])) or f[-1] <= 0:
            return None
        lo, hi = _GRID[below[-1]], _GRID[below[-1] + 1]
        try:
            eta = _brent(lambda e: pressure_eta(mix, T, e) - P, lo, hi)
        except ValueError:  # the bracket of the scan does not hold point by point: pressure lost to rounding
            return None
        rho = eta / mix.eta_per_rho(T) / TO_A3
        if not dpdrho(mix, T, rho) > 0:
            return None
    return rho
