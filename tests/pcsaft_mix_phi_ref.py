"""Test-only oracle of the mixture fugacity coefficients of csrc/gnx_pcsaft_mix_phi.hip, on top of the
mixture oracle of tests/pcsaft_mix_ref.py, which is used as it is.

It shares no mechanism with the kernel (forward duals in the composition through every term, implicit differentiation
of the site fractions): ln phi_i = dF/dN_i - ln Z with F(N) = (sum N) a_res(x = N / sum N, T, rho0 sum N), the residual
Helmholtz energy of N molecules in the fixed volume 1 / rho0, differentiated by a five-point central difference in N_i
around N = x.  ``Mixture`` normalises N itself.  The step is relative to x_i, and every result is returned at two steps,
1e-3 x_i and 3e-4 x_i: their disagreement is the oracle's own error (convergence is h^4 down to the floor that the
site-fraction residual sets).

Densities here are number densities in 1/Å^3 (``rho_mol * pcsaft_ref.TO_A3``).
"""
from __future__ import annotations

import numpy as np

from tests import pcsaft_mix_ref as MR

STEPS = (1e-3, 3e-4)


def _F(rows, N, T, rho0, kij, eab):
    s = float(np.sum(N))
    return s * MR.a_res(MR.Mixture(rows, N, kij=kij, eab=eab), T, rho0 * s)


def mu_res(rows, x, T, rho0, kij=None, eab=None, step=STEPS[0], relative=True):
    """d F / d N_i at N = x / sum x, fixed T and volume: [nc]"""
    x = np.asarray(x, dtype=np.float64)
    x = x / x.sum()
    out = np.empty(len(x))
    for i in range(len(x)):
        h = step * x[i] if relative else step
        f = []
        for k in (-2, -1, 1, 2):
            N = x.copy()
            N[i] += k * h
            f.append(_F(rows, N, T, rho0, kij, eab))
        out[i] = (f[0] - 8.0 * f[1] + 8.0 * f[2] - f[3]) / (12.0 * h)
    return out


def ln_phi(rows, x, T, rho0, kij=None, eab=None, steps=STEPS, relative=True):
    """ln phi_i at number density rho0, once per step: a tuple of [nc] arrays"""
    ln_z = np.log(MR.compressibility(MR.Mixture(rows, x, kij=kij, eab=eab), T, rho0))
    return tuple(mu_res(rows, x, T, rho0, kij, eab, s, relative) - ln_z for s in steps)


def ln_phi_one(row, T, rho0):
    """one component: ln phi = a + Z - 1 - ln Z"""
    mix = MR.Mixture([row], [1.0])
    z = MR.compressibility(mix, T, rho0)
    return MR.a_res(mix, T, rho0) + z - 1.0 - np.log(z)


def sum_identity(rows, x, T, rho0, kij=None, eab=None):
    """a_res + Z - 1 - ln Z, what sum_i x_i ln phi_i must equal"""
    mix = MR.Mixture(rows, x, kij=kij, eab=eab)
    z = MR.compressibility(mix, T, rho0)
    return MR.a_res(mix, T, rho0) + z - 1.0 - np.log(z)


def scaled(a, b):
    """|a - b| on the scale max(1, |b|), entry-wise"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def sample():
    """indices of every third fixture point, those with all x > 0.02: 49 points"""
    from tests import pcsaft_mix_cases as C
    x = C.fixture_points()[5]
    idx = np.arange(0, len(x), 3)
    return idx[np.all(x[idx] > 0.02, axis=1)]
