"""Every mixture entry reads its own mixture's slices (csrc/gnx_pcsaft_mix.hpp: mix_of): each of the six tensor forms on
one pooled table of five mixtures in nc = 3 slots (nc * nc = 9, so a slip between the strides of comp [M, nc] and of
kij / eab [M, nc, nc] shows), owners unsorted and repeated, against one launch per mixture on a table that holds that
mixture alone (M = 1: its comp row and its kij / eab matrices).  Every output, status included, must have the same bytes.

The mixtures are tie-line feeds of tests/pcsaft_mix_flash_ref.py of at most three components (named points of
tests/pcsaft_mix_vle_ref.py and a system of the binary fixture of tests/pcsaft_mix_cases.py), so that one table serves
all six entries: T and the liquid x for the bubble point, (T, P, x) for the density and the fugacity coefficients, (T, P,
z) for the flash, (T, a gas-like rho, x) for the two state forms."""
import functools

import numpy as np
import pytest
import torch

from tests import pcsaft_mix_flash_ref as F

pytestmark = pytest.mark.gpu

NC = 3
RHO = 50.0  # mol/m³ for the state forms: a gas, so that Z > 0 and ln phi exists (packing fraction below 0.003)
# (tie-line point, the slots its components take, further used slots: (slot, tie-line point, component) at x = 0)
MIXTURES = ((4, (0, 1, 2), ()),             # methane + butane + hexane: every slot used
            (3, (0, 2), ()),                # ethanol + water around a -1 slot: the associating pair, pair entry [0][2]
            (2, (0, 1), ((2, 0, 0),)),      # butane + hexane with methane in a used slot at x = 0
            (0, (1, 2), ()),                # methane + hexane behind a -1 slot
            (6, (0, 1), ()))                # the first system of the binary fixture, 5.2 MPa
OWNER = (3, 0, 4, 1, 2, 0, 3, 1, 4, 2, 1, 0)
ENTRIES = ("state", "density", "ln_phi_state", "ln_phi", "bubble", "flash")


@functools.lru_cache(maxsize=None)
def _table():
    """params [B, 9], comp [M, NC], kij / eab [M, NC, NC], and per mixture T, P, liquid x [NC], feed z [NC]"""
    tie = F.tie_line_points()
    M = len(MIXTURES)
    params, comp = [], np.full((M, NC), -1, dtype=np.int64)
    T, P, x, z = np.zeros(M), np.zeros(M), np.zeros((M, NC)), np.zeros((M, NC))
    kij, eab = np.zeros((M, NC, NC)), np.full((M, NC, NC), np.nan)
    for m, (point, slots, extra) in enumerate(MIXTURES):
        _, rows, T[m], P[m], zi, xi, _, _ = tie[point]
        assert len(rows) == len(slots) <= NC
        for s, row, zs, xs in zip(slots, rows, zi, xi):
            comp[m, s], z[m, s], x[m, s] = len(params), zs, xs
            params.append(list(row))
        for s, point2, k in extra:
            comp[m, s] = len(params)
            params.append(list(tie[point2][1][k]))
        # a different k_ij for every pair of every mixture, none of them zero; the lower triangle is not read
        for i in range(NC):
            for j in range(i + 1, NC):
                kij[m, i, j] = kij[m, j, i] = 0.004 * (m + 1) + 0.001 * (i + j)
    eab[1, 0, 2] = eab[1, 2, 0] = 2400.0  # ethanol + water: a cross value in place of the combining rule
    return np.array(params, dtype=np.float64), comp, kij, eab, T, P, x, z


def _launch(dev, entry, comp, kij, eab, owner, of):
    """outputs of one entry as host arrays; ``of``: the mixture of the table whose state each point takes"""
    from gnnepcsaft_amd import pcsaft
    params, _, _, _, T, P, x, z = _table()
    p, c, k, e, o, t, pp, xx, zz, rho = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
        params, comp, kij, eab, np.asarray(owner, dtype=np.int64), T[of], P[of], x[of], z[of], np.full(len(of), RHO))]
    out = {"state": lambda: pcsaft.mixture_state(p, c, xx, t, rho, o, k, e),
           "density": lambda: pcsaft.mixture_density(p, c, xx, t, pp, o, k, e),
           "ln_phi_state": lambda: pcsaft.mixture_ln_phi_state(p, c, xx, t, rho, o, k, e),
           "ln_phi": lambda: pcsaft.mixture_ln_phi(p, c, xx, t, pp, o, k, e, pure=True),
           "bubble": lambda: pcsaft.mixture_bubble_pressure(p, c, xx, t, o, k, e),
           "flash": lambda: pcsaft.mixture_tp_flash(p, c, zz, t, pp, o, k, e)}[entry]()
    return [v.cpu().numpy() for v in out]


def test_the_table_covers_what_it_should():
    _, comp, kij, eab, _, _, x, _ = _table()
    owner = np.array(OWNER)
    assert len(MIXTURES) >= 4 and set(OWNER) == set(range(len(MIXTURES))) and np.all(owner != np.arange(len(owner)))
    assert np.any(np.diff(owner) < 0) and len(owner) > len(set(OWNER))  # unsorted and repeated
    assert np.any(comp == -1) and np.any((comp != -1) & (x == 0.0)) and np.isfinite(eab).sum() == 2
    upper = kij[:, np.triu_indices(NC, 1)[0], np.triu_indices(NC, 1)[1]]
    assert np.all(upper != 0.0) and len(np.unique(upper)) == upper.size


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_point_reads_its_own_mixture(gpu_device, entry):
    _, comp, kij, eab, _, _, _, _ = _table()
    owner = np.array(OWNER)
    pooled = _launch(gpu_device, entry, comp, kij, eab, owner, owner)
    status = pooled[-1]
    # the k_ij here are this test's own, so no sibling test pins status 0 at these points: at least half of the launch
    # must solve, or most of it could go to a failure status unnoticed
    assert status.dtype == np.int32 and (status == 0).sum() >= len(owner) // 2, status.tolist()
    for m in range(len(MIXTURES)):
        sel = np.nonzero(owner == m)[0]
        alone = _launch(gpu_device, entry, comp[m:m + 1], kij[m:m + 1], eab[m:m + 1], np.zeros(len(sel)), owner[sel])
        assert len(alone) == len(pooled)
        for k, (a, b) in enumerate(zip(alone, pooled)):
            assert a.dtype == b.dtype and a.tobytes() == b[sel].tobytes(), (entry, "mixture", m, "output", k)
    # not vacuous: without the k_ij some output of the entry has other bytes
    plain = _launch(gpu_device, entry, comp, np.zeros_like(kij), eab, owner, owner)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(plain, pooled))
