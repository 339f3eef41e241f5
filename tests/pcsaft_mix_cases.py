"""Shared inputs of the mixture PC-SAFT tests (tests/test_pcsaft_mix_cpu.py, tests/test_pcsaft_mix_gpu.py): the points of
the binary ThermoML fixture with their oracle densities (computed once per session), and the seeded random mixtures with
the oracle results recorded in tests/golden/pcsaft_mix_random.json (tests/golden/make_pcsaft_mix_random.py writes it;
the CPU test recomputes a sample of it)."""
import functools
import json
import os

import numpy as np

from tests import pcsaft_mix_ref as MR
from tests import pcsaft_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "pcsaft_binary_thermoml.json")
RANDOM = os.path.join(GOLDEN, "pcsaft_mix_random.json")
PAIRS = ("NN", "DN", "DD", "AN", "AD", "AA")
SEED = 11
# 300 mixtures: (slots nc, mixtures, of which one slot is marked -1)
GROUPS = ((1, 40, 0), (2, 100, 30), (3, 80, 35), (4, 80, 35))
STATES = 4


@functools.lru_cache(maxsize=None)
def systems():
    with open(FIXTURE) as fh:
        return json.load(fh)["systems"]


@functools.lru_cache(maxsize=None)
def fixture_points():
    """(params [48, 9], comp [24, 2], owner [n], T [n], P [n], x [n, 2], measured rho [n])"""
    sy = systems()
    params = np.array([p for s in sy for p in s["params"]], dtype=np.float64)
    comp = np.arange(2 * len(sy), dtype=np.int64).reshape(-1, 2)
    owner = np.array([i for i, s in enumerate(sy) for _ in s["points"]], dtype=np.int64)
    pts = np.array([p for s in sy for p in s["points"]], dtype=np.float64)
    return params, comp, owner, pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2:4].copy(), pts[:, 4].copy()


@functools.lru_cache(maxsize=None)
def fixture_oracle():
    """oracle density (mol/m³) of every fixture point with k_ij = 0; NaN where the oracle finds no root"""
    params, comp, owner, T, P, x, _ = fixture_points()
    out = [MR.density(MR.Mixture(params[comp[o]], xi), t, p) for o, t, p, xi in zip(owner, T, P, x)]
    return np.array([np.nan if r is None else r for r in out])


def random_rows(rng, n):
    """n rows drawn with the ranges, and in the order, of tests/test_pcsaft_gpu.py::_random_rows (restated here so that
    the CPU suite and the fixture generator do not import a GPU test module; the recorded results pin the draws)"""
    m = rng.uniform(1.0, 25.0, n)
    sigma = rng.uniform(1.9, 4.5, n)
    eps = rng.uniform(50.0, 550.0, n)
    kab = rng.uniform(1e-4, 0.9, n)
    eab = rng.uniform(200.0, 5000.0, n)
    mu = rng.uniform(0.0, 4.0, n)
    na, nb = rng.integers(0, 3, n).astype(np.float64), rng.integers(0, 3, n).astype(np.float64)
    return np.stack([m, sigma, eps, kab, eab, mu, na, nb, np.full(n, 100.0)], axis=1)


def random_groups(tc=None):
    """The seeded random mixtures, one dict per slot count nc: rows [B, 9], comp [M, nc] (-1 = unused slot), kij
    [M, nc, nc] (symmetric, from [-0.1, 0.1]), light [M] (row of the present component with the fewest segments), and
    -- when the critical temperatures ``tc`` [300] of those rows are given -- owner / T / P [M * 4], x [M * 4, nc]: T
    from 0.5 to 0.9 of tc, P log-uniform in [1e5, 1e7] Pa."""
    rng = np.random.default_rng(SEED)
    groups, first = [], 0
    for nc, M, holes in GROUPS:
        rows = random_rows(rng, M * nc)
        comp = np.arange(M * nc, dtype=np.int64).reshape(M, nc)
        for i in rng.choice(M, holes, replace=False):
            comp[i, rng.integers(0, nc)] = -1
        k = rng.uniform(-0.1, 0.1, (M, nc, nc))
        kij = np.triu(k, 1) + np.transpose(np.triu(k, 1), (0, 2, 1))
        used = comp >= 0
        mseg = np.where(used, rows[np.maximum(comp, 0), 0], np.inf)
        light = comp[np.arange(M), np.argmin(mseg, axis=1)]
        g = {"nc": nc, "rows": rows, "comp": comp, "kij": kij, "light": light, "first": first}
        frac = rng.uniform(0.5, 0.9, (M, STATES))
        P = 10.0 ** rng.uniform(5.0, 7.0, (M, STATES))
        x = rng.uniform(0.05, 1.0, (M, STATES, nc)) * used[:, None, :]
        if tc is not None:
            g.update(owner=np.repeat(np.arange(M), STATES), P=P.reshape(-1), x=x.reshape(-1, nc),
                     T=(frac * np.asarray(tc)[first:first + M, None]).reshape(-1))
        groups.append(g)
        first += M
    return groups


def oracle_point(g, j):
    """oracle density of point j of a random group, None where there is no root"""
    o = g["owner"][j]
    slots = g["comp"][o] >= 0
    mix = MR.Mixture(g["rows"][g["comp"][o][slots]], g["x"][j][slots], kij=g["kij"][o][np.ix_(slots, slots)])
    return MR.density(mix, g["T"][j], g["P"][j])


@functools.lru_cache(maxsize=None)
def recorded():
    """(groups with states, oracle rho [1200] with NaN where the oracle found no root)"""
    with open(RANDOM) as fh:
        doc = json.load(fh)
    assert doc["seed"] == SEED
    rho = np.array([np.nan if r is None else r for r in doc["rho"]], dtype=np.float64)
    return random_groups(doc["tc"]), rho
