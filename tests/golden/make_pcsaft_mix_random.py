"""Writes tests/golden/pcsaft_mix_random.json: the oracle's results on the seeded random mixtures of
tests/pcsaft_mix_cases.py -- the critical temperature of the lightest component of each of the 300 mixtures
(tests/pcsaft_ref.py critical_temperature) and the oracle density of each of the 1200 points (tests/pcsaft_mix_ref.py
density, null where it finds no root).  These take minutes on a CPU, so the GPU test reads them from here;
tests/test_pcsaft_mix_cpu.py recomputes a sample on every run.

Run from the repository root:  python tests/golden/make_pcsaft_mix_random.py
"""
import json
import os
import sys
from multiprocessing import Pool

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import pcsaft_mix_cases as C  # noqa: E402


def _tc(row):
    return C.R.critical_temperature(row, tol=0.5)


def _rho(job):
    return C.oracle_point(C.random_groups(job[0])[job[1]], job[2])


def main():
    with Pool(8) as pool:
        tc = pool.map(_tc, [g["rows"][r].tolist() for g in C.random_groups() for r in g["light"]])
        jobs = [(tuple(tc), k, j) for k, g in enumerate(C.random_groups(tc)) for j in range(len(g["owner"]))]
        rho = pool.map(_rho, jobs, chunksize=25)
    with open(C.RANDOM, "w") as fh:
        json.dump({"source": "written by tests/golden/make_pcsaft_mix_random.py", "seed": C.SEED, "tc": tc, "rho": rho},
                  fh, separators=(",", ":"))
    ok = sum(r is not None for r in rho)
    print("wrote", C.RANDOM, os.path.getsize(C.RANDOM), "bytes;", ok, "of", len(rho), "points have a root")


if __name__ == "__main__":
    main()
