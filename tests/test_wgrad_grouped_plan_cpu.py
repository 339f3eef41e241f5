"""The host-only plan of the per-class weight gradient (csrc/gnx_wgrad_plan.hpp: which kernel a gnx_gemm_wgrad_grouped call
takes, how many ranges k_gemm_wgrad3p_grouped cuts the chunk table into and how many chunks each owns), through the
stand-alone probe tests/wgrad_grouped_plan_probe.cpp, against a plain restatement of the rule -- no GPU."""
import itertools
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NONE, F32_VEC, F32_GENERIC, SPLIT3, SPLIT3P_GROUPED = range(5)
DEFAULT_BUDGET = 256   # WGRAD_GROUPED_WGS


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++ or $CXX)")
    exe = tmp_path_factory.mktemp("wgrad_plan") / "wgrad_grouped_plan_probe"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'gnnepcsaft_amd' / 'csrc'}",
                    str(ROOT / "tests" / "wgrad_grouped_plan_probe.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)

    def ask(queries):
        text = "\n".join(" ".join(str(int(v)) for v in q) for q in queries) + "\n"
        r = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True)
        lines = r.stdout.splitlines()
        assert len(lines) == len(queries)
        return [tuple(int(v) for v in line.split()) for line in lines]
    return ask


def _cdiv(a, b):
    return -(-a // b)


def expected(M, N, K, budget, max_chunks, off_x=0, off_a=0, lddc=0, lda=0, split=1, pipe=1):
    lddc, lda = lddc or N, lda or K
    vec = off_x % 16 == 0 and off_a % 16 == 0 and lddc % 4 == 0 and lda % 4 == 0 and N % 4 == 0 and K % 4 == 0
    wsplit = M >= 4096 and split != 0 and M * lddc < 2 ** 32 and M * lda < 2 ** 32
    tiles = _cdiv(N, 128) * _cdiv(K, 128)
    ranges = max(1, (budget if budget > 0 else DEFAULT_BUDGET) // tiles)
    S = _cdiv(max_chunks, ranges)
    if M == 0:
        return NONE, ranges, S, 0
    if wsplit and vec and pipe != 0:
        return SPLIT3P_GROUPED, ranges, S, _cdiv(max_chunks, S)
    return (SPLIT3 if wsplit else (F32_VEC if vec else F32_GENERIC)), ranges, S, max_chunks


def test_ranges_and_chunks_per_range_over_a_grid(probe):
    """Budgets above the chunk count (S = 1, grid_x = max_chunks), below the number of output tiles (one range) and the
    default (0); one to twelve output tiles; chunk tables of 1 to 645 entries."""
    grid = list(itertools.product((4096, 4327, 81920), (32, 128, 260), (128, 512, 516), (0, 1, 3, 4, 16, 64, 128, 256, 1000),
                                  (1, 9, 12, 85, 645)))
    queries = [(M, N, K, b, mc, 0, 0, 0, 0, 1, 1) for M, N, K, b, mc in grid]
    got = probe(queries)
    wrong = [(q, g, expected(*q)) for q, g in zip(queries, got) if g != expected(*q)]
    assert not wrong, wrong[:5]
    kinds = {g[0] for g in got}
    assert kinds == {SPLIT3P_GROUPED}
    assert any(g[2] == 1 and g[3] == q[4] for q, g in zip(queries, got) if q[3] > q[4] > 1)   # budget > chunks
    assert any(g[1] == 1 and g[3] == 1 for q, g in zip(queries, got) if 0 < q[3] < 4 and q[1] == 128 and q[2] == 512)


def test_the_cases_of_the_benchmark_and_of_the_gpu_tests(probe):
    got = probe([(81920, 128, 512, 0, 85, 0, 0, 128, 512, 1, 1),      # cfg-2: 64 ranges of 2 chunks, 43 of them launched
                 (4327, 32, 128, 4, 12, 0, 0, 64, 256, 1, 1),         # tests/test_wgrad_grouped_pipe_gpu.py
                 (4327, 128, 512, 16, 12, 0, 0, 256, 1024, 1, 1),
                 (4327, 128, 512, 4, 12, 0, 0, 256, 1024, 1, 1)])
    assert got == [(SPLIT3P_GROUPED, 64, 2, 43), (SPLIT3P_GROUPED, 4, 3, 4), (SPLIT3P_GROUPED, 4, 3, 4),
                   (SPLIT3P_GROUPED, 1, 12, 1)]


def test_which_calls_keep_the_older_kernels(probe):
    """(query, kernel): misaligned by four bytes, a leading dimension or a shape that is no multiple of 4, the switches, a
    row count below the split path, offsets that need more than 32 bits, no rows."""
    table = [((4327, 32, 128, 4, 12, 4, 0, 0, 0, 1, 1), SPLIT3), ((4327, 32, 128, 4, 12, 0, 4, 0, 0, 1, 1), SPLIT3),
             ((4327, 32, 128, 4, 12, 0, 0, 33, 0, 1, 1), SPLIT3), ((4327, 32, 128, 4, 12, 0, 0, 0, 130, 1, 1), SPLIT3),
             ((4500, 65, 260, 4, 12, 0, 0, 0, 0, 1, 1), SPLIT3), ((4327, 32, 128, 4, 12, 0, 0, 0, 0, 1, 0), SPLIT3),
             ((4327, 32, 128, 4, 12, 0, 0, 0, 0, 0, 1), F32_VEC), ((4327, 32, 128, 4, 12, 4, 0, 0, 0, 0, 1), F32_GENERIC),
             ((4095, 32, 128, 4, 12, 0, 0, 0, 0, 1, 1), F32_VEC), ((700, 65, 260, 4, 8, 0, 0, 0, 0, 1, 1), F32_GENERIC),
             ((2 ** 23, 128, 512, 0, 8200, 0, 0, 0, 0, 1, 1), F32_VEC), ((2 ** 22, 128, 512, 0, 4100, 0, 0, 0, 0, 1, 1), SPLIT3P_GROUPED),
             ((0, 32, 128, 4, 12, 0, 0, 0, 0, 1, 1), NONE)]
    got = probe([q for q, _ in table])
    for (q, kernel), g in zip(table, got):
        assert g == expected(*q) and g[0] == kernel, (q, g, kernel)
