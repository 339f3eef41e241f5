"""The host-only plan of the fused dA product + scatter-aggregate backward (pna_dA_agg_plan_of, csrc/gnx_gemm_plan.hpp: whether
a tower's call takes k_pna_dA_agg_bwd or keeps the two launches), through the stand-alone probe tests/dA_agg_plan_probe.cpp:
both sides of every eligibility condition -- no GPU."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
TILED_VEC, TILED_GENERIC, GEMM3, AS3 = 1, 2, 7, 10     # GNX_GEMM_KERNEL_*
LDS = 3 * 32 * 272 + 32 * 4                            # three bf16 images of a 32-row tile + its row ids
FIELDS = ("N", "E", "T", "F", "D", "max_tiles", "off_g", "off_dA", "off_m", "off_ge", "off_w", "have_ws", "FUSED", "SPLIT", "AS",
          "grouped")
BASE = dict(N=4096, E=9000, T=1, F=128, D=5, max_tiles=37, off_g=0, off_dA=0, off_m=0, off_ge=0, off_w=0, have_ws=1, FUSED=1,
            SPLIT=1, AS=1, grouped=1)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++ or $CXX)")
    exe = tmp_path_factory.mktemp("dA_agg_plan") / "dA_agg_plan_probe"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'gnnepcsaft_amd' / 'csrc'}",
                    str(ROOT / "tests" / "dA_agg_plan_probe.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)

    def ask(**changes):
        q = dict(BASE, **changes)
        text = " ".join(str(int(q[k])) for k in FIELDS) + "\n"
        r = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True)
        fused, kernel, grid_x, lds = (int(v) for v in r.stdout.split())
        return fused, kernel, grid_x, lds
    return ask


def test_the_eligible_call_and_its_launch_shape(probe):
    """Four 32-row parts per (96- or 128-row) class tile, the tile's three images and row ids in LDS."""
    assert probe() == (1, AS3, 4 * 37, LDS)
    assert probe(T=2) == (1, AS3, 4 * 37, LDS)
    assert probe(N=81920, E=163840, max_tiles=645) == (1, AS3, 4 * 645, LDS)      # the cfg-2 layer


@pytest.mark.parametrize("changes,kernel", [
    (dict(FUSED=0), AS3),            # the option
    (dict(N=4095), TILED_VEC),       # below the split path's 4096 rows
    (dict(F=64), GEMM3),             # two K-tiles: the product is not k_gemm_as3's
    (dict(F=96), GEMM3),
    (dict(AS=0), GEMM3),
    (dict(SPLIT=0), TILED_VEC),
    (dict(have_ws=0), TILED_VEC),    # no workspace, no images
    (dict(grouped=0), AS3),          # k_gemm_as3, but not over degree classes
    (dict(max_tiles=0), AS3),
    (dict(off_m=4), AS3),            # messages or their gradient not 16-byte aligned
    (dict(off_ge=4), AS3),
    (dict(off_g=4), TILED_GENERIC),  # an unaligned product operand leaves the split path altogether
    (dict(off_w=4), TILED_GENERIC),
    (dict(off_dA=4), GEMM3),         # k_gemm_as3 stores 16 bytes at a time
])
def test_what_keeps_the_two_launches(probe, changes, kernel):
    assert probe(**changes) == (0, kernel, 0, 0)


def test_offsets_beyond_32_bits(probe):
    """(E + 1) H < 2^31 for the message rows; the product's own bound (M ldc + N < 2^30, k_gemm_as3) is the tighter one on N."""
    assert probe(E=2 ** 24 - 2)[0] == 1              # (E + 1) 128 = 2^31 - 128
    assert probe(E=2 ** 24 - 1) == (0, AS3, 0, 0)    # 2^31
    assert probe(E=2 ** 23 - 2, T=2)[0] == 1
    assert probe(E=2 ** 23 - 1, T=2) == (0, AS3, 0, 0)
    assert probe(N=2 ** 21 - 2, max_tiles=2 ** 14 + 5)[0] == 1
    assert probe(N=2 ** 21 - 1, max_tiles=2 ** 14 + 5) == (0, GEMM3, 0, 0)
