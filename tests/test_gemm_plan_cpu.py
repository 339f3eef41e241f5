"""The decision table of gnx_gemm / gnx_gemm_grouped / gnx_gemm_grouped_rows (csrc/gnx_gemm_plan.hpp), pinned without a
device: tests/gemm_plan_probe.cpp is built with the host C++ compiler and asked for the plan of every row below.

The expected values were worked out BY HAND from gemm_launch as it stood before the plan existed (weights-stationary test
first, then SPLIT_ONLY below 4096 rows, small, mid, split images, fp32 fallback), never produced by the code under test.
Every row: 256 CUs, the option defaults of gnx_create (SPLIT 1, PIPE 1, AS 1, WS_FAST 2, TILE_ROWS 0, MID 1), b_trans,
K = N = 128, one segment, 16-byte aligned operands and a workspace, unless the query says otherwise.

Arithmetic used below: image bytes = classes * 3 * pad(N, 128) * Kpad * 2; persistent grid of k_gemm3 / k_gemm3p =
min(cdiv(row tiles, 8) * 8 * ny, 512 rounded down to a multiple of 8 * ny)."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NONE, VEC, GENERIC, WS, WS3, WS3_FAST8, WS3_FAST4, GEMM3, GEMM3P_96, GEMM3P_128, AS3, MID, SMALL = range(13)
NOTHING = (NONE, 0, 1, 256, 0, 0)

# (query, (kernel, grid_x, grid_y, block, tile_rows, image_bytes)[, {lds, run_split, stop, frag, Kpad}])
TABLE = [
    # ---- M = 0
    ("M=0", NOTHING),
    # ---- weights-stationary region: M 8191 | 8192; every condition of the shape broken in turn
    ("M=8192", (WS3_FAST4, 256, 1, 256, 32, 0), {"lds": 65536}),               # 256 tiles of 32 rows < 512 slots
    ("M=8191", (GEMM3, 64, 1, 256, 128, 98304), {"run_split": 1, "frag": 0, "Kpad": 128}),  # 4 K-tiles: not pipelined
    ("M=81920", (WS3_FAST4, 512, 1, 256, 32, 0)),                              # 2560 tiles on 2 x 256 workgroups
    ("M=81920 cus=304", (WS3_FAST4, 608, 1, 256, 32, 0)),
    ("M=8192 rowscale=1", (VEC, 64, 1, 256, 128, 0)),                          # row scale: no split either
    ("M=8192 mask=1 acc=1", (GEMM3, 64, 1, 256, 128, 98304)),                  # mask + accumulate is not weights-stationary
    ("M=8192 k=32", (WS3_FAST4, 256, 1, 256, 32, 0)),
    ("M=8192 k=28", (VEC, 64, 1, 256, 128, 0)),                                # K < 32; one K-tile: no split
    ("M=8192 k=132", (GEMM3, 64, 1, 256, 128, 122880), {"Kpad": 160}),         # K > 128
    ("M=8192 N=32", (WS3, 128, 1, 512, 64, 0), {"lds": 104448}),               # N != 128: predicated form
    ("M=8192 N=28", (GEMM3, 64, 1, 256, 128, 98304)),                          # N < 32
    ("M=8192 N=132", (GEMM3, 128, 1, 256, 128, 196608)),                       # N > 128: two column tiles
    ("M=8192 k=126 lda=128 ldb=128", (GENERIC, 64, 1, 256, 128, 0)),           # K % 4
    ("M=8192 N=126", (GEMM3, 64, 1, 256, 128, 98304)),                         # N % 4 (b_trans: the split path takes it)
    ("M=8192 a_off=4", (GENERIC, 64, 1, 256, 128, 0)),
    ("M=8192 lda=130", (GENERIC, 64, 1, 256, 128, 0)),
    ("M=8192 b_off=4", (GENERIC, 64, 1, 256, 128, 0)),
    ("M=8192 ldb=130", (GENERIC, 64, 1, 256, 128, 0)),
    ("M=8192 nseg=2 k=64", (GEMM3, 64, 1, 256, 128, 98304)),                   # two segments
    ("M=8192 grouped=1 max_tiles=70", (GEMM3, 72, 1, 256, 128, 98304)),        # grouped calls never go there
    # the forms of k_gemm_ws3: every WS_FAST value with N = 128 | 96, the accumulate epilogue, alignment of C and mask
    ("M=8192 WS_FAST=1", (WS3_FAST8, 128, 1, 512, 64, 0), {"lds": 104448}),
    ("M=81920 WS_FAST=1", (WS3_FAST8, 256, 1, 512, 64, 0)),
    ("M=8192 WS_FAST=0", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 N=96 WS_FAST=2", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 N=96 WS_FAST=1", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 N=96 WS_FAST=0", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 acc=1 WS_FAST=2", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 acc=1 WS_FAST=1", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 acc=1 WS_FAST=0", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 mask=1", (WS3_FAST4, 256, 1, 256, 32, 0)),
    ("M=8192 c_off=4", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 ldc=130", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 mask=1 mask_off=4", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 mask=1 ldmask=130", (WS3, 128, 1, 512, 64, 0)),
    ("M=8192 SPLIT=0", (WS, 128, 1, 512, 64, 0), {"lds": 135168}),
    ("M=8192 SPLIT=0 WS_FAST=1 N=96", (WS, 128, 1, 512, 64, 0)),
    ("M=8192 bt=0", (WS3_FAST4, 256, 1, 256, 32, 0)),
    ("M=8192 split_only=1", NOTHING),
    ("M=8192 presplit=1", (WS3_FAST4, 256, 1, 256, 32, 0), {"run_split": 0}),
    ("M=8192 ws=0", (WS3_FAST4, 256, 1, 256, 32, 0)),
    # ---- M 4095 | 4096: the split floor (and the end of the mid-size product)
    ("M=4096", (GEMM3, 32, 1, 256, 128, 98304)),
    ("M=4095", (MID, 256, 8, 256, 16, 0)),                                     # 32 tiles of 128 x 128 <= 48
    ("M=4095 split_only=1", NOTHING),
    ("M=4095 presplit=1", (MID, 256, 8, 256, 16, 0), {"run_split": 0}),
    ("M=4095 MID=0", (VEC, 32, 1, 256, 128, 0)),
    # ---- small product: M 256 | 257 with MID off; each condition broken
    ("M=256 MID=0", (SMALL, 128, 1, 256, 16, 0)),                              # 16 x 8 patches
    ("M=257 MID=0", (VEC, 3, 1, 256, 128, 0)),
    ("M=256", (MID, 16, 8, 256, 16, 0)),
    ("M=256 MID=0 mask=1", (VEC, 2, 1, 256, 128, 0)),
    ("M=256 MID=0 rowscale=1", (VEC, 2, 1, 256, 128, 0)),
    ("M=256 MID=0 nseg=2", (VEC, 2, 1, 256, 128, 0)),
    ("M=256 MID=0 grouped=1 max_tiles=5", (VEC, 5, 1, 256, 128, 0)),
    ("M=200 MID=0 split_only=1", NOTHING),
    ("M=200 MID=0 N=100 k=30 acc=1 bt=0", (SMALL, 91, 1, 256, 16, 0)),         # 13 x 7 patches, any shape
    # ---- mid-size product: 48 | 49 tiles of 128 x 128, plain and grouped
    ("M=768 N=1024", (MID, 48, 64, 256, 16, 0)),                               # 6 x 8 = 48
    ("M=896 N=896", (VEC, 7, 7, 256, 128, 0)),                                 # 7 x 7 = 49
    ("M=3072 N=256", (MID, 192, 16, 256, 16, 0)),                              # 24 x 2 = 48
    ("M=3073 N=256", (VEC, 25, 2, 256, 128, 0)),                               # 25 x 2 = 50
    ("M=650", (MID, 41, 8, 256, 16, 0)),
    ("M=650 grouped=1 max_tiles=9 classes=4 cls_stride=16384", (MID, 72, 8, 256, 16, 0)),  # 8 patches per table tile
    ("M=650 rowscale=1 k=30 N=50 bt=0 mask=1", (MID, 41, 4, 256, 16, 0)),       # the whole contract
    ("M=650 MID=0", (VEC, 6, 1, 256, 128, 0)),
    # ---- split images: 1 | 2 K-tiles
    ("M=5000 N=256 k=32", (VEC, 40, 2, 256, 128, 0)),
    ("M=5000 N=256 k=36", (GEMM3, 80, 1, 256, 128, 98304), {"Kpad": 64}),
    ("M=5000 N=256 nseg=2 k=16", (GEMM3, 80, 1, 256, 128, 98304), {"Kpad": 64}),  # every segment is padded to 32
    # ---- pipelined kernel: 7 | 8 K-tiles, tile height, PIPE off
    ("M=5000 k=224", (GEMM3, 40, 1, 256, 128, 172032), {"frag": 0, "lds": 0}),
    ("M=5000 k=256", (GEMM3P_96, 56, 1, 256, 96, 196608), {"frag": 1, "lds": 46848, "run_split": 1, "stop": 0}),  # 53 tiles of 96
    ("M=5000 k=256 TILE_ROWS=128", (GEMM3P_128, 40, 1, 256, 128, 196608), {"lds": 62464}),
    ("M=65536 k=256", (GEMM3P_128, 512, 1, 256, 128, 196608)),                 # exactly one round of 128-row tiles
    ("M=65536 k=256 TILE_ROWS=96", (GEMM3P_96, 512, 1, 256, 96, 196608)),
    ("M=5000 k=256 PIPE=0", (GEMM3, 40, 1, 256, 128, 196608), {"frag": 0}),
    ("M=5000 nseg=2 k0=128 k1=512", (GEMM3P_96, 56, 1, 256, 96, 491520), {"Kpad": 640}),
    # grouped: the caller's tile height, or 128; grid from the table's tile count
    ("M=5000 k=256 grouped=1 max_tiles=45 classes=2 cls_stride=32768", (GEMM3P_128, 48, 1, 256, 128, 393216)),
    ("M=5000 k=256 grouped=1 max_tiles=45 classes=2 cls_stride=32768 tile_rows=96", (GEMM3P_96, 48, 1, 256, 96, 393216)),
    ("M=5000 k=256 grouped=1 max_tiles=45 classes=2 cls_stride=32768 TILE_ROWS=96", (GEMM3P_128, 48, 1, 256, 128, 393216)),
    # ---- each condition of the split path broken in turn (base: the 8-K-tile row above)
    ("M=5000 k=256 SPLIT=0", (VEC, 40, 1, 256, 128, 0)),
    ("M=5000 k=256 rowscale=1", (VEC, 40, 1, 256, 128, 0)),
    ("M=5000 k=254 lda=256 ldb=256", (GENERIC, 40, 1, 256, 128, 0)),
    ("M=5000 k=256 bt=0 N=130 ldb=132", (GENERIC, 40, 2, 256, 128, 0)),        # N % 4 counts for [k][n] weights only
    ("M=5000 k=256 N=130", (GEMM3P_96, 112, 1, 256, 96, 393216)),              # 53 row tiles x 2 column tiles
    ("M=5000 k=256 a_off=4", (GENERIC, 40, 1, 256, 128, 0)),
    ("M=5000 k=256 lda=258", (GENERIC, 40, 1, 256, 128, 0)),
    ("M=5000 k=256 b_off=8", (GENERIC, 40, 1, 256, 128, 0)),
    ("M=5000 k=256 ldb=258", (GENERIC, 40, 1, 256, 128, 0)),
    ("M=5000 k=256 grouped=1 max_tiles=45 classes=2 cls_stride=6", (GENERIC, 45, 1, 256, 128, 0)),
    ("M=5000 k=256 ws=0", (VEC, 40, 1, 256, 128, 196608), {"run_split": 0}),   # no workspace: fp32 kernel, bytes still told
    ("M=5000 k=256 c_off=4 ldc=130", (GEMM3P_96, 56, 1, 256, 96, 196608)),     # C's alignment plays no part here
    # SPLIT_ONLY / PRESPLIT in the tiled region
    ("M=5000 k=256 split_only=1", (GEMM3P_96, 56, 1, 256, 96, 196608), {"run_split": 1, "stop": 1}),
    ("M=5000 k=256 presplit=1", (GEMM3P_96, 56, 1, 256, 96, 196608), {"run_split": 0, "stop": 0}),
    ("M=5000 k=256 split_only=1 presplit=1", (GEMM3P_96, 56, 1, 256, 96, 196608), {"run_split": 0, "stop": 1}),
    ("M=5000 k=256 split_only=1 rowscale=1", NOTHING),
    ("M=5000 k=256 split_only=1 ws=0", (NONE, 0, 1, 256, 0, 196608)),
    # ---- activation-stationary kernel: Kpad 96 | 128 | 160, N 128 | 256 | 320, the 2^30 bound, alignment, AS off
    ("M=5000 N=256", (AS3, 79, 1, 256, 64, 196608), {"frag": 1, "lds": 52736}),
    ("M=5000 N=256 k=100", (AS3, 79, 1, 256, 64, 196608), {"Kpad": 128}),
    ("M=5000 N=256 k=96", (GEMM3, 80, 1, 256, 128, 147456), {"Kpad": 96, "frag": 0}),
    ("M=5000 N=256 k=160", (GEMM3, 80, 1, 256, 128, 245760), {"Kpad": 160}),
    ("M=5000 N=128", (GEMM3, 40, 1, 256, 128, 98304)),
    ("M=5000 N=320", (GEMM3, 120, 1, 256, 128, 294912)),                       # 40 x 3 tiles; 504 slots
    ("M=5000 N=384", (AS3, 79, 1, 256, 64, 294912)),
    ("M=5000 N=256 AS=0", (GEMM3, 80, 1, 256, 128, 196608)),
    ("M=5000 N=256 nseg=2 k=64", (GEMM3, 80, 1, 256, 128, 196608), {"Kpad": 128}),
    ("M=5000 N=256 bt=0 relu=1 bias=1", (AS3, 79, 1, 256, 64, 196608)),
    ("M=4194302 N=256", (AS3, 65536, 1, 256, 64, 196608)),                     # M * ldc + N = 2^30 - 256
    ("M=4194303 N=256", (GEMM3, 512, 1, 256, 128, 196608)),                    # = 2^30
    ("M=2097151 N=256 mask=1 ldmask=512", (AS3, 32768, 1, 256, 64, 196608)),   # the wider of ldc and ldmask counts
    ("M=2097152 N=256 mask=1 ldmask=512", (GEMM3, 512, 1, 256, 128, 196608)),
    ("M=5000 N=256 c_off=4", (GEMM3, 80, 1, 256, 128, 196608)),
    ("M=5000 N=256 ldc=258", (GEMM3, 80, 1, 256, 128, 196608)),
    ("M=5000 N=256 mask=1", (AS3, 79, 1, 256, 64, 196608)),
    ("M=5000 N=256 mask=1 mask_off=4", (GEMM3, 80, 1, 256, 128, 196608)),
    ("M=5000 N=256 mask=1 ldmask=258", (GEMM3, 80, 1, 256, 128, 196608)),
    ("M=5000 N=256 bias=1 bias_off=4", (GEMM3, 80, 1, 256, 128, 196608)),
    ("M=5000 N=256 grouped=1 max_tiles=50 classes=3 cls_stride=32768", (AS3, 100, 1, 256, 64, 589824)),  # two per table tile
    ("M=5000 N=256 split_only=1", (AS3, 79, 1, 256, 64, 196608), {"run_split": 1, "stop": 1, "frag": 1}),
]
EXTRA_COLUMNS = {"lds": 6, "run_split": 7, "stop": 8, "frag": 9, "Kpad": 10}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++ or $CXX)")
    exe = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_probe"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'gnnepcsaft_amd' / 'csrc'}", str(ROOT / "tests" / "gemm_plan_probe.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)

    def ask(queries):
        r = subprocess.run([str(exe)], input="\n".join(queries) + "\n", check=True, capture_output=True, text=True)
        lines = r.stdout.splitlines()
        assert len(lines) == len(queries)
        return [[int(v) for v in line.split()] for line in lines]
    return ask


def test_decision_table(probe):
    answers = probe([row[0] for row in TABLE])
    wrong = []
    for row, got in zip(TABLE, answers):
        want = list(row[1])
        extra = row[2] if len(row) > 2 else {}
        if got[:6] != want or any(got[EXTRA_COLUMNS[k]] != v for k, v in extra.items()):
            wrong.append((row[0], got, want, extra))
    assert not wrong, "\n".join(f"{q}: got {g}, expected {w} {e}" for q, g, w, e in wrong)


def test_every_kernel_kind_is_in_the_table():
    assert {row[1][0] for row in TABLE} == set(range(13))


def test_tile_rows_choice(probe):
    """The three facts tests/test_gemm_split_gpu.py pins through gnx_gemm_tile_rows, and the forced heights."""
    got = probe(["op=tile_rows M=81920 N=128",    # 640 tiles on 512 slots -> 854 tiles of 96
                 "op=tile_rows M=65536 N=128",    # exactly one round of 512
                 "op=tile_rows M=327680 N=128",   # five rounds of 128 rows against seven of 96
                 "op=tile_rows M=65536 N=128 forced=96", "op=tile_rows M=81920 N=128 forced=128",
                 "op=tile_rows M=81920 N=128 forced=64"])
    assert [g[0] for g in got] == [96, 128, 128, 96, 128, 96]


@pytest.mark.parametrize("T,F,D", [(1, 128, 5), (4, 32, 13), (1, 20, 1)])
def test_image_bytes_match_the_layer_workspace_formulas(probe, T, F, D):
    """gnx_pna_conv's workspace regions (pna_ws_sizes, gnx_layer.hip) as they were spelled by hand: N padded to 128, every k
    to 32, 3 pieces, 2 bytes, x classes."""
    def pad(v, m):
        return (v + m - 1) // m * m
    grouped = D * 3 * pad(4 * F, 128) * pad(F, 32) * 2
    dx = 3 * pad(F, 128) * (3 * pad(F, 32)) * 2
    lin = 3 * pad(T * F, 128) * pad(T * F, 32) * 2
    post0 = D * 3 * pad(F, 128) * (pad(F, 32) + pad(4 * F, 32)) * 2
    kF, k4F, kH = (g[0] for g in probe([f"op=kpad k={F}", f"op=kpad k={4 * F}", f"op=kpad k={T * F}"]))
    assert (kF, k4F, kH) == (pad(F, 32), pad(4 * F, 32), pad(T * F, 32))
    got = probe([f"op=image_bytes classes={D} N={4 * F} kpad={kF}", f"op=image_bytes classes=1 N={F} kpad={3 * kF}",
                 f"op=image_bytes classes=1 N={T * F} kpad={kH}", f"op=image_bytes classes={D} N={F} kpad={kF + k4F}"])
    assert [g[0] for g in got] == [grouped, dx, lin, post0]
    # and through whole plans: the grouped dA product (N = 4F, K = F) and the 3-segment dx product (N = F, K = 3F)
    # (a dA product with K = F <= 32 has one K-tile and takes no images: the layer's figure is an upper bound there)
    plans = probe([f"M=5000 N={4 * F} k={F} bt=0 grouped=1 max_tiles=60 classes={D} cls_stride={4 * F * F}",
                   f"M=5000 N={F} nseg=3 k={F} bt=0"])
    assert plans[0][5] == (grouped if kF >= 64 else 0) and plans[1][5] == dx
