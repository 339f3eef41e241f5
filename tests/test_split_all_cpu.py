"""Where gnx_pna_split_all puts every PNA layer's split weight images, and what the records say (csrc/gnx_gemm_plan.hpp:
pna_images_layout, gemm_image_of, gemm_image_equal), pinned without a device: tests/split_all_probe.cpp is built with the
host C++ compiler.

Expected values are worked out BY HAND from DESIGN.md's formula, image bytes = classes * 3 * pad(N, 128) * sum pad(k, 32) * 2,
and from the layer's three products (F = features per tower, D = degree classes):
    post-layer 0   N = F,  K = F + 4F, D classes, [n][k] weights
    dA             N = 4F, K = F,      D classes, [k][n] weights
    dx             N = F,  K = 3 x F,  1 class,   [k][n] weights
A product reads images from 4096 rows and two K-tiles (of 32) on; its images are fragment-major from 8 K-tiles on, or when
it takes the one-segment 4-K-tile kernel with N >= 256 (k_gemm_as3: dA at F = 128).  Regions lie back to back per (layer,
tower) in the order post-layer 0, dA, dx."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++ or $CXX)")
    exe = tmp_path_factory.mktemp("split_all") / "split_all_probe"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'gnnepcsaft_amd' / 'csrc'}",
                    str(ROOT / "tests" / "split_all_probe.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)

    def ask(query):
        r = subprocess.run([str(exe)], input=query + "\n", check=True, capture_output=True, text=True)
        parts = [[int(v) for v in p.split() if v != "rec"] for p in r.stdout.strip().split("|")]
        return parts
    return ask


POST0_128, DA_128, DX_128 = 5 * 491520, 5 * 393216, 294912  # 5*3*128*640*2, 5*3*512*128*2, 1*3*128*384*2
LAYER_128 = 4718592


def test_one_layer_f128(probe):
    assert POST0_128 == 5 * 3 * 128 * (128 + 512) * 2 and DA_128 == 5 * 3 * 512 * 128 * 2 and DX_128 == 3 * 128 * 384 * 2
    assert POST0_128 + DA_128 + DX_128 == LAYER_128
    head, regions, rec = probe("F=128 T=1 D=5 N=4096")
    assert head == [LAYER_128, 3]
    assert regions == [0, POST0_128, POST0_128, DA_128, POST0_128 + DA_128, DX_128]
    #              bytes  classes Npad Kpad koff[5]                 frag bt
    assert rec == [POST0_128, 5, 128, 640, 0, 128, 640, 640, 640, 1, 1,    # 20 K-tiles: fragment-major; [n][k]
                   DA_128, 5, 512, 128, 0, 128, 128, 128, 128, 1, 0,       # 4 K-tiles, N = 512: k_gemm_as3, fragment-major
                   DX_128, 1, 128, 384, 0, 128, 256, 384, 384, 1, 0]       # 12 K-tiles


def test_six_layers_offsets(probe):
    parts = probe("L=6 F=128 T=1 D=5 N=4096")
    assert parts[0] == [6 * LAYER_128, 18]      # cfg-2: 18 problems, one launch of up to 32
    for l in range(6):
        o = l * LAYER_128
        assert parts[1 + l] == [o, POST0_128, o + POST0_128, DA_128, o + POST0_128 + DA_128, DX_128]


def test_d1(probe):
    head, regions, _ = probe("F=128 T=1 D=1 N=4096")
    assert head == [491520 + 393216 + 294912, 3]
    assert regions == [0, 491520, 491520, 393216, 491520 + 393216, 294912]


def test_f32_single_k_tile_has_no_image(probe):
    """F = 32: N pads 32 -> 128; dA has K = 32 = one K-tile: no image, no problem, no room."""
    post0, dx = 5 * 3 * 128 * (32 + 128) * 2, 3 * 128 * 96 * 2
    assert (post0, dx) == (614400, 73728)
    head, regions, rec = probe("F=32 T=1 D=5 N=4096")
    assert head == [post0 + dx, 2]
    assert regions == [0, post0, -1, 0, post0, dx]
    assert rec == [post0, 5, 128, 160, 0, 32, 160, 160, 160, 0, 1,   # 5 K-tiles: tile-major
                   0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                   dx, 1, 128, 96, 0, 32, 64, 96, 96, 0, 0]
    # two towers: tower 1's regions follow tower 0's
    parts = probe("F=32 T=2 D=5 N=4096")
    assert parts[0] == [2 * (post0 + dx), 4]
    assert parts[1] == [0, post0, -1, 0, post0, dx]
    assert parts[2] == [post0 + dx, post0, -1, 0, 2 * post0 + dx, dx]


def test_f64_layouts(probe):
    """F = 64: post-layer 0 has 10 K-tiles (fragment-major), dA 2 and dx 6 (tile-major)."""
    head, _, rec = probe("F=64 T=1 D=5 N=4096")
    post0, dA, dx = 5 * 3 * 128 * 320 * 2, 5 * 3 * 256 * 64 * 2, 3 * 128 * 192 * 2
    assert head == [post0 + dA + dx, 3]
    assert rec == [post0, 5, 128, 320, 0, 64, 320, 320, 320, 1, 1,
                   dA, 5, 256, 64, 0, 64, 64, 64, 64, 0, 0,
                   dx, 1, 128, 192, 0, 64, 128, 192, 192, 0, 0]


def test_nothing_below_4096_rows(probe):
    head, regions, rec = probe("F=128 T=1 D=5 N=4095")
    assert head == [0, 0]
    assert regions == [-1, 0, -1, 0, -1, 0]
    assert rec == [0] * 33
    assert probe("L=6 F=128 T=1 D=5 N=0")[0] == [0, 0]


def test_split_option_off_gives_nothing(probe):
    assert probe("F=128 T=1 D=5 N=4096 SPLIT=0")[0] == [0, 0]


def test_unaligned_weight_gives_no_image(probe):
    """Post-layer 0's weight 4 bytes off 16-byte alignment: the two products that read it (post-layer 0, dx) stay on the
    fp32 kernel and bring no image; dA reads Weff alone."""
    head, regions, _ = probe("F=128 T=1 D=5 N=4096 w_off=4")
    assert head == [DA_128, 1]
    assert regions == [-1, 0, 0, DA_128, -1, 0]


def test_record_equality(probe):
    base = "a_F=128 a_D=5 b_F=128 b_D=5 "
    eq = lambda q: probe("op=equal " + base + q)[0]  # noqa: E731
    # the row count enters the images only through the 4096-row threshold
    assert eq("a_N=4096 b_N=4096") == [1, 1, 1]
    assert eq("a_N=4096 b_N=8192") == [1, 1, 1]
    assert eq("a_N=4096 b_N=4095") == [0, 0, 0]
    assert eq("a_N=4095 b_N=100") == [1, 1, 1]           # (both empty)
    # GNX_OPT_GEMM_SPLIT
    assert eq("a_N=4096 b_N=4096 b_SPLIT=0") == [0, 0, 0]
    assert eq("a_N=4096 a_SPLIT=0 b_N=4096 b_SPLIT=0") == [1, 1, 1]
    # the tile height of the forward's degree-class table picks k_gemm3p<96> or <128>; both read the same fragment-major
    # images, so the height does NOT enter the record: pinned here
    assert eq("a_N=4096 a_tile_rows=96 b_N=4096 b_tile_rows=128") == [1, 1, 1]
    # the layout does: without the pipelined kernel post-layer 0 and dx are tile-major, without k_gemm_as3 dA is
    assert eq("a_N=4096 b_N=4096 b_PIPE=0") == [0, 1, 0]
    assert eq("a_N=4096 b_N=4096 b_AS=0") == [1, 0, 1]
    # another class count or width
    assert probe("op=equal a_F=128 a_D=5 b_F=128 b_D=4")[0] == [0, 0, 1]
    assert probe("op=equal a_F=128 a_D=5 b_F=64 b_D=5")[0] == [0, 0, 0]
