"""k_gemm_wgrad3p_grouped (gnx_wgrad.hip): the per-degree-class weight gradient over merged class runs, against the exact
references of tests/wgrad_ref.py.  Which kernel a case reaches is asked of the library (gnx_gemm_wgrad_grouped_plan), not of
a mirror.

The class sizes give 9 chunks in a table of 12; with four ranges every workgroup owns S = 3 chunks:
  range 0: runs of 37, 1 and 1024 rows (a run shorter than the prologue depth, a one-row run, the class after an empty one);
  range 1: one merged run of 1025 rows (chunk of 1024 + chunk of 1), then the first 1024 rows of the next class;
  range 2: runs of 1023 (the rest of that class), 33 and 160 rows;          range 3: no chunk.
With one range a single workgroup walks all seven runs (37, 1, 1024, 1025, 2047, 33, 160)."""
import functools

import pytest
import torch

from tests import test_wgrad_gpu as T
from tests import wgrad_ref as R

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZES = (37, 1, 0, 1024, 1025, 2047, 33, 160)
NEW, OLD = "k_gemm_wgrad3p_grouped", "k_gemm_wgrad3<true>"
# first positions (in dperm) of the runs of ranges 0, 1, 2 at S = 3
RUNS_S3 = ((0, 37), (37, 1), (38, 1024), (1062, 1025), (2087, 1024), (3111, 1023), (4134, 33), (4167, 160))


def _graph():
    g, pack, dc = T._class_graph(SIZES)
    assert g.N == 4327 and g.D == 8 and dc.max_chunks == 12
    assert g.chunks() == [(0, 37, 0), (37, 1, 1), (38, 1024, 3), (1062, 1024, 4), (2086, 1, 4), (2087, 1024, 5),
                          (3111, 1023, 5), (4134, 33, 6), (4167, 160, 7)]
    return g, pack, dc


@functools.lru_cache(maxsize=None)
def _ints(F):
    g, _, _ = _graph()
    gen = torch.Generator().manual_seed(1000 + F)
    gr = torch.randint(-8, 9, (g.N, F), generator=gen).float()
    A = torch.randint(-8, 9, (g.N, 4 * F), generator=gen).float()
    init = torch.randint(1, 100, (g.D, F, 4 * F), generator=gen).float()
    return gr, A, init, R.class_sums_int(gr, A, g)


def _tower_views(gr, A, shift=0):
    """The operands as the layer passes them for tower 1 of T = 2: columns [F, 2F) of a [N, 2F] buffer and [4F, 8F) of a
    [N, 8F] one; ``shift`` floats further right (4-byte misaligned for shift = 1) in buffers that much wider."""
    F = gr.size(1)
    gb = torch.full((gr.size(0), 2 * F + shift), 5.0)
    ab = torch.full((A.size(0), 8 * F + shift), -3.0)
    gb[:, F + shift:2 * F + shift] = gr
    ab[:, 4 * F + shift:8 * F + shift] = A
    return gb.to(DEV)[:, F + shift:2 * F + shift], ab.to(DEV)[:, 4 * F + shift:8 * F + shift]


def _guarded(init, guard=64):
    n = init.numel()
    host = torch.full((n + 2 * guard,), 9.0)
    host[guard:guard + n] = init.flatten()
    flat = host.to(DEV)
    return host, flat, flat[guard:guard + n].view(init.shape)


def _check_plan(ops, grd, Ad, dc, kernel, ranges=None, S=None):
    name, info = ops.gemm_wgrad_grouped_plan(grd, Ad, dc.max_chunks)
    assert name == kernel, (name, kernel)
    if ranges is not None:
        assert (info.ranges, info.chunks_per_range, info.grid_x) == (ranges, S, -(-dc.max_chunks // S))
        assert (info.grid_y, info.grid_z, info.block) == (-(-grd.size(1) // 128), -(-Ad.size(1) // 128), 512)


# id: (F, GNX_OPT_WGRAD_WGS, ranges, S)
INT_CASES = {"F32_four_ranges": (32, 4, 4, 3), "F128_four_ranges": (128, 16, 4, 3), "F128_one_range_seven_runs": (128, 4, 1, 12)}


@pytest.mark.parametrize("name", sorted(INT_CASES))
def test_integer_exact_over_merged_runs(gpu_device, name):
    """Integer operands as column views of wider buffers, dW pre-filled with non-zero integers between guard words: every
    class must EQUAL init + the int64 class sum, and the guards keep their bytes."""
    from gnnepcsaft_amd import ops
    F, wgs, ranges, S = INT_CASES[name]
    g, _, dc = _graph()
    gr, A, init, sums = _ints(F)
    grd, Ad = _tower_views(gr, A)
    assert grd.data_ptr() % 16 == 0 and Ad.data_ptr() % 16 == 0 and grd.stride(0) == 2 * F and Ad.stride(0) == 8 * F
    host, flat, dW = _guarded(init)
    with T._options(wgs):
        _check_plan(ops, grd, Ad, dc, NEW, ranges, S)
        ops.gemm_wgrad_grouped(grd, Ad, dW, dc)
        torch.cuda.synchronize()
    got = flat.cpu()
    assert torch.equal(got[:64], host[:64]) and torch.equal(got[-64:], host[-64:])
    got = got[64:-64].view(init.shape)
    for c in range(g.D):
        T._assert_same(got[c], init[c] + sums[c], f"{name}: class {c} of {SIZES[c]} rows")


@pytest.mark.parametrize("F", [32, 128])
def test_misaligned_views_keep_the_two_barrier_kernel(gpu_device, F):
    """The same call on views that start 4 bytes off a 16-byte boundary: the plan names k_gemm_wgrad3<true>, and the result
    equals the same reference."""
    from gnnepcsaft_amd import ops
    g, _, dc = _graph()
    gr, A, init, sums = _ints(F)
    grd, Ad = _tower_views(gr, A, shift=1)
    assert grd.data_ptr() % 16 == 4 and Ad.data_ptr() % 16 == 4
    host, flat, dW = _guarded(init)
    with T._options(4 * (F // 32)):
        _check_plan(ops, grd, Ad, dc, OLD)
        ops.gemm_wgrad_grouped(grd, Ad, dW, dc)
        torch.cuda.synchronize()
    got = flat.cpu()
    assert torch.equal(got[:64], host[:64]) and torch.equal(got[-64:], host[-64:])
    got = got[64:-64].view(init.shape)
    for c in range(g.D):
        T._assert_same(got[c], init[c] + sums[c], f"misaligned F={F}: class {c}")


def test_pipe_switch_off_keeps_the_two_barrier_kernel(gpu_device):
    from gnnepcsaft_amd import ops
    _, _, dc = _graph()
    gr, A, _, _ = _ints(32)
    grd, Ad = _tower_views(gr, A)
    with T._options(4, pipe=0):
        _check_plan(ops, grd, Ad, dc, OLD)
    with T._options(4, split=0):
        _check_plan(ops, grd, Ad, dc, "k_gemm_wgrad<true,true>")


# ---------------------------------------------------------------------------------------------------------------------
# the split-operand arithmetic at the edges of runs, chunks and the prologue
# ---------------------------------------------------------------------------------------------------------------------
HOT_N, HOT_K, HOT_WGS = 128, 128, 4   # one output tile, four ranges, S = 3
# first | last position of a run; both sides of the class boundaries inside ranges 0 and 1 (36 | 37 | 38, 2086 | 2087); both
# sides of the chunk boundary inside the merged run (2085 | 2086); positions 127, 128, 159, 160 of the run at 2087 (the ends
# of the four steps the prologue loads and of the step it loads after them); the last position of all
HOT_POS = (0, 36, 37, 38, 1062, 2085, 2086, 2087, 2087 + 127, 2087 + 128, 2087 + 159, 2087 + 160, 3110, 3111, 4134, 4326)


def _run_hot(h):
    from gnnepcsaft_amd import ops
    g, _, dc = _graph()
    dC, A = T._framed(h.dC, 4, 4, 5.0)[2], T._framed(h.A, 8, 4, -3.0)[2]
    out = torch.zeros(g.D, HOT_N, HOT_K, device=DEV)
    with T._options(HOT_WGS):
        _check_plan(ops, dC, A, dc, NEW, 4, 3)
        ops.gemm_wgrad_grouped(dC, A, out, dc)
        torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("role", ["dC", "A"])
def test_one_term_products_are_exact(gpu_device, role):
    """Every dW entry of a class is ONE fp32 product of a full-mantissa value and a power of two and must come out
    exactly, wherever in a run, a chunk or the prologue its row sits."""
    g, _, _ = _graph()
    assert all(any(p in (a, a + n - 1) for p in HOT_POS) for a, n in RUNS_S3 if n > 1)
    rows = [int(g.dperm[p]) for p in HOT_POS]
    h = R.hot_rows_exact(g.N, HOT_N, HOT_K, rows, role, seed=80)
    out = _run_hot(h)
    for c in range(g.D):
        idx = torch.tensor([r for r in h.rows if int(g.degree[r]) == c], dtype=torch.long)
        ref = (h.dC[idx].double().T @ h.A[idx].double()).float()
        assert bool(ref.any()) == (SIZES[c] > 0)
        T._assert_same(out[c], ref, f"{role}: class {c}")


DENSE_POS = {"one_slab_behind_the_prologue": (2087 + 160, 2087 + 167, 2087 + 168, 2087 + 175),
             "merged_run_both_chunks": (1062 + 5, 1062 + 1023, 2086, 2087 + 159),
             "four_runs": (36, 37, 3111 + 128, 4326)}


@pytest.mark.parametrize("spread", sorted(DENSE_POS))
def test_dense_hot_rows_are_fp32_faithful_entry_wise(gpu_device, spread):
    """Four dense full-mantissa rows: max |dW - fp64| / (|dC|^T |A|) <= wgrad_ref.DENSE_BOUND_U per class.  A merged run
    flushes once where the per-chunk kernel flushed per chunk, so the derivation (at most four slabs, at most four
    flushes) covers it."""
    g, _, _ = _graph()
    rows = [int(g.dperm[p]) for p in DENSE_POS[spread]]
    h = R.hot_rows_dense(g.N, HOT_N, HOT_K, rows, seed=90)
    out = _run_hot(h)
    worst = 0.0
    for c in range(g.D):
        sel = [r for r in h.rows if int(g.degree[r]) == c]
        if not sel:
            assert not bool(out[c].any()), f"class {c} has no hot row"
            continue
        idx = torch.tensor(sel, dtype=torch.long)
        ref = h.dC[idx].double().T @ h.A[idx].double()
        norm = h.dC[idx].double().abs().T @ h.A[idx].double().abs()
        worst = max(worst, float(((out[c].double() - ref).abs() / norm).max()) / R.U32)
    print(spread, "entry-wise error / u:", worst, "bound", R.DENSE_BOUND_U)
    assert worst <= R.DENSE_BOUND_U


# ---------------------------------------------------------------------------------------------------------------------
# graph capture, and the layer-level entry
# ---------------------------------------------------------------------------------------------------------------------
def test_captured_launch_replays_exactly(gpu_device):
    """Eager, and captured in a HIP graph that is replayed twice into a re-zeroed dW: all three equal the int64 sums."""
    from gnnepcsaft_amd import ops
    g, _, dc = _graph()
    gr, A, _, sums = _ints(32)
    grd, Ad = _tower_views(gr, A)
    dW = torch.zeros(g.D, 32, 128, device=DEV)
    prev = torch.cuda.current_stream(gpu_device)
    s = torch.cuda.Stream(device=gpu_device)
    torch.cuda.synchronize()
    torch.cuda.set_stream(s)
    try:
        with T._options(4):
            _check_plan(ops, grd, Ad, dc, NEW, 4, 3)
            ops.gemm_wgrad_grouped(grd, Ad, dW, dc)
            torch.cuda.synchronize()
            T._assert_same(dW, sums, "eager")
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
                ops.gemm_wgrad_grouped(grd, Ad, dW, dc)
            for k in range(2):
                dW.zero_()
                graph.replay()
                torch.cuda.synchronize()
                T._assert_same(dW, sums, f"replay {k}")
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)


@pytest.mark.parametrize("F", [32, 128])
def test_post0_weight_gradient_through_the_classes(gpu_device, F):
    """pna_post0_wgrad_classes through the run-merging kernel: the class sums are exact, the D-term sums with the fp32 amp /
    att factors round: entry-wise within (D + 2) u (|dW0| + sum_d |term|) of fp64, as in tests/test_wgrad_gpu.py."""
    from gnnepcsaft_amd import ops
    g, _, dc = _graph()
    gr, A, _, sums = _ints(F)
    avg = 1.37
    dW0 = torch.randint(1, 100, (F, 13 * F), generator=torch.Generator().manual_seed(3)).float()
    host, dev, dW = T._framed(dW0, 3, 5, 9.0, top=1)
    grd, Ad = gr.to(DEV), A.to(DEV)
    with T._options(4 * (F // 32)):
        _check_plan(ops, grd, Ad, dc, NEW, 4, 3)
        ops.pna_post0_wgrad_classes(grd, Ad, dc, F, avg, dW)
        ops.join_side_stream(DEV)
        torch.cuda.synchronize()
    ref, S = R.weff_bwd_ref(sums, dW0, F, g.D, avg)
    got = dev.cpu()
    frame = got.clone()
    frame[1:1 + F, 3 + F:3 + 13 * F] = host[1:1 + F, 3 + F:3 + 13 * F]
    assert torch.equal(frame, host), "columns [0, F) or the frame of the dW view changed"
    err = ((got[1:1 + F, 3:3 + 13 * F].double() - ref).abs() / S)[:, F:]
    print("F", F, "max entry-wise error / u:", float(err.max()) / R.U32, "bound", g.D + 2)
    assert float(err.max()) <= (g.D + 2) * R.U32
