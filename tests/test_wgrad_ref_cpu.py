"""The inputs of tests/test_wgrad_gpu.py have teeth: a CPU emulation of the split-operand weight gradient
(tests/wgrad_ref.py: three bf16 pieces, the six products of mfma_3x3 in its order, one fp32 rounding per 16-row slab
and term) passes every criterion the GPU tests apply, and each of three damaged variants -- the third piece lost, the
a2 b0 term lost, only four terms -- fails at least one of them.  Also pins the mirrors of the host dispatch to
hand-computed values at the shapes the GPU tests use."""
import pytest
import torch

from tests import wgrad_ref as R

FIVE_TERMS = tuple(t for t in R.MFMA_3X3_TERMS if t != (2, 0))
FOUR_TERMS = tuple(t for t in R.MFMA_3X3_TERMS if t not in ((2, 0), (0, 2)))
DAMAGED = {"two_pieces": dict(pieces=2), "no_a2_b0": dict(terms=FIVE_TERMS), "four_terms": dict(terms=FOUR_TERMS)}

M, N, K = 160, 40, 36
ONE_SLAB = (32, 39, 40, 47)        # positions 0, 7, 8, 15 of one 16-row slab
FOUR_SLABS = (0, 31, 32, 159)      # four slabs; with 32-row chunks: three chunks


def _criteria(**emu):
    """name -> passed, for every criterion of the GPU tests, applied to the emulation ``emu``."""
    out = {}
    c = R.int_case(M, N, K, seed=1)
    out["integer"] = torch.equal(c.dW0 + R.split_emulation(c.dC, c.A, **emu), c.dW)
    for role in ("dC", "A"):
        for name, rows in (("one_row", (77,)), ("slab", ONE_SLAB), ("slabs", FOUR_SLABS)):
            h = R.hot_rows_exact(M, N, K, rows, role, seed=2)
            out[f"exact_{role}_{name}"] = torch.equal(R.split_emulation(h.dC, h.A, chunk_rows=32, **emu), h.ref)
    for name, rows in (("one_slab", ONE_SLAB), ("four_slabs", FOUR_SLABS)):
        for seed in range(4):
            d = R.hot_rows_dense(M, N, K, rows, seed=seed)
            err = R.dense_error_u(R.split_emulation(d.dC, d.A, chunk_rows=32, **emu), d)
            out[f"dense_{name}_{seed}"] = err <= R.DENSE_BOUND_U
            out[f"dense_{name}_{seed}_u"] = err
    return out


def test_faithful_emulation_passes_every_gpu_criterion():
    res = _criteria()
    print({k: v for k, v in res.items() if k.endswith("_u")})
    assert all(v for k, v in res.items() if not k.endswith("_u")), res
    # the derived budgets, not only the common bound: 9.1 u for one slab, 30.1 u for four slabs
    assert max(v for k, v in res.items() if k.startswith("dense_one_slab") and k.endswith("_u")) <= 9.1
    assert max(v for k, v in res.items() if k.startswith("dense_four_slabs") and k.endswith("_u")) <= 30.1


@pytest.mark.parametrize("variant", sorted(DAMAGED))
def test_damaged_emulation_fails(variant):
    res = _criteria(**DAMAGED[variant])
    failed = sorted(k for k, v in res.items() if not k.endswith("_u") and not v)
    print(variant, failed, {k: round(v, 1) for k, v in res.items() if k.endswith("_u")})
    assert res["integer"], "small integers live in the first piece: no damage to the lower pieces can show there"
    # the one-term inputs see the loss whichever operand carries the full-mantissa values, except that a2 b0 only
    # exists when that operand is dC
    assert not res["exact_dC_one_row"] and not res["exact_dC_slab"] and not res["exact_dC_slabs"]
    if variant != "no_a2_b0":
        assert not res["exact_A_one_row"] and not res["exact_A_slab"] and not res["exact_A_slabs"]
    # and the dense inputs see it with margin: every draw lands beyond twice the bound
    for k, v in res.items():
        if k.endswith("_u"):
            assert v > 2 * R.DENSE_BOUND_U, (k, v)


def test_sequential_fp32_sum_of_the_dense_terms_is_inside_the_bound():
    """The yardstick: an fp32 loop over the same four terms (what the fp32-MFMA kernel does) sits at a few u."""
    d = R.hot_rows_dense(M, N, K, FOUR_SLABS, seed=0)
    acc = torch.zeros(N, K)
    for r in d.rows:
        acc = acc + d.dC[r][:, None] * d.A[r][None, :]
    assert R.dense_error_u(acc, d) <= 4.0


def test_int_case_is_exact_by_construction():
    c = R.int_case(777, 36, 40, seed=3, rowscale=True)
    assert set(c.rowscale.tolist()) <= {1.0, 2.0, 4.0} and float(c.dC.abs().max()) == 8.0
    assert (c.dW0 != 0).all() and (c.db0 != 0).all()
    ref = c.dW0.double() + c.dC.double().T @ (c.A.double() * c.rowscale.double()[:, None])
    assert torch.equal(c.dW.double(), ref) and torch.equal(c.db.double(), c.db0.double() + c.dC.double().sum(0))
    with pytest.raises(AssertionError):
        R.int_case(70000, 4, 4, seed=0)  # 256 * 70000 > 2^24: a partial sum could round


def test_rows_per_block_and_kernel_choice_at_the_gpu_test_shapes():
    # fp32 MFMA, single launch: M < 4096, or a row scale
    assert R.wgrad_rows_per_block(777, 128, 128, 4) == 224          # cdiv(777, 4) = 195 -> 224
    assert R.wgrad_kernel_name(777, 128, 128, 4) == "k_gemm_wgrad<true,false>"
    assert R.wgrad_rows_per_block(777, 260, 36, 4) == 416           # 3 tiles -> 2 chunks of cdiv(777, 2) = 389 -> 416
    assert R.wgrad_kernel_name(4131, 128, 128, 4, rowscale=True) == "k_gemm_wgrad<true,false>"
    assert R.wgrad_kernel_name(777, 130, 36, 4) == "k_gemm_wgrad<false,false>"
    assert R.wgrad_kernel_name(777, 3, 32, 4) == "k_gemm_wgrad<false,false>"
    assert R.wgrad_kernel_name(777, 128, 36, 4, vec=False) == "k_gemm_wgrad<false,false>"
    assert R.wgrad_rows_per_block(100, 128, 128, 64) == 128         # the floor of 128 rows
    # two-barrier split kernel: pipe off, rows < 512, or not vec
    assert R.wgrad_kernel_name(4131, 128, 128, 4, pipe=False) == "k_gemm_wgrad3<false>"
    assert R.wgrad_rows_per_block(4131, 128, 128, 16) == 288 and not R.takes_wave_specialised(4131, 128, 128, 16)
    assert R.wgrad_kernel_name(4100, 130, 260, 4) == "k_gemm_wgrad3<false>"
    assert R.wgrad_kernel_name(4131, 128, 128, 4, split=False) == "k_gemm_wgrad<true,false>"
    # wave-specialised: one tile, WGS = 4 -> four chunks of 1056 rows for 4096 < M <= 4224
    for m in (4113, 4160, 4161, 4208, 4131):
        assert R.wgrad_rows_per_block(m, 128, 128, 4) == 1056 and R.takes_wave_specialised(m, 128, 128, 4)
        assert R.wgrad_rows_per_block(m, 260, 132, 24) == 1056 and R.takes_wave_specialised(m, 260, 132, 24)  # 6 tiles
    last = {m: R.wgrad_chunks(m, 1056)[-1] for m in (4113, 4160, 4161, 4208)}
    assert {m: e - b for m, (b, e) in last.items()} == {4113: 945, 4160: 992, 4161: 993, 4208: 1040}
    # steps of the last chunk modulo 4, rows of its last step
    assert [(R._cdiv(n, 32) % 4, (n - 1) % 32 + 1) for n in (945, 992, 993, 1040)] == [(2, 17), (3, 32), (0, 1), (1, 16)]
    # a last chunk of ONE row: 16 chunks of 512 rows, 7681 = 15 * 512 + 1
    assert R.wgrad_rows_per_block(7681, 128, 128, 16) == 512 and R.takes_wave_specialised(7681, 128, 128, 16)
    assert R.wgrad_rows_per_block(7681, 260, 132, 96) == 512 and R.wgrad_chunks(7681, 512)[-1] == (7680, 7681)
    # the shapes of test_split_weight_gradient_single (tests/test_gemm_split_gpu.py) under WGS = 8 and at 256 CUs
    assert R.wgrad_rows_per_block(20001, 128, 128, 8) == 2528 and R.takes_wave_specialised(20001, 128, 128, 8)
    assert R.wgrad_rows_per_block(8192, 36, 100, 8) == 1024 and R.takes_wave_specialised(8192, 36, 100, 8)
    assert not R.takes_wave_specialised(5000, 130, 260, 8)
    assert R.wgrad_rows_per_block(20001, 128, 128, 256) == 128 and not R.takes_wave_specialised(20001, 128, 128, 256)
    # grouped launches never take it
    assert R.wgrad_kernel_name(4500, 32, 128, 4, grouped=True) == "k_gemm_wgrad3<true>"
    assert R.wgrad_kernel_name(700, 32, 128, 4, grouped=True) == "k_gemm_wgrad<true,true>"
    assert R.wgrad_kernel_name(700, 65, 260, 4, grouped=True) == "k_gemm_wgrad<false,true>"


def test_batched_plan_at_the_gpu_test_shapes():
    # eight 128 x 128 problems, budget 16: cost shares 9000 : 9000 : 9000 : 5000 : 4099 : 4096 : 640 : 33 of 40868
    shapes = [(m, 128, 128) for m in (9000, 9000, 9000, 5000, 4099, 4096, 640, 33)]
    name, rows = R.wgrad_batched_plan(shapes, 16)
    assert name == "k_gemm_wgrad3p_batched"
    # chunks = round(16 * share): 4 (3.52), 4, 4, 2 (1.96), 2 (1.60), 2 (1.60), 1 (0.25 -> at least 1), 1
    assert rows == [2272, 2272, 2272, 2528, 2080, 2048, 640, 64]
    assert R.wgrad_batched_plan(shapes, 16, pipe=False)[0] == "k_gemm_wgrad3_batched"
    assert R.wgrad_batched_plan(shapes, 16, split=False)[0] == "k_gemm_wgrad_batched"
    assert R.wgrad_batched_plan(shapes, 16, any_rowscale=True)[0] == "k_gemm_wgrad_batched"
    assert R.wgrad_batched_plan([(2, 128, 128)], 16) == ("k_gemm_wgrad_batched", [32])
    # the launches of tests/test_wgrad_gpu.py.  Nine problems, budget 64, the eight largest: cost = rows x tiles = 9000 +
    # 36000 + 9000 + 15000 + 12297 + 12288 + 1920 + 132 = 95637; chunks = round(64 rows / 95637) = 6, 6, 6, 3, 3, 3, 1, 1
    nine = [(9000, 128, 128), (9000, 128, 512), (9000, 128, 128), (5000, 36, 260), (4099, 260, 36), (4096, 36, 260),
            (640, 260, 36), (33, 128, 512)]
    assert R.wgrad_batched_plan(nine, 64)[1] == [1504, 1504, 1504, 1696, 1376, 1376, 640, 64]
    # budget 8: 2 + 9000 + 3 * 33 = 9101 -> 1 (0.002), 8 (7.91), 1 chunks;  4131 + 4500 -> 4 (3.83), 4 (4.17) chunks
    assert R.wgrad_batched_plan([(2, 128, 128), (9000, 128, 128), (33, 36, 260)], 8)[1] == [32, 1152, 64]
    assert R.wgrad_batched_plan([(4131, 128, 128), (4500, 128, 128)], 8) == ("k_gemm_wgrad3p_batched", [1056, 1152])
    # at most one chunk per 128 rows
    assert R.wgrad_batched_plan([(640, 128, 128), (4096, 128, 128)], 512)[1] == [128, 128]


def test_graph_with_class_sizes():
    sizes = [40, 5, 0, 3, 1]
    g = R.graph_with_class_sizes(sizes, seed=5)
    assert g.N == 49 and g.D == 5 and g.edge_index.shape == (2, 5 + 9 + 4)
    indeg = torch.bincount(g.edge_index[1], minlength=g.N)
    assert torch.equal(indeg, g.degree) and torch.bincount(indeg, minlength=5).tolist() == sizes
    assert g.cls_ptr.tolist() == [0, 40, 45, 45, 48, 49]
    assert torch.equal(g.degree[g.dperm], torch.sort(g.degree, stable=True).values)
    for c in range(g.D):  # ascending node ids inside a class
        ids = g.dperm[g.cls_ptr[c]:g.cls_ptr[c + 1]]
        assert torch.equal(ids, torch.sort(ids).values)
    assert not torch.equal(g.dperm, torch.arange(g.N))
    assert g.chunks() == [(0, 40, 0), (40, 5, 1), (45, 3, 3), (48, 1, 4)]
    big = R.graph_with_class_sizes([2049, 1], seed=1)
    assert big.chunks() == [(0, 1024, 0), (1024, 1024, 0), (2048, 1, 0), (2049, 1, 1)]


def test_weff_references():
    F, D, avg = 2, 3, 1.3
    amp, att = R.degree_factors(D, avg)
    assert float(amp[0]) == 0.0 and float(att[0]) == float(att[1])   # att uses max(d, 1)
    W = torch.arange(F * 13 * F, dtype=torch.float32).reshape(F, 13 * F) - 20
    ref, S = R.weff_ref(W, F, D, avg)
    assert ref.shape == (D, F, 4 * F)
    o, j, d = 1, 5, 2
    want = float(W[o, F + j]) + float(amp[d]) * float(W[o, 5 * F + j]) + float(att[d]) * float(W[o, 9 * F + j])
    assert abs(float(ref[d, o, j]) - want) < 1e-12 and float(S[d, o, j]) >= abs(want)
    dWeff = torch.ones(D, F, 4 * F)
    dW0 = torch.full((F, 13 * F), 3.0)
    back, Sb = R.weff_bwd_ref(dWeff, dW0, F, D, avg)
    assert torch.equal(back[:, :F], dW0[:, :F].double())
    assert abs(float(back[0, F]) - (3 + D)) < 1e-12 and abs(float(back[0, 5 * F]) - (3 + float(amp.sum()))) < 1e-12
    assert abs(float(back[1, 13 * F - 1]) - (3 + float(att.sum()))) < 1e-12 and torch.equal(Sb, back)
