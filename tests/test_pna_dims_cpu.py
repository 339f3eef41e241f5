"""The one description of a PNA layer's shape (pna_native.PnaDims), the named tuples of PNAConvFn's plumbing and the pointer
array helper, pinned without a device.  Every expected number below was worked out BY HAND from the parameter order
(enc_w, enc_b, lin_w, lin_b, then per tower: pre (w, b) x pre_layers, post (w, b) x post_layers) and from the accumulator
shapes dTe [R,H], dEE [R,F], dWm [H,H], dbm [H], dWeff [T,D,F,4F]."""
from pathlib import Path

import pytest
import torch

from gnnepcsaft_amd import _lib, functional as Fn, pna_native
from gnnepcsaft_amd.pna_native import PnaLayerGrads, PnaDims


def test_two_towers_merged():
    d = PnaDims(T=2, F=4, pre_layers=2, post_layers=2, R=60, D=3, merged=True)
    assert tuple(d) == (2, 4, 2, 2, 60, 3, True)
    assert (d.H, d.per_tower, d.n_params) == (8, 8, 20)
    # 60*8, 60*4, 8*8, 8, 2*3*4*16
    assert d.small_sizes() == (480, 240, 64, 8, 384)
    assert d.small_total == 1176
    assert d.param_index(0, "pre", 0) == 4
    assert d.param_index(0, "pre", 1) == 6
    assert d.param_index(0, "post", 0) == 8
    assert d.param_index(1, "pre", 0) == 12
    assert d.param_index(1, "post", 1) == 18


def test_one_tower_unmerged_ungrouped():
    d = PnaDims(T=1, F=5, pre_layers=1, post_layers=1, R=60, D=0, merged=False)
    assert (d.H, d.per_tower, d.n_params) == (5, 4, 8)
    assert d.small_sizes() == (300, 300, 25, 5, 0)
    assert d.small_total == 630
    assert d.param_index(0, "post", 0) == 6


def test_prep_and_cfg_keep_their_positions():
    prep = Fn.PnaPrep("EE", "Te", "weffs", "Wm", "bm")
    assert prep.images is None and len(prep) == 6
    prep = Fn.PnaPrep("EE", "Te", "weffs", "Wm", "bm", "images")
    assert tuple(prep) == (prep.EE, prep.Te, prep.weffs, prep.Wm, prep.bm, prep.images)
    assert prep[5] == "images"
    cfg = Fn.PnaCfg(4, 32, 2, 3, 1.5)
    assert cfg[5:] == (None, None, 0) and (cfg.prepared, cfg.bond_acc, cfg.layer_index) == (None, None, 0)
    cfg = Fn.PnaCfg(4, 32, 2, 3, 1.5, "prepared", "acc", 7)
    assert tuple(cfg) == (cfg.T, cfg.F, cfg.pre_layers, cfg.post_layers, cfg.avg_deg_log, cfg.prepared, cfg.bond_acc,
                          cfg.layer_index) == (4, 32, 2, 3, 1.5, "prepared", "acc", 7)
    assert Fn.PnaCfg(*(4, 32, 2, 3, 1.5, "prepared")) == (4, 32, 2, 3, 1.5, "prepared", None, 0)


def test_ptr_array():
    ts = [torch.zeros(3), None, torch.zeros(2, 2), torch.zeros(5)[1:]]
    arr = pna_native.ptr_array(ts)
    assert len(arr) == 4
    for i in (0, 2, 3):
        assert arr[i] == ts[i].data_ptr() != 0
    assert arr[1] is None  # ctypes reads a null void* back as None
    assert ts[3].data_ptr() == ts[3]._base.data_ptr() + 4
    padded = pna_native.ptr_array(ts[:1], 3)
    assert len(padded) == 3 and padded[0] == ts[0].data_ptr() and padded[1] is None and padded[2] is None
    assert len(pna_native.ptr_array([])) == 0


def test_small_accumulators_are_walked_in_slab_order():
    d = PnaDims(T=2, F=4, pre_layers=2, post_layers=2, R=60, D=3, merged=True)
    small = torch.zeros(d.small_total)
    base = small.data_ptr()
    assert pna_native._small_ptrs(small, d) == [base, base + 4 * 480, base + 4 * 720, base + 4 * 784, base + 4 * 792]


def test_stack_finish_rejects_layers_of_different_shapes():
    d0 = PnaDims(2, 4, 2, 2, 60, 3, True)
    t = torch.zeros(1)
    recs = [PnaLayerGrads(d0, 1.0, t, t, [], [], t), PnaLayerGrads(d0._replace(F=8), 1.0, t, t, [], [], t)]
    with pytest.raises(_lib.GnxError) as e:
        pna_native.stack_finish(t.device, recs, t)
    assert e.value.status == _lib.GNX_E_INVALID
    acc = Fn.BondGradAccumulator(60, 8, t.device, 2)
    acc.deferred = recs
    with pytest.raises(_lib.GnxError):
        acc.finish_deferred(t.device)


def test_functional_is_the_autograd_layer_only():
    text = (Path(Fn.__file__)).read_text()
    assert "ctypes" not in text and "_lib" not in text
