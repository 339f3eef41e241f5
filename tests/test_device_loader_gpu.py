"""Device-resident dataset and on-device collation (csrc/gnx_collate.hip, data/device.py) against the host path it
replaces: every field of ``DeviceDataset.collate(idx)`` must equal ``Batch.from_data_list([data[j] for j in idx]).to(dev)``
in dtype, shape and value (integer copies: exact), for every graph shape and index pattern the kernels branch on; the
loader must draw ``DataLoader``'s batches; and ``Trainer.fit`` must train, checkpoint and resume with it unchanged."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024  # slots per workgroup of gnx_collate_ptr's scan; 256 tiles per round of its offsets pass


def _lone(k):
    from tests.conv_cases import lone_atom
    d = lone_atom()
    d.x = d.x + torch.tensor([[k, 0, 0, 0, 0, 0, 0, 0, 0]])  # tell the copies apart
    return d


def _build(name):
    from gnnepcsaft_amd.data import synthetic_batch
    from tests import conv_cases
    if name == "syn64":  # + an fp64 [1,1] and an int64 [1,3] label field
        data = synthetic_batch(64, 3).to_data_list()
        g = torch.Generator().manual_seed(1)
        for d in data:
            d.mw = torch.rand(1, 1, dtype=torch.float64, generator=g) * 300
            d.munanb = torch.randint(-3, 9, (1, 3), generator=g)
        return data
    if name == "syn200":  # 5-80 atoms, odd node counts: x blocks that are only 8-byte aligned
        return synthetic_batch(200, 5).to_data_list()
    if name == "syn70":
        return synthetic_batch(70, 5).to_data_list()
    if name == "lone":  # 1-atom graphs with edge_index[2,0] between regular ones
        return conv_cases.lone_atom_batch().to_data_list()
    if name == "hub":  # 70- and 97-leaf stars
        return conv_cases.hub_batch().to_data_list()
    if name == "edgeless_ends":  # first, middle and last graph without edges
        reg = synthetic_batch(4, 5, seed=11).to_data_list()
        return [_lone(0), reg[0], reg[1], _lone(1), reg[2], reg[3], _lone(2)]
    if name == "all_edgeless":  # E = 0
        return [_lone(k) for k in range(5)]
    raise KeyError(name)


_CACHE = {}


def _dataset(name, dev):
    """(host list, DeviceDataset), built and uploaded once per module run."""
    if name not in _CACHE:
        from gnnepcsaft_amd.data import DeviceDataset
        data = _build(name)
        _CACHE[name] = (data, DeviceDataset(data, dev))
    return _CACHE[name]


def _reference(data, idx, dev):
    from gnnepcsaft_amd.data import Batch
    return Batch.from_data_list([data[int(j)] for j in idx]).to(dev)


def _assert_same(got, want, what=""):
    assert got.keys() == want.keys(), (what, got.keys(), want.keys())
    for key in want.keys():
        a, b = getattr(got, key), getattr(want, key)
        if isinstance(b, torch.Tensor):
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, (what, key, a.dtype, a.shape)
            assert torch.equal(a, b), (what, key)
        else:
            assert a == b, (what, key, a, b)


def _patterns(G):
    rng = np.random.Generator(np.random.PCG64(G))
    yield "identity", np.arange(G)
    yield "reversed", np.arange(G)[::-1]
    yield "permutation", rng.permutation(G)
    yield "repeats", np.resize(np.arange(G), G + 5)[1::2] if G > 2 else np.array([0, 0, G - 1, 0])
    yield "drawn", rng.integers(0, G, size=2 * G + 3)
    yield "single", np.array([G // 2])
    yield "last", [G - 1]  # a plain list, B = 1
    yield "first_as_tensor", torch.tensor([0, 0])


@pytest.mark.parametrize("name", ["syn64", "syn200", "lone", "hub", "edgeless_ends", "all_edgeless"])
def test_collate_equals_host_collate(gpu_device, name):
    from gnnepcsaft_amd import ops
    data, ds = _dataset(name, gpu_device)
    assert len(ds) == len(data)
    assert isinstance(ds.num_nodes, np.ndarray) and np.array_equal(ds.num_nodes, [d.num_nodes for d in data])
    assert isinstance(ds.num_edges, np.ndarray) and np.array_equal(ds.num_edges, [d.num_edges for d in data])
    for what, idx in _patterns(len(data)):
        got = ds.collate(idx)
        _assert_same(got, _reference(data, np.asarray(idx).reshape(-1), gpu_device), f"{name}/{what}")
        assert got.edge_index.shape[0] == 2 and got.edge_attr.shape[1] == 3 and got.x.is_contiguous()
    if name == "all_edgeless":
        assert got.edge_index.shape == (2, 0) and got.edge_attr.shape == (0, 3)
    if name == "syn64":
        assert got.mw.dtype == torch.float64 and got.munanb.dtype == torch.int64 and got.para.dtype == torch.float32
        assert got.para.shape == (2, 3) and got.assoc.shape == (2, 2) and got.mw.shape == (2, 1)
    ops.check_range(gpu_device)


@pytest.mark.parametrize("B", [1, 63, 64, 65, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_prefix_sum_boundaries(gpu_device, B):
    """``ptr`` and ``batch`` exact around the scan's wave, workgroup-tile and multi-tile boundaries (uniform 20-atom
    graphs as the issue sets; the variable-size set on top, where a wrong offset cannot hide behind equal sizes)."""
    for name in ("syn64", "syn200"):
        data, ds = _dataset(name, gpu_device)
        idx = np.random.Generator(np.random.PCG64(B)).integers(0, len(data), size=B)
        got, want = ds.collate(idx), _reference(data, idx, gpu_device)
        assert torch.equal(got.ptr, want.ptr) and torch.equal(got.batch, want.batch), (name, B)
        _assert_same(got, want, f"{name}/B={B}")


@pytest.mark.parametrize("B", [256 * SCAN_TILE - 1, 256 * SCAN_TILE + 1, (1 << 20) + SCAN_TILE + 1])
def test_prefix_sum_beyond_one_round_of_tile_offsets(gpu_device, B):
    """gnx_collate_ptr alone at B up to 2^20 and past it: the offsets pass walks the tile totals 256 at a time."""
    from gnnepcsaft_amd import ops
    data, ds = _dataset("syn200", gpu_device)
    idx = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).integers(0, len(data), size=B)).to(gpu_device)
    ptr, eptr = ops.collate_ptr(ds._node_ptr, ds._edge_ptr, idx)
    zero = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    for got, sizes in ((ptr, ds.num_nodes), (eptr, ds.num_edges)):
        want = torch.cat([zero, torch.cumsum(torch.from_numpy(sizes).to(gpu_device)[idx], 0)])
        assert got.dtype == torch.int64 and torch.equal(got, want)
    ops.check_range(gpu_device)


@pytest.mark.parametrize("shard", [None, (0, 3), (1, 3), (2, 3)])
def test_loader_yields_the_host_loaders_batches(gpu_device, shard):
    from gnnepcsaft_amd.data import DeviceDataLoader
    from gnnepcsaft_amd.train.trainer import DataLoader
    data, ds = _dataset("syn70", gpu_device)
    kw = dict(batch_size=32, shuffle=True, seed=4)
    if shard is not None:
        kw.update(rank=shard[0], world=shard[1])
    host, dev = DataLoader(data, **kw), DeviceDataLoader(ds, **kw)
    for epoch in range(3):
        hb, db = list(host), list(dev)
        assert np.array_equal(host.last_order, dev.last_order)
        assert len(hb) == len(db) == len(dev) == (3 if shard is None else 1)
        for k, (h, d) in enumerate(zip(hb, db)):
            _assert_same(d, h.to(gpu_device), f"epoch {epoch} batch {k}")
    if shard is None:
        assert db[-1].num_graphs == 6  # the short last batch is kept
    from_list = DeviceDataLoader(data[:5], batch_size=4, device=gpu_device, fields=("para",))  # a list plus a device
    last = list(from_list)[-1]
    assert last.num_graphs == 1 and last.keys() == ["x", "edge_index", "edge_attr", "batch", "ptr", "num_graphs", "para"]


def test_repeatable_stream_ordered_and_already_on_the_device(gpu_device):
    data, ds = _dataset("syn200", gpu_device)
    idx = np.random.Generator(np.random.PCG64(3)).integers(0, len(data), size=97)
    a, b = ds.collate(idx), ds.collate(idx)
    _assert_same(b, a, "second call")
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        c = ds.collate(idx)
    side.synchronize()
    _assert_same(c, a, "side stream")
    moved = a.to(gpu_device, non_blocking=True)  # what Trainer.fit does with every batch: no copy
    for key in a.keys():
        if isinstance(getattr(a, key), torch.Tensor):
            assert getattr(moved, key).data_ptr() == getattr(a, key).data_ptr(), key


def test_out_of_range_index_is_clamped_and_reported(gpu_device):
    from gnnepcsaft_amd import _lib, ops
    data, ds = _dataset("syn200", gpu_device)
    G = len(data)
    ops.check_range(gpu_device)
    got = ds.collate([3, G, 7, -1, 5])
    with pytest.raises(_lib.GnxError) as e:
        ops.check_range(gpu_device)
    assert e.value.status == _lib.GNX_E_RANGE and "batch index" in str(e.value)
    _assert_same(got, _reference(data, [3, G - 1, 7, 0, 5], gpu_device), "clamped")
    ds.collate([3, G - 1, 7, 0, 5])
    ops.check_range(gpu_device)  # the flag is sticky until read, not beyond


def test_wrappers_reject_bad_dtype_and_shape(gpu_device):
    from gnnepcsaft_amd import _lib, ops
    _, ds = _dataset("syn64", gpu_device)
    idx = torch.arange(4, device=gpu_device)
    bad = [lambda: ops.collate_ptr(ds._node_ptr, ds._edge_ptr, idx.int()),
           lambda: ops.collate_ptr(ds._node_ptr, ds._edge_ptr[:-1], idx),
           lambda: ops.collate_ptr(ds._node_ptr, ds._edge_ptr, idx[:0]),
           lambda: ops.collate_ptr(ds._node_ptr, ds._edge_ptr, idx.cpu()),
           lambda: ops.collate_rows(ds._labels["para"].half(), idx),
           lambda: ops.collate_rows(ds._labels["para"], idx.reshape(2, 2)),
           lambda: ops.collate_gather(ds._node_ptr, ds._edge_ptr, ds._x[:, :8].contiguous(), ds._edge_index,
                                      ds._edge_attr, idx, ds._node_ptr[:5], ds._edge_ptr[:5], 80, 160),
           lambda: ops.collate_gather(ds._node_ptr, ds._edge_ptr, ds._x, ds._edge_index, ds._edge_attr, idx,
                                      ds._node_ptr[:4], ds._edge_ptr[:5], 80, 160)]
    for k, call in enumerate(bad):
        with pytest.raises(_lib.GnxError) as e:
            call()
        assert e.value.status == _lib.GNX_E_INVALID, k


def test_training_with_the_device_loader_matches_the_host_loader_and_resumes(gpu_device, tmp_path):
    """4 steps of Trainer.fit (GINE, H=32, 2 layers, 64 graphs, batches of 32, shuffled, same seed) once per loader: the
    batches are identical, so the logged losses agree to the run-to-run reproducibility of the step (5e-5 relative: the
    bound of the resume tests in test_trainer_gpu.py / test_transformer_gpu.py; weight gradients accumulate with fp32
    atomics).  The device-loader run stopped after 1 step (mid-epoch: 2 batches per epoch) resumes from its checkpoint
    with a fresh model, trainer and wrongly seeded loader and reproduces steps 2-4 within the same bound."""
    from gnnepcsaft_amd.data import DeviceDataLoader, calc_deg, default_config, synthetic_batch
    from gnnepcsaft_amd.train.models import create_model
    from gnnepcsaft_amd.train.trainer import DataLoader, Trainer, read_checkpoint
    cfg = default_config(2)
    cfg.update(conv="GINE", hidden_dim=32, propagation_depth=2, warmup_steps=2, learning_rate=2e-3)
    dataset = synthetic_batch(64, 3).to_data_list()
    deg = calc_deg(dataset)
    ds = _dataset("syn64", gpu_device)[1]  # the same 64 graphs, already on the device

    def new_model():
        torch.manual_seed(0)
        return create_model(copy.deepcopy(cfg), deg)

    def losses(tr):
        return [r["train_huber"] for r in tr.logged]

    def worst(a, b):
        return max(abs(x - y) / abs(x) for x, y in zip(a, b))

    tr_host = Trainer(max_steps=4, log_every_n_steps=1, enable_checkpointing=False)
    tr_host.fit(new_model(), DataLoader(dataset, batch_size=32, shuffle=True, seed=3))
    tr_dev = Trainer(max_steps=4, log_every_n_steps=1, enable_checkpointing=False)
    loader = DeviceDataLoader(ds, batch_size=32, shuffle=True, seed=3)
    tr_dev.fit(new_model(), loader)
    h, d = losses(tr_host), losses(tr_dev)
    print("train_huber host loader:", h, "device loader:", d, "worst relative difference:", worst(h, d))
    assert len(h) == len(d) == 4 and worst(h, d) <= 5e-5, (h, d)

    tr_stop = Trainer(max_steps=1, log_every_n_steps=1, default_root_dir=str(tmp_path), enable_checkpointing=True)
    tr_stop.fit(new_model(), DeviceDataLoader(ds, batch_size=32, shuffle=True, seed=3))
    path = os.path.join(str(tmp_path), "last.ckpt")
    ckpt = read_checkpoint(path)
    assert ckpt["global_step"] == 1 and ckpt["epoch"] == 0 and ckpt["loops"]["batch_in_epoch"] == 1
    assert ckpt["loops"]["loader_rng_at_epoch_start"] is not None
    model = new_model()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)  # everything must come from the file
    tr_res = Trainer(max_steps=4, log_every_n_steps=1, enable_checkpointing=False)
    resumed = DeviceDataLoader(ds, batch_size=32, shuffle=True, seed=999)
    tr_res.fit(model, resumed, ckpt_path=path)
    r = losses(tr_res)
    print("resumed:", r, "uninterrupted:", d[1:], "worst relative difference:", worst(d[1:], r))
    assert [x["step"] for x in tr_res.logged] == [2, 3, 4]
    assert np.array_equal(resumed.last_order, loader.last_order)
    assert worst(d[1:], r) <= 5e-5, (d[1:], r)
