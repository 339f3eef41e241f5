"""Host side of the device-resident loader (no GPU): the three collate symbols are declared in the bindings at ABI 7,
``DeviceDataLoader`` draws the epoch order of ``DataLoader`` (one shared implementation, ``data.EpochOrder``), and
``pack_dataset`` validates the fields a ``DeviceDataset`` can hold."""
import numpy as np
import pytest
import torch


class _HostSet:
    """Stands in for a DeviceDataset where only the order matters: ``collate`` hands the indices back."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def collate(self, idx):
        return np.array(idx)


def _graphs(n):
    from gnnepcsaft_amd.data import synthetic_batch
    return synthetic_batch(n, 3).to_data_list()


def test_bindings_declare_the_collate_symbols_at_abi_7():
    from gnnepcsaft_amd import _lib
    assert _lib.ABI_VERSION == 7
    for name in ("gnx_collate_ptr", "gnx_collate_gather", "gnx_collate_rows"):
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.gnx_abi_version() == 7


@pytest.mark.parametrize("shard", [None, (0, 3), (1, 3), (2, 3)])
def test_device_loader_draws_the_host_loaders_epoch_order(shard):
    from gnnepcsaft_amd.data import DeviceDataLoader, EpochOrder
    from gnnepcsaft_amd.train.trainer import DataLoader
    assert issubclass(DataLoader, EpochOrder) and issubclass(DeviceDataLoader, EpochOrder)
    for name in ("index_batches", "__len__", "rng_state", "set_rng_state", "_shard"):  # shared, not copied
        assert getattr(DataLoader, name) is getattr(DeviceDataLoader, name) is getattr(EpochOrder, name), name
    kw = dict(batch_size=32, shuffle=True, seed=5)
    if shard is not None:
        kw.update(rank=shard[0], world=shard[1])
    data = _graphs(70)
    host, dev = DataLoader(data, **kw), DeviceDataLoader(_HostSet(70), **kw)
    assert len(host) == len(dev) == (3 if shard is None else 1)
    orders = []
    for _ in range(3):
        hb = list(host)
        db = list(dev)
        assert np.array_equal(host.last_order, dev.last_order)
        assert len(hb) == len(db) == len(host)
        assert np.array_equal(np.concatenate(db), dev.last_order)
        assert [b.num_graphs for b in hb] == [len(i) for i in db]
        orders.append(dev.last_order.copy())
    assert len(orders[0]) == (70 if shard is None else 24)  # world 3: padded by wrapping to 72, 24 per rank
    assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[2])
    assert host.rng_state() == dev.rng_state()


def test_rng_state_round_trip_reproduces_the_next_epoch():
    from gnnepcsaft_amd.data import DeviceDataLoader
    from gnnepcsaft_amd.train.trainer import DataLoader
    a = DeviceDataLoader(_HostSet(70), batch_size=32, shuffle=True, seed=5)
    list(a)
    st = a.rng_state()
    list(a)
    want = a.last_order.copy()
    b = DeviceDataLoader(_HostSet(70), batch_size=32, shuffle=True, seed=999)
    b.set_rng_state(st)
    list(b)
    assert np.array_equal(b.last_order, want)
    c = DataLoader(_graphs(70), batch_size=32, shuffle=True, seed=1)  # a host loader resumes a device loader's state
    c.set_rng_state(st)
    list(c)
    assert np.array_equal(c.last_order, want)
    with pytest.raises(ValueError, match="rank and world"):
        DeviceDataLoader(_HostSet(3), rank=0)


def test_pack_dataset_layout_and_field_validation():
    from gnnepcsaft_amd.data import Batch, pack_dataset
    data = _graphs(6)
    host = pack_dataset(data)
    whole = Batch.from_data_list(data)
    assert torch.equal(host["x"], whole.x) and torch.equal(host["edge_attr"], whole.edge_attr)
    assert torch.equal(host["node_ptr"], whole.ptr) and host["node_ptr"].dtype == torch.int64
    assert torch.equal(host["edge_index"], torch.cat([d.edge_index for d in data], 1))  # graph-local ids
    assert list(host["labels"]) == ["para", "assoc"] and torch.equal(host["labels"]["para"], whole.para)
    assert np.array_equal(host["num_nodes"], [d.num_nodes for d in data])
    assert np.array_equal(host["num_edges"], [d.num_edges for d in data])

    for d in data:
        d.rho = [[300.0, 101325.0, 1.0]] * 2  # ragged table kept as a list (validation sets)
    with pytest.raises(ValueError, match="'rho'"):
        pack_dataset(data)
    assert list(pack_dataset(data, fields=("para",))["labels"]) == ["para"]  # explicit fields leave it out
    for d in data:
        d.rho = torch.zeros(2, 5)  # a tensor, but two rows per graph
    with pytest.raises(ValueError, match="'rho'"):
        pack_dataset(data)
    assert list(pack_dataset(data, fields=("para",))["labels"]) == ["para"]
    for d in data:
        del d.rho
    data[3].x = data[3].x.int()
    with pytest.raises(ValueError, match="'x'"):
        pack_dataset(data)
    data[3].x = data[3].x.long()
    data[2].edge_attr = data[2].edge_attr[:, :2]
    with pytest.raises(ValueError, match="'edge_attr'"):
        pack_dataset(data)
    with pytest.raises(ValueError, match="empty"):
        pack_dataset([])


def test_device_dataset_needs_a_hip_device():
    from gnnepcsaft_amd._lib import GNX_E_INVALID, GnxError
    from gnnepcsaft_amd.data import DeviceDataLoader, DeviceDataset
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(GnxError) as e:
        DeviceDataset(_graphs(2))
    assert e.value.status == GNX_E_INVALID
    with pytest.raises(GnxError):
        DeviceDataLoader(_graphs(2), batch_size=2, device="cuda:0")
