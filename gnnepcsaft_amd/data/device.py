"""Device-resident training set and on-device batch collation (csrc/gnx_collate.hip).

``Trainer.fit`` with the host ``DataLoader`` builds every batch in Python (``Batch.from_data_list``: one ``torch.cat``
per field over B small tensors) and then copies each field to the device.  The datasets are tiny (the Esper table is
~1.3 MB as int64), so ``DeviceDataset`` uploads the whole set once, stored as the concatenation of its graphs plus
per-graph offsets, and a batch becomes one small index upload and a gather of contiguous per-graph blocks::

    from gnnepcsaft_amd.data import DeviceDataLoader
    loader = DeviceDataLoader(train_list, batch_size=512, shuffle=True, seed=0, device="cuda:0")
    trainer.fit(model, loader)            # in place of train.DataLoader(train_list, batch_size=512, shuffle=True, seed=0)

Batches equal ``Batch.from_data_list([data_list[j] for j in idx]).to(device)`` field for field (dtype, shape, values).
Fields without exactly one tensor row per graph (the ragged ``rho`` / ``vp`` tables of the validation sets) cannot be
stored this way: validation loaders stay on the host ``DataLoader``.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from .. import _lib, ops
from .batching import Batch, Data
from .order import EpochOrder

_STRUCTURE = {"x": (None, 9), "edge_index": (2, None), "edge_attr": (None, 3)}
_RESERVED = ("x", "edge_index", "edge_attr", "batch", "ptr", "num_graphs")


def pack_dataset(data_list: Sequence[Data], fields: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """Host half of ``DeviceDataset``: validates ``data_list`` and returns its stored layout as CPU tensors --
    ``x`` int64[sumN,9], ``edge_index`` int64[2,sumE] (graph-local node ids), ``edge_attr`` int64[sumE,3], ``node_ptr`` /
    ``edge_ptr`` int64[G+1] and ``labels``: {field: [G, ...]} for every label field.

    ``fields=None`` takes every key of ``data_list[0]``; a field that is not a tensor with exactly one row per graph (same
    trailing shape and a 4- or 8-byte dtype throughout) raises a ``ValueError`` naming it.  Explicit ``fields`` leave
    every other key out."""
    data_list = list(data_list)
    if not data_list:
        raise ValueError("empty data_list")
    for key, shape in _STRUCTURE.items():
        for g, d in enumerate(data_list):
            t = getattr(d, key, None)
            want = ",".join("*" if s is None else str(s) for s in shape)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2 or \
                    any(s is not None and int(n) != s for n, s in zip(t.shape, shape)):
                got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"field '{key}' of graph {g}: expected int64[{want}], got {got}")
    n = np.array([d.x.shape[0] for d in data_list], dtype=np.int64)
    e = np.array([d.edge_index.shape[1] for d in data_list], dtype=np.int64)
    for g, d in enumerate(data_list):
        if d.edge_attr.shape[0] != e[g]:
            raise ValueError(f"field 'edge_attr' of graph {g}: {d.edge_attr.shape[0]} rows for {e[g]} edges")
        if e[g] and (int(d.edge_index.min()) < 0 or int(d.edge_index.max()) >= n[g]):
            raise ValueError(f"field 'edge_index' of graph {g}: node id outside [0,{n[g]})")
    if fields is None:
        fields = [k for k in data_list[0].keys() if k not in _RESERVED]
    labels = {}
    for key in fields:
        if key in _RESERVED:
            raise ValueError(f"field '{key}' is part of the graph structure, not a label field")
        vals = [getattr(d, key, None) for d in data_list]
        first = vals[0]
        for g, v in enumerate(vals):
            if not isinstance(v, torch.Tensor):
                raise ValueError(f"field '{key}' of graph {g} is {type(v).__name__}, not a tensor: only fields with one "
                                 "tensor row per graph can live on the device (pass `fields` to leave it out)")
            if v.dim() < 1 or v.shape[0] != 1 or v.shape[1:] != first.shape[1:] or v.dtype != first.dtype:
                raise ValueError(f"field '{key}' of graph {g}: expected one row {first.dtype} "
                                 f"{(1,) + tuple(first.shape[1:])}, got {v.dtype} {tuple(v.shape)} (pass `fields` to "
                                 "leave it out)")
        if first.element_size() not in (4, 8):
            raise ValueError(f"field '{key}': dtype {first.dtype} is not 4 or 8 bytes wide")
        labels[key] = torch.cat(vals, dim=0).contiguous()
    node_ptr, edge_ptr = np.zeros(len(data_list) + 1, dtype=np.int64), np.zeros(len(data_list) + 1, dtype=np.int64)
    np.cumsum(n, out=node_ptr[1:])
    np.cumsum(e, out=edge_ptr[1:])
    return {"x": torch.cat([d.x for d in data_list], dim=0).contiguous(),
            "edge_index": torch.cat([d.edge_index for d in data_list], dim=1).contiguous(),
            "edge_attr": torch.cat([d.edge_attr for d in data_list], dim=0).contiguous(),
            "node_ptr": torch.from_numpy(node_ptr), "edge_ptr": torch.from_numpy(edge_ptr), "labels": labels,
            "num_nodes": n, "num_edges": e}


def _device(device) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.GnxError(_lib.GNX_E_INVALID, "gnnepcsaft_amd.data.DeviceDataset needs a HIP device; there is no CPU "
                                                "fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"gnnepcsaft_amd.data.DeviceDataset needs a HIP device, got {dev}")
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


class DeviceDataset:
    """A list of ``Data`` validated on the host (``pack_dataset``) and uploaded once; ``collate(idx)`` builds the
    ``Batch`` of graphs ``idx`` on the device."""

    def __init__(self, data_list: Sequence[Data], device=None, fields: Optional[Sequence[str]] = None):
        self.device = _device(device)
        host = pack_dataset(data_list, fields)
        self.num_nodes, self.num_edges = host["num_nodes"], host["num_edges"]
        self._x, self._edge_index, self._edge_attr, self._node_ptr, self._edge_ptr = (
            host[k].to(self.device) for k in ("x", "edge_index", "edge_attr", "node_ptr", "edge_ptr"))
        self._labels = {k: v.to(self.device) for k, v in host["labels"].items()}

    def __len__(self) -> int:
        return len(self.num_nodes)

    @property
    def fields(self):
        return list(self._labels)

    def collate(self, idx: Union[Sequence[int], np.ndarray, torch.Tensor]) -> Batch:
        """The batch whose slot b is graph ``idx[b]`` (repeats allowed).  One upload of ``idx`` from pinned memory and a
        handful of launches on the current stream; nothing is read back.  An index outside the dataset is clamped on the
        device and reported by ``ops.check_range``."""
        if isinstance(idx, torch.Tensor):
            idx = idx.detach().cpu().numpy()
        idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), dtype=np.int64)
        if idx.size == 0:
            raise ValueError("empty batch")
        g = np.clip(idx, 0, len(self) - 1)  # what the kernels do with an out-of-range index
        N, E = int(self.num_nodes[g].sum()), int(self.num_edges[g].sum())
        d_idx = torch.from_numpy(idx).pin_memory().to(self.device, non_blocking=True)
        ptr, eptr = ops.collate_ptr(self._node_ptr, self._edge_ptr, d_idx)
        x, edge_index, edge_attr, batch = ops.collate_gather(self._node_ptr, self._edge_ptr, self._x, self._edge_index,
                                                             self._edge_attr, d_idx, ptr, eptr, N, E)
        out = Batch(x=x, edge_index=edge_index, edge_attr=edge_attr)
        out.batch, out.ptr, out.num_graphs = batch, ptr, int(idx.size)
        for key, src in self._labels.items():
            setattr(out, key, ops.collate_rows(src, d_idx))
        return out


class DeviceDataLoader(EpochOrder):
    """``train.DataLoader`` for training batches, collated on the device: same arguments, same epoch order and
    data-parallel shards (``EpochOrder``), same ``__len__`` / ``last_order`` / ``rng_state`` / ``set_rng_state``, so
    ``Trainer.fit`` -- checkpoints and mid-epoch resume included -- runs with it unchanged.  ``dataset`` is a
    ``DeviceDataset``, or a list of ``Data`` that is uploaded to ``device`` (``fields``: see ``pack_dataset``)."""

    def __init__(self, dataset, batch_size: int = 1, shuffle: bool = False, seed: int = 0, rank: Optional[int] = None,
                 world: Optional[int] = None, device=None, fields: Optional[Sequence[str]] = None, **_ignored):
        if isinstance(dataset, (list, tuple)):
            dataset = DeviceDataset(dataset, device, fields)
        self.dataset = dataset
        super().__init__(len(dataset), batch_size, shuffle, seed, rank, world)

    def __iter__(self):
        for idx in self.index_batches():
            yield self.dataset.collate(idx)
