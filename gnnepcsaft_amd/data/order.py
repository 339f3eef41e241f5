"""Epoch order of the training loaders: which graphs go into which batch.  Host code (numpy only), shared by the host
``DataLoader`` (train/trainer.py) and the ``DeviceDataLoader`` (data/device.py), so that both draw the same batches
from the same seed and a checkpoint of one resumes with either."""
from __future__ import annotations

from typing import Iterator, Optional

import numpy as np


class EpochOrder:
    """PyG DataLoader semantics over ``n`` items: optional shuffle per epoch (PCG64 seeded with ``seed``), batches of
    ``batch_size`` indices, the last short batch kept.

    Data parallelism: with ``torch.distributed`` initialised and world size W > 1 (or explicit ``rank`` / ``world``) every
    rank draws the SAME epoch order (same seed on every rank) and takes its strided share ``order[rank::W]`` of it, the
    order being padded by wrapping to a multiple of W -- what Lightning injects into the reference's loaders under DDP
    (``torch.utils.data.DistributedSampler``; /root/reference/gnnepcsaft/train/train.py:85-88): ranks see disjoint
    graphs, every rank iterates the same number of batches, and the effective batch is W x ``batch_size``."""

    def __init__(self, n: int, batch_size: int = 1, shuffle: bool = False, seed: int = 0, rank: Optional[int] = None,
                 world: Optional[int] = None):
        self._n, self.batch_size, self.shuffle = int(n), int(batch_size), bool(shuffle)
        self._rng = np.random.Generator(np.random.PCG64(seed))
        if (rank is None) != (world is None):
            raise ValueError(f"{type(self).__name__}: pass rank and world together (or neither: taken from "
                             "torch.distributed)")
        self._rank, self._world = rank, world

    def _shard(self):
        if self._world is not None:
            return int(self._rank), int(self._world)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def _per_rank(self) -> int:
        _, world = self._shard()
        return (self._n + world - 1) // world

    def __len__(self) -> int:
        return (self._per_rank() + self.batch_size - 1) // self.batch_size

    def index_batches(self) -> Iterator[np.ndarray]:
        """Draws the next epoch's order (kept as ``last_order``) and yields it in slices of ``batch_size``."""
        order = np.arange(self._n)
        if self.shuffle:
            self._rng.shuffle(order)
        rank, world = self._shard()
        if world > 1 and len(order):
            total = self._per_rank() * world
            order = np.resize(order, total)[rank::world]  # np.resize pads by repeating the order from its start
        self.last_order = order
        for i in range(0, len(order), self.batch_size):
            yield order[i:i + self.batch_size]

    def rng_state(self) -> dict:
        """The shuffle generator's state as plain ints (PCG64: 128-bit state and increment)."""
        st = self._rng.bit_generator.state
        return {"state": int(st["state"]["state"]), "inc": int(st["state"]["inc"]), "has_uint32": int(st["has_uint32"]),
                "uinteger": int(st["uinteger"])}

    def set_rng_state(self, st: dict) -> None:
        self._rng.bit_generator.state = {"bit_generator": "PCG64", "state": {"state": int(st["state"]), "inc": int(st["inc"])},
                                         "has_uint32": int(st["has_uint32"]), "uinteger": int(st["uinteger"])}
