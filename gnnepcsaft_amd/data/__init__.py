"""Input side of the hot path: graph containers, PyG-style collation (host and on-device), degree histogram,
synthetic graphs."""
from .batching import ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS, Batch, Data, calc_deg, in_degree, shard_by_graph
from .device import DeviceDataLoader, DeviceDataset, pack_dataset
from .featurize import from_smiles, smiles2graph
from .order import EpochOrder
from .synthetic import default_config, synthetic_batch

__all__ = ["ATOM_FEATURE_DIMS", "BOND_FEATURE_DIMS", "Batch", "Data", "calc_deg", "in_degree", "shard_by_graph",
           "default_config", "synthetic_batch", "from_smiles", "smiles2graph", "DeviceDataLoader", "DeviceDataset", "EpochOrder",
           "pack_dataset"]
