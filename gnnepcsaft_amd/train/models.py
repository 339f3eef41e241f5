"""Drop-in for the GNN part of ``/root/reference/gnnepcsaft/train/models.py``: same class / function / attribute /
state-dict names and config keys, with the forward/backward running on hand-written gfx950 kernels.

Mirrors: ``GNNePCSAFTL`` (:23-156), ``GNNePCSAFT`` (:159-254), ``get_conv`` (:441-584), ``get_global_pool`` (:587-595),
``create_model`` (:598-606).  Out of scope: the HabitchNN MLP baseline (:257-438) and every conv other
than PNA / GINE / Transformer — the dispatch is kept and raises for them.
"""
from __future__ import annotations

import math
from typing import Any, Optional, Union

import torch
from torch.nn import ModuleList, Sequential
from torch.optim.lr_scheduler import CosineAnnealingWarmRestarts

from .. import functional as Fn
from .. import nn as gnn
from .. import ops
from ..nn import BatchNorm, BatchNorm1d, Linear, ReLU
from ..ops import GraphPack
from .lightning_lite import LightningModuleLite

_OUT_OF_SCOPE_CONVS = ("GCN", "GAT", "GATv2", "SAGE", "GIN", "Edge", "GatedGraph", "Graph", "ARMA", "SG")
_ASSOC_DATASETS = ("esper_assoc", "esper_assoc_only")  # datasets whose label is ``graphs.assoc`` (reference :80-87)
# parameter bounds (reference :167-172): m, sigma, epsilon/k | log10 kappa_ab (negated), log10 epsilon_ab
_LOWER = (1.0, 1.9, 50.0, -math.log10(0.9), math.log10(200.0))
_UPPER = (25.0, 4.5, 550.0, -math.log10(0.0001), math.log10(5000.0))


def _pack_of(graphs, validate: bool, max_degree_hint: Optional[int] = None,
             model: Optional["GNNePCSAFT"] = None) -> GraphPack:
    """GraphPack of a Batch-like object, cached on it (the packer runs once per batch, like PyG's collate).  With a degree
    hint and the model that will consume it, the same native call also builds its getters' tables (``ops.pack_batch``);
    without a hint the degree classes need the batch's maximum in-degree first (one sync)."""
    pack = getattr(graphs, "_gnx_pack", None)
    if pack is None or pack.device != graphs.x.device:
        batch = getattr(graphs, "batch", None)
        num_graphs = getattr(graphs, "num_graphs", None) if batch is not None else None
        spec = model.pack_spec() if model is not None else {"classes": False}
        pack = ops.pack_batch(graphs.edge_index, graphs.edge_attr, batch, graphs.x.size(0), num_graphs,
                              max_degree_hint=max_degree_hint, validate=validate, **spec)
        try:
            graphs._gnx_pack = pack
        except AttributeError:
            pass
    return pack


class GNNePCSAFTL(LightningModuleLite):
    """Lightning-style wrapper around ``GNNePCSAFT`` (reference :23-156): ``.model``, ``.config``, ``training_step``,
    ``validation_step`` / ``test_step``, ``configure_optimizers``."""

    def __init__(self, config: dict[str, Any]):
        super().__init__()
        self.save_hyperparameters()
        self.config, self.model = config, GNNePCSAFT(config)
        # PC-SAFT solvers of validation_step (reference train/utils.py:252-300); None = validation off.  The native ones:
        # self.rho_batch, self.vp_batch = gnnepcsaft_amd.pcsaft.rho_batch, gnnepcsaft_amd.pcsaft.vp_batch
        self.rho_batch = self.vp_batch = None

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor,
                batch: torch.Tensor, pack: Optional[GraphPack] = None) -> torch.Tensor:
        return self.model(x, edge_index, edge_attr, batch, pack=pack)

    def configure_optimizers(self):
        """AdamW(amsgrad, eps 1e-5) or plain SGD + cosine warm restarts stepped every 10 epochs (reference :47-75)."""
        cfg, kind = self.config, self.config["optimizer"]
        if kind == "adam":
            opt = torch.optim.AdamW(self.parameters(), lr=cfg["learning_rate"], weight_decay=cfg["weight_decay"],
                                    amsgrad=True, eps=1e-5)
        elif kind == "sgd":
            opt = torch.optim.SGD(self.parameters(), lr=cfg["learning_rate"], momentum=0.0, weight_decay=0.0,
                                  nesterov=False)
        else:
            raise ValueError(f"Unsupported optimizer: {self.config['optimizer']}.")
        schedule = CosineAnnealingWarmRestarts(opt, cfg["warmup_steps"], T_mult=2, eta_min=1e-6)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": schedule, "interval": "epoch", "frequency": 10}}

    def _target(self, graphs) -> torch.Tensor:
        return graphs.assoc if self.config["dataset"] in _ASSOC_DATASETS else graphs.para

    def training_step(self, graphs, batch_idx):  # pylint: disable=W0613
        target = self._target(graphs)
        pack = _pack_of(graphs, self.model.validate_inputs, self.model.max_degree_hint, self.model)
        pred = self(graphs.x, graphs.edge_index, graphs.edge_attr, graphs.batch, pack=pack)
        # ape = (pred - target) / target ; huber(ape, 0, delta=0.01) ; mape(pred, target) -- one kernel
        loss, both = Fn.HuberAPEFn.apply(pred, target, 0.01)
        n = target.shape[0]
        self.log("train_huber", loss, on_step=True, batch_size=n, sync_dist=True)
        self.log("train_mape", both[1], on_step=True, batch_size=n, sync_dist=True)
        return loss

    def validation_step(self, graphs, batch_idx, dataloader_idx: int = 0):  # pylint: disable=W0613
        """Same contract as the reference (:110-153): mean absolute percentage errors of liquid density and vapour
        pressure computed from the predicted parameters.  That evaluation needs a PC-SAFT solver with the contract of
        ``rho_batch`` / ``vp_batch`` of the reference's train/utils.py:252-300 (feos there): assign callables to
        ``self.rho_batch`` / ``self.vp_batch`` to enable it, e.g. the GPU solver of ``gnnepcsaft_amd.pcsaft``."""
        import numpy as np

        if self.rho_batch is None or self.vp_batch is None:
            raise RuntimeError("validation_step needs PC-SAFT solvers: set .rho_batch and .vp_batch, e.g. to "
                               "gnnepcsaft_amd.pcsaft.rho_batch / vp_batch (reference gnnepcsaft/train/utils.py:252-300)")
        predicted = self.model.pred_with_bounds(graphs).squeeze().detach()
        signs = torch.tensor([-1.0, 1.0], device=predicted.device)  # labels hold (-log10 kappa_ab, log10 epsilon_ab)
        if self.config["num_para"] == 2:  # the model predicts the association pair, m/sigma/epsilon come as labels
            msigmae, assoc = graphs.para, 10 ** (predicted * signs)
        else:
            msigmae, assoc = predicted, 10 ** (graphs.assoc * signs)
        rows = torch.hstack([msigmae, assoc, graphs.munanb, graphs.mw]).cpu().to(torch.float64).tolist()

        def mape(solver, tables) -> float:
            measured = [t[:, -1] for t in tables if t.shape[0] > 0]
            errs = [np.mean(np.abs(p - m) / m).item() for p, m in zip(solver(rows, tables), measured)]
            return np.asarray(errs).mean().item()

        metrics = {"mape_den": mape(self.rho_batch, graphs.rho), "mape_vp": mape(self.vp_batch, graphs.vp)}
        self.log_dict(metrics, on_step=False, on_epoch=True, batch_size=1, sync_dist=True)
        return metrics

    def test_step(self, graphs, batch_idx, dataloader_idx=0):
        return self.validation_step(graphs, batch_idx, dataloader_idx)


class GNNePCSAFT(torch.nn.Module):  # pylint: disable=R0902
    """Atom / bond encoders -> L x [dropout, conv, BatchNorm, ReLU] -> global pool -> readout MLP (reference :159-254).
    Attribute and state-dict names follow the reference."""

    def __init__(self, config: dict):
        super().__init__()
        H, P = config["hidden_dim"], config["num_para"]
        self.num_para = P
        self.lower_bounds, self.upper_bounds = torch.tensor(_LOWER), torch.tensor(_UPPER)
        self.node_embed, self.edge_embed = gnn.AtomEncoder(H), gnn.BondEncoder(H)
        self.dropout = gnn.Dropout(p=config["dropout"])
        self.global_pool_type = config["global_pool"]
        self.global_pool = get_global_pool(config)
        depth = config["propagation_depth"]
        self.convs = ModuleList(get_conv(config) for _ in range(depth))
        self.batch_norms = ModuleList(BatchNorm(H) for _ in range(depth))
        widths = (H, H // 2, H // 4)
        self.mlp = Sequential(Linear(widths[0], widths[1]), BatchNorm1d(widths[1]), ReLU(),
                              Linear(widths[1], widths[2]), BatchNorm1d(widths[2]), ReLU(),
                              Linear(widths[2], P))
        # integer inputs are range-checked on device; True = read the flag back (one sync) when a batch is packed
        self.validate_inputs = True
        # sync-free packing (HIP-graph capture): upper bound of the in-degree, e.g. len(config["deg"]) - 1; a batch that
        # exceeds it trips the range flag (ops.check_range).  None = read the batch's maximum back (one sync).
        self.max_degree_hint = None
        self._bounds_cache = {}

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor,
                batch: Union[torch.Tensor, None], pack: Optional[GraphPack] = None) -> torch.Tensor:
        """``pack`` (optional) is the pre-built GraphPack of (edge_index, edge_attr, batch)."""
        if pack is None:
            pack = ops.pack_graph(edge_index, edge_attr, batch, x.size(0), None, validate=self.validate_inputs)
        h = self.node_embed(x)
        bond_table = self.edge_embed.table()  # 60 encoded bond-feature combinations; edges index it by pack.code
        # weight-only work of PNA layer l+1 (bond-table chain, Weff(d), merged lin o last post layer: ~5 tiny dependent
        # launches) is issued on the library's side stream while layer l runs, so it leaves the critical path
        convs = list(self.convs)
        ahead = ahead_all = None
        if h.is_cuda and Fn.batch_weight_only_enabled() and isinstance(convs[0], gnn.PNAConv) and convs[0].towers <= 8:
            # ... of ALL layers in three launches (60-row products and Weff(d) batched over the layers)
            ahead_all = gnn.PNAConv.prepare_all(convs, pack, bond_table)
        elif h.is_cuda and ops.wgrad_stream_enabled() and hasattr(convs[0], "prepare_ahead"):
            ahead = convs[0].prepare_ahead(pack, bond_table)
        # every layer's bond-embedding gradient is accumulated into one buffer on a side stream (its chain feeds no
        # activation gradient); layer 0, whose backward runs last, returns the total
        acc = None
        if h.is_cuda and bond_table.requires_grad and torch.is_grad_enabled():
            acc = Fn.BondGradAccumulator(bond_table.size(0), bond_table.size(1), h.device, len(convs))
            acc.encoder = (self.edge_embed.combos, self.edge_embed.offsets, self.edge_embed._weights())
        for l, (layer, norm) in enumerate(zip(convs, self.batch_norms)):
            extra = {} if acc is None else {"bond_acc": acc, "layer_index": l}
            if ahead_all is not None:
                extra["prepared"] = ahead_all.get(l)
            elif ahead is not None:
                extra["prepared"] = ahead.wait()
                ahead = convs[l + 1].prepare_ahead(pack, bond_table) if l + 1 < len(convs) else None
            # PNA, GINE and Transformer all take edge_attr (reference :211-214); the ReLU is fused into the BatchNorm kernel
            h = norm(layer(x=self.dropout(h), edge_index=pack, edge_attr=bond_table, **extra), relu=True)
        if batch is not None or pack.has_batch:
            h = self.global_pool(h, pack)
        else:  # batch None: reduce over all rows, keepdim (reference :220-225)
            h = Fn.SegmentPoolFn.apply(h, pack.graph_ptr, 1, self.global_pool_type)
        # readout mlp (reference :186-194, :226): Linear -> BN -> ReLU -> Linear -> BN -> ReLU -> Linear
        lin0, bn0, _, lin1, bn1, _, lin2 = self.mlp
        return lin2(bn1(lin1(bn0(lin0(h), relu=True)), relu=True))

    def pack_spec(self) -> dict:
        """What ``ops.pack_batch`` should build for this model's layers: the bond-code count, and for PNA the degree
        classes (when enabled) and the degree scalers of the layers' ``avg_deg_log`` values."""
        is_pna = isinstance(self.convs[0], gnn.PNAConv)
        avgs = [conv.aggr_module.avg_log() for conv in self.convs] if is_pna else []
        return {"R": int(self.edge_embed.combos.size(0)), "avg_deg_logs": avgs,
                "classes": is_pna and Fn.degree_classes_enabled(), "edge_tiles": is_pna}

    def _bounds(self, device):
        key = (device, self.num_para)
        if key not in self._bounds_cache:
            cols = slice(0, 3) if self.num_para == 3 else slice(3, None)
            self._bounds_cache[key] = (self.lower_bounds[cols].to(device=device).contiguous(),
                                       self.upper_bounds[cols].to(device=device).contiguous())
        return self._bounds_cache[key]

    def pred_with_bounds(self, data):
        """``forward`` clipped to the physical parameter bounds (reference :229-254)."""
        tensors = (data.x, data.edge_index, data.edge_attr)
        if not all(isinstance(t, torch.Tensor) for t in tensors):
            raise ValueError("Invalid input data")
        out = self.forward(*tensors, data.batch, pack=_pack_of(data, self.validate_inputs))
        return ops.clip_rows(out, *self._bounds(data.x.device))


def get_conv(config: dict):
    """The message-passing layer named by ``config["conv"]`` with the reference's constructor arguments (:441-584)."""
    kind, H = config["conv"], config["hidden_dim"]
    if kind == "PNA":
        return gnn.PNAConv(H, H, aggregators=["mean", "min", "max", "std"],
                           scalers=["identity", "amplification", "attenuation"],
                           deg=torch.tensor(config["deg"], dtype=torch.long), edge_dim=H, towers=config["towers"],
                           pre_layers=config["pre_layers"], post_layers=config["post_layers"], divide_input=True)
    if kind == "GINE":
        return gnn.GINEConv(nn=Sequential(Linear(H, H), ReLU(), Linear(H, H)), train_eps=False, edge_dim=H)
    if kind == "Transformer":
        assert H % config["heads"] == 0, "hidden_dim must be divisible by heads"
        return gnn.TransformerConv(in_channels=H, out_channels=H // config["heads"], heads=config["heads"], concat=True,
                                   dropout=config["dropout"], edge_dim=H)
    if kind in _OUT_OF_SCOPE_CONVS:
        raise NotImplementedError(
            f"conv={config['conv']!r} is outside the MI355X hot-path scope (PNA, GINE, Transformer); see SURVEY.md §2 row 2")
    raise ValueError(f"Unsupported convolution: {config['conv']}.")


_POOLS = {"mean": gnn.MeanAggregation, "max": gnn.MaxAggregation, "add": gnn.SumAggregation}


def get_global_pool(config: dict):
    """The readout aggregation named by ``config["global_pool"]`` (:587-595)."""
    pool = _POOLS.get(config["global_pool"])
    if pool is None:
        raise ValueError(f"Unsupported global pooling: {config['global_pool']}.")
    return pool()


def create_model(config: dict[str, Any], deg: list[int]):
    """``GNNePCSAFTL(config)`` for ``config["model"] == "gnn"``; stores ``deg`` in the config like the reference (:598-606)."""
    config["deg"] = deg
    kind = config["model"].lower()
    if kind == "gnn":
        return GNNePCSAFTL(config)
    if kind == "habitch":
        raise NotImplementedError("HabitchNN (dense MLP baseline, reference :257-438) is out of the hot-path scope")
    raise ValueError(f"Unsupported model: {config['model']}.")
