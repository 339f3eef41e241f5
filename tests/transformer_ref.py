"""Test-only fp64 restatement of [3P] torch_geometric.nn.TransformerConv as the reference builds it
(``train/models.py:497-511``: concat=True, beta=False, root_weight=True, bias=True, edge_dim=H, aggregation "add", no
self-loops), written op for op like PyG's CPU path: index_select / F.linear / utils.softmax over the destination /
scatter-add.  ``keep`` (optional, [E, heads] in the ORIGINAL edge order) replays a dropout mask on alpha instead of
drawing one, so a native run with p > 0 can be checked exactly."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch.nn import Linear

from oracle.pyg_restatement import scatter


def softmax(src: torch.Tensor, index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """[3P] torch_geometric.utils.softmax(src, index, num_nodes=N) along dim 0."""
    src_max = scatter(src.detach(), index, 0, num_nodes, "max")
    out = (src - src_max.index_select(0, index)).exp()
    out_sum = scatter(out, index, 0, num_nodes, "sum") + 1e-16
    return out / out_sum.index_select(0, index)


class TransformerConv(torch.nn.Module):
    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, dropout: float = 0.0,
                 edge_dim: Optional[int] = None):
        super().__init__()
        self.in_channels, self.out_channels, self.heads, self.dropout = in_channels, out_channels, heads, dropout
        H = heads * out_channels
        self.lin_key = Linear(in_channels, H)
        self.lin_query = Linear(in_channels, H)
        self.lin_value = Linear(in_channels, H)
        self.lin_edge = Linear(edge_dim, H, bias=False)
        self.lin_skip = Linear(in_channels, H, bias=True)
        self.keep: Optional[torch.Tensor] = None  # replayed dropout mask [E, heads], original edge order

    def forward(self, x, edge_index, edge_attr):
        Hh, C = self.heads, self.out_channels
        N = x.size(0)
        j, i = edge_index[0], edge_index[1]
        query = self.lin_query(x).view(-1, Hh, C)
        key = self.lin_key(x).view(-1, Hh, C)
        value = self.lin_value(x).view(-1, Hh, C)
        edge = self.lin_edge(edge_attr).view(-1, Hh, C)
        key_j = key.index_select(0, j) + edge
        alpha = (query.index_select(0, i) * key_j).sum(dim=-1) / math.sqrt(C)
        alpha = softmax(alpha, i, N)
        if self.keep is not None:
            alpha = alpha * self.keep.to(alpha.dtype) / (1.0 - self.dropout)
        else:
            alpha = F.dropout(alpha, p=self.dropout, training=self.training)
        msg = (value.index_select(0, j) + edge) * alpha.view(-1, Hh, 1)
        out = scatter(msg, i, 0, N, "sum").view(-1, Hh * C)
        return out + self.lin_skip(x)


def reference_model(cfg: dict):
    """The oracle's GNNePCSAFT with its convs swapped for this restatement (its forward dispatches on the conv's
    signature, so nothing else changes)."""
    from oracle import pyg_restatement as O
    m = O.GNNePCSAFT(dict(cfg, conv="GINE"))
    H, heads = cfg["hidden_dim"], cfg["heads"]
    m.convs = torch.nn.ModuleList(TransformerConv(H, H // heads, heads, cfg["dropout"], edge_dim=H)
                                  for _ in range(cfg["propagation_depth"]))
    return m
