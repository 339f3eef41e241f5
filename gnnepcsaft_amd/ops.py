"""Tensor-level wrappers over the C ABI (include/gnx.h): torch tensors in, ``data_ptr()`` + sizes across ctypes.

torch is used for device memory and streams only; every arithmetic op on the hot path is a gnx kernel.  All wrappers
require HIP-device fp32 / int64 / int32 tensors and raise ``GnxError`` otherwise — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import GemmSeg, check, handle

_I32 = C.c_int32


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: expected float32, got {t.dtype}")
    return t


def _mat(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """(data_ptr, leading dimension) of a 2-D fp32 view whose rows are contiguous."""
    if t.dtype is not torch.float32:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: expected float32, got {t.dtype}")
    shape, strides = t.shape, t.stride()
    if len(shape) != 2 or (shape[1] > 1 and strides[1] != 1):
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: need a 2-D view with unit column stride, got "
                                                f"shape {tuple(shape)} strides {strides}")
    ld = strides[0]
    return t.data_ptr(), (ld if ld > shape[1] else shape[1])


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _carr(vals: Sequence[int]):
    return (_I32 * len(vals))(*vals)


def zeros(*shape: int, device: torch.device) -> torch.Tensor:
    """fp32 zeros through a fill launch: ``torch.zeros`` / ``zero_()`` go through hipMemsetAsync, which costs ~50 us of
    host time per call here (the launch path is on the critical path of the step)."""
    t = torch.empty(*shape, dtype=torch.float32, device=device)
    return zero_(t)


_ONES: dict = {}


def ones_vector(device: torch.device, n: int) -> torch.Tensor:
    """A cached fp32 vector of >= n ones on ``device`` (column sums as 1 x R products in gnx_gemm_small_batched)."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    t = _ONES.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 256), dtype=torch.float32, device=device)
        check(_lib.load().gnx_fill(handle(device), t.data_ptr(), t.numel(), 1.0))
        _ONES[key] = t
    return t


def zero_(t: torch.Tensor) -> torch.Tensor:
    if t.is_cuda and t.dtype is torch.float32 and t.is_contiguous():
        if t.numel():
            check(_lib.load().gnx_fill(handle(t.device), t.data_ptr(), t.numel(), 0.0))
        return t
    return t.zero_()


# ------------------------------------------------------------------------------------------------------------------
# packer
# ------------------------------------------------------------------------------------------------------------------
class GraphPack:
    """Device-resident integer structure of one batch: dst-sorted CSR + by-source index + bond codes + graph_ptr.

    Everything the kernels need in place of ``edge_index`` / ``batch``.  int32 throughout.
    """

    __slots__ = ("N", "E", "B", "rowptr", "perm", "src", "dst", "colptr", "cpos", "code", "graph_ptr", "device",
                 "_scalers", "has_batch", "_classes", "_code_index", "max_degree_hint", "_edge_tiles")

    EDGE_TILE_ROWS = 64     # message rows of one tile of the fused edge kernels (gnx_pna_edge_fwd)
    EDGE_TILE_MAX_DEG = 16  # above this in-degree bound the tiles would be mostly padding: unfused kernels instead

    def __init__(self, N: int, E: int, B: int, has_batch: bool, device: torch.device,
                 max_degree_hint: Optional[int] = None):
        self.N, self.E, self.B, self.has_batch, self.device = N, E, B, has_batch, device
        self.max_degree_hint = max_degree_hint
        self.rowptr = self.perm = self.src = self.dst = self.colptr = self.cpos = self.code = self.graph_ptr = None
        self._scalers, self._classes, self._code_index, self._edge_tiles = {}, None, None, None

    @staticmethod
    def edge_tile_width(max_degree: int) -> Optional[int]:
        """Nodes' first CSR positions per edge tile for in-degrees <= ``max_degree``: 65 - max_degree, so no tile exceeds
        64 message rows; None when the bound is too large for the fused edge kernels."""
        if max_degree > GraphPack.EDGE_TILE_MAX_DEG:
            return None
        return GraphPack.EDGE_TILE_ROWS + 1 - max(int(max_degree), 1)

    @staticmethod
    def has_code_index(R: int) -> bool:
        """Whether positions can be grouped by R bond codes (gnx_group_by_small_key takes at most 64 keys)."""
        return R <= 64

    def edge_tiles(self, max_degree: int) -> Optional[Tuple[torch.Tensor, int]]:
        """(tile_info int32[2 (count + 1)], tile width w) of gnx_edge_tiles for in-degrees <= ``max_degree`` (tile j = the
        nodes whose first CSR position lies in [w j, w (j + 1)), w = ``edge_tile_width``); None when the bound is too
        large for the fused edge kernels or the batch has no edges.  Built once."""
        w = GraphPack.edge_tile_width(max_degree)
        if w is None or self.E == 0 or self.N == 0:
            return None
        hit = self._edge_tiles
        if hit is None or hit[1] != w:
            lib = _lib.load()
            count = lib.gnx_edge_tiles_count(self.E, w)
            info = torch.empty(2 * (count + 1), dtype=torch.int32, device=self.device)
            check(lib.gnx_edge_tiles(handle(self.device), self.rowptr.data_ptr(), self.N, self.E, w, info.data_ptr()))
            hit = self._edge_tiles = (info, w)
        return hit

    def code_index(self, R: int) -> Optional[torch.Tensor]:
        """CSR positions stably grouped by bond code (inverted index for the bond-table gradient); None if R > 64."""
        if not GraphPack.has_code_index(R):
            return None
        if self._code_index is None or self._code_index[0] != R:
            lib, h = _lib.load(), handle(self.device)
            pos = torch.empty(max(self.E, 1), dtype=torch.int32, device=self.device)
            ptr = torch.empty(R + 1, dtype=torch.int32, device=self.device)
            nbytes = lib.gnx_degree_classes_workspace_bytes(self.E, R)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            check(lib.gnx_group_by_small_key(h, self.code.data_ptr(), self.E, R, pos.data_ptr(), ptr.data_ptr(),
                                             ws.data_ptr(), nbytes))
            self._code_index = (R, pos, ptr)
        return self._code_index[1]

    def degree_classes(self, max_degree_hint: Optional[int] = None) -> Optional["DegreeClasses"]:
        """Nodes grouped by in-degree (for PNA's per-degree effective post-layer-0 weight); ``None`` when the batch
        has more than 64 distinct degrees up to its maximum (hub-heavy graphs use the ungrouped 4-segment product).
        Built once per batch.  Without a hint the maximum in-degree is read back from the device (one sync, like
        PyG's ``batch.max()``); with ``max_degree_hint`` (e.g. ``len(config["deg"]) - 1``) nothing synchronises and a
        node above the hint sets the sticky range flag reported by ``check_range`` (needed under HIP-graph capture)."""
        if self._classes is None:
            self._classes = DegreeClasses.build(self, max_degree_hint)
        return self._classes if self._classes.D <= DegreeClasses.MAX_D else None

    def degree_scalers(self, avg_deg_log: float) -> Tuple[torch.Tensor, torch.Tensor]:
        key = float(avg_deg_log)
        hit = self._scalers.get(key)
        if hit is None:
            amp = torch.empty(self.N, dtype=torch.float32, device=self.device)
            att = torch.empty(self.N, dtype=torch.float32, device=self.device)
            check(_lib.load().gnx_degree_scalers(handle(self.device), self.rowptr.data_ptr(), self.N, key,
                                                 amp.data_ptr(), att.data_ptr()))
            hit = (amp, att)
            self._scalers[key] = hit
        return hit


class DegreeClasses:
    """dperm / cls_ptr / tile tables of gnx_degree_classes + gnx_class_tiles (see include/gnx.h)."""
    MAX_D = 64
    GEMM_ROWS = 128    # k_gemm's BM
    WGRAD_ROWS = 1024  # rows per weight-gradient chunk (512 -> 1024: -0.1 ms per cfg-2 step, fewer atomic flushes)

    __slots__ = ("D", "dperm", "cls_ptr", "tiles", "ntiles", "max_tiles", "chunks", "nchunks", "max_chunks",
                 "tiles_p", "ntiles_p", "max_tiles_p", "tile_rows_p")

    def __init__(self, D: int):
        self.D = D  # the tables exist only for D <= MAX_D

    def layout(self, lib, h, N: int) -> List[Tuple[str, int]]:
        """[(table, int32 count)] of the tables over N nodes, to be handed to ``take`` as tensors; sets their bounds.
        The tile table of the pipelined forward product (post-layer 0) has 96-row tiles where 128-row ones would leave the
        last round of its persistent workgroups mostly idle (gnx_gemm_tile_rows); otherwise, and for the input-gradient
        product always, it is ``tiles`` itself and has no entry."""
        D = self.D
        self.tile_rows_p = int(lib.gnx_gemm_tile_rows(h, N, 128))
        self.max_tiles, self.max_chunks = N // DegreeClasses.GEMM_ROWS + D, N // DegreeClasses.WGRAD_ROWS + D
        sizes = [("dperm", max(N, 1)), ("cls_ptr", D + 1), ("tiles", 3 * self.max_tiles), ("ntiles", 1),
                 ("chunks", 3 * self.max_chunks), ("nchunks", 1)]
        if self.tile_rows_p == DegreeClasses.GEMM_ROWS:
            self.max_tiles_p = self.max_tiles
        else:
            self.max_tiles_p = N // self.tile_rows_p + D
            sizes += [("tiles_p", 3 * self.max_tiles_p), ("ntiles_p", 1)]
        return sizes

    def take(self, v: dict) -> List[Tuple[int, torch.Tensor, torch.Tensor]]:
        """Adopt the tensors v[table]; returns (tile rows, table, count) of every tile table to fill."""
        self.dperm, self.cls_ptr, self.tiles, self.ntiles, self.chunks, self.nchunks = (
            v["dperm"], v["cls_ptr"], v["tiles"], v["ntiles"], v["chunks"], v["nchunks"])
        self.tiles_p, self.ntiles_p = v.get("tiles_p", self.tiles), v.get("ntiles_p", self.ntiles)
        tables = [(DegreeClasses.GEMM_ROWS, self.tiles, self.ntiles), (DegreeClasses.WGRAD_ROWS, self.chunks, self.nchunks)]
        if self.tiles_p is not self.tiles:
            tables.append((self.tile_rows_p, self.tiles_p, self.ntiles_p))
        return tables

    @staticmethod
    def build(g: "GraphPack", max_degree_hint: Optional[int] = None) -> "DegreeClasses":
        lib, h = _lib.load(), handle(g.device)
        if max_degree_hint is None:
            mx = _I32(0)
            check(lib.gnx_degree_max(h, g.rowptr.data_ptr(), g.N, C.byref(mx)))
            max_degree_hint = mx.value
        dc = DegreeClasses(int(max_degree_hint) + 1)
        if dc.D > DegreeClasses.MAX_D:
            return dc
        tables = dc.take({name: torch.empty(n, dtype=torch.int32, device=g.device) for name, n in dc.layout(lib, h, g.N)})
        nbytes = lib.gnx_degree_classes_workspace_bytes(g.N, dc.D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
        check(lib.gnx_degree_classes(h, g.rowptr.data_ptr(), g.N, dc.D, dc.dperm.data_ptr(), dc.cls_ptr.data_ptr(),
                                     ws.data_ptr(), nbytes))
        for rows, tiles, ntiles in tables:
            check(lib.gnx_class_tiles(h, dc.cls_ptr.data_ptr(), dc.D, rows, tiles.data_ptr(), ntiles.data_ptr()))
        return dc


def set_option(device: torch.device, opt: int, value: int) -> int:
    """Set an A/B switch of the device's handle (``_lib.OPT_*``; kernel selection only); returns the previous value."""
    lib, h = _lib.load(), handle(device)
    old = _I32(0)
    check(lib.gnx_get_option(h, opt, C.byref(old)))
    check(lib.gnx_set_option(h, opt, int(value)))
    return int(old.value)


def check_range(device: torch.device) -> None:
    """Synchronise and raise ``GnxError(GNX_E_RANGE)`` if any packer / embedding kernel saw an out-of-range integer."""
    check(_lib.load().gnx_check_range(handle(device)))


def pack_graph(edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], batch: Optional[torch.Tensor],
               num_nodes: int, num_graphs: Optional[int] = None, bond_dims: Sequence[int] = (5, 6, 2),
               validate: bool = True) -> GraphPack:
    """edge_index int64[2,E], edge_attr int64[E,K], batch int64[N]|None  ->  GraphPack (all on edge_index.device):
    ``pack_batch`` without a degree hint, i.e. the base arrays alone; the getters build the rest on first use."""
    return pack_batch(edge_index, edge_attr, batch, num_nodes, num_graphs, bond_dims, max_degree_hint=None,
                      validate=validate)


def pack_batch(edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], batch: Optional[torch.Tensor],
               num_nodes: int, num_graphs: Optional[int] = None, bond_dims: Sequence[int] = (5, 6, 2), *,
               max_degree_hint: Optional[int], R: Optional[int] = None, avg_deg_logs: Sequence[float] = (),
               classes: bool = True, edge_tiles: Optional[bool] = None, validate: bool = True,
               tiled_scan: bool = False) -> GraphPack:
    """The GraphPack of a batch in one native call (gnx_pack_batch, 8 launches; 6 for the base arrays alone).  With
    ``max_degree_hint``, an upper bound of the in-degree, the pack has the hint set and everything its getters would build
    later in its caches: the degree classes (``classes``; PNA only), the bond-code index for ``R`` codes, the edge tiles
    for the hint (``edge_tiles``, default = ``classes``) and the degree scalers of up to 4 ``avg_deg_logs``, bit-identical
    to what the getters build; a getter asked for another ``R``, width or ``avg_deg_log`` builds its own.  With
    ``max_degree_hint=None`` only the base arrays are built, ``g.max_degree_hint`` stays None and the other arguments
    are ignored (``degree_classes()`` then reads the maximum in-degree back).  Every output and the call's workspace are
    views of one int32 allocation, so the workspace (a few MB at most here) lives as long as the pack.
    ``tiled_scan`` forces the multi-launch scan that batches above ``gnx_pack_batch_scan_bound()`` nodes take (tests)."""
    dev = edge_index.device
    lib, h = _lib.load(), handle(dev)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"edge_index must be int64[2,E], got {edge_index.dtype} "
                                                f"{tuple(edge_index.shape)}")
    edge_index = edge_index.contiguous()
    N, E = int(num_nodes), int(edge_index.size(1))
    a = _lib.PackBatchArgs()
    a.edge_index, a.N, a.E = edge_index.data_ptr(), N, E
    if edge_attr is not None:
        if edge_attr.dtype != torch.int64 or edge_attr.dim() != 2 or edge_attr.size(0) != E or \
                edge_attr.size(1) != len(bond_dims):
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"edge_attr must be int64[E,{len(bond_dims)}], got "
                                                    f"{edge_attr.dtype} {tuple(edge_attr.shape)}")
        edge_attr = edge_attr.contiguous()
        a.edge_attr, a.K = edge_attr.data_ptr(), len(bond_dims)
        for k, d in enumerate(bond_dims):
            a.bond_dims[k] = int(d)
    B = 1
    if batch is not None:
        if batch.dtype != torch.int64 or batch.dim() != 1 or batch.size(0) != N:
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"batch must be int64[N], got {batch.dtype} {tuple(batch.shape)}")
        if num_graphs is None:
            # PyG: dim_size = batch.max() + 1 (device sync); pass num_graphs to avoid it
            num_graphs = int(batch.max()) + 1 if N > 0 else 0
        batch = batch.contiguous()
        B = int(num_graphs)
        a.batch, a.B = batch.data_ptr(), B
    if max_degree_hint is None:
        R, avg_deg_logs, classes, edge_tiles = None, (), False, False
    g = GraphPack(N, E, B, batch is not None, dev, None if max_degree_hint is None else int(max_degree_hint))
    # which parts: where the getters would build one for this hint
    D = (g.max_degree_hint or 0) + 1
    dc = g._classes = DegreeClasses(D) if classes else None
    build_dc = classes and D <= DegreeClasses.MAX_D
    build_ci = R is not None and GraphPack.has_code_index(R) and E > 0
    if edge_tiles is None:
        edge_tiles = classes
    w = GraphPack.edge_tile_width(g.max_degree_hint) if edge_tiles and E > 0 and N > 0 else None
    avgs = [float(v) for v in dict.fromkeys(float(v) for v in avg_deg_logs)][:_lib.PACK_MAX_AVG]
    a.max_degree, a.R, a.n_avg = D - 1, int(R) if R is not None else 0, len(avgs)
    a.parts = (_lib.PACK_CLASSES if build_dc else 0) | (_lib.PACK_CODE_INDEX if build_ci else 0) | \
        (_lib.PACK_EDGE_TILES if w is not None else 0) | (_lib.PACK_TILED_SCAN if tiled_scan else 0)
    # one allocation: every piece starts on a 256-byte boundary
    base = ("rowptr", "colptr", "perm", "src", "dst", "cpos", "code", "graph_ptr")
    sizes: List[Tuple[str, int]] = list(zip(base, (N + 1, N + 1, E, E, E, E, E, B + 1)))
    for i in range(len(avgs)):
        sizes += [(f"amp{i}", N), (f"att{i}", N)]
    if build_dc:
        sizes += dc.layout(lib, h, N)
    if build_ci:
        sizes += [("code_pos", E), ("code_ptr", R + 1)]
    if w is not None:
        a.edge_tile_w = w
        sizes.append(("edge_tiles", 2 * (lib.gnx_edge_tiles_count(E, w) + 1)))
    ws_bytes = lib.gnx_pack_batch_workspace_bytes(N, E, D if build_dc else 1, R if build_ci else 1)
    sizes.append(("ws", (ws_bytes + 3) // 4))
    off, total = {}, 0
    for name, n in sizes:
        off[name] = total
        total += (n + 63) & ~63
    buf = torch.empty(total, dtype=torch.int32, device=dev)
    v = {name: buf[off[name]:off[name] + n] for name, n in sizes}
    for name in base:
        setattr(g, name, v[name])
        setattr(a, name, v[name].data_ptr())
    for i, key in enumerate(avgs):
        amp, att = v[f"amp{i}"].view(torch.float32), v[f"att{i}"].view(torch.float32)
        a.avg_deg_log[i], a.amp[i], a.att[i] = key, amp.data_ptr(), att.data_ptr()
        g._scalers[key] = (amp, att)
    if build_dc:
        for i, (rows, tiles, ntiles) in enumerate(dc.take(v)):
            a.tile_rows[i], a.tiles[i], a.ntiles[i] = rows, tiles.data_ptr(), ntiles.data_ptr()
        a.dperm, a.cls_ptr = dc.dperm.data_ptr(), dc.cls_ptr.data_ptr()
    if build_ci:
        a.code_pos, a.code_ptr = v["code_pos"].data_ptr(), v["code_ptr"].data_ptr()
        g._code_index = (int(R), v["code_pos"], v["code_ptr"])
    if w is not None:
        a.edge_tiles = v["edge_tiles"].data_ptr()
        g._edge_tiles = (v["edge_tiles"], w)
    a.ws, a.ws_bytes = v["ws"].data_ptr(), ws_bytes
    check(lib.gnx_pack_batch(h, C.byref(a)))
    if validate:
        check_range(dev)
    return g


# ------------------------------------------------------------------------------------------------------------------
# batch collation from a device-resident dataset (data/device.py)
# ------------------------------------------------------------------------------------------------------------------
def _i64c(t: torch.Tensor, name: str, shape: Sequence[Optional[int]]) -> torch.Tensor:
    """``t`` if it is a contiguous int64 tensor of ``shape`` (None = any extent), else GnxError(GNX_E_INVALID)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != len(shape) or not t.is_contiguous() or \
            any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        want = ",".join("*" if s is None else str(s) for s in shape)
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: expected contiguous int64[{want}], got {got}")
    return t


def _on(dev: torch.device, *tensors: torch.Tensor) -> None:
    for t in tensors:
        if t.device != dev:
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"collate: every tensor must be on {dev}, got one on {t.device}")


def collate_ptr(node_ptr: torch.Tensor, edge_ptr: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ptr, eptr) int64[B+1]: exclusive prefix sums of the node / edge counts of graphs ``idx`` int64[B] of a dataset
    with offsets ``node_ptr`` / ``edge_ptr`` int64[G+1].  An index outside [0,G) is clamped and trips ``check_range``."""
    _i64c(node_ptr, "node_ptr", (None,))
    G = node_ptr.size(0) - 1
    _i64c(edge_ptr, "edge_ptr", (G + 1,))
    _i64c(idx, "idx", (None,))
    B = idx.size(0)
    if G < 1 or B < 1:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"collate_ptr: need at least one graph and one index, got G={G} B={B}")
    dev = node_ptr.device
    _on(dev, edge_ptr, idx)
    out = torch.empty(2, B + 1, dtype=torch.int64, device=dev)
    check(_lib.load().gnx_collate_ptr(handle(dev), node_ptr.data_ptr(), edge_ptr.data_ptr(), G, idx.data_ptr(), B,
                                      out[0].data_ptr(), out[1].data_ptr()))
    return out[0], out[1]


def collate_gather(node_ptr: torch.Tensor, edge_ptr: torch.Tensor, x: torch.Tensor, edge_index: torch.Tensor,
                   edge_attr: torch.Tensor, idx: torch.Tensor, ptr: torch.Tensor, eptr: torch.Tensor, N: int, E: int
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(x [N,9], edge_index [2,E], edge_attr [E,3], batch [N]) of the batch ``idx`` from the stored concatenation
    ``x`` [sumN,9] / ``edge_index`` [2,sumE] (graph-local ids) / ``edge_attr`` [sumE,3]; ``ptr`` / ``eptr`` come from
    ``collate_ptr`` and ``N`` / ``E`` are the batch totals the caller computed from its host copy of the sizes."""
    _i64c(node_ptr, "node_ptr", (None,))
    G = node_ptr.size(0) - 1
    _i64c(edge_ptr, "edge_ptr", (G + 1,))
    _i64c(x, "x", (None, 9))
    _i64c(edge_index, "edge_index", (2, None))
    E_src = edge_index.size(1)
    _i64c(edge_attr, "edge_attr", (E_src, 3))
    _i64c(idx, "idx", (None,))
    B = idx.size(0)
    _i64c(ptr, "ptr", (B + 1,))
    _i64c(eptr, "eptr", (B + 1,))
    N, E = int(N), int(E)
    if G < 1 or B < 1 or N < 0 or E < 0:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"collate_gather: bad sizes G={G} B={B} N={N} E={E}")
    dev = x.device
    _on(dev, node_ptr, edge_ptr, edge_index, edge_attr, idx, ptr, eptr)
    i64 = dict(dtype=torch.int64, device=dev)
    x_out, ei_out, ea_out = torch.empty(N, 9, **i64), torch.empty(2, E, **i64), torch.empty(E, 3, **i64)
    batch = torch.empty(N, **i64)
    check(_lib.load().gnx_collate_gather(handle(dev), node_ptr.data_ptr(), edge_ptr.data_ptr(), G, x.data_ptr(),
                                         edge_index.data_ptr(), edge_attr.data_ptr(), E_src, idx.data_ptr(), B,
                                         ptr.data_ptr(), eptr.data_ptr(), N, E, x_out.data_ptr(), ei_out.data_ptr(),
                                         ea_out.data_ptr(), batch.data_ptr()))
    return x_out, ei_out, ea_out, batch


def collate_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``src[idx]`` for a one-row-per-graph field ``src`` [G, ...] of any 4- or 8-byte dtype (moved as raw words)."""
    if not isinstance(src, torch.Tensor) or src.dim() < 1 or not src.is_contiguous() or src.element_size() not in (4, 8):
        got = f"{src.dtype} {tuple(src.shape)}" if isinstance(src, torch.Tensor) else type(src).__name__
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"collate_rows: expected a contiguous [G, ...] tensor of a 4- or 8-byte "
                                                f"dtype, got {got}")
    _i64c(idx, "idx", (None,))
    G, B = src.size(0), idx.size(0)
    if G < 1 or B < 1:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"collate_rows: need at least one row and one index, got G={G} B={B}")
    K = src.numel() // G
    _on(src.device, idx)
    dst = torch.empty((B,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    check(_lib.load().gnx_collate_rows(handle(src.device), src.data_ptr(), G, idx.data_ptr(), B, src.element_size(), K,
                                       dst.data_ptr()))
    return dst


# ------------------------------------------------------------------------------------------------------------------
# embeddings
# ------------------------------------------------------------------------------------------------------------------
def embed_sum_fwd(idx: torch.Tensor, table: torch.Tensor, offsets: Sequence[int]) -> torch.Tensor:
    K = len(offsets) - 1
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.size(1) != K:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"embedding index must be int64[N,{K}], got {idx.dtype} "
                                                f"{tuple(idx.shape)}")
    idx = idx.contiguous()
    table = _f32(table, "table").contiguous()
    N, H = idx.size(0), table.size(1)
    out = torch.empty(N, H, dtype=torch.float32, device=table.device)
    check(_lib.load().gnx_embed_sum_fwd(handle(table.device), idx.data_ptr(), N, K, _carr(list(offsets)),
                                        table.data_ptr(), H, out.data_ptr()))
    return out


def embed_sum_bwd(idx: torch.Tensor, offsets: Sequence[int], dout: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of the concatenated tables; ``out`` (fp32 [R,H], contiguous) is accumulated into (+=) when given."""
    K, R = len(offsets) - 1, offsets[-1]
    dout = _f32(dout, "dout").contiguous()
    idx = idx.contiguous()
    H = dout.size(1)
    if out is not None:
        if out.shape != (R, H) or not out.is_contiguous() or out.dtype is not torch.float32:
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"embed_sum_bwd: out must be contiguous fp32 [{R},{H}]")
        dtable = out
    else:
        dtable = zeros(R, H, device=dout.device)
    lib = _lib.load()
    nbytes = lib.gnx_table_scatter_workspace_bytes(idx.size(0), R, H)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dout.device)
    check(lib.gnx_embed_sum_bwd(handle(dout.device), idx.data_ptr(), idx.size(0), K, _carr(list(offsets)), R,
                                dout.data_ptr(), H, dtable.data_ptr(), ws.data_ptr(), nbytes))
    return dtable


# ------------------------------------------------------------------------------------------------------------------
# dense
# ------------------------------------------------------------------------------------------------------------------
Seg = Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]  # (A view [M,k], rowscale [M] | None, B view)


class _SegArrays(threading.local):
    """Per-thread reusable descriptor arrays (forward runs on the caller's thread, backward on autograd's)."""

    def __init__(self):
        self.by_len = {n: (GemmSeg * n)() for n in range(1, 5)}


_SEG_ARRAYS = _SegArrays()


GSeg = Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, int]  # (A view, rowscale|None, B of class 0, stride)


def _gemm_args(segs, out, dc, bias, mask, relu, accumulate, b_trans, forward_tiles):
    """Marshals a gemm() (``dc`` None, Seg tuples) or gemm_grouped() (GSeg tuples) call: the arguments of
    gnx_gemm_grouped_rows / gnx_gemm_plan from the handle to tile_rows (NULL grouping arrays: ungrouped; tile_rows 0: the
    128-row table), and the workspace tensor they point into (None: the call needs no split weight images)."""
    M, N = out.shape
    cptr, ldc = _mat(out, "out")
    n = len(segs)
    if dc is None:
        arr, strides = _SEG_ARRAYS.by_len[n], None  # reused: the library copies the descriptors during the call
    else:
        arr, strides = (GemmSeg * n)(), (C.c_int64 * n)()
    for i, sg in enumerate(segs):
        a, rs, b = sg[0], sg[1], sg[2]
        ap, lda = _mat(a, "A")
        bp, ldb = _mat(b, "B")
        k = a.size(1)
        if dc is None:
            if a.size(0) != M or tuple(b.shape) != ((N, k) if b_trans else (k, N)):
                raise _lib.GnxError(_lib.GNX_E_INVALID, f"gemm segment {i}: A {tuple(a.shape)} B {tuple(b.shape)} "
                                                        f"out {tuple(out.shape)} b_trans={b_trans}")
        else:
            strides[i] = sg[3]
        e = arr[i]
        e.a, e.lda, e.rowscale = ap, lda, (None if rs is None else rs.data_ptr())
        e.b, e.ldb, e.k = bp, ldb, k
    flags = (_lib.GEMM_RELU if relu else 0) | (_lib.GEMM_ACCUMULATE if accumulate else 0) | \
            (_lib.GEMM_B_TRANS if b_trans else 0)
    mp, ldm = (None, 0) if mask is None else _mat(mask, "mask")
    lib, h = _lib.load(), handle(out.device)
    # split weight images of the tiled split-operand kernel live in caller-owned scratch (0 bytes for most calls; the
    # split path needs >= 4096 rows, so small products skip the query: host time matters in tiny-kernel phases)
    D = 1 if dc is None else dc.D
    nbytes = lib.gnx_gemm_workspace_bytes(h, n, arr, strides, D, M, N, mp, flags, int(dc is not None)) if M >= 4096 else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device) if nbytes else None
    if dc is None:
        table = (None, None, None, 0)
    elif forward_tiles:
        table = (dc.dperm.data_ptr(), dc.tiles_p.data_ptr(), dc.ntiles_p.data_ptr(), dc.max_tiles_p)
    else:
        table = (dc.dperm.data_ptr(), dc.tiles.data_ptr(), dc.ntiles.data_ptr(), dc.max_tiles)
    tile_rows = dc.tile_rows_p if dc is not None and forward_tiles else 0
    return (h, n, arr, strides, D, M, N, _ptr(bias), mp, ldm, cptr, ldc, flags, *table, _ptr(ws), nbytes, tile_rows), ws


def gemm(segs: Sequence[Seg], out: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
         mask: Optional[torch.Tensor] = None, relu: bool = False, accumulate: bool = False,
         b_trans: bool = True) -> torch.Tensor:
    """out[M,N] (+)= act(sum_s (rs_s * A_s) @ B_s(^T) + bias), optionally * (mask > 0).  See gnx_gemm in gnx.h.

    b_trans=True: B_s is a [N,k] weight view (forward Linear); False: B_s is a [k,N] view (input gradient).
    """
    if out.size(0) == 0:
        return out
    a, _ws = _gemm_args(segs, out, None, bias, mask, relu, accumulate, b_trans, False)
    check(_lib.load().gnx_gemm(*a[0:3], *a[5:13], *a[17:19]))
    return out


def gemm_grouped(segs: Sequence[GSeg], out: torch.Tensor, dc: DegreeClasses, *, bias: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, relu: bool = False, b_trans: bool = True,
                 forward_tiles: bool = False) -> torch.Tensor:
    """gemm() over the degree-class tiles of ``dc``: A rows gathered / out rows scattered through ``dc.dperm``; segment
    s reads its weight at ``B_s + class * stride_s`` elements (stride 0 = the same weight for every class).
    ``forward_tiles``: walk ``dc.tiles_p`` (the 96- or 128-row table of the pipelined forward product) instead of the
    128-row table."""
    if out.size(0) == 0:
        return out
    a, _ws = _gemm_args(segs, out, dc, bias, mask, relu, False, b_trans, forward_tiles)
    lib = _lib.load()
    check(lib.gnx_gemm_grouped_rows(*a) if forward_tiles else lib.gnx_gemm_grouped(*a[:19]))
    return out


def gemm_plan(segs, out: torch.Tensor, *, bias: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              relu: bool = False, accumulate: bool = False, b_trans: bool = True, dc: Optional[DegreeClasses] = None,
              forward_tiles: bool = False) -> Tuple[str, "_lib.GemmPlanInfo"]:
    """Which kernel gemm() (``dc`` None) or gemm_grouped() takes for these arguments, marshalled as they marshal them:
    (its name, one of _lib.GEMM_KERNEL_NAMES, and the gnx_gemm_plan_info).  Launches nothing."""
    a, _ws = _gemm_args(segs, out, dc, bias, mask, relu, accumulate, b_trans, forward_tiles)
    info = _lib.GemmPlanInfo()
    check(_lib.load().gnx_gemm_plan(*a, C.byref(info)))
    return _lib.GEMM_KERNEL_NAMES[info.kernel], info


def gemm_wgrad_grouped(dC: torch.Tensor, A: torch.Tensor, dW_cls: torch.Tensor, dc: DegreeClasses) -> None:
    """dW_cls[c] (fp32[D, N, K], contiguous) += sum over rows of class c of dC[row]^T A[row]."""
    M, N = dC.shape
    if M == 0:
        return
    xp, ldx = _mat(dC, "dC")
    ap, lda = _mat(A, "A")
    K = A.size(1)
    if dW_cls.shape != (dc.D, N, K) or not dW_cls.is_contiguous():
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"dW_cls must be contiguous [{dc.D},{N},{K}], got {tuple(dW_cls.shape)}")
    check(_lib.load().gnx_gemm_wgrad_grouped(handle(dC.device), xp, ldx, ap, lda, M, N, K, dW_cls.data_ptr(), K, N * K,
                                             dc.dperm.data_ptr(), dc.chunks.data_ptr(), dc.nchunks.data_ptr(),
                                             dc.max_chunks))


def gemm_wgrad_grouped_plan(dC: torch.Tensor, A: torch.Tensor, max_chunks: int) -> Tuple[str, "_lib.WgradGroupedPlanInfo"]:
    """Which kernel gemm_wgrad_grouped() takes for these operands and a chunk table of ``max_chunks`` entries, marshalled
    as it marshals them: (its name, one of _lib.WGRAD_KERNEL_NAMES, and the gnx_wgrad_grouped_plan_info).  Launches
    nothing."""
    xp, ldx = _mat(dC, "dC")
    ap, lda = _mat(A, "A")
    info = _lib.WgradGroupedPlanInfo()
    check(_lib.load().gnx_gemm_wgrad_grouped_plan(handle(dC.device), ldx, lda, xp, ap, dC.size(0), dC.size(1), A.size(1),
                                                  int(max_chunks), C.byref(info)))
    return _lib.WGRAD_KERNEL_NAMES[info.kernel], info


def pna_weff(W: torch.Tensor, F: int, D: int, avg_deg_log: float) -> torch.Tensor:
    """Weff fp32[D, F, 4F] from post_nns[t][0].weight ([F, 13F])."""
    wp, ldw = _mat(W, "W")
    out = torch.empty(D, F, 4 * F, dtype=torch.float32, device=W.device)
    check(_lib.load().gnx_pna_weff(handle(W.device), wp, ldw, F, D, float(avg_deg_log), out.data_ptr()))
    return out


def pna_weff_bwd(dWeff: torch.Tensor, F: int, D: int, avg_deg_log: float, dW: torch.Tensor) -> None:
    wp, ldw = _mat(dW, "dW")
    check(_lib.load().gnx_pna_weff_bwd(handle(dW.device), dWeff.data_ptr(), F, D, float(avg_deg_log), wp, ldw))


_SIDE_ENABLED = False
_SIDE_PENDING = set()   # device indices with weight-gradient launches not yet joined
_SIDE_KEEP: dict = {}   # device index -> buffers those launches touch, kept alive until the join


def set_wgrad_side_stream(enabled: bool) -> None:
    """Run weight-gradient kernels on a second HIP stream so they overlap the input-gradient chain (the two are
    independent inside a layer's backward).  A Function whose weight gradients all go into persistent in-place sinks
    (``functional.set_grad_in_place``) defers the join to the end of the whole backward pass
    (``join_side_stream_at_end_of_backward``); a Function that hands a freshly allocated gradient back to autograd joins
    before it returns (``finish_backward``), because AccumulateGrad consumes that tensor on the main stream at once."""
    global _SIDE_ENABLED
    _SIDE_ENABLED = bool(enabled)


_JOIN_QUEUED = False


_SIDE_USED: dict = {}    # device index -> set of side-stream indices with launches not yet joined


def _join(idx: int, which: Optional[int] = None) -> None:
    """Main stream waits for side stream ``which`` of device ``idx`` (None = every side stream in use)."""
    dev = torch.device("cuda", idx)
    used = _SIDE_USED.get(idx, set())
    for w in sorted(used if which is None else (used & {which})):
        check(_lib.load().gnx_side_join_n(handle(dev), w))
        used.discard(w)
    if not used:
        _SIDE_PENDING.discard(idx)
        _SIDE_KEEP.pop(idx, None)  # later users of these blocks are ordered behind the join on the main stream


def _join_all_side_streams() -> None:
    global _JOIN_QUEUED
    _JOIN_QUEUED = False
    for idx in list(_SIDE_PENDING):
        _join(idx)


def join_side_stream_at_end_of_backward() -> None:
    """Called from inside an autograd backward: the main stream waits for the weight-gradient stream ONCE, when the
    autograd engine finishes this backward pass (gradients are only consumed after it), so weight-gradient kernels of
    one layer overlap the input-gradient chain of the next layers too."""
    global _JOIN_QUEUED
    if _SIDE_PENDING and not _JOIN_QUEUED:
        _JOIN_QUEUED = True
        torch.autograd.Variable._execution_engine.queue_callback(_join_all_side_streams)


_WGRAD_DONE_HOOK = None


def set_wgrad_done_hook(fn) -> None:
    """``fn(sinks)`` is called at the end of every conv / Linear backward whose weight gradients all went into
    persistent in-place sinks, right after their launches were issued (on the side stream when enabled): the
    data-parallel exchange uses it to start a layer's slice of the all-reduce while backward continues."""
    global _WGRAD_DONE_HOOK
    _WGRAD_DONE_HOOK = fn


def wgrad_done_hook_set() -> bool:
    return _WGRAD_DONE_HOOK is not None


def side_stream(device: torch.device, which: int = 0) -> "torch.cuda.Stream":
    """One of the library's side streams (0 = weight gradients, 1 = bond-table chain) as a torch stream (no ownership)."""
    out = C.c_void_p()
    check(_lib.load().gnx_side_stream_n(handle(device), which, C.byref(out)))
    return torch.cuda.ExternalStream(out.value, device=device)


def second_side_stream_in_use(device: torch.device) -> bool:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return 1 in _SIDE_USED.get(idx, set())


def wgrad_stream_enabled() -> bool:
    return _SIDE_ENABLED


def scale_(t: torch.Tensor, v: float) -> torch.Tensor:
    """t *= v through a gnx launch (flat fp32 HIP buffers; anything else falls back to torch's mul_)."""
    if t.is_cuda and t.dtype is torch.float32 and t.is_contiguous():
        if t.numel():
            check(_lib.load().gnx_scale(handle(t.device), t.data_ptr(), t.numel(), float(v)))
        return t
    return t.mul_(v)


def finish_backward(device: torch.device, all_in_place: bool, sinks=None) -> None:
    """Last call of an autograd backward that issued weight-gradient launches.  ``all_in_place``: every destination of
    those launches is a persistent gradient buffer nobody reads before the backward pass ends -> one deferred join for
    the whole pass.  Otherwise the Function is about to return fresh tensors that autograd accumulates on the main
    stream immediately -> the main stream waits for the side stream now."""
    if all_in_place:
        if _WGRAD_DONE_HOOK is not None and sinks:
            _WGRAD_DONE_HOOK(sinks)
        join_side_stream_at_end_of_backward()
    else:
        join_side_stream(device)


_WGRAD_QUEUE: List[tuple] = []
_WGRAD_BATCHING = True


def set_wgrad_batching(enabled: bool) -> None:
    """A/B switch: queue a layer's weight gradients and launch them as one batched kernel (default on)."""
    global _WGRAD_BATCHING
    _WGRAD_BATCHING = bool(enabled)


def queue_wgrad(dC: torch.Tensor, A: torch.Tensor, dW: torch.Tensor, *, rowscale: Optional[torch.Tensor] = None,
                dbias: Optional[torch.Tensor] = None) -> None:
    """Like gemm_wgrad, but deferred until flush_wgrads() so that independent weight gradients share one launch."""
    if dC.size(0) == 0:
        return
    if not _WGRAD_BATCHING:
        gemm_wgrad(dC, A, dW, rowscale=rowscale, dbias=dbias)
        return
    _WGRAD_QUEUE.append((dC, A, dW, rowscale, dbias))


def flush_wgrads() -> None:
    """Launch every queued weight gradient: up to 8 problems per kernel (gnx_gemm_wgrad_batched), on the side stream
    when enabled.  Problems that do not meet the batched kernel's alignment rules go through gemm_wgrad."""
    global _WGRAD_QUEUE
    jobs, _WGRAD_QUEUE = _WGRAD_QUEUE, []
    if not jobs:
        return
    batchable, rest = [], []
    for j in jobs:
        dC, A, dW, rs, db = j
        ok = all(t is None or t.data_ptr() % 16 == 0 for t in (dC, A)) and dC.stride(0) % 4 == 0 and \
            A.stride(0) % 4 == 0 and dC.size(1) % 4 == 0 and A.size(1) % 4 == 0 and dC.size(0) > 1 and \
            (dC.size(1) == 1 or dC.stride(1) == 1) and (A.size(1) == 1 or A.stride(1) == 1)
        (batchable if ok else rest).append(j)
    for dC, A, dW, rs, db in rest:
        gemm_wgrad(dC, A, dW, rowscale=rs, dbias=db)
    # largest row counts first so that problems of similar size share a launch
    batchable.sort(key=lambda j: -j[0].size(0))
    for i in range(0, len(batchable), 8):
        chunk = batchable[i:i + 8]
        arr = (_lib.WgradProb * len(chunk))()
        keep = []
        for k, (dC, A, dW, rs, db) in enumerate(chunk):
            xp, ldx = _mat(dC, "dC")
            ap, lda = _mat(A, "A")
            wp, ldw = _mat(dW, "dW")
            M, N = dC.shape
            K = A.size(1)
            if A.size(0) != M or dW.size(0) != N or dW.size(1) != K:
                raise _lib.GnxError(_lib.GNX_E_INVALID, f"wgrad shapes dC {tuple(dC.shape)} A {tuple(A.shape)} "
                                                        f"dW {tuple(dW.shape)}")
            arr[k].dC, arr[k].lddc, arr[k].A, arr[k].lda = xp, ldx, ap, lda
            arr[k].rowscale, arr[k].dW, arr[k].lddw, arr[k].dbias = _ptr(rs), wp, ldw, _ptr(db)
            arr[k].M, arr[k].N, arr[k].K = M, N, K
            keep += [dC, A, rs, dW, db]
        ref = chunk[0][0]
        n = len(chunk)
        _run_on_side(ref, keep, lambda arr=arr, n=n, ref=ref: check(
            _lib.load().gnx_gemm_wgrad_batched(handle(ref.device), n, arr)))


def join_side_stream(device: torch.device, which: Optional[int] = None) -> None:
    """Make the current stream wait for the launches issued on the side stream(s) (``which`` = one of them)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _SIDE_PENDING:
        _join(idx, which)


def _run_on_side(ref: torch.Tensor, tensors, fn, which: int = 0) -> None:
    """Run ``fn`` (weight-gradient launches) on the library's side stream when enabled, else inline.  ``tensors`` are
    the device buffers the launches read or write; they are kept referenced until the join so the caching allocator
    cannot hand them out again under the side kernels (fork / join are two HIP event calls inside the library:
    gnx_side_begin / gnx_side_join)."""
    if _SIDE_ENABLED and ref.is_cuda:
        idx = ref.device.index
        lib, h = _lib.load(), handle(ref.device)
        check(lib.gnx_side_begin_n(h, which))
        try:
            fn()
        finally:
            check(lib.gnx_side_end(h))
        _SIDE_KEEP.setdefault(idx, []).extend(t for t in tensors if t is not None)
        _SIDE_PENDING.add(idx)
        _SIDE_USED.setdefault(idx, set()).add(which)
        return
    fn()


def run_after_wgrads(ref: torch.Tensor, tensors, fn) -> None:
    """Run ``fn`` (launches that consume a freshly computed weight gradient) on the stream the weight gradients run
    on, i.e. ordered behind them; ``tensors`` are kept alive until the join like every side-stream operand."""
    _run_on_side(ref, tensors, fn)


def keep_until_join(device: torch.device, tensors, whichs=(0, 1)) -> None:
    """Register buffers that launches issued on the side streams by a native composite call (gnx_pna_conv_bwd) read or
    write: they stay referenced until the join, exactly like the operands of ``_run_on_side``."""
    if not _SIDE_ENABLED:
        return
    idx = device.index if device.index is not None else torch.cuda.current_device()
    _SIDE_KEEP.setdefault(idx, []).extend(t for t in tensors if t is not None)
    _SIDE_PENDING.add(idx)
    _SIDE_USED.setdefault(idx, set()).update(whichs)


def split_launch_counts(device: torch.device) -> Tuple[int, int]:
    """(per-call, batched) split launches the library has issued on ``device`` so far: k_split_weights in front of one
    product, k_split_weights_batched of gnx_pna_split_all (host counters; tests take differences)."""
    per_call, batched = C.c_int64(0), C.c_int64(0)
    check(_lib.load().gnx_gemm_split_counts(handle(device), C.byref(per_call), C.byref(batched)))
    return int(per_call.value), int(batched.value)


def run_on_second_side_stream(ref: torch.Tensor, tensors, fn) -> None:
    """Run ``fn`` on side stream 1 (inline when side streams are off): the bond-table gradient chain of a conv layer's
    backward -- it forks from the main stream here, feeds parameter gradients and the bond-embedding gradient only, and
    is joined with the rest at the end of backward (or by ``join_side_stream(device, 1)``)."""
    _run_on_side(ref, tensors, fn, which=1)


def gemm_wgrad_inline(dC: torch.Tensor, A: torch.Tensor, dW: torch.Tensor, dbias: Optional[torch.Tensor] = None) -> None:
    """dW += dC^T A (dbias += column sums of dC) on the CURRENT stream of the library handle -- inside
    ``run_after_wgrads`` / ``run_on_second_side_stream`` that is the side stream."""
    _gemm_wgrad_launch(dC, A, dW, None, dbias)


def axpy_(y: torch.Tensor, x: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """y += alpha * x for contiguous fp32 HIP vectors of equal size."""
    if y.numel() != x.numel() or not (y.is_contiguous() and x.is_contiguous()):
        raise _lib.GnxError(_lib.GNX_E_INVALID, "axpy_: need contiguous tensors of equal size")
    check(_lib.load().gnx_axpy(handle(y.device), _f32(y, "y").data_ptr(), _f32(x, "x").data_ptr(), y.numel(),
                               float(alpha)))
    return y


def gemm_wgrad(dC: torch.Tensor, A: torch.Tensor, dW: torch.Tensor, *, rowscale: Optional[torch.Tensor] = None,
               dbias: Optional[torch.Tensor] = None) -> None:
    """dW[N,K] += dC[M,N]^T @ (rowscale * A[M,K]);  dbias[N] += column sums of dC."""
    if dC.size(0) == 0:
        return
    _run_on_side(dC, (dC, A, rowscale, dW, dbias), lambda: _gemm_wgrad_launch(dC, A, dW, rowscale, dbias))


def pna_post0_wgrad_classes(g: torch.Tensor, A: torch.Tensor, dc: "DegreeClasses", F: int, avg_deg_log: float,
                            dW: torch.Tensor) -> None:
    """dW[:, F:13F] += the three A-blocks of post-layer 0's weight gradient, through per-degree-class partial sums."""
    if g.size(0) == 0:
        return
    dWeff = zeros(dc.D, F, 4 * F, device=g.device)

    def run():
        gemm_wgrad_grouped(g, A, dWeff, dc)
        pna_weff_bwd(dWeff, F, dc.D, avg_deg_log, dW)

    _run_on_side(g, (g, A, dWeff, dW), run)


def _gemm_wgrad_launch(dC, A, dW, rowscale, dbias) -> None:
    M, N = dC.shape
    xp, ldx = _mat(dC, "dC")
    ap, lda = _mat(A, "A")
    wp, ldw = _mat(dW, "dW")
    K = A.size(1)
    if A.size(0) != M or dW.size(0) != N or dW.size(1) != K:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"wgrad shapes dC {tuple(dC.shape)} A {tuple(A.shape)} "
                                                f"dW {tuple(dW.shape)}")
    check(_lib.load().gnx_gemm_wgrad(handle(dW.device), xp, ldx, ap, lda, _ptr(rowscale), M, N, K, wp, ldw,
                                     _ptr(dbias)))


# ------------------------------------------------------------------------------------------------------------------
# message passing
# ------------------------------------------------------------------------------------------------------------------
def edge_combine_fwd(P: torch.Tensor, Q: torch.Tensor, Te: torch.Tensor, g: GraphPack, relu: bool) -> torch.Tensor:
    H = P.size(1)
    h1 = torch.empty(g.E, H, dtype=torch.float32, device=P.device)
    check(_lib.load().gnx_edge_combine_fwd(handle(P.device), P.data_ptr(), Q.data_ptr(), Te.data_ptr(),
                                           g.src.data_ptr(), g.dst.data_ptr(), g.code.data_ptr(), g.E, H, int(relu),
                                           h1.data_ptr()))
    return h1


def edge_combine_bwd_pq(gr: torch.Tensor, g: GraphPack) -> Tuple[torch.Tensor, torch.Tensor]:
    """dP[i] = sum of g over CSR row i, dQ[j] = sum of g over the edges leaving j (no bond-table gradient)."""
    H = gr.size(1)
    dP = torch.empty(g.N, H, dtype=torch.float32, device=gr.device)
    dQ = torch.empty(g.N, H, dtype=torch.float32, device=gr.device)
    check(_lib.load().gnx_edge_combine_bwd(handle(gr.device), gr.data_ptr(), g.rowptr.data_ptr(), g.colptr.data_ptr(),
                                           g.cpos.data_ptr(), g.code.data_ptr(), g.N, g.E, H, 0, dP.data_ptr(),
                                           dQ.data_ptr(), None, None, 0))
    return dP, dQ


def bond_table_grad(gr: torch.Tensor, g: GraphPack, R: int, pos: Optional[torch.Tensor]) -> torch.Tensor:
    """dTe[r] = sum of g over the edges with bond code r; ``pos`` = ``g.code_index(R)`` fetched by the caller (it may
    build the index, which must not happen on a side stream)."""
    H = gr.size(1)
    dTe = zeros(R, H, device=gr.device)
    lib = _lib.load()
    if g.E == 0:
        return dTe
    if pos is not None:
        check(lib.gnx_key_segment_sum(handle(gr.device), gr.data_ptr(), pos.data_ptr(), g.code.data_ptr(), g.E, H,
                                      dTe.data_ptr()))
        return dTe
    # more than 64 codes (never the 60-row bond table): the LDS-privatised scatter inside gnx_edge_combine_bwd
    nbytes = lib.gnx_table_scatter_workspace_bytes(g.E, R, H)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=gr.device)
    tmp = torch.empty(2, g.N, H, dtype=torch.float32, device=gr.device)
    check(lib.gnx_edge_combine_bwd(handle(gr.device), gr.data_ptr(), g.rowptr.data_ptr(), g.colptr.data_ptr(),
                                   g.cpos.data_ptr(), g.code.data_ptr(), g.N, g.E, H, R, tmp[0].data_ptr(),
                                   tmp[1].data_ptr(), dTe.data_ptr(), ws.data_ptr(), nbytes))
    return dTe


def bond_code_index(g: GraphPack, R: int, H: int) -> Optional[torch.Tensor]:
    return g.code_index(R) if ((H % 4 == 0 and H <= 1024) or H <= 256) and g.E > 0 else None


def edge_combine_bwd(gr: torch.Tensor, g: GraphPack, R: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    dP, dQ = edge_combine_bwd_pq(gr, g)
    return dP, dQ, bond_table_grad(gr, g, R, bond_code_index(g, R, gr.size(1)))


def pna_edge_fwd(P: torch.Tensor, Q: torch.Tensor, Te: torch.Tensor, g: GraphPack, T: int, F: int,
                 weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], max_degree: int,
                 keep: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], torch.Tensor]:
    """Fused message assembly -> pre-layer 1 -> aggregate (gnx_pna_edge_fwd): returns (h1 [E,H], m [E,H], A [N,T*4F]);
    ``keep=False`` does not materialise h1 / m (inference).  ``weights`` / ``biases``: pre-layer 1 of every tower."""
    H = T * F
    tiles = g.edge_tiles(max_degree)
    if tiles is None and g.E > 0:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"pna_edge_fwd: in-degree bound {max_degree} too large for edge tiles")
    dev = P.device
    h1 = torch.empty(g.E, H, dtype=torch.float32, device=dev) if keep else None
    m = torch.empty(g.E, H, dtype=torch.float32, device=dev) if keep else None
    A = torch.empty(g.N, T * 4 * F, dtype=torch.float32, device=dev)
    warr = (C.c_void_p * T)(*[_f32(w, "W1").data_ptr() for w in weights])
    barr = (C.c_void_p * T)(*[_f32(b, "b1").data_ptr() for b in biases])
    for w in weights:
        if tuple(w.shape) != (F, F) or not w.is_contiguous():
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"pna_edge_fwd: pre-layer 1 weight must be contiguous [{F},{F}]")
    info, w_ = tiles if tiles is not None else (None, 1)
    check(_lib.load().gnx_pna_edge_fwd(handle(dev), P.data_ptr(), Q.data_ptr(), Te.data_ptr(), g.src.data_ptr(),
                                       g.dst.data_ptr(), g.code.data_ptr(), g.rowptr.data_ptr(), _ptr(info), w_, g.N, g.E,
                                       T, F, C.cast(warr, C.POINTER(C.c_void_p)), C.cast(barr, C.POINTER(C.c_void_p)),
                                       _ptr(h1), _ptr(m), A.data_ptr()))
    return h1, m, A


def pna_edge_bwd(ge: torch.Tensor, h1: torch.Tensor, g: GraphPack, T: int, F: int, R: int,
                 weights: Sequence[torch.Tensor], max_degree: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fused masked input gradient of pre-layer 1 + destination sums + bond-table sums (gnx_pna_edge_bwd): returns
    (gh1 [E,H], dP [N,H], dTe [R,H]).  ``weights``: pre-layer 1 ([F,F]) of every tower."""
    H = T * F
    tiles = g.edge_tiles(max_degree)
    if tiles is None and g.E > 0:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"pna_edge_bwd: in-degree bound {max_degree} too large for edge tiles")
    dev = ge.device
    gh1 = torch.empty(g.E, H, dtype=torch.float32, device=dev)
    dP = torch.empty(g.N, H, dtype=torch.float32, device=dev)
    dTe = zeros(R, H, device=dev)
    warr = (C.c_void_p * T)(*[_f32(w, "W1").data_ptr() for w in weights])
    info, w_ = tiles if tiles is not None else (None, 1)
    check(_lib.load().gnx_pna_edge_bwd(handle(dev), _f32(ge, "ge").contiguous().data_ptr(), _f32(h1, "h1").contiguous().data_ptr(),
                                       g.code.data_ptr(), g.rowptr.data_ptr(), _ptr(info), w_, g.N, g.E, T, F, R,
                                       C.cast(warr, C.POINTER(C.c_void_p)), gh1.data_ptr(), dP.data_ptr(), dTe.data_ptr()))
    return gh1, dP, dTe


def pna_aggregate_fwd(m: torch.Tensor, g: GraphPack, T: int, F: int) -> torch.Tensor:
    A = torch.empty(g.N, T * 4 * F, dtype=torch.float32, device=m.device)
    check(_lib.load().gnx_pna_aggregate_fwd(handle(m.device), m.data_ptr(), g.rowptr.data_ptr(), g.N, g.E, T, F,
                                            A.data_ptr()))
    return A


def pna_aggregate_bwd(dA: torch.Tensor, m: torch.Tensor, A: torch.Tensor, g: GraphPack, T: int, F: int) -> torch.Tensor:
    dm = torch.empty_like(m)
    check(_lib.load().gnx_pna_aggregate_bwd(handle(m.device), dA.data_ptr(), m.data_ptr(), A.data_ptr(),
                                            g.rowptr.data_ptr(), g.N, g.E, T, F, dm.data_ptr()))
    return dm


def pna_dA_aggregate_bwd(gout: torch.Tensor, weffs: Sequence[torch.Tensor], m: torch.Tensor, A: torch.Tensor, g: GraphPack,
                         dc: DegreeClasses, T: int, F: int, *, dA: Optional[torch.Tensor] = None,
                         dm: Optional[torch.Tensor] = None, forward_tiles: bool = False) -> Tuple[torch.Tensor, bool]:
    """dm = pna_aggregate_bwd(dA) with dA[:, t] = gout[:, tF:(t+1)F] @ weffs[t][class], and whether every tower took the
    fused launch (gnx_pna_da_aggregate_bwd: dA is then neither written nor read).  A tower whose call is not eligible sends
    the whole call down the two launches (gemm_grouped per tower into ``dA``, pna_aggregate_bwd).  ``weffs[t]``: fp32
    [D, F, 4F]; ``dA`` (fp32 [N, T 4F]) and ``dm`` (like ``m``) are allocated when not given."""
    N = gout.size(0)
    if dA is None:
        dA = torch.empty(N, T * 4 * F, dtype=torch.float32, device=m.device)
    if dm is None:
        dm = torch.empty_like(m)
    lib, h = _lib.load(), handle(m.device)
    nbytes = lib.gnx_pna_conv_bwd_workspace_bytes(T, F, dc.D)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=m.device)
    if forward_tiles:
        table = (dc.dperm.data_ptr(), dc.tiles_p.data_ptr(), dc.ntiles_p.data_ptr(), dc.max_tiles_p)
    else:
        table = (dc.dperm.data_ptr(), dc.tiles.data_ptr(), dc.ntiles.data_ptr(), dc.max_tiles)
    took = C.c_int32(0)
    for t in range(T):
        check(lib.gnx_pna_da_aggregate_bwd(h, weffs[t].data_ptr(), T, F, dc.D, t, gout.data_ptr(), dA.data_ptr(), m.data_ptr(),
                                           g.rowptr.data_ptr(), N, g.E, dm.data_ptr(), *table, None, None, ws.data_ptr(), nbytes,
                                           C.byref(took)))
        if not took.value:
            break
    else:
        return dm, True
    for t in range(T):
        gemm_grouped([(gout[:, t * F:(t + 1) * F], None, weffs[t][0], 4 * F * F)], dA[:, t * 4 * F:(t + 1) * 4 * F], dc,
                     b_trans=False, forward_tiles=forward_tiles)
    check(lib.gnx_pna_aggregate_bwd(h, dA.data_ptr(), m.data_ptr(), A.data_ptr(), g.rowptr.data_ptr(), N, g.E, T, F,
                                    dm.data_ptr()))
    return dm, False


def gine_aggregate_fwd(x: torch.Tensor, Le: torch.Tensor, g: GraphPack, eps: float) -> torch.Tensor:
    out = torch.empty_like(x)
    check(_lib.load().gnx_gine_aggregate_fwd(handle(x.device), x.data_ptr(), Le.data_ptr(), g.rowptr.data_ptr(),
                                             g.src.data_ptr(), g.code.data_ptr(), g.N, g.E, x.size(1), float(eps),
                                             out.data_ptr()))
    return out


def gine_aggregate_bwd(dout: torch.Tensor, x: torch.Tensor, Le: torch.Tensor, g: GraphPack,
                       eps: float, want_dle: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dx (and, with ``want_dle``, the bond-table gradient dLe from the same call)."""
    dx = torch.empty_like(x)
    dLe = zeros(*Le.shape, device=Le.device) if want_dle else None
    pos = g.code_index(Le.size(0)) if (g.E > 0 and want_dle) else None  # inverted index by bond code (None above 64 codes)
    check(_lib.load().gnx_gine_aggregate_bwd(handle(x.device), dout.data_ptr(), x.data_ptr(), Le.data_ptr(),
                                             g.colptr.data_ptr(), g.cpos.data_ptr(), g.src.data_ptr(),
                                             g.dst.data_ptr(), g.code.data_ptr(), _ptr(pos), g.N, g.E, x.size(1),
                                             Le.size(0), float(eps), dx.data_ptr(), _ptr(dLe)))
    return dx, dLe


def gine_dle(dout: torch.Tensor, x: torch.Tensor, Le: torch.Tensor, g: GraphPack, pos: Optional[torch.Tensor]) -> torch.Tensor:
    """dLe[r] = sum over the edges with bond code r of dout[dst] * (x[src] + Le[r] > 0), on the handle's current stream."""
    dLe = zeros(*Le.shape, device=Le.device)
    check(_lib.load().gnx_gine_dle(handle(x.device), dout.data_ptr(), x.data_ptr(), Le.data_ptr(), g.src.data_ptr(),
                                   g.dst.data_ptr(), g.code.data_ptr(), _ptr(pos), g.E, x.size(1), Le.size(0),
                                   dLe.data_ptr()))
    return dLe


def transformer_attn_fwd(qkvs: torch.Tensor, Le: torch.Tensor, g: GraphPack, heads: int, p: float = 0.0,
                         seed: int = 0, offset: int = 0, want_mask: bool = False
                         ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """TransformerConv attention over the CSR (gnx_transformer_attn_fwd): qkvs [N,4H] = q|k|v|s, Le [R,H] ->
    (out [N,H], alpha [E,heads] in CSR order, keep mask uint8 [E,heads] if ``want_mask``).  p > 0: dropout on alpha with
    the mask keyed by (seed, offset)."""
    qkvs = _f32(qkvs, "qkvs").contiguous()
    Le = _f32(Le, "Le").contiguous()
    N, H = qkvs.size(0), qkvs.size(1) // 4
    if qkvs.size(1) != 4 * H or Le.size(1) != H or heads <= 0 or H % heads != 0:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"transformer_attn_fwd: qkvs {tuple(qkvs.shape)} Le {tuple(Le.shape)} "
                                                f"heads {heads}")
    dev = qkvs.device
    out = torch.empty(N, H, dtype=torch.float32, device=dev)
    alpha = torch.empty(g.E, heads, dtype=torch.float32, device=dev)
    keep = torch.empty(g.E, heads, dtype=torch.uint8, device=dev) if want_mask else None
    check(_lib.load().gnx_transformer_attn_fwd(handle(dev), qkvs.data_ptr(), Le.data_ptr(), g.rowptr.data_ptr(),
                                               g.src.data_ptr(), g.code.data_ptr(), N, g.E, int(heads), H // int(heads),
                                               float(p), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                               out.data_ptr(), alpha.data_ptr(), _ptr(keep)))
    return out, alpha, keep


def transformer_attn_bwd(dout: torch.Tensor, qkvs: torch.Tensor, Le: torch.Tensor, alpha: torch.Tensor, g: GraphPack,
                         heads: int, p: float = 0.0, seed: int = 0, offset: int = 0, want_dle: bool = True
                         ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Backward of ``transformer_attn_fwd``: (dqkv [N,3H] = dq|dk|dv (deterministic), scratch [2,E,heads] for
    ``transformer_attn_dle``, dLe [R,H] if ``want_dle``)."""
    dout = _f32(dout, "dout").contiguous()
    N, H = dout.shape
    dev = dout.device
    dqkv = torch.empty(N, 3 * H, dtype=torch.float32, device=dev)
    scratch = torch.empty(2, g.E, heads, dtype=torch.float32, device=dev)
    dLe = zeros(*Le.shape, device=dev) if want_dle else None
    pos = g.code_index(Le.size(0)) if (want_dle and g.E > 0) else None
    if want_dle and g.E > 0 and pos is None:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"transformer_attn_bwd: {Le.size(0)} bond codes exceed the inverted index")
    check(_lib.load().gnx_transformer_attn_bwd(handle(dev), dout.data_ptr(), qkvs.data_ptr(), Le.data_ptr(),
                                               alpha.data_ptr(), g.rowptr.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(),
                                               g.code.data_ptr(), g.colptr.data_ptr(), g.cpos.data_ptr(), _ptr(pos), N,
                                               g.E, int(heads), H // int(heads), Le.size(0), float(p),
                                               int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), dqkv.data_ptr(),
                                               scratch.data_ptr(), _ptr(dLe)))
    return dqkv, scratch, dLe


def transformer_attn_dle(dout: torch.Tensor, qkvs: torch.Tensor, scratch: torch.Tensor, Le: torch.Tensor, g: GraphPack,
                         heads: int, pos: Optional[torch.Tensor]) -> torch.Tensor:
    """dLe [R,H] from the scratch of ``transformer_attn_bwd``, on the handle's current stream; ``pos`` =
    ``g.code_index(R)`` fetched by the caller (it may build the index, which must not happen on a side stream)."""
    R, H = Le.shape
    dLe = zeros(R, H, device=dout.device)
    if g.E == 0:
        return dLe
    if pos is None:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"transformer_attn_dle: {R} bond codes exceed the inverted index")
    check(_lib.load().gnx_transformer_attn_dle(handle(dout.device), dout.data_ptr(), qkvs.data_ptr(), scratch.data_ptr(),
                                               g.dst.data_ptr(), g.code.data_ptr(), pos.data_ptr(), g.E, int(heads),
                                               H // int(heads), R, dLe.data_ptr()))
    return dLe


def _f64_on(t: torch.Tensor, name: str, dev: torch.device) -> torch.Tensor:
    if t.dtype != torch.float64 or t.device != dev:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: expected float64 on {dev}, got {t.dtype} on {t.device}")
    return t.contiguous()


def _pcsaft_args(params: torch.Tensor, owner: torch.Tensor, T: torch.Tensor, name: str):
    dev = params.device
    params = _f64_on(params, f"{name}: params", dev)
    if params.dim() != 2 or params.size(1) != 9:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: params must be [B, 9], got {tuple(params.shape)}")
    if owner.dtype != torch.int64 or owner.device != dev or owner.dim() != 1:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: owner must be a 1-D int64 tensor on {dev}")
    T = _f64_on(T, f"{name}: T", dev)
    if T.shape != owner.shape:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: T {tuple(T.shape)} and owner {tuple(owner.shape)} differ")
    return params, owner.contiguous(), T


_F64, _ST = torch.float64, torch.int32


def _pcsaft_outs(out, specs, dev: torch.device, name: str):
    """The output tensors of one PC-SAFT entry in its argument order: new ones of ``specs`` ((shape, dtype), or None for
    one that is not asked for), or the caller's ``out`` checked against them.  A None in ``out`` reaches the entry as
    NULL.  A caller that wants every output in one buffer passes views of it."""
    if out is None:
        return tuple(None if s is None else torch.empty(s[0], dtype=s[1], device=dev) for s in specs)
    if len(out) != len(specs):
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: out must hold {len(specs)} tensors, got {len(out)}")
    for t, s in zip(out, specs):
        if t is not None and (s is None or tuple(t.shape) != s[0] or t.dtype != s[1] or t.device != dev
                              or not t.is_contiguous()):
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: out does not match the outputs of this call")
    return tuple(out)


def _pcsaft_density(params, owner, T, P, out=None):
    """``pcsaft_density`` writing into ``out`` = (rho, status) where given: the one call site of the entry."""
    params, owner, T = _pcsaft_args(params, owner, T, "pcsaft_density")
    P = _f64_on(P, "pcsaft_density: P", params.device)
    if P.shape != T.shape:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"pcsaft_density: P {tuple(P.shape)} and T {tuple(T.shape)} differ")
    n, dev = T.numel(), params.device
    rho, status = _pcsaft_outs(out, [((n,), _F64), ((n,), _ST)], dev, "pcsaft_density")
    check(_lib.load().gnx_pcsaft_density(handle(dev), params.data_ptr(), params.size(0), owner.data_ptr(),
                                         T.data_ptr(), P.data_ptr(), n, rho.data_ptr(), status.data_ptr()))
    return rho, status


def pcsaft_density(params: torch.Tensor, owner: torch.Tensor, T: torch.Tensor, P: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """PC-SAFT liquid density (gnx_pcsaft_density): params [B, 9] fp64 rows, owner [n] int64, T [n] K, P [n] Pa ->
    (rho [n] fp64 mol/m^3, status [n] int32); rho is 0.0 where status != 0.  One launch, no host synchronisation."""
    return _pcsaft_density(params, owner, T, P)


def _pcsaft_vapor_pressure(params, owner, T, out=None):
    """``pcsaft_vapor_pressure`` writing into ``out`` = (psat, rho_l, rho_v, status) where given; rho_l and rho_v may
    be None there: the one call site of the entry."""
    params, owner, T = _pcsaft_args(params, owner, T, "pcsaft_vapor_pressure")
    n, dev = T.numel(), params.device
    out = _pcsaft_outs(out, [((n,), _F64)] * 3 + [((n,), _ST)], dev, "pcsaft_vapor_pressure")
    check(_lib.load().gnx_pcsaft_vapor_pressure(handle(dev), params.data_ptr(), params.size(0), owner.data_ptr(),
                                                T.data_ptr(), n, *map(_ptr, out)))
    return out


def pcsaft_vapor_pressure(params: torch.Tensor, owner: torch.Tensor, T: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """PC-SAFT vapour pressure (gnx_pcsaft_vapor_pressure): params [B, 9] fp64, owner [n] int64, T [n] K ->
    (psat [n] Pa, rho_l [n], rho_v [n] mol/m^3, status [n] int32); all 0.0 where status != 0 (2 = supercritical)."""
    return _pcsaft_vapor_pressure(params, owner, T)


def _pcsaft_saturation(params, owner, T, out=None):
    """``pcsaft_saturation`` writing into ``out`` = (psat, rho_l, rho_v, h_l, h_v, s_l, s_v, status) where given; each of
    the seven fp64 tensors may be None there: the one call site of the entry."""
    params, owner, T = _pcsaft_args(params, owner, T, "pcsaft_saturation")
    n, dev = T.numel(), params.device
    out = _pcsaft_outs(out, [((n,), _F64)] * 7 + [((n,), _ST)], dev, "pcsaft_saturation")
    if out[7] is None:
        raise _lib.GnxError(_lib.GNX_E_INVALID, "pcsaft_saturation: out must hold a status tensor")
    check(_lib.load().gnx_pcsaft_saturation(handle(dev), params.data_ptr(), params.size(0), owner.data_ptr(),
                                            T.data_ptr(), n, *map(_ptr, out)))
    return out


def pcsaft_saturation(params: torch.Tensor, owner: torch.Tensor, T: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    """PC-SAFT saturation line (gnx_pcsaft_saturation): params [B, 9] fp64, owner [n] int64, T [n] K -> (psat [n] Pa,
    rho_l [n], rho_v [n] mol/m^3, h_l [n], h_v [n] J/mol, s_l [n], s_v [n] J/mol/K, status [n] int32): the state of
    ``pcsaft_vapor_pressure`` with the residual molar enthalpy and the residual molar entropy (at the same T and V) of
    both phases; all 0.0 where status != 0 (2 = supercritical).  One launch, no host synchronisation."""
    return _pcsaft_saturation(params, owner, T)


def _pcsaft_critical_point(params, out=None):
    """``pcsaft_critical_point`` writing into ``out`` = (Tc, Pc, rho_c, h_c, s_c, status) where given; h_c and s_c, the
    residual molar enthalpy (J/mol) and entropy (J/mol/K) at the critical point, may be None there and are not computed
    without ``out``: the one call site of the entry."""
    dev = params.device
    params = _f64_on(params, "pcsaft_critical_point: params", dev)
    if params.dim() != 2 or params.size(1) != 9:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"pcsaft_critical_point: params must be [B, 9], got {tuple(params.shape)}")
    B = params.size(0)
    if out is None:
        out = [torch.empty((B,), dtype=_F64, device=dev) for _ in range(3)] + [None, None,
                                                                               torch.empty((B,), dtype=_ST, device=dev)]
    out = _pcsaft_outs(out, [((B,), _F64)] * 5 + [((B,), _ST)], dev, "pcsaft_critical_point")
    if any(out[k] is None for k in (0, 1, 2, 5)):
        raise _lib.GnxError(_lib.GNX_E_INVALID, "pcsaft_critical_point: out must hold Tc, Pc, rho_c and status")
    check(_lib.load().gnx_pcsaft_critical_point(handle(dev), params.data_ptr(), B, *map(_ptr, out)))
    return out


def pcsaft_critical_point(params: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """PC-SAFT vapour-liquid critical points (gnx_pcsaft_critical_point): params [B, 9] fp64 -> (Tc [B] K, Pc [B] Pa,
    rho_c [B] mol/m^3, status [B] int32), one lane per row; all 0.0 where status != 0 (1 = no loop found or the polish
    did not converge, 3 = invalid row).  One launch, no host synchronisation."""
    Tc, Pc, rho_c, _, _, status = _pcsaft_critical_point(params)
    return Tc, Pc, rho_c, status


# the mixture forms: entry point and fp64 outputs in argument order (0: [n], 1: [n, nc]); the status follows them
_PCSAFT_MIX = {"pcsaft_mix_state": ("gnx_pcsaft_mix_state", (0, 0, 0)),
               "pcsaft_mix_density": ("gnx_pcsaft_mix_density", (0,)),
               "pcsaft_mix_lnphi_state": ("gnx_pcsaft_mix_lnphi_state", (1, 0)),
               "pcsaft_mix_lnphi": ("gnx_pcsaft_mix_lnphi", (0, 1, 1)),
               "pcsaft_mix_bubble": ("gnx_pcsaft_mix_bubble", (0, 1, 0, 0)),
               "pcsaft_mix_dew": ("gnx_pcsaft_mix_dew", (0, 1, 0, 0)),
               "pcsaft_mix_bubble_t": ("gnx_pcsaft_mix_bubble_t", (0, 1, 0, 0)),
               "pcsaft_mix_dew_t": ("gnx_pcsaft_mix_dew_t", (0, 1, 0, 0)),
               "pcsaft_mix_flash": ("gnx_pcsaft_mix_flash", (0, 1, 1, 0, 0)),
               "pcsaft_mix_stability": ("gnx_pcsaft_mix_stability", (0, 1, 0, 0)),
               "pcsaft_mix_lle": ("gnx_pcsaft_mix_lle", (0, 1, 1, 0, 0))}


_NO_START = object()  # an entry without a start column (None there is the NULL of one that has it)


def _pcsaft_mix(params, comp, kij, eab, owner, T, second, x, name, out=None, last=True, trial=None, start=_NO_START,
                w0=None):
    """The mixture form ``name`` of ``_PCSAFT_MIX``: validate, take ``out`` or make the outputs, call.  ``second`` is the
    state beside T (rho or P), None for the bubble point, which has none.  ``last`` False leaves the last fp64 output
    (lnphi_pure) out: None in the result, NULL for the entry.  ``trial``: the int64 column that the stability entry
    takes beside ``owner``, and it alone.  ``start``: the fp64 column of start values that the bubble- and dew-temperature
    entries take after ``x`` (there ``T`` holds the pressures), None for NULL.  ``w0``: the [n, nc] fp64 start
    compositions that the liquid-liquid entry takes after ``x``, and it alone."""
    entry, widths = _PCSAFT_MIX[name]
    params, owner, T = _pcsaft_args(params, owner, T, name)
    dev = params.device
    if comp.dtype != torch.int64 or comp.device != dev or comp.dim() != 2 or not 1 <= comp.size(1) <= 4:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: comp must be an int64 [M, nc] tensor on {dev} with 1 <= nc <= 4")
    comp = comp.contiguous()
    M, nc = comp.shape
    mats = []
    for label, t in (("kij", kij), ("eab", eab)):
        if t is not None:
            t = _f64_on(t, f"{name}: {label}", dev)
            if tuple(t.shape) != (M, nc, nc):
                raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: {label} must be [{M}, {nc}, {nc}], got {tuple(t.shape)}")
        mats.append(t)
    rows = []
    if trial is not None:
        if trial.dtype != torch.int64 or trial.device != dev or trial.shape != owner.shape:
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: trial must be an int64 tensor on {dev} of the shape of "
                                                    f"owner, {tuple(owner.shape)}")
        rows.append(trial.contiguous())
    state = [] if second is None else [_f64_on(second, f"{name}: state", dev)]
    x = _f64_on(x, f"{name}: x", dev)
    n = T.numel()
    if any(t.shape != T.shape for t in state) or tuple(x.shape) != (n, nc):
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: T {tuple(T.shape)}, state {[tuple(t.shape) for t in state]} "
                                                f"and x {tuple(x.shape)} do not describe n points of {nc} components")
    after = []
    if start is not _NO_START:
        if start is not None:
            start = _f64_on(start, f"{name}: start", dev)
            if start.shape != T.shape:
                raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: start {tuple(start.shape)} and the state "
                                                        f"{tuple(T.shape)} differ")
        after.append(_ptr(start))
    if w0 is not None:
        w0 = _f64_on(w0, f"{name}: w0", dev)
        if w0.shape != x.shape:
            raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: w0 {tuple(w0.shape)} and the feed {tuple(x.shape)} differ")
        after.append(w0.data_ptr())
    specs = [((n, nc) if w else (n,), _F64) for w in widths] + [((n,), _ST)]
    if not last:
        specs[-2] = None
    out = _pcsaft_outs(out, specs, dev, name)
    check(getattr(_lib.load(), entry)(handle(dev), params.data_ptr(), params.size(0), comp.data_ptr(), _ptr(mats[0]),
                                      _ptr(mats[1]), M, nc, owner.data_ptr(), *(t.data_ptr() for t in rows),
                                      T.data_ptr(), *(t.data_ptr() for t in state), x.data_ptr(), *after, n,
                                      *map(_ptr, out)))
    return out


def pcsaft_mix_state(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor], eab: Optional[torch.Tensor],
                     owner: torch.Tensor, T: torch.Tensor, rho: torch.Tensor, x: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT state (gnx_pcsaft_mix_state): params [B, 9] fp64 pool of component rows, comp [M, nc] int64 rows
    of each mixture (-1 = unused slot), kij / eab [M, nc, nc] fp64 or None, owner [n] int64 mixture of each point, T [n] K,
    rho [n] mol/m^3, x [n, nc] -> (a_res [n], p [n] Pa, dpdrho [n] Pa m^3/mol, status [n] int32); all 0.0 where
    status != 0.  One launch, no host synchronisation."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, rho, x, "pcsaft_mix_state")


def pcsaft_mix_density(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                       eab: Optional[torch.Tensor], owner: torch.Tensor, T: torch.Tensor, P: torch.Tensor,
                       x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT liquid density (gnx_pcsaft_mix_density): arguments as ``pcsaft_mix_state`` with P [n] Pa in
    place of rho -> (rho [n] mol/m^3, status [n] int32); rho is 0.0 where status != 0."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, P, x, "pcsaft_mix_density")


def pcsaft_mix_lnphi_state(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                           eab: Optional[torch.Tensor], owner: torch.Tensor, T: torch.Tensor, rho: torch.Tensor,
                           x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT fugacity coefficients at (T, rho, x) (gnx_pcsaft_mix_lnphi_state): arguments as
    ``pcsaft_mix_state`` -> (lnphi [n, nc], Z [n], status [n] int32); NaN in a -1 slot and in the whole row where
    status != 0.  A used slot with x = 0 stays in the mixture (infinite dilution)."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, rho, x, "pcsaft_mix_lnphi_state")


def pcsaft_mix_lnphi(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor], eab: Optional[torch.Tensor],
                     owner: torch.Tensor, T: torch.Tensor, P: torch.Tensor, x: torch.Tensor, pure: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """Mixture PC-SAFT fugacity coefficients at the liquid root of (T, P, x) (gnx_pcsaft_mix_lnphi): arguments as
    ``pcsaft_mix_density`` -> (rho [n] mol/m^3, the bits of ``pcsaft_mix_density``; lnphi [n, nc]; lnphi_pure [n, nc] if
    ``pure`` else None: each component alone at its own liquid root, NaN where it has none; status [n] int32)."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, P, x, "pcsaft_mix_lnphi", last=pure)


def _pcsaft_mix_bubble(params, comp, kij, eab, owner, T, x, out=None):
    """``pcsaft_mix_bubble`` writing into ``out`` = (P, y, rho_l, rho_v, status) where given; rho_l and rho_v may be None
    there."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, None, x, "pcsaft_mix_bubble", out=out)


def pcsaft_mix_bubble(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                      eab: Optional[torch.Tensor], owner: torch.Tensor, T: torch.Tensor, x: torch.Tensor
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT bubble point at (T, x) (gnx_pcsaft_mix_bubble): arguments as ``pcsaft_mix_state`` without rho
    -> (P [n] Pa, y [n, nc], rho_l [n], rho_v [n] mol/m^3, status [n] int32).  A used slot with x = 0 is dropped (y = 0.0),
    a -1 slot has y = NaN; where status != 0, P and the densities are 0.0 and the y row is NaN."""
    return _pcsaft_mix_bubble(params, comp, kij, eab, owner, T, x)


def _pcsaft_mix_dew(params, comp, kij, eab, owner, T, y, out=None):
    """``pcsaft_mix_dew`` writing into ``out`` = (P, x, rho_l, rho_v, status) where given; rho_l and rho_v may be None
    there."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, None, y, "pcsaft_mix_dew", out=out)


def pcsaft_mix_dew(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                   eab: Optional[torch.Tensor], owner: torch.Tensor, T: torch.Tensor, y: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT dew point at (T, y) (gnx_pcsaft_mix_dew): arguments as ``pcsaft_mix_bubble`` with the vapour y
    [n, nc] in place of x -> (P [n] Pa, x [n, nc], rho_l [n], rho_v [n] mol/m^3, status [n] int32).  A used slot with
    y = 0 is dropped (x = 0.0), a -1 slot has x = NaN; where status != 0, P and the densities are 0.0 and the x row is
    NaN."""
    return _pcsaft_mix_dew(params, comp, kij, eab, owner, T, y)


def _pcsaft_mix_bubble_t(params, comp, kij, eab, owner, P, x, T0=None, out=None):
    """``pcsaft_mix_bubble_t`` writing into ``out`` = (T, y, rho_l, rho_v, status) where given; rho_l and rho_v may be
    None there."""
    return _pcsaft_mix(params, comp, kij, eab, owner, P, None, x, "pcsaft_mix_bubble_t", out=out, start=T0)


def pcsaft_mix_bubble_t(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                        eab: Optional[torch.Tensor], owner: torch.Tensor, P: torch.Tensor, x: torch.Tensor,
                        T0: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT bubble temperature at (P, x) (gnx_pcsaft_mix_bubble_t): arguments as ``pcsaft_mix_bubble`` with
    P [n] Pa in place of T, and T0 [n] K or None, the temperature each solve starts from (NaN: the kernel's own start)
    -> (T [n] K, y [n, nc], rho_l [n], rho_v [n] mol/m^3, status [n] int32).  A used slot with x = 0 is dropped
    (y = 0.0), a -1 slot has y = NaN; where status != 0, T and the densities are 0.0 and the y row is NaN."""
    return _pcsaft_mix_bubble_t(params, comp, kij, eab, owner, P, x, T0)


def _pcsaft_mix_dew_t(params, comp, kij, eab, owner, P, y, T0=None, out=None):
    """``pcsaft_mix_dew_t`` writing into ``out`` = (T, x, rho_l, rho_v, status) where given; rho_l and rho_v may be None
    there."""
    return _pcsaft_mix(params, comp, kij, eab, owner, P, None, y, "pcsaft_mix_dew_t", out=out, start=T0)


def pcsaft_mix_dew_t(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                     eab: Optional[torch.Tensor], owner: torch.Tensor, P: torch.Tensor, y: torch.Tensor,
                     T0: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT dew temperature at (P, y) (gnx_pcsaft_mix_dew_t): arguments as ``pcsaft_mix_bubble_t`` with the
    vapour y [n, nc] in place of x -> (T [n] K, x [n, nc], rho_l [n], rho_v [n] mol/m^3, status [n] int32).  A used slot
    with y = 0 is dropped (x = 0.0), a -1 slot has x = NaN; where status != 0, T and the densities are 0.0 and the x row
    is NaN."""
    return _pcsaft_mix_dew_t(params, comp, kij, eab, owner, P, y, T0)


def _pcsaft_mix_flash(params, comp, kij, eab, owner, T, P, z, out=None):
    """``pcsaft_mix_flash`` writing into ``out`` = (beta, x, y, rho_l, rho_v, status) where given; rho_l and rho_v may be
    None there."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, P, z, "pcsaft_mix_flash", out=out)


def pcsaft_mix_flash(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                     eab: Optional[torch.Tensor], owner: torch.Tensor, T: torch.Tensor, P: torch.Tensor, z: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT two-phase flash at (T, P, z) (gnx_pcsaft_mix_flash): arguments as ``pcsaft_mix_density`` with the
    feed z [n, nc] in place of x -> (beta [n] vapour mole fraction, x [n, nc], y [n, nc], rho_l [n], rho_v [n] mol/m^3,
    status [n] int32; 4 = no vapour-liquid split).  A used slot with z = 0 is dropped (x = y = 0.0), a -1 slot has NaN;
    where status != 0, beta and the densities are 0.0 and the x and y rows are NaN."""
    return _pcsaft_mix_flash(params, comp, kij, eab, owner, T, P, z)


def _pcsaft_mix_stability(params, comp, kij, eab, owner, trial, T, P, z, out=None):
    """``pcsaft_mix_stability`` writing into ``out`` = (tpd, w, rho_w, rho_z, status) where given; rho_w and rho_z may be
    None there."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, P, z, "pcsaft_mix_stability", out=out, trial=trial)


def pcsaft_mix_stability(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                         eab: Optional[torch.Tensor], owner: torch.Tensor, trial: torch.Tensor, T: torch.Tensor,
                         P: torch.Tensor, z: torch.Tensor
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT tangent-plane stability test, one trial per row (gnx_pcsaft_mix_stability): arguments as
    ``pcsaft_mix_flash`` with trial [n] int64 beside owner, 0 = vapour-like, 1 = liquid-like, 2 + s = rich in slot s ->
    (tpd [n], w [n, nc], rho_w [n], rho_z [n] mol/m^3, status [n] int32).  tpd is 0.0 exactly where the trial fell onto
    the feed (w = z), negative where it proves the feed unstable, else the distance at the stationary point it reached.
    A used slot with z = 0 is dropped (w = 0.0), a -1 slot has NaN; where status != 0 (3 also for a trial outside
    [0, nc + 2)), tpd is NaN, the densities are 0.0 and the w row is NaN."""
    return _pcsaft_mix_stability(params, comp, kij, eab, owner, trial, T, P, z)


def _pcsaft_mix_lle(params, comp, kij, eab, owner, T, P, z, w0, out=None):
    """``pcsaft_mix_lle`` writing into ``out`` = (beta, x, y, rho_x, rho_y, status) where given; rho_x and rho_y may be
    None there."""
    return _pcsaft_mix(params, comp, kij, eab, owner, T, P, z, "pcsaft_mix_lle", out=out, w0=w0)


def pcsaft_mix_lle(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor],
                   eab: Optional[torch.Tensor], owner: torch.Tensor, T: torch.Tensor, P: torch.Tensor, z: torch.Tensor,
                   w0: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Mixture PC-SAFT liquid-liquid flash at (T, P, z) started from w0 (gnx_pcsaft_mix_lle): arguments as
    ``pcsaft_mix_flash`` with w0 [n, nc], the composition the second phase starts from (in practice the w of the
    stability test) -> (beta [n], x [n, nc], y [n, nc], rho_x [n], rho_y [n] mol/m^3, status [n] int32; 4 = no split).  x is
    the phase of higher molar density, beta the mole fraction of the other one.  A used slot with z = 0 is dropped (x = y =
    0.0), a -1 slot has NaN; where status != 0 (3 also for a w0 that is not a positive number in a slot where z > 0), beta
    and the densities are 0.0 and the x and y rows are NaN."""
    return _pcsaft_mix_lle(params, comp, kij, eab, owner, T, P, z, w0)


def _pcsaft_kij_x1(params, comp, kij, eab, owner, T, P, x1_exp, feeds, out=None):
    """``pcsaft_kij_x1`` writing into ``out`` = (x1, feed, residual, status) where given: the one call site of the
    entry."""
    name = "pcsaft_kij_x1"
    params, owner, T = _pcsaft_args(params, owner, T, name)
    dev = params.device
    if comp.dtype != torch.int64 or comp.device != dev or comp.dim() != 2 or comp.size(1) != 2:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: comp must be an int64 [M, 2] tensor on {dev} (binaries only)")
    comp = comp.contiguous()
    M = comp.size(0)
    mats = []
    for label, t in (("kij", kij), ("eab", eab)):
        if t is not None:
            t = _f64_on(t, f"{name}: {label}", dev)
            if tuple(t.shape) != (M, 2, 2):
                raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: {label} must be [{M}, 2, 2], got {tuple(t.shape)}")
        mats.append(t)
    P, x1_exp, feeds = (_f64_on(t, f"{name}: {label}", dev) for label, t in (("P", P), ("x1_exp", x1_exp), ("feeds", feeds)))
    if P.shape != T.shape or x1_exp.shape != T.shape or feeds.dim() != 1 or feeds.numel() < 1:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: T {tuple(T.shape)}, P {tuple(P.shape)} and x1_exp "
                                                f"{tuple(x1_exp.shape)} must be [n] and feeds {tuple(feeds.shape)} [F], F >= 1")
    n = T.numel()
    out = _pcsaft_outs(out, [((n,), _F64), ((n,), _ST), ((n,), _F64), ((n,), _ST)], dev, name)
    check(_lib.load().gnx_pcsaft_kij_x1(handle(dev), params.data_ptr(), params.size(0), comp.data_ptr(), _ptr(mats[0]),
                                        _ptr(mats[1]), M, 2, owner.data_ptr(), T.data_ptr(), P.data_ptr(),
                                        x1_exp.data_ptr(), feeds.data_ptr(), feeds.numel(), n, *map(_ptr, out)))
    return out


def pcsaft_kij_x1(params: torch.Tensor, comp: torch.Tensor, kij: Optional[torch.Tensor], eab: Optional[torch.Tensor],
                  owner: torch.Tensor, T: torch.Tensor, P: torch.Tensor, x1_exp: torch.Tensor, feeds: torch.Tensor
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Liquid x_1 of a binary at every row over a list of trial feeds, and its residual (gnx_pcsaft_kij_x1): params,
    comp [M, 2], kij, eab, owner as ``pcsaft_mix_flash``, T [n] K, P [n] Pa, x1_exp [n] the measured x_1, feeds [F] the
    trial z_1 -> (x1 [n] of the first feed that splits, feed [n] int32 its index, residual [n] = log((x1 + 1e-6) /
    (x1_exp + 1e-6)), status [n] int32); NaN, -1, 10.0 and a status != 0 where no feed splits.  One wave per row, one
    launch, no host synchronisation."""
    return _pcsaft_kij_x1(params, comp, kij, eab, owner, T, P, x1_exp, feeds)


def _pcsaft_kij_sums(residual, x1, x1_exp, status, seg, h, out=None):
    """``pcsaft_kij_sums`` writing into ``out`` = (sums,) where given: the one call site of the entry."""
    name = "pcsaft_kij_sums"
    dev = residual.device
    residual, x1, x1_exp = (_f64_on(t, f"{name}: {label}", dev)
                            for label, t in (("residual", residual), ("x1", x1), ("x1_exp", x1_exp)))
    n = residual.numel()
    if residual.dim() != 1 or x1.shape != residual.shape or x1_exp.shape != residual.shape or \
            status.dtype != _ST or status.device != dev or status.shape != residual.shape:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: residual, x1, x1_exp (float64) and status (int32) must be [n] "
                                                f"tensors on {dev}")
    if seg.dtype != torch.int64 or seg.device != dev or seg.dim() != 1 or seg.numel() < 1:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"{name}: seg must be an int64 [S + 1] tensor on {dev}")
    S = seg.numel() - 1
    (sums,) = _pcsaft_outs(out, [((S, 8), _F64)], dev, name)
    check(_lib.load().gnx_pcsaft_kij_sums(handle(dev), residual.data_ptr(), x1.data_ptr(), x1_exp.data_ptr(),
                                          status.contiguous().data_ptr(), seg.contiguous().data_ptr(), S, n, float(h),
                                          sums.data_ptr()))
    return sums


def pcsaft_kij_sums(residual: torch.Tensor, x1: torch.Tensor, x1_exp: torch.Tensor, status: torch.Tensor,
                    seg: torch.Tensor, h: float) -> torch.Tensor:
    """The sums of one Levenberg-Marquardt step in k_12 (gnx_pcsaft_kij_sums) over the [n] rows of a ``pcsaft_kij_x1``
    launch laid out [system][candidate][point], candidate 0 at k and candidate 1 at k + ``h``; seg [S + 1] int64 the
    point ranges of the systems (system s owns the rows 2 seg[s] .. 2 seg[s + 1]) -> sums [S, 8] fp64: sum r0^2, penalised
    rows of candidate 0, sum |r0| and sum |x1_0 - x1_exp| / x1_exp over its other rows, sum r1^2, sum J r0, sum J^2, rows
    with J = (r1 - r0) / h defined (neither row penalised; J = 0 elsewhere).  One wave per system, one launch."""
    return _pcsaft_kij_sums(residual, x1, x1_exp, status, seg, h)


_POOL = {"add": _lib.POOL_ADD, "sum": _lib.POOL_ADD, "mean": _lib.POOL_MEAN, "max": _lib.POOL_MAX}


def segment_pool_fwd(x: torch.Tensor, ptr: torch.Tensor, B: int, mode: str) -> torch.Tensor:
    out = torch.empty(B, x.size(1), dtype=torch.float32, device=x.device)
    check(_lib.load().gnx_segment_pool_fwd(handle(x.device), x.data_ptr(), ptr.data_ptr(), B, x.size(1), _POOL[mode],
                                           out.data_ptr()))
    return out


def segment_pool_bwd(dout: torch.Tensor, x: torch.Tensor, out: torch.Tensor, ptr: torch.Tensor, B: int,
                     mode: str) -> torch.Tensor:
    dx = torch.empty_like(x)
    check(_lib.load().gnx_segment_pool_bwd(handle(x.device), dout.data_ptr(), x.data_ptr(), out.data_ptr(),
                                           ptr.data_ptr(), B, x.size(1), _POOL[mode], dx.data_ptr()))
    return dx


# ------------------------------------------------------------------------------------------------------------------
# normalisation / loss
# ------------------------------------------------------------------------------------------------------------------
def _bn_ws(M: int, H: int, dev) -> Tuple[torch.Tensor, int]:
    nbytes = _lib.load().gnx_batchnorm_workspace_bytes(M, H)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def batchnorm_fwd(x, gamma, beta, running_mean, running_var, momentum: float, eps: float, training: bool, relu: bool,
                  num_batches_tracked: Optional[torch.Tensor] = None):
    """``num_batches_tracked`` (int64[1] device tensor) is incremented by the kernel in training mode."""
    M, H = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(H, dtype=torch.float32, device=x.device)
    rstd = torch.empty(H, dtype=torch.float32, device=x.device)
    ws, nbytes = _bn_ws(M, H, x.device)
    check(_lib.load().gnx_batchnorm_fwd(handle(x.device), x.data_ptr(), M, H, _ptr(gamma), _ptr(beta),
                                        _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked),
                                        float(momentum), float(eps),
                                        int(training), int(relu), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        ws.data_ptr(), nbytes))
    return y, mean, rstd


_NO_BETA = object()  # batchnorm_bwd(beta=...) not given (None is a value: a BatchNorm without affine parameters)


def batchnorm_bwd(dy, x, y, gamma, mean, rstd, relu: bool, dgamma=None, dbeta=None, *, beta=_NO_BETA):
    """dgamma / dbeta: optional existing buffers to accumulate (+=) into; fresh zero buffers otherwise.

    With ``beta=`` (the forward's beta, or None where the forward had none) the ReLU mask is recomputed from ``x``
    (gnx_batchnorm_bwd_x) and ``y`` is ignored (may be None): the same bits, two passes over [M, H] less."""
    M, H = x.shape
    dx = torch.empty_like(x)
    if dgamma is None:
        dgamma = zeros(H, device=x.device)
    if dbeta is None:
        dbeta = zeros(H, device=x.device)
    ws, nbytes = _bn_ws(M, H, x.device)
    if beta is not _NO_BETA:
        check(_lib.load().gnx_batchnorm_bwd_x(handle(x.device), dy.data_ptr(), x.data_ptr(), M, H, _ptr(gamma), _ptr(beta),
                                              mean.data_ptr(), rstd.data_ptr(), int(relu), dx.data_ptr(),
                                              dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), nbytes))
        return dx, dgamma, dbeta
    check(_lib.load().gnx_batchnorm_bwd(handle(x.device), dy.data_ptr(), x.data_ptr(), y.data_ptr(), M, H, _ptr(gamma),
                                        mean.data_ptr(), rstd.data_ptr(), int(relu), dx.data_ptr(), dgamma.data_ptr(),
                                        dbeta.data_ptr(), ws.data_ptr(), nbytes))
    return dx, dgamma, dbeta


def dropout(x: torch.Tensor, p: float, seed: int, offset: int) -> torch.Tensor:
    """x * mask / (1 - p), mask from Philox keyed by (seed, offset); the same call on a gradient is the backward."""
    x = _f32(x, "x").contiguous()
    y = torch.empty_like(x)
    check(_lib.load().gnx_dropout(handle(x.device), x.data_ptr(), x.numel(), float(p), int(seed) & (2 ** 64 - 1),
                                  int(offset) & (2 ** 64 - 1), y.data_ptr()))
    return y


def huber_ape(pred: torch.Tensor, target: torch.Tensor, delta: float, need_grad: bool):
    pred = _f32(pred, "pred").contiguous()
    target = _f32(target, "target").contiguous()
    if pred.shape != target.shape:
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"pred {tuple(pred.shape)} vs target {tuple(target.shape)}")
    out2 = torch.empty(2, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if need_grad else None
    check(_lib.load().gnx_huber_ape(handle(pred.device), pred.data_ptr(), target.data_ptr(), pred.numel(), float(delta),
                                    out2.data_ptr(), _ptr(dpred)))
    return out2, dpred


def clip_rows(x: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    x = _f32(x, "x").contiguous()
    y = torch.empty_like(x)
    check(_lib.load().gnx_clip_rows(handle(x.device), x.data_ptr(), x.size(0), x.size(1), lo.data_ptr(), hi.data_ptr(),
                                    y.data_ptr()))
    return y


def prof_begin(device: torch.device, kernel_ids: Sequence[int]) -> None:
    """Record HIP event pairs (on the stream the kernels run on) around every launch of the given GNX_K_* kernels."""
    mask = 0
    for k in kernel_ids:
        mask |= 1 << k
    check(_lib.load().gnx_prof_begin(handle(device), mask))


def prof_read(device: torch.device, kernel_id: int) -> Tuple[int, float]:
    """(launches, total milliseconds) of one kernel group since prof_begin; synchronises."""
    d = prof_read_work(device, kernel_id)
    return d["launches"], d["ms"]


def prof_read_work(device: torch.device, kernel_id: int) -> dict:
    """launches, total ms, algorithmic bytes, algorithmic FLOPs and executed bf16-MFMA FLOPs of one kernel group."""
    n, ms = C.c_int64(0), C.c_double(0.0)
    by, fl, mf = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    check(_lib.load().gnx_prof_read(handle(device), kernel_id, C.byref(n), C.byref(ms), C.byref(by), C.byref(fl),
                                    C.byref(mf)))
    return {"launches": n.value, "ms": ms.value, "bytes": by.value, "flops": fl.value, "mfma_bf16_flops": mf.value}


def prof_end(device: torch.device) -> None:
    check(_lib.load().gnx_prof_end(handle(device)))
