"""The native composite calls of a PNA layer (gnx_pna_* of include/gnx.h), one function per entry point, and ``PnaDims``, the
one description of a layer's shape that every parameter index and accumulator size is derived from.  Each function takes
tensors, a ``PnaDims`` and the pack / degree-class objects, fills the argument block and calls the library.
``functional.py`` decides which tensors exist and allocates them (``stack_finish`` fetches the cached ones vector)."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import NamedTuple, Sequence

import torch

from . import _lib, ops
from ._lib import PNA_MAX_LAYERS as LAYERS, check, handle


class PnaDims(NamedTuple):
    """T towers of width F, R bond-table rows, D degree classes (0 = ungrouped); ``merged``: the last post layer and ``lin``
    run as ONE product with an H x H weight.  The parameter list of a layer is enc_w, enc_b, lin_w, lin_b, then per tower:
    pre (w, b) x pre_layers, post (w, b) x post_layers."""
    T: int
    F: int
    pre_layers: int
    post_layers: int
    R: int
    D: int
    merged: bool

    H = property(lambda d: d.T * d.F)
    per_tower = property(lambda d: 2 * (d.pre_layers + d.post_layers))
    n_params = property(lambda d: 4 + d.T * d.per_tower)
    small_total = property(lambda d: sum(d.small_sizes()))

    def param_index(self, t: int, kind: str, i: int) -> int:
        """Index of the weight of tower t's ``kind`` ("pre" | "post") layer i in the parameter list; its bias follows it."""
        return 4 + t * self.per_tower + 2 * (i if kind == "pre" else self.pre_layers + i)

    def small_sizes(self) -> tuple:
        """Element counts of a layer's small accumulators dTe [R,H], dEE [R,F], dWm [H,H], dbm [H], dWeff [T,D,F,4F], in
        the order they lie in the model's slab (and in a layer's private scratch)."""
        return (self.R * self.H, self.R * self.F, self.H * self.H, self.H, self.T * self.D * self.F * 4 * self.F)


# What the gradients of one layer's weights are formed from and go to: the argument group of ``conv_bwd``, and for a layer
# that defers its small work the record of ``stack_finish``.  ``small``: ``dims.small_total`` fp32 accumulators.
PnaLayerGrads = namedtuple("PnaLayerGrads", "dims avg_deg_log BE EE params sinks small")


def _addr(t):
    return t.data_ptr() if isinstance(t, torch.Tensor) else t


def ptr_array(items: Sequence, n: int = 0):
    """``c_void_p`` array, at least ``n`` long, of the tensors' data pointers (``None`` -> null; an address stands for
    itself).  A ``void**`` structure field keeps the array alive with the structure, a call argument only for the call."""
    return (C.c_void_p * max(len(items), n))(*map(_addr, items))


def _block_ptrs(t, n: int, size: int = 0):
    """``ptr_array`` of the n equal consecutive blocks of a contiguous tensor, without creating views (None -> None)."""
    step = 0 if t is None else t.numel() // n * t.element_size()
    return None if t is None else ptr_array([t.data_ptr() + i * step for i in range(n)], size)


def _small_ptrs(small: torch.Tensor, dims: PnaDims) -> list:
    """Addresses of (dTe, dEE, dWm, dbm, dWeff) inside a layer's ``small_total`` fp32 accumulators."""
    sizes = dims.small_sizes()
    return [small.data_ptr() + 4 * sum(sizes[:k]) for k in range(len(sizes))]


def _fill_layer(a, dims: PnaDims, pack, dc, etiles, x, A, hs, zs, weffs, Wm, ws) -> None:
    """The fields that PnaFwdArgs and PnaBwdArgs share."""
    a.T, a.F, a.pre_layers, a.post_layers, a.D, a.merged = *dims[:4], dims.D, int(dims.merged)
    a.N, a.E, a.rowptr, a.code, a.dperm = x.size(0), pack.E, pack.rowptr.data_ptr(), pack.code.data_ptr(), dc.dperm.data_ptr()
    a.x, a.A, a.Wm, a.ws, a.ws_bytes = x.data_ptr(), A.data_ptr(), _addr(Wm), ws.data_ptr(), ws.numel()
    for field, tensors in ((a.hs, hs), (a.zs, zs), (a.weff, weffs)):
        for i, t in enumerate(tensors):
            field[i] = t.data_ptr()
    a.etile_info, a.etile_w = (etiles[0].data_ptr(), etiles[1]) if etiles is not None else (None, 0)


def workspace_bytes(dims: PnaDims) -> int:
    """Size of the ``ws`` buffer of ``conv_fwd`` / ``conv_bwd``."""
    return _lib.load().gnx_pna_conv_bwd_workspace_bytes(dims.T, dims.F, dims.D)


def split_all_bytes(device, L: int, dims: PnaDims, n_rows: int, tile_rows: int) -> int:
    """Bytes of the slab that holds the split weight images of L layers (0: these products read no images)."""
    return _lib.load().gnx_pna_split_all_bytes(handle(device), L, *dims[:4], dims.D, n_rows, tile_rows)


def weight_only(BE, dims: PnaDims, avg_deg_log: float, params, EE, Te, weffs, Wm, bm) -> None:
    """gnx_pna_weight_only: EE, Te, Weff(d) per tower and the merged weight / bias of one layer in one call."""
    check(_lib.load().gnx_pna_weight_only(
        handle(BE.device), BE.data_ptr(), dims.R, *dims[:4], dims.D, float(avg_deg_log), ptr_array(params),
        int(dims.merged), EE.data_ptr(), Te.data_ptr(), ptr_array(weffs) if weffs else None, _addr(Wm), _addr(bm)))


def weight_only_all(BE, dims: PnaDims, layers, EE, Te, weff, Wm, bm, slab=None, n_rows: int = 0, tile_rows: int = 0):
    """gnx_pna_weight_only_all over ``layers`` = [(avg_deg_log, params)], outputs stacked over the layers ([L, ...]; None
    where the shape has none), issued on the stream the weight gradients run on (``ops.run_after_wgrads``).  With ``slab``
    (``split_all_bytes``), gnx_pna_split_all follows directly behind; returns its ``PnaLayerImages`` array, else None."""
    L, lib, h = len(layers), _lib.load(), handle(BE.device)
    flat = [p for _, ps in layers for p in ps]
    avg = (C.c_float * L)(*[float(a) for a, _ in layers])
    params, a_weff = ptr_array(flat), _block_ptrs(weff, L * dims.T)
    a_EE, a_Te, a_Wm, a_bm = (_block_ptrs(t, L) for t in (EE, Te, Wm, bm))
    images = (_lib.PnaLayerImages * L)() if slab is not None else None

    def launch():
        check(lib.gnx_pna_weight_only_all(h, L, BE.data_ptr(), dims.R, *dims[:4], dims.D, avg, params, int(dims.merged),
                                          a_EE, a_Te, a_weff, a_Wm, a_bm))
        if slab is not None:
            check(lib.gnx_pna_split_all(h, L, *dims[:4], dims.D, n_rows, tile_rows, params, a_weff, slab.data_ptr(),
                                        slab.numel(), images))

    ops.run_after_wgrads(BE, [BE, EE, Te, weff, Wm, bm, slab] + flat, launch)
    return images


def conv_fwd(dims: PnaDims, pack, dc, etiles, prep, params, *, x, PQ, A, hs, zs, ws, out):
    """gnx_pna_conv_fwd_images: one layer's forward behind the weight-only part ``prep`` (a ``PnaPrep``; without its ``images``
    the layer splits its weights in place).  ``etiles``: the pack's edge-tile table of the fused edge kernel or None (three
    launches).  Returns the pointer array of ``params`` for ``conv_bwd``'s ``parr``: they are saved tensors, built once."""
    a = _lib.PnaFwdArgs()
    _fill_layer(a, dims, pack, dc, etiles, x, A, hs, zs, prep.weffs, prep.Wm, ws)
    a.src, a.dst, a.Te, a.bm = pack.src.data_ptr(), pack.dst.data_ptr(), prep.Te.data_ptr(), _addr(prep.bm)
    a.tiles, a.ntiles, a.max_tiles, a.tile_rows = dc.tiles_p.data_ptr(), dc.ntiles_p.data_ptr(), dc.max_tiles_p, dc.tile_rows_p
    a.params = parr = ptr_array(params)
    (a.P, a.Q), a.out = _block_ptrs(PQ, 2), out.data_ptr()
    check(_lib.load().gnx_pna_conv_fwd_images(handle(x.device), C.byref(a), C.byref(prep.images[0]) if prep.images else None))
    return parr


def conv_bwd(g: PnaLayerGrads, pack, dc, etiles, code_pos, *, x, A, hs, zs, weffs, Wm, dout, gbuf, gebuf, dA, dPQ, ws,
             acc_buf, dx, acc_first: bool, defer: bool, last_of_pass: bool, images=None, parr=None) -> list:
    """gnx_pna_conv_bwd_images: one layer's backward.  ``g.small``: private scratch, or with ``defer`` the layer's zeroed
    part of the model's slab, finished by ``stack_finish``; ``gbuf`` / ``gebuf`` / ``dPQ``: stacked temporaries, one block
    per post layer / pre layer / of dP, dQ; ``images``: the layer's ``PnaLayerImages`` or None.  Returns every tensor the
    block points to: the launches on the side streams use them until the join."""
    a = _lib.PnaBwdArgs()
    _fill_layer(a, g.dims, pack, dc, etiles, x, A, hs, zs, weffs, Wm, ws)
    a.R, a.avg_deg_log, a.n_h, a.n_z = g.dims.R, float(g.avg_deg_log), len(hs), len(zs)
    a.acc_first, a.use_side_streams = int(acc_first), int(ops.wgrad_stream_enabled())
    a.colptr, a.cpos, a.code_pos = pack.colptr.data_ptr(), pack.cpos.data_ptr(), _addr(code_pos)
    a.tiles, a.ntiles, a.max_tiles = dc.tiles.data_ptr(), dc.ntiles.data_ptr(), dc.max_tiles
    a.chunks, a.nchunks, a.max_chunks = dc.chunks.data_ptr(), dc.nchunks.data_ptr(), dc.max_chunks
    a.BE, a.EE, a.dout, a.dA, a.acc_buf, a.dx = (t.data_ptr() for t in (g.BE, g.EE, dout, dA, acc_buf, dx))
    a.params, a.grads = parr if parr is not None else ptr_array(g.params), ptr_array(g.sinks)
    a.gbuf, a.gebuf = _block_ptrs(gbuf, gbuf.size(0), LAYERS), _block_ptrs(gebuf, gebuf.size(0), LAYERS)
    (a.dP, a.dQ), (a.dTe, a.dEE, a.dWm, a.dbm, a.dWeff) = _block_ptrs(dPQ, 2), _small_ptrs(g.small, g.dims)
    # LAST_OF_PASS: the layer's batched weight gradients take every CU, at the end of the layer (6.760 -> 6.687 ms; the post
    # layers' ones launched earlier, before the edge backward, compete with it: 6.612 vs 6.554 ms)
    a.flags = (_lib.PNA_BWD_DEFER_SMALL if defer else 0) | (_lib.PNA_BWD_LAST_OF_PASS if last_of_pass else 0)
    check(_lib.load().gnx_pna_conv_bwd_images(handle(x.device), C.byref(a), None if images is None else C.byref(images)))
    return [dout, x, g.BE, g.EE, A, *hs, *zs, *weffs, Wm, gbuf, gebuf, dA, dPQ, g.small, ws, acc_buf, *g.params, *g.sinks]


def stack_finish(device, records: Sequence[PnaLayerGrads], acc_buf) -> list:
    """gnx_pna_stack_finish over the layers that deferred their small work (side stream 1: bond chain tails; side stream
    0: un-merge and Weff gradients, behind the layers' weight gradients).  Returns every tensor the block points to."""
    dims, L = records[0].dims, len(records)
    if any(r.dims != dims for r in records):
        raise _lib.GnxError(_lib.GNX_E_INVALID, f"stack_finish: layers of different shapes deferred to one finish: "
                                                f"{[tuple(r.dims) for r in records]}")
    ones = ops.ones_vector(device, max(dims.R, 1))
    a = _lib.PnaFinishArgs()
    a.T, a.F, a.pre_layers, a.post_layers, a.D, a.merged = *dims[:4], dims.D, int(dims.merged)
    a.L, a.R, a.use_side_streams = L, dims.R, int(ops.wgrad_stream_enabled())
    a.BE, a.acc_buf, a.ones = records[0].BE.data_ptr(), acc_buf.data_ptr(), ones.data_ptr()
    a.avg_deg_log = (C.c_float * L)(*[r.avg_deg_log for r in records])
    a.params, a.grads = ptr_array([p for r in records for p in r.params]), ptr_array([s for r in records for s in r.sinks])
    small, per_w = [_small_ptrs(r.small, dims) for r in records], 4 * dims.D * dims.F * 4 * dims.F
    a.EE, a.dTe, a.dEE, a.dWm, a.dbm = [ptr_array([r.EE for r in records])] + [ptr_array([s[k] for s in small]) for k in range(4)]
    a.dWeff = ptr_array([s[4] + t * per_w for s in small for t in range(dims.T)])
    check(_lib.load().gnx_pna_stack_finish(handle(device), C.byref(a)))
    return [ones] + [t for r in records for t in (r.BE, r.EE, r.small, *r.params, *r.sinks)]
