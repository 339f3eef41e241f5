"""``ops.pack_batch`` (gnx_pack_batch: one native call, 8 launches) against ``ops.pack_graph`` + the getters of GraphPack /
DegreeClasses on the same tensors: every output array equal (``torch.equal``, counts included; a table is compared up to
its own count, the rest of its buffer is unwritten in both) and the same sticky range-flag report on bad input.  The
getters' tables come from the single-purpose entries, a separate implementation; the eight base arrays come from the same
launches in both, so they are held to the numpy references of tests/pack_ref.py on every case, as is gnx_pack_csr called
directly.

The range-flag bit that the PACKER sets for an in-degree above the hint is bit 5 (the class histogram clamps the degree);
bit 6 belongs to the fused edge kernels that consume the edge tiles.  Both paths must report the same bits here.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pack_ref as R

pytestmark = pytest.mark.gpu

AVGS = (1.2345, 0.875)


def _flag(dev) -> str:
    """The sticky range flag's report ('' when clean); reading clears it."""
    from gnnepcsaft_amd import _lib, ops
    try:
        ops.check_range(dev)
    except _lib.GnxError as e:
        return str(e)
    return ""


class Case:
    def __init__(self, name, ei, ea, batch, N, B, hint, R=60, bond_dims=(5, 6, 2), **kw):
        self.name, self.ei, self.ea, self.batch, self.N, self.B = name, ei, ea, batch, N, B
        self.hint, self.R, self.bond_dims, self.kw = hint, R, bond_dims, kw

    def max_in_degree(self):
        d = self.ei[1].clamp(0, max(self.N - 1, 0))
        return int(np.bincount(d.numpy(), minlength=1).max()) if d.numel() else 0


def _random(name, N, E, seed, lo=0, hi=None, hint=None, **kw):
    rng = np.random.Generator(np.random.PCG64(seed))
    hi = N if hi is None else hi
    ei = torch.from_numpy(rng.integers(lo, hi, size=(2, E)).astype(np.int64))
    ea = torch.from_numpy(np.stack([rng.integers(0, d, size=E) for d in (5, 6, 2)], axis=1).astype(np.int64))
    c = Case(name, ei, ea, None, N, 1, 0, **kw)
    c.hint = c.max_in_degree() if hint is None else hint
    return c


def _molecules(name, graphs, with_batch=True, seed=None):
    from gnnepcsaft_amd.data import synthetic_batch
    b = synthetic_batch(graphs, 2, seed=seed)
    return Case(name, b.edge_index, b.edge_attr, b.batch if with_batch else None, b.x.size(0), graphs, 4)


def _cases():
    from gnnepcsaft_amd import _lib
    lib = _lib.load()
    chunk, bound = int(lib.gnx_pack_batch_scan_chunk()), int(lib.gnx_pack_batch_scan_bound())
    z = torch.zeros
    out = [Case("E0_N5", z(2, 0, dtype=torch.int64), z(0, 3, dtype=torch.int64), z(5, dtype=torch.int64), 5, 1, 4),
           Case("N1_self_loops", z(2, 3, dtype=torch.int64), torch.tensor([[1, 2, 0], [0, 0, 1], [4, 5, 1]]), None, 1, 1, 4),
           _molecules("one_molecule", 1, with_batch=False), _molecules("32_molecules", 32)]
    iso = _random("isolated_start_middle_end", 300, 700, 1, lo=3, hi=281)
    keep = (iso.ei < 100) | (iso.ei >= 150)
    iso.ei = iso.ei[:, keep.all(0)]
    iso.ea = iso.ea[keep.all(0)]
    iso.hint = iso.max_in_degree()
    out.append(iso)
    multi = _random("multi_edges_self_loops", 12, 400, 2)  # 400 edges over 144 pairs: repeats and loops
    out.append(multi)
    for N in (chunk - 1, chunk, chunk + 1):
        out.append(_random(f"scan_tile_N{N}", N, 3 * N + 5, N))
    out.append(_random("past_scan_bound", bound + 1, 5000, 3))
    out.append(_random("multi_launch_scan_forced", 3000, 7001, 4, tiled_scan=True))
    at = _random("degree_at_hint", 40, 90, 5)
    out.append(at)
    above = _random("degree_above_hint", 40, 90, 5)
    above.hint -= 1
    out.append(above)
    hub = _random("hub_17", 64, 100, 6, lo=1)
    hub.ei = torch.cat([hub.ei, torch.stack([torch.arange(1, 18), torch.zeros(17, dtype=torch.int64)])], 1)
    hub.ea = torch.cat([hub.ea, hub.ea[:17]])
    hub.hint = 17
    assert hub.max_in_degree() == 17
    out.append(hub)
    r65 = _random("R65", 30, 80, 7, R=65, bond_dims=(5, 13))
    r65.ea = torch.from_numpy(np.random.Generator(np.random.PCG64(8)).integers(0, 5, size=(80, 2)).astype(np.int64))
    out.append(r65)
    out.append(_random("gine_flags", 50, 120, 9, classes=False))
    bad_n = _random("bad_node_index", 50, 120, 10)
    bad_n.ei[0, 7], bad_n.ei[1, 50] = 50, -1
    bad_n.hint = bad_n.max_in_degree() + 2
    out.append(bad_n)
    bad_f = _random("bad_bond_feature", 50, 120, 11)
    bad_f.ea[3, 1], bad_f.ea[90, 0] = 6, -2
    out.append(bad_f)
    gaps = _random("empty_graphs_start_middle_end", 6, 14, 12)  # graphs 0, 2, 4, 6 and 7 of 8 have no node
    gaps.batch, gaps.B = torch.tensor([1, 1, 3, 3, 3, 5]), 8
    out.append(gaps)
    return out


_CASES = None


def _all_cases():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in _cases()}
    return _CASES


CASE_NAMES = ["E0_N5", "N1_self_loops", "one_molecule", "32_molecules", "isolated_start_middle_end", "multi_edges_self_loops",
              "scan_tile_N1023", "scan_tile_N1024", "scan_tile_N1025", "past_scan_bound", "multi_launch_scan_forced",
              "degree_at_hint", "degree_above_hint", "hub_17", "R65", "gine_flags", "bad_node_index", "bad_bond_feature",
              "empty_graphs_start_middle_end"]


def _new(c, dev, **kw):
    from gnnepcsaft_amd import ops
    _flag(dev)
    t = lambda x: None if x is None else x.to(dev)
    args = dict(max_degree_hint=c.hint, R=c.R, avg_deg_logs=AVGS, validate=False)
    args.update(c.kw)
    args.update(kw)
    g = ops.pack_batch(t(c.ei), t(c.ea), t(c.batch), c.N, c.B if c.batch is not None else None, c.bond_dims, **args)
    return g, _flag(dev)


def _today(c, dev):
    """pack_graph and then the getters, the way the layers call them today."""
    from gnnepcsaft_amd import ops
    _flag(dev)
    t = lambda x: None if x is None else x.to(dev)
    g = ops.pack_graph(t(c.ei), t(c.ea), t(c.batch), c.N, c.B if c.batch is not None else None, c.bond_dims, validate=False)
    g.max_degree_hint = c.hint
    if c.kw.get("classes", True):
        g.degree_classes(c.hint)
        g.edge_tiles(c.hint)
    if c.ei.size(1) > 0 and c.R <= 64:
        g.code_index(c.R)
    for a in AVGS:
        g.degree_scalers(a)
    return g, _flag(dev)


def _assert_same(a, b):
    """GraphPack a (pack_batch) against GraphPack b (today's calls): every array, every cache."""
    assert (a.N, a.E, a.B, a.has_batch, a.max_degree_hint) == (b.N, b.E, b.B, b.has_batch, b.max_degree_hint)
    for name in ("rowptr", "perm", "src", "dst", "colptr", "cpos", "code", "graph_ptr"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == torch.int32 and torch.equal(x, y), name
    assert set(a._scalers) == set(b._scalers)
    for k in b._scalers:
        assert torch.equal(a._scalers[k][0], b._scalers[k][0]) and torch.equal(a._scalers[k][1], b._scalers[k][1]), k
    assert (a._classes is None) == (b._classes is None)
    if b._classes is not None:
        da, db = a._classes, b._classes
        assert da.D == db.D
        if db.D <= 64:
            assert torch.equal(da.dperm[:a.N], db.dperm[:a.N]) and torch.equal(da.cls_ptr, db.cls_ptr)
            assert (da.max_tiles, da.max_chunks, da.max_tiles_p, da.tile_rows_p) == \
                   (db.max_tiles, db.max_chunks, db.max_tiles_p, db.tile_rows_p)
            for tab, cnt in (("tiles", "ntiles"), ("chunks", "nchunks"), ("tiles_p", "ntiles_p")):
                na, nb = getattr(da, cnt), getattr(db, cnt)
                assert torch.equal(na, nb), cnt
                n = 3 * int(nb.item())
                assert getattr(da, tab).numel() == getattr(db, tab).numel()
                assert torch.equal(getattr(da, tab)[:n], getattr(db, tab)[:n]), tab
    assert (a._code_index is None) == (b._code_index is None)
    if b._code_index is not None:
        assert a._code_index[0] == b._code_index[0]
        assert torch.equal(a._code_index[1][:a.E], b._code_index[1][:a.E]) and torch.equal(a._code_index[2], b._code_index[2])
    assert (a._edge_tiles is None) == (b._edge_tiles is None)
    if b._edge_tiles is not None:
        assert a._edge_tiles[1] == b._edge_tiles[1] and torch.equal(a._edge_tiles[0], b._edge_tiles[0])


def _base_reference(c):
    """The eight base arrays of case c by numpy (tests/pack_ref.py)."""
    ref = R.csr_reference(c.ei.numpy(), c.N)
    ref["code"] = R.code_reference(None if c.ea is None else c.ea.numpy(), c.bond_dims, ref["perm"])
    ref["graph_ptr"] = R.graph_ptr_reference(None if c.batch is None else c.batch.numpy(), c.N, c.B)
    return ref


def _assert_base_arrays_are_the_reference(g, c):
    for name, ref in _base_reference(c).items():
        assert np.array_equal(getattr(g, name).cpu().numpy(), ref), name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_output_equals_todays_calls(gpu_device, name):
    c = _all_cases()[name]
    new, flag_new = _new(c, gpu_device)
    old, flag_old = _today(c, gpu_device)
    print(name, "N", c.N, "E", c.ei.size(1), "hint", c.hint, "flag:", flag_new or "clean")
    assert flag_new == flag_old
    _assert_same(new, old)
    _assert_base_arrays_are_the_reference(new, c)
    _assert_base_arrays_are_the_reference(old, c)
    # what the case is about
    if name == "degree_above_hint":
        assert "in-degree" in flag_new
    elif name == "degree_at_hint":
        assert flag_new == "" and c.max_in_degree() == c.hint
    elif name == "hub_17":
        assert new._edge_tiles is None and new.edge_tiles(17) is None and new._classes.dperm is not None
    elif name == "R65":
        assert new._code_index is None and new.code_index(65) is None
    elif name == "gine_flags":
        assert new._classes is None and new._edge_tiles is None and new._code_index is not None
    elif name == "bad_node_index":
        assert "node id" in flag_new
    elif name == "bad_bond_feature":
        assert "vocabulary" in flag_new
    elif name in ("32_molecules", "one_molecule"):
        assert new._edge_tiles is not None and new._code_index is not None and new._classes.D == 5


def test_unbuilt_parts_are_not_touched(gpu_device):
    """parts = 0 (a GINE or Transformer batch): the buffers behind the class, code-index and edge-tile pointers keep their bytes."""
    from gnnepcsaft_amd import _lib
    lib, dev = _lib.load(), gpu_device
    c = _all_cases()["gine_flags"]
    N, E = c.N, c.ei.size(1)
    ei, ea = c.ei.to(dev), c.ea.to(dev)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=dev)
    a = _lib.PackBatchArgs()
    a.edge_index, a.edge_attr, a.N, a.E, a.K, a.max_degree, a.R, a.edge_tile_w = ei.data_ptr(), ea.data_ptr(), N, E, 3, 4, 60, 61
    for k, d in enumerate((5, 6, 2)):
        a.bond_dims[k] = d
    need = {n: i32(E if n in ("perm", "src", "dst", "cpos", "code") else N + 1)
            for n in ("rowptr", "perm", "src", "dst", "colptr", "cpos", "code", "graph_ptr")}
    spare = {n: i32(4 * (N + E)) for n in ("dperm", "cls_ptr", "code_pos", "code_ptr", "edge_tiles", "tiles", "ntiles")}
    for n, t in list(need.items()) + list(spare.items())[:5]:
        setattr(a, n, t.data_ptr())
    for i in range(3):
        a.tile_rows[i], a.tiles[i], a.ntiles[i] = 128, spare["tiles"].data_ptr(), spare["ntiles"].data_ptr()
    nbytes = lib.gnx_pack_batch_workspace_bytes(N, E, 1, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes, a.parts = ws.data_ptr(), nbytes, 0
    _lib.check(lib.gnx_pack_batch(_lib.handle(dev), C.byref(a)))
    assert _flag(dev) == ""
    for n, t in spare.items():
        assert bool((t == -7).all()), n
    old, _ = _today(c, dev)
    for n in ("rowptr", "perm", "src", "dst", "colptr", "cpos", "code"):
        assert torch.equal(need[n], getattr(old, n)), n
    assert need["graph_ptr"][:2].tolist() == [0, N]


def _pack_csr(c, dev, short_by=0):
    """gnx_pack_csr called the way a C caller would, outputs and one spare buffer pre-filled with -7, the workspace
    ``short_by`` bytes below the queried size: (status, outputs, spare)."""
    from gnnepcsaft_amd import _lib
    lib = _lib.load()
    N, E = c.N, c.ei.size(1)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=dev)
    out = {n: i32(N + 1 if n in ("rowptr", "colptr") else E) for n in ("rowptr", "perm", "src", "dst", "colptr", "cpos")}
    spare = i32(4 * (N + E))
    ei = c.ei.to(dev).contiguous()
    p = lambda t: t.data_ptr() if E > 0 else None  # E = 0: the edge arrays may be NULL
    nbytes = lib.gnx_pack_csr_workspace_bytes(N, E)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = lib.gnx_pack_csr(_lib.handle(dev), p(ei), E, N, out["rowptr"].data_ptr(), p(out["perm"]), p(out["src"]),
                          p(out["dst"]), out["colptr"].data_ptr(), p(out["cpos"]), ws.data_ptr(), nbytes - short_by)
    return st, out, spare


@pytest.mark.parametrize("name", ["E0_N5", "N1_self_loops", "scan_tile_N1023", "scan_tile_N1024", "scan_tile_N1025",
                                  "multi_edges_self_loops", "bad_node_index"])
def test_pack_csr_called_directly(gpu_device, name):
    """Nothing in ``ops`` calls gnx_pack_csr: its six arrays against the numpy reference, through ctypes."""
    from gnnepcsaft_amd import _lib
    c = _all_cases()[name]
    _flag(gpu_device)
    st, out, spare = _pack_csr(c, gpu_device)
    _lib.check(st)
    flag = _flag(gpu_device)
    ref = R.csr_reference(c.ei.numpy(), c.N)
    for n, t in out.items():
        assert np.array_equal(t.cpu().numpy(), ref[n]), n
    assert bool((spare == -7).all())
    if name == "bad_node_index":  # one id equal to N, one equal to -1: both endpoints of those edges become 0
        assert "node id" in flag
        pos = {int(e): p for p, e in enumerate(out["perm"].tolist())}
        assert [(int(out["src"][pos[e]]), int(out["dst"][pos[e]])) for e in (7, 50)] == [(0, 0), (0, 0)]
    else:
        assert flag == ""


def test_pack_csr_short_workspace_writes_nothing(gpu_device):
    from gnnepcsaft_amd import _lib
    st, out, spare = _pack_csr(_all_cases()["multi_edges_self_loops"], gpu_device, short_by=1)
    assert st == _lib.GNX_E_WORKSPACE
    torch.cuda.synchronize()
    for n, t in list(out.items()) + [("spare", spare)]:
        assert bool((t == -7).all()), n
    assert _flag(gpu_device) == ""


def test_two_calls_give_identical_bytes(gpu_device):
    c = _all_cases()["multi_edges_self_loops"]
    a, _ = _new(c, gpu_device)
    b, _ = _new(c, gpu_device)
    _assert_same(a, b)
    c = _all_cases()["32_molecules"]
    a, _ = _new(c, gpu_device)
    b, _ = _new(c, gpu_device)
    _assert_same(a, b)


def test_getters_return_the_packed_tensors(gpu_device):
    """After pack_batch the getters launch nothing: they hand out the views that the one call filled."""
    c = _all_cases()["32_molecules"]
    g, _ = _new(c, gpu_device)
    dc, ci, et, sc = g._classes, g._code_index, g._edge_tiles, dict(g._scalers)
    assert g.degree_classes(c.hint) is dc and g.degree_classes(c.hint).dperm.data_ptr() == dc.dperm.data_ptr()
    assert g.code_index(60).data_ptr() == ci[1].data_ptr() and g._code_index is ci
    assert g.edge_tiles(c.hint)[0].data_ptr() == et[0].data_ptr() and g._edge_tiles is et
    for a in AVGS:
        amp, att = g.degree_scalers(a)
        assert amp.data_ptr() == sc[a][0].data_ptr() and att.data_ptr() == sc[a][1].data_ptr()
    # one allocation behind everything
    base = g.rowptr.untyped_storage().data_ptr()
    for t in (g.perm, g.cpos, g.code, g.graph_ptr, dc.dperm, dc.tiles, dc.chunks, ci[1], ci[2], et[0], sc[AVGS[0]][0]):
        assert t.untyped_storage().data_ptr() == base
    # another R / width / avg_deg_log: the single-purpose entry builds its own
    assert g.code_index(64).data_ptr() != ci[1].data_ptr()
    assert g.edge_tiles(3)[1] != et[1]
    assert g.degree_scalers(2.5)[0].data_ptr() != sc[AVGS[0]][0].data_ptr()
    assert _flag(gpu_device) == ""


def test_pack_and_forward_capture_and_replay_with_a_new_batch(gpu_device):
    """pack_batch + a 32-graph PNA forward captured into a HIP graph; the graph replayed with a second batch copied into the
    static buffers gives the eager result of that batch, bit for bit."""
    from gnnepcsaft_amd import ops
    from gnnepcsaft_amd.data import calc_deg, default_config, synthetic_batch
    from gnnepcsaft_amd.train.models import GNNePCSAFT
    dev = gpu_device
    b1, b2 = synthetic_batch(32, 2, seed=11), synthetic_batch(32, 2, seed=12)
    assert b1.edge_index.shape == b2.edge_index.shape and not torch.equal(b1.edge_index, b2.edge_index)
    cfg = default_config(2)
    cfg.update(hidden_dim=64, propagation_depth=2, deg=calc_deg(b1))
    torch.manual_seed(0)
    model = GNNePCSAFT(cfg).to(dev).eval()
    hint = 4
    spec = model.pack_spec()

    def run(x, ei, ea, bt):
        pack = ops.pack_batch(ei, ea, bt, x.size(0), 32, max_degree_hint=hint, validate=False, **spec)
        return model(x, ei, ea, bt, pack=pack)

    prev_stream = torch.cuda.current_stream(dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    try:
        with torch.no_grad():
            static = [t.to(dev).clone() for t in (b1.x, b1.edge_index, b1.edge_attr, b1.batch)]
            eager2 = run(*[t.to(dev) for t in (b2.x, b2.edge_index, b2.edge_attr, b2.batch)]).clone()
            eager1 = run(*static).clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                out = run(*static)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager1)
            for t, src in zip(static, (b2.x, b2.edge_index, b2.edge_attr, b2.batch)):
                t.copy_(src.to(dev))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager2) and not torch.equal(eager1, eager2)
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev_stream)
    assert _flag(dev) == ""
