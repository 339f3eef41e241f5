"""numpy references of the packer's eight base arrays (tests/test_pack_batch_gpu.py), and plain Python loops that pin
those references themselves (tests/test_pack_ref_cpu.py)."""
import numpy as np


def clamped_endpoints(ei, N):
    """(source, target) of every edge; an edge with an id outside [0, N) counts as the loop 0 -> 0."""
    bad = ((ei < 0) | (ei >= N)).any(0)
    return np.where(bad, 0, ei[0]), np.where(bad, 0, ei[1])


def csr_reference(ei, N):
    """The dst-sorted CSR and its by-source index of edge_index ``ei`` int64[2, E]: a stable sort has one answer."""
    s0, d0 = clamped_endpoints(ei, N)
    perm = np.argsort(d0, kind="stable")
    src = s0[perm]
    ptr = lambda k: np.concatenate([[0], np.cumsum(np.bincount(k, minlength=N))])
    return {"perm": perm, "src": src, "dst": d0[perm], "rowptr": ptr(d0), "colptr": ptr(s0),
            "cpos": np.argsort(src, kind="stable")}


def code_reference(ea, bond_dims, perm):
    """Mixed-radix bond code of every CSR position: features ``ea`` int64[E, K] (None: all codes 0) with a feature outside
    its vocabulary counted as 0, gathered through ``perm``."""
    if ea is None:
        return np.zeros(len(perm), dtype=np.int64)
    dims = np.asarray(bond_dims, dtype=np.int64)
    f = np.where((ea < 0) | (ea >= dims), 0, ea)
    code = np.zeros(len(ea), dtype=np.int64)
    for k, d in enumerate(dims):
        code = code * d + f[:, k]
    return code[perm]


def graph_ptr_reference(batch, N, B):
    """First node of every graph and N at the end, from the non-decreasing ``batch`` int64[N]; [0, N] without one."""
    if batch is None:
        return np.array([0, N])
    return np.searchsorted(batch, np.arange(B + 1), side="left")


# ---- the same by loops ------------------------------------------------------------------------------------------------
def csr_loops(ei, N):
    E = ei.shape[1]
    edges = []
    for e in range(E):
        s, d = int(ei[0, e]), int(ei[1, e])
        if not (0 <= s < N and 0 <= d < N):
            s = d = 0
        edges.append((s, d))
    rows = [[] for _ in range(N)]  # edge ids entering node n, in the order met
    for e in range(E):
        rows[edges[e][1]].append(e)
    perm = [e for row in rows for e in row]
    src, dst = [edges[e][0] for e in perm], [edges[e][1] for e in perm]
    cols = [[] for _ in range(N)]  # CSR positions leaving node n
    for p in range(E):
        cols[src[p]].append(p)

    def ptr(groups):
        out = [0]
        for g in groups:
            out.append(out[-1] + len(g))
        return out
    return {"perm": perm, "src": src, "dst": dst, "rowptr": ptr(rows), "colptr": ptr(cols),
            "cpos": [p for col in cols for p in col]}


def code_loops(ea, bond_dims, perm):
    if ea is None:
        return [0] * len(perm)
    out = []
    for e in perm:
        c = 0
        for k, d in enumerate(bond_dims):
            f = int(ea[e][k])
            if f < 0 or f >= d:
                f = 0
            c = c * d + f
        out.append(c)
    return out


def graph_ptr_loops(batch, N, B):
    if batch is None:
        return [0, N]
    ptr = []
    for g in range(B + 1):
        n = 0
        while n < N and batch[n] < g:
            n += 1
        ptr.append(n)
    return ptr
