"""The numpy references of the packer's base arrays (tests/pack_ref.py) against plain Python loops, on the cases of
tests/test_pack_batch_gpu.py, so that the GPU tests compare against a pinned reference."""
import numpy as np
import pytest

from tests import pack_ref as R
from tests import test_pack_batch_gpu as G

# past_scan_bound has a million nodes: its point is the device scan, and the loops would only repeat scan_tile_N1025
NAMES = [n for n in G.CASE_NAMES if n != "past_scan_bound"]


@pytest.mark.parametrize("name", NAMES)
def test_references_equal_the_loops(name):
    c = G._all_cases()[name]
    ei = c.ei.numpy()
    ea = None if c.ea is None else c.ea.numpy()
    batch = None if c.batch is None else c.batch.numpy()
    ref, loops = R.csr_reference(ei, c.N), R.csr_loops(ei, c.N)
    for key in ("perm", "src", "dst", "rowptr", "colptr", "cpos"):
        assert np.asarray(ref[key]).tolist() == loops[key], key
    assert R.code_reference(ea, c.bond_dims, ref["perm"]).tolist() == R.code_loops(ea, c.bond_dims, loops["perm"])
    assert R.code_reference(None, c.bond_dims, ref["perm"]).tolist() == [0] * ei.shape[1]
    assert R.graph_ptr_reference(batch, c.N, c.B).tolist() == R.graph_ptr_loops(batch, c.N, c.B)
    assert R.graph_ptr_reference(None, c.N, c.B).tolist() == [0, c.N]


def test_the_written_out_answers():
    """Three answers worked out by hand."""
    assert R.graph_ptr_reference(np.array([1, 1, 3, 3, 3, 5]), 6, 8).tolist() == [0, 0, 2, 2, 5, 5, 6, 6, 6]
    ea = np.array([[1, 2, 0], [0, 0, 1], [4, 5, 1], [5, 0, 0], [0, -1, 1]])  # the last two: one feature outside each
    assert R.code_reference(ea, (5, 6, 2), np.array([4, 3, 2, 1, 0])).tolist() == [1, 0, 59, 1, 16]
    ref = R.csr_reference(np.array([[2, 0, 1, 3, 2], [1, 1, 0, 1, -1]]), 3)  # edge 3: source 3 = N, edge 4: target -1
    assert ref["perm"].tolist() == [2, 3, 4, 0, 1] and ref["src"].tolist() == [1, 0, 0, 2, 0]
    assert ref["rowptr"].tolist() == [0, 3, 5, 5] and ref["colptr"].tolist() == [0, 3, 4, 5]
    assert ref["cpos"].tolist() == [1, 2, 4, 0, 3]
