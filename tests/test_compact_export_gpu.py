"""GPU tier: the two stable compactions pinned to each other.  gs_compact and the exports run one scheme (csrc/gs_cloud_pass.h: k_compact_count<P>,
k_compact_offsets, compact_slot) over two predicates, and "not hidden" is the state filter (GS_STATE_HIDDEN, 0): for the same cloud and the
same state bytes, out_index of gs_export_splat(GS_STATE_HIDDEN, 0) and out_old_index of gs_compact are the same array -- and both are
numpy's stable filter of the state bytes.

Sizes around one chunk (CH = GS_EDIT_IPT * GS_BLOCK splats, one workgroup) and STEP * CH + 1 = 524 289, the smallest cloud at which the
one-workgroup offsets kernel makes a second trip of its loop.  tests/test_edit_edges_gpu.py already takes gs_compact across that trip
(test_compact_sizes_and_hidden_sets[524289] and the sizes above it, against numpy); what this module adds there is the export side, held
against the same array.  Per size: a seeded random half hidden, only the last splat hidden, only the first splat kept."""
import numpy as np
import pytest

from conftest import pkg
from test_edit_edges_gpu import CH, STEP, big_rows, rng, states_of

pytestmark = pytest.mark.gpu
capi = pkg("capi")

HIDDEN = capi.STATE_HIDDEN
SIZES = [CH - 1, CH, CH + 1, STEP * CH + 1]
assert SIZES[-1] == 256 * 2048 + 1


def hidden_patterns(n):
    """(name, hidden set), each keeping and hiding at least one splat"""
    i = np.arange(n)
    return [("random_half", rng(6100, n).random(n) < 0.5), ("last_hidden", i == n - 1), ("first_kept", i != 0)]


def kept_of(state):
    """numpy's stable filter: the indices whose byte passes (GS_STATE_HIDDEN, 0), ascending"""
    return np.flatnonzero((state & np.uint8(HIDDEN)) == 0).astype(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_export_index_equals_compact_old_index(n):
    rows = big_rows(n)
    with capi.Context(0) as c:
        for name, hid in hidden_patterns(n):
            state = states_of(hid, rng(6200, n))                        # the hidden bit under random user bits
            want = kept_of(state)
            assert 0 < want.size < n and np.array_equal(want, np.flatnonzero(~hid)), (n, name)
            c.clear()
            c.push_splat(rows)
            c.set_state(0, state)
            _, index = c.export_splat((HIDDEN, 0), want_index=True)
            old = c.compact()
            assert index.size == old.size == want.size, (n, name, index.size, old.size, want.size)
            assert np.array_equal(index, old), (n, name, "export against compact")
            assert np.array_equal(old, want), (n, name, "against numpy")
