"""The host half of the sparse map path's HBM tier (csrc/map_plan.h planMapLarge), without a device.

native.map_large_plan(op_counts, overflow_docs) is checked against the documented layout restated
here: slot counts are the smallest powers of two >= 2 x ops, the five slot regions, the op-slot
words, the tile counts and the last-clear words tile the scratch without a gap or an overlap, and the
tile table covers each overflowing document's ops exactly once, in order, the last tile short.
"""
import numpy as np
import pytest

from fluidframework_amd import native
from fluidframework_amd.native import FMT_E_USAGE, FMT_OK

T = 256  # csrc/map_plan.h kMapLargeTile


def test_library_exports_what_fmt_map_tiered_declares():
    """include/fmt_map_tiered.h declares the tiered run, beside fmt.h (whose own list is unchanged)."""
    import ctypes
    import os
    import re

    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    declared = lambda h: sorted(set(re.findall(r"^(?:int|void|const char\*)\s+(fmt_\w+)\(", open(os.path.join(inc, h)).read(), re.M)))  # noqa: E731
    fns = declared("fmt_map_tiered.h")
    assert fns == sorted(native.EXPORTED_SYMBOLS_MAP_TIERED) == ["fmt_map_run_sparse_tiered"]
    assert not set(fns) & set(native.EXPORTED_SYMBOLS) and not set(fns) & set(declared("fmt.h"))
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, f) for f in fns) and hasattr(lib, "fmt_internal_map_large_plan")


def _pow2_at_least(x):
    s = 1
    while s < x:
        s *= 2
    return s


def _check(op_counts, overflow):
    p = native.map_large_plan(op_counts, overflow)
    assert p.status == FMT_OK and p.message is None
    assert p.tile == T
    docs = [dict(zip(native.MAP_LARGE_DOC_FIELDS, (int(x) for x in row))) for row in p.docs]
    assert [d["doc"] for d in docs] == list(overflow)
    slots = ops = tiles = 0
    for d in docs:
        n = int(op_counts[d["doc"]])
        assert d["n_ops"] == n
        assert d["slots"] == _pow2_at_least(2 * n) and d["slots"] >= 2 * n and d["slots"] & (d["slots"] - 1) == 0
        assert d["slots"] < 4 * n                      # the documented bound: under 80 B of tables per op
        assert d["shift"] == 32 - (d["slots"].bit_length() - 1)
        assert d["table_off"] == slots and d["op_slot_off"] == ops and d["first_tile"] == tiles  # back to back
        assert d["n_tiles"] == -(-n // T)
        slots, ops, tiles = slots + d["slots"], ops + n, tiles + d["n_tiles"]
    assert (p.slots, p.ops, len(p.tile_doc), len(p.tile_first)) == (slots, ops, tiles, tiles)
    # regions, in 32-bit words: key, first, D, last, value (slots each), op slots, tile counts, last clears
    sizes = [slots] * 5 + [ops, tiles, len(docs)]
    at = 0
    for name, size in zip(native.MAP_LARGE_REGIONS, sizes):
        assert p.regions[name] == at, name
        at += size
    assert p.scratch_bytes == 4 * at == 4 * (5 * slots + ops + tiles + len(docs))
    assert p.scratch_bytes <= 84.02 * ops + 8 * len(docs)
    # tiles: each document's ops exactly once, in order
    want_doc, want_first = [], []
    for j, d in enumerate(docs):
        firsts = list(range(0, d["n_ops"], T))
        assert d["n_ops"] - firsts[-1] in range(1, T + 1)  # the last tile: short or whole, never empty
        want_doc += [j] * len(firsts)
        want_first += firsts
    assert p.tile_doc.tolist() == want_doc and p.tile_first.tolist() == want_first
    return p


def test_empty_overflow_list_is_an_empty_plan():
    p = _check([5, 0, 70000], [])
    assert p.scratch_bytes == 0 and p.slots == 0 and p.ops == 0 and len(p.docs) == 0 and len(p.tile_doc) == 0


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 2049, 4096, 16385, 65 * T - 1, 65 * T, 65 * T + 1, 32768, 32769,
                               1_000_000])
def test_one_document(n):
    p = _check([n], [0])
    assert p.docs[0, 2] == _pow2_at_least(2 * n)


@pytest.mark.parametrize("overflow", [[0], [4], [2], [1, 2], [0, 4], [0, 1, 2, 3, 4]])
def test_overflowing_document_first_last_alone_adjacent(overflow):
    _check([16385, 4096, 20000, 5, 17 * T], list(overflow))


def test_neighbours_do_not_enter_the_plan():
    a = _check([300, 16385, 2000], [1])
    b = _check([16385], [0])
    assert a.scratch_bytes == b.scratch_bytes and np.array_equal(a.tile_first, b.tile_first)
    assert a.docs[0, 0] == 1 and b.docs[0, 0] == 0


@pytest.mark.parametrize("counts,overflow", [([10, 20], [2]), ([10, 20], [1, 0]), ([10, 20], [1, 1]), ([10, 0], [1]),
                                             ([1 << 30], [0])])
def test_lists_that_cannot_be_planned(counts, overflow):
    p = native.map_large_plan(counts, overflow)
    assert p.status == FMT_E_USAGE and p.message
