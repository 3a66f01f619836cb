"""The huge-document engine past the thresholds T3's shape stays inside of (huge_edges.py): proofs
from the ops and the oracle alone that the streams cross them, then the emulated engine at production
constants (and with 16-slot groups), its per-op invariant checker on, bit-exact against the oracle."""
import re

import numpy as np
import pytest

import huge_edges as he
from mt_compare import (compare_doc, emu_huge_replay, emu_huge_replay_adjust, emu_huge_replay_hi, oracle_rm_clients_hi,
                        oracle_rm_clients_hi2)
from test_huge_emulated import _removers_match

K = he.engine_constants()


def test_constants_are_read_from_the_header():
    assert K["kFill"] * 2 <= K["kSlotCap"] and K["kWinLds"] % 64 == 0
    assert K["kWinLds"] > 1024 and K["kWinLds"] % 512 != 0  # (a 512-entry pass step straddles the mirror's end)


# ------------------------------------------------------------------ the bounds are honest
@pytest.mark.parametrize("name", list(he.WINDOW_STREAMS))
def test_window_streams_cross_the_mirror(name):
    ws = he.WINDOW_STREAMS[name]
    ops = he.stream(name).ops
    assert (np.diff(ops["min_seq"]) >= 0).all() and (ops["min_seq"] <= ops["ref_seq"]).all()
    lo, hi = he.window_lower_bound(ops), he.window_upper_bound(ops, ws.max_range)
    assert (lo <= hi).all()
    holds = range(0, len(ops), ws.period)
    full = [k for k in holds if k + ws.period <= len(ops)]
    assert len(full) >= 3
    for k in full:
        assert lo[k + ws.period - 1] > K["kWinLds"], (k, int(lo[k + ws.period - 1]))
    for k in holds[1:]:
        assert hi[k] < K["kWinLds"], (k, int(hi[k]))
    up, down = he.crossings(ops, ws.period, ws.max_range, K["kWinLds"])
    assert up >= 3 and down >= 3


@pytest.mark.parametrize("name", list(he.WINDOW_STREAMS))
def test_a_weaker_hold_does_not_cross(name):
    """Half the period no longer proves a crossing: the assertion above measures the stream."""
    ws = he.WINDOW_STREAMS[name]
    ops = ws.batch(ws.period // 2).ops
    assert he.crossings(ops, ws.period // 2, ws.max_range, K["kWinLds"]) == (0, 0)


def test_hold_min_seq_changes_min_seq_alone():
    ws = he.WINDOW_STREAMS["window_sawtooth"]
    from fluidframework_amd import workloads
    base = workloads.t3_stream(ws.n_segments, ws.n_ops, n_clients=ws.n_clients, max_lag=ws.max_lag, max_range=ws.max_range,
                               seed=ws.seed)
    held = he.stream("window_sawtooth")
    for f in base.ops.dtype.names:
        if f != "min_seq":
            assert np.array_equal(base.ops[f], held.ops[f]), f
    assert (held.ops["min_seq"] <= base.ops["min_seq"]).all()
    assert np.array_equal(held.ops["min_seq"][:: ws.period], base.ops["min_seq"][:: ws.period])
    assert np.array_equal(base.text, held.text) and np.array_equal(base.snapshot_segs, held.snapshot_segs)


@pytest.mark.parametrize("name", list(he.DEEP_STREAMS))
def test_deep_streams_pass_the_mirror_and_end_past_it(name):
    """One full hold, its release, and a second hold the stream ends in: the lower bound is past kWinLds
    at the end of the first hold, minSeq advances at the release (which graduates entries while the table
    is past the mirror), and the bound is past kWinLds again at the last op, whose minSeq is the final one."""
    ws = he.DEEP_STREAMS[name]
    ops = he.stream(name).ops
    assert len(ops) == 2 * ws.period
    assert (np.diff(ops["min_seq"]) >= 0).all() and (ops["min_seq"] <= ops["ref_seq"]).all()
    lo = he.window_lower_bound(ops)
    assert lo[ws.period - 1] > K["kWinLds"] and lo[-1] > K["kWinLds"], (int(lo[ws.period - 1]), int(lo[-1]))
    assert ops["min_seq"][ws.period] > ops["min_seq"][ws.period - 1]
    if name == "window_many_writers":
        assert int(ops["client"].max()) > 63


# ------------------------------------------------------------------ group proofs
def _one_group_at_load(orc, batch):
    """A load lists kFill leaf blocks per group: the oracle's tree with no op replayed has at most that many."""
    rc, loaded = he.oracle_state(orc, he.prefix(batch, 0))
    assert rc == 0
    return he.leaf_blocks(loaded[1]) <= K["kFill"]


def test_group_split_stream_outgrows_one_group(orc):
    batch = he.stream("group_split")
    assert _one_group_at_load(orc, batch)
    assert he.leaf_blocks(he.expected(orc, "group_split")[1]) > K["kSlotCap"]


def test_split_with_tail_splits_while_the_window_is_past_the_mirror(orc):
    batch = he.stream("split_with_tail")
    assert _one_group_at_load(orc, batch)
    assert len(np.unique(batch.ops["min_seq"])) == 1  # one hold
    lo = he.window_lower_bound(batch.ops)
    assert lo[he.SPLIT_TAIL_BEFORE - 1] > K["kWinLds"]
    rc, before = he.oracle_state(orc, he.prefix(batch, he.SPLIT_TAIL_BEFORE))
    assert rc == 0 and he.leaf_blocks(before[1]) <= K["kSlotCap"]
    assert he.SPLIT_TAIL_AFTER == len(batch.ops)
    assert he.leaf_blocks(he.expected(orc, "split_with_tail")[1]) > K["kSlotCap"]


# ------------------------------------------------------------------ emulated parity
def _replay(batch, exp, tiny):
    if int(batch.ops["client"].max()) > 63:
        return _replay_many_writers(batch, exp, tiny)
    got = emu_huge_replay(batch, tiny_groups=tiny)
    assert int(got[0]["status"]) == 0, f"engine status {int(got[0]['status'])} at seq {int(got[0]['fail_seq'])}"
    assert compare_doc(exp, got) == []


def _replay_many_writers(batch, exp, tiny):
    """Writers past 63: the engine with its side table for short ids 64..253; those ids of every leaf's
    remove-client set == the oracle's remove stamps."""
    n = int(exp[0]["n_leaves"])
    h, lv, ch, pr, hi, hi2 = emu_huge_replay_hi(batch, 0, tiny_groups=tiny, hi2=True)
    assert int(h["status"]) == 0, f"engine status {int(h['status'])} at seq {int(h['fail_seq'])}"
    assert compare_doc(exp, (h, lv, ch, pr)) == []
    want = oracle_rm_clients_hi(batch, 0, n)
    assert np.array_equal(hi, want) and np.array_equal(hi2, oracle_rm_clients_hi2(batch, 0, n))
    assert int((want != 0).sum()) > 100


@pytest.mark.parametrize("name", [n for n in he.STREAMS if n != "compaction"])  # (compaction: its own test below)
def test_emulated_engine_at_production_constants(orc, name):
    _replay(he.stream(name), he.expected(orc, name), False)


@pytest.mark.parametrize("name", list(he.WINDOW_STREAMS) + list(he.DEEP_STREAMS))
def test_emulated_engine_with_tiny_groups(orc, name):
    """16-slot groups: groups split in the middle of a long window and retag entries past the mirror."""
    _replay(he.stream(name), he.expected(orc, name), True)


def test_compaction_under_the_runtime_merge_area(orc, monkeypatch, capfd):
    """The churn stream compacts the merge area at the size the runtime itself gives the document
    (normal groups; FMT_EMU_TEXTCAP set to the same formula only makes the emulation report)."""
    batch = he.stream("compaction")
    monkeypatch.setenv("FMT_EMU_TEXTCAP", str(len(batch.text) + he.merge_area_units(batch)))
    capfd.readouterr()
    _replay(batch, he.expected(orc, "compaction"), False)
    assert int(re.search(r"compactions (\d+)", capfd.readouterr().err).group(1)) >= 1


# ------------------------------------------------------------------ the Rm and Adj instantiations
def test_deep_window_remove_order(orc):
    """HugeDocT<false, true> on window_deep, which ends inside a hold: more than kWinLds leaves are
    still above the final minSeq, many of them removed by several writers, so their stamp lists come
    from the recorded remove-order entries (through the release's swaps and every split since) and
    == the oracle's."""
    batch = he.with_remove_order(he.stream("window_deep"))
    got = emu_huge_replay(batch, cap_rm=1 << 18)
    assert int(got[0]["status"]) == 0, f"engine status {int(got[0]['status'])} at seq {int(got[0]['fail_seq'])}"
    assert compare_doc(he.expected(orc, "window_deep"), got[:4]) == []
    assert int(got[0]["n_rm_order"]) > 0
    assert _removers_match(orc, batch, got, got[4]) > 0  # (leaves with more than one remover compared)


def test_sawtooth_annotate_adjust(orc):
    """HugeDocT<true, false> on the sawtooth with every second annotate an adjust: state and computed
    numbers == the oracle's."""
    batch = he.with_adjusts(he.stream("window_sawtooth"))
    nums = []
    rc, exp = he.oracle_state(orc, batch, numbers=nums)
    assert rc == 0 and len(nums[0]) > 4
    h, lv, ch, pr, _, got_nums = emu_huge_replay_adjust(batch)
    assert int(h["status"]) == 0, (int(h["status"]), int(h["fail_seq"]))
    assert compare_doc(exp, (h, lv, ch, pr)) == []
    assert np.array_equal(got_nums, nums[0])
