"""The summary-edge corpus (tests/summary_edges.py) on the CPU: every family reaches the decisions
it exists for, the census reproduces the reference's segment boundaries, the two references agree
byte for byte at every chunk size, and the bulk paths' host formatters (runtime.cpp legacyBlobs and
v1Blobs through fmt_internal_legacy_format / fmt_internal_v1_format: jsonQuote16, propsObject,
arrayIndexOfQuoted and both chunkers) write the references' bytes from the runs the kernels' rule
yields. No GPU: the kernels themselves are held to the same references in test_gpu_summary_edges.py."""
import ctypes
import os
import subprocess
from collections import Counter

import pytest

import summary_edges as se
from fluidframework_amd import native, summary

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = list(se.FAMILIES)
CPU_TIERS = {f: se.TIERS for f in FAMILIES}
CPU_TIERS["props_adjust"] = ["asis", "large"]  # (its getAtSeq view comes from the emulation; huge: on the GPU)
FAMILY_TIERS = [(f, t) for f in FAMILIES for t in CPU_TIERS[f]]


@pytest.fixture(scope="module")
def libfmt():
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "fluidframework_amd", "csrc")], check=True)
    return ctypes.CDLL(native.LIB_PATH)


@pytest.mark.parametrize("family,tier", FAMILY_TIERS)
def test_family_reaches_its_decisions(orc, family, tier):
    seen = Counter()
    for d, (h, l, c, p, view) in enumerate(se.legacy_view_state(family, tier)):
        ms = int(h["min_seq"])
        cen, runs = se.census(h, l, c, p, ms, view)
        seen += cen
        segs = summary.legacy_segments(h, l, c, p, ms, view)
        assert runs == [summary._utf16_len(t) for t, _, _ in segs], d  # the census, checked against the reference
        assert runs == [int(x) for x in summary.legacy_run_records(h, l, c, p, ms, view)[0]["len"]], d
    assert [k for k in se.promises(family, tier) if not seen[k]] == []


@pytest.mark.parametrize("tier", se.TIERS)
def test_first_remover_documents_keep_their_shape(orc, tier):
    bt, names = se.batch("first_remover", tier)
    state, _ = se.oracle_state("first_remover", tier)
    facts = {name: se.remover_census(bt, d, state) for d, name in enumerate(names)}
    for n in (64, 65, 4097):
        f = facts[f"{n}_records"]
        assert (f["n_records"], f["first"], f["middle"], f["last"], f["loadseg_prefix"]) == (n, 1, 1, 1, 0), n
    assert facts["remover_second_in_group"]["not_first_of_seq"] >= 1
    f = facts["loaded_then_removed"]
    assert f["loadseg_prefix"] == 3 and f["first"] + f["middle"] + f["last"] >= 2


def test_adjust_batch_reads_another_view_than_v1(orc):
    """In the annotate-adjust batch the legacy summary reads getAtSeq(minSeq) and SnapshotV1 the leaf's
    own props: they decide the pair around an adjust above minSeq differently. A plain annotate above
    minSeq is not rolled back, and an adjust at or below minSeq reads the same in both."""
    differ = [se.census(h, l, c, p, int(h["min_seq"]), view)[1] != se.census(h, l, c, p, int(h["min_seq"]))[1]
              for h, l, c, p, view in se.legacy_view_state("props_adjust", "asis")]
    assert differ == [False, True, False]


@pytest.mark.parametrize("family,tier", FAMILY_TIERS)
def test_legacy_references_agree_and_the_formatter_writes_them(orc, libfmt, family, tier):
    bt, _ = se.batch(family, tier)
    _, numbers = se.oracle_state(family, tier)
    state = se.legacy_view_state(family, tier)
    want = se.legacy_reference(family, tier)
    assert len({c for _, c in want}) >= 3
    for (d, chunk), blobs in want.items():
        h, l, c, p, view = state[d]
        vals = se.doc_values(bt, numbers, d)
        assert summary.legacy_summary(h, l, c, p, bt.keys, vals, chunk, view) == blobs, (d, chunk)
        runs, text = summary.legacy_run_records(h, l, c, p, int(h["min_seq"]), view)
        got = native.legacy_format(runs, text, p[: int(h["n_props"])], bt.keys, bt.values, int(h["min_seq"]), chunk,
                                   None if numbers is None else numbers[d])
        assert got == blobs, (d, chunk)


@pytest.mark.parametrize("family,tier", FAMILY_TIERS)
def test_v1_reference_equals_the_formatter(orc, libfmt, family, tier):
    bt, _ = se.batch(family, tier)
    state, numbers = se.oracle_state(family, tier)
    want = se.v1_reference(family, tier)
    for (d, chunk), blobs in want.items():
        h, l, c, p, rm = state[d]
        segs, text, later = summary.v1_segment_records(h, l, c, p, rm)
        got = native.v1_format(segs, text, p[: int(h["n_props"])], later, bt.keys, bt.values, bt.clients[d],
                               int(h["min_seq"]), int(h["cur_seq"]), chunk, None if numbers is None else numbers[d])
        assert got == blobs, (d, chunk)


def test_chunk_sizes_cut_where_the_family_says(orc):
    """The chunks family at its own totals: a header that takes exactly the total or stops one unit
    short of it, and SnapshotV1's do-while with a body per segment."""
    want = se.legacy_reference("chunks")
    v1 = se.v1_reference("chunks")
    import json

    for d in range(se.batch("chunks")[0].n_docs):
        total = json.loads(want[d, 10000][0])["totalLengthChars"]
        n = json.loads(want[d, 10000][0])["totalSegmentCount"]
        assert want[d, total][1] is None and want[d, 10000][1] is None
        last = se._len(json.loads(want[d, 10000][0])["segmentTexts"][-1])  # the last run's units
        # one unit short of the total: the header still takes the last run, unless that run is one unit
        assert (want[d, max(total - 1, 1)][1] is not None) == (n > 1 and last == 1), d
        assert (want[d, 1][1] is None) == (n == 1)
        assert len(v1[d, 1][1]) == n - 1  # a body per segment past the header's
    assert any(want[d, max(json.loads(want[d, 10000][0])["totalLengthChars"] - 1, 1)][1] is not None for d in range(5))
    assert any(json.loads(want[d, 10000][0])["totalSegmentCount"] >= 5 for d in range(5))


def test_a_failed_neighbour_is_refused_by_the_oracle_alone(orc):
    bt = se.neighbours_batch()
    with pytest.raises(RuntimeError):
        orc.mt_replay_summary(bt, 1, bt.keys, bt.values)
    rc, h, l, c, p, _ = orc.mt_replay_batch(bt, cap_leaves=se.CAP_LEAVES, cap_chars=1 << 14, cap_props=se.CAP_PROPS)
    assert [int(s) for s in h["status"]] == [0, native.FMT_E_DATA, 0]
    for d in (0, 2):
        assert summary.legacy_summary(h[d], l[d], c[d], p[d], bt.keys, bt.values) == orc.mt_replay_summary(bt, d, bt.keys, bt.values)
