"""The huge tier on the GPU past the thresholds T3's shape stays inside of (huge_edges.py; the CPU
proofs that the streams cross them are in test_huge_edges.py): window entries beyond the LDS mirror,
a group split at the production slot count, both in one hold, and merge-area compaction under the
runtime's own sizing. Every document equals the oracle on every leaf field, the text, the props and the
header, and its state digest; the device's own profile counters witness the reach a second time."""
import numpy as np
import pytest

import huge_edges as he
from fluidframework_amd import native, workloads
from mt_compare import compare_doc, oracle_rm_clients_hi, oracle_rm_clients_hi2

pytestmark = pytest.mark.gpu

K = he.engine_constants()


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _run(engine, batch):
    engine.mt_load(batch)
    engine.mt_run()
    hdrs = engine.mt_headers()
    assert (hdrs["status"] == 0).all(), [(int(h["status"]), int(h["fail_seq"])) for h in hdrs]
    return hdrs


def _equals_oracle(orc, engine, hdrs, d, exp):
    lv, ch, pr = engine.mt_doc(d, hdrs[d])
    assert compare_doc(exp, (hdrs[d], lv, ch, pr)) == [], d
    return lv


def _mean_window(p):
    return p["sum_window_entries"] / p["n_group_passes"]


def _reach(name, p):
    """What the device's profile of the document must show (existing slots of huge_profile)."""
    assert p["n_group_passes"] > 0
    if name in he.WINDOW_STREAMS:
        assert _mean_window(p) > K["kWinLds"], (name, _mean_window(p))  # (a mean above it: the peak crossed it)
    if name in ("group_split", "split_with_tail"):
        assert p["sum_groups"] > p["n_group_passes"], name  # (loaded as one group: passes saw more)
    if name == "compaction":
        assert p["text_compactions"] >= 1


@pytest.mark.parametrize("name", list(he.STREAMS))
def test_edge_stream_matches_oracle(orc, engine, name):
    batch, exp = he.stream(name), he.expected(orc, name)
    hdrs = _run(engine, batch)
    _equals_oracle(orc, engine, hdrs, 0, exp)
    if name == "window_many_writers":  # short ids 64..253 of every leaf's remove-client set
        n = int(exp[0]["n_leaves"])
        assert np.array_equal(engine.mt_rm_clients_hi(0, hdrs[0]), oracle_rm_clients_hi(batch, 0, n))
        assert np.array_equal(engine.mt_rm_clients_hi2(0, hdrs[0]), oracle_rm_clients_hi2(batch, 0, n))
    dig = engine.mt_digests()
    assert int(dig[0]) == he.expected_digest(orc, name)
    p = engine.huge_profile(0)
    print(name, "mean window", round(_mean_window(p), 1), "mean groups", round(p["sum_groups"] / p["n_group_passes"], 3),
          "compactions", p["text_compactions"], "merge units", p["merge_units_in_use"], "leaf blocks", he.leaf_blocks(exp[1]))
    _reach(name, p)
    engine.mt_run()  # the mirror and the tail are rebuilt from scratch
    assert np.array_equal(engine.mt_headers(), hdrs)
    assert np.array_equal(engine.mt_digests(), dig)


def test_deep_window_remove_order_on_gpu(orc, engine):
    """hugeDocKernel<false, true> on window_deep, which ends inside a hold with more than kWinLds leaves
    above the final minSeq: leaves with several removers take their stamp lists from the recorded entries."""
    from test_huge_emulated import _removers_match
    batch = he.with_remove_order(he.stream("window_deep"))
    hdrs = _run(engine, batch)
    lv = _equals_oracle(orc, engine, hdrs, 0, he.expected(orc, "window_deep"))
    rm = engine.mt_remove_order(0, hdrs[0])
    assert len(rm) > 0
    assert _removers_match(orc, batch, (hdrs[0], lv), rm) > 0  # (leaves with more than one remover compared)


def test_sawtooth_annotate_adjust_on_gpu(orc, engine):
    """hugeDocKernel<true, false>: state and computed numbers of the sawtooth with adjusts."""
    batch = he.with_adjusts(he.stream("window_sawtooth"))
    nums = []
    rc, exp = he.oracle_state(orc, batch, numbers=nums)
    assert rc == 0
    hdrs = _run(engine, batch)
    _equals_oracle(orc, engine, hdrs, 0, exp)
    assert np.array_equal(engine.mt_numbers(0), nums[0])
    assert _mean_window(engine.huge_profile(0)) > K["kWinLds"]


def test_edge_documents_side_by_side(orc, engine):
    """The window streams, both split streams and window_deep in one batch with a small conflict farm: several huge
    documents replay at once, each with its own window tail."""
    names = ["window_sawtooth", None, "window_sawtooth_wide", "split_with_tail", "group_split", "window_deep"]
    farm = workloads.conflict_farm(6, n_clients=8, ops_per_doc=300, seed=8)
    batch = he.concat_batches([farm if n is None else he.stream(n) for n in names])
    hdrs = _run(engine, batch)
    d = 0
    for n in names:
        if n is None:
            for k in range(farm.n_docs):
                rc, exp = he.oracle_state(orc, he.one_doc(farm, k))
                assert rc == 0
                _equals_oracle(orc, engine, hdrs, d + k, exp)
            d += farm.n_docs
        else:
            _equals_oracle(orc, engine, hdrs, d, he.expected(orc, n))
            _reach(n, engine.huge_profile(d))
            d += 1
    assert d == batch.n_docs
