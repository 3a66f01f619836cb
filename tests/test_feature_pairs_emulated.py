"""Merge-tree feature pairs under host emulation against the oracle's replay of the same batch
(streams and checks: feature_pairs.py). Every test first asserts, on the oracle's result, that the pair
is live in its batch; no document is left out of a comparison: one the emulated small tier reports
as outgrown (-3) is compared on the next tier's route in the same test.
"""
import pytest

import feature_pairs as fp
from mt_compare import (emu_caps, emu_grow_replay, emu_huge_replay, emu_huge_replay_adjust, emu_legacy_props, emu_numbers,
                        emu_replay)

CAP_RM, CAP_CU = fp.CAP_RM, fp.CAP_CU


def _emu_docs(batch, large, cap_rm=0, cap_catchup=0):
    """emu_replay of the batch on one route -> (headers, per-document results for fp.check_doc)."""
    r = emu_replay(batch, large=large, cap_rm=cap_rm, cap_catchup=cap_catchup)
    hdr, leaves, chars, props = r[:4]
    cu = r[4] if cap_catchup else None
    rm = r[4 + bool(cap_catchup)] if cap_rm else None
    adjust = batch.adjusts is not None
    docs = []
    for d in range(batch.n_docs):
        h = hdr[d]
        lg = emu_legacy_props(d) if adjust else None
        docs.append(dict(got=(h, leaves[d], chars[d], props[d]), nums=emu_numbers(d) if adjust else None,
                         legacy=lg[: int(h["n_leaves"])] if lg is not None else None,
                         rm=rm[d][: int(h["n_rm_order"])] if cap_rm else None, cu=cu[d] if cap_catchup else None))
    return hdr, docs


def _check_cascade(o, batch, finals, escalate, **caps):
    """The small tier alone, then the runtime's small -> large route: a document the small tier
    finishes is compared there, one it reports as outgrown (-3) on the large route; `escalate`:
    (least, most) such documents expected."""
    small, sdocs = _emu_docs(batch, False, **caps)
    up = [d for d in range(batch.n_docs) if int(small[d]["status"]) == -3]
    assert escalate[0] <= len(up) <= escalate[1], len(up)
    # (an Adj batch's large route is the small tier, then the large tier over what it could not hold;
    # others: the large tier from op 0, as the runtime restarts remove-order and catch-up batches)
    _, ldocs = _emu_docs(batch, 1, **caps) if up else (None, None)
    for d in range(batch.n_docs):
        r = ldocs[d] if d in up else sdocs[d]
        fp.check_doc(o, d, r["got"], nums=r["nums"], legacy=r["legacy"], rm=r["rm"], cu=r["cu"],
                     final=finals[d] if finals else None)
    return up


@pytest.mark.parametrize("narrow", [True, False])
def test_emulated_adjust_x_remove_order(orc, narrow):
    """Doc<true, S, true, Adj> (narrow) and Doc<true, G, true, Adj> (most documents escalate through
    the 32-prop-set limit): numbers, getAtSeq summaries, stamp lists and V1 summaries == oracle."""
    batch, finals = fp.adjust_rm_batch(narrow)
    o = fp.Oracle(orc, batch, emu_caps(True))
    nums, multi = fp.live_adjust_rm(o)
    assert nums > 0 and multi > 0, (nums, multi)
    n = batch.n_docs  # (the 0.40 message bundle holds 6 of the farms)
    up = _check_cascade(o, batch, finals, (0, 0) if narrow else ((n + 1) // 2, n), cap_rm=CAP_RM)
    print(f"narrow={narrow}: computed numbers {nums}, multi-remover adjusted leaves {multi}, escalated {len(up)}")


@pytest.mark.parametrize("long", [False, True])
def test_emulated_adjust_x_obliterate(orc, long):
    """Doc<true, S, false, Adj> on streams that hold obliterates, and (long: every document past the
    small tier's text) Doc<true, G, false, Adj>."""
    batch, _ = fp.adjust_ob_batch(long)
    o = fp.Oracle(orc, batch, emu_caps(True))
    nums, hit = fp.live_adjust_ob(o)
    assert nums > 0 and hit > 0, (nums, hit)
    n = batch.n_docs
    up = _check_cascade(o, batch, None, (n, n) if long else (0, n // 4))
    print(f"long={long}: computed numbers {nums}, obliterated adjusted leaves {hit}, escalated {len(up)}")


def test_emulated_obliterate_x_remove_order_past_small_tier(orc):
    """Doc<true, G, true> from op 0 over the long obliterate farms."""
    batch, _ = fp.ob_rm_long_batch()
    o = fp.Oracle(orc, batch, emu_caps(True))
    both = fp.live_both_stamps(o)
    assert both > 0
    up = _check_cascade(o, batch, None, (15, 30), cap_rm=CAP_RM)
    print(f"leaves with both kinds of stamp {both}, escalated {len(up)}")


@pytest.mark.parametrize("kind", ["adjust", "rm"])
def test_emulated_catchup_pairs(orc, kind):
    """Catch-up ranges beside the Adj variant's records / beside the remove-order slab."""
    batch, finals = fp.catchup_pair_batches(only=kind)[kind]
    o = fp.Oracle(orc, batch, emu_caps(True), cap_catchup=CAP_CU)
    fp.assert_catchup_live(o, kind)
    _check_cascade(o, batch, finals, (0, 0), cap_catchup=CAP_CU, **({"cap_rm": CAP_RM} if kind == "rm" else {}))


GROWTH = {
    "adjust_rm": (fp.adjust_rm_growth, dict(cap_rm=fp.CAP_RM)),
    "ob_rm": (fp.ob_rm_growth, dict(cap_rm=fp.CAP_RM)),
    "ob_adjust": (fp.ob_adjust_growth, {}),
    "catchup_adjust": (lambda: fp.catchup_pair_batches(only="adjust_growth")["adjust_growth"], dict(cap_catchup=fp.CAP_CU)),
    "catchup_rm": (lambda: fp.catchup_pair_batches(only="rm_growth")["rm_growth"],
                   dict(cap_catchup=fp.CAP_CU, cap_rm=fp.CAP_RM)),
}


@pytest.mark.parametrize("kind", list(GROWTH))
def test_emulated_pair_crosses_the_large_to_huge_checkpoint(orc, kind):
    """The large tier's variant for the pair stops at its checkpoint with every slab count carried
    (kCuN, kRmN, kPmN) and HugeDocT<Adj, Rm> resumes: == the oracle's whole replay."""
    build, caps = GROWTH[kind]
    batch = build()
    o = fp.Oracle(orc, batch, fp.HUGE_CAPS, cap_catchup=caps.get("cap_catchup", 0), index=True)
    fp.assert_growth_live(o, kind)
    got, resumed = emu_grow_replay(batch, **caps)
    assert resumed[0] > 0
    r = list(got[0][4:])
    cu = r.pop(0) if "cap_catchup" in caps else None
    rm = r.pop(0) if "cap_rm" in caps else None
    legacy, nums = r if batch.adjusts is not None else (None, None)
    fp.check_doc(o, 0, got[0][:4], nums=nums, legacy=legacy, rm=rm, cu=cu)
    fp.assert_carried(o, kind, resumed[0])
    print(f"{kind}: resumed at op {resumed[0]} of {len(batch.ops)}")


@pytest.mark.parametrize("kind", ["adjust_rm", "ob_rm"])
def test_emulated_pair_loaded_in_the_huge_tier(orc, kind):
    """A summary-loaded document over the large tier at load: HugeDocT<Adj, true> from its first message."""
    batch = fp.load_time_huge(kind)
    o = fp.Oracle(orc, batch, fp.HUGE_CAPS, index=True)
    if kind == "adjust_rm":
        nums, multi = fp.live_adjust_rm(o)
        assert nums > 0 and multi > 0, (nums, multi)
        h, lv, ch, pr, legacy, got_nums, rm = emu_huge_replay_adjust(batch, cap_rm=CAP_RM)
        fp.check_doc(o, 0, (h, lv, ch, pr), nums=got_nums, legacy=legacy, rm=rm)
    else:
        assert fp.live_both_stamps(o) > 0
        h, lv, ch, pr, rm = emu_huge_replay(batch, cap_rm=CAP_RM)
        fp.check_doc(o, 0, (h, lv, ch, pr), rm=rm)
