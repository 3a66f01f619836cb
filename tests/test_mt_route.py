"""The route of a merge-tree batch through the tier cascade (csrc/mt_route.h planRoute) through its
device-free hook (native.mt_route): for every flag set the steps in order, each step's lists, variant,
dealing counter and step-down switch, the five out-slab booleans, the large pass's variant and
fmt_stats.launches, against a table written here by hand from the cascade as it stood before the route
existed (launchMergeTree / launchMergeTreeLocal / launchMergeTreeLarge and fmt_mt_run's result views), never
from planRoute. Then the same program under host emulation (descend_cascade, mt_compare.emu_replay): it
finishes the documents of the GPU route tests (route_cases.py) in the tiers they are built for."""
import numpy as np
import pytest

from fluidframework_amd import native
from fluidframework_amd.native import mt_variant_key as key
from fluidframework_amd.streams import MT_F_LOCAL, MT_F_RMORDER, MT_OBLITERATE, NO_PROPS
from test_mt_load_plan import ADJ_KV, LEAVES, ann, ins, make, op

# ---------------------------------------------------------------------------------------- the batches
PLAIN = dict(docs=[[ins(), op()]])
OB = dict(docs=[[ins(), op(MT_OBLITERATE)]])
RM = dict(docs=[[ins(), op(flags=MT_F_RMORDER)]])
OB_RM = dict(docs=[[ins(), op(MT_OBLITERATE), op(flags=MT_F_RMORDER)]])
ADJUST = dict(docs=[[ins(), ann(0)]], **ADJ_KV)
ADJUST_RM = dict(docs=[[ins(), ann(0), op(flags=MT_F_RMORDER)]], **ADJ_KV)
LOCAL = dict(docs=[[ins(flags=MT_F_LOCAL)]])
LOCAL_ADJUST = dict(docs=[[ins(flags=MT_F_LOCAL), ann(0)]], **ADJ_KV)
# a summary-loaded document past the large tier goes to the huge tier: the others run from the caller's list
HUGE = dict(docs=[[ins()], [op()]], snapshots=[None, (0, LEAVES + 1, 0, 0, 5)], segs=[(0, 1, NO_PROPS)] * (LEAVES + 1))


def route_of(spec, ckpt=True, desc=True, **kw):
    b, keep = make(**spec)
    return native.mt_route(None, ckpt, desc, struct=b, **kw)


# ------------------------------------------------------------------------------------------ the table
def step(tier, variant, src, up, down="none", order="none", deal=None, descend=False):
    return {"tier": tier, "variant": variant, "in": src, "up": up, "down": down, "order_into": order,
            "deal": deal or tier, "descend": descend}


def plain_steps(ckpt, desc, src="every", rounds=2):
    """micro over everything, then per round compact and small; with the checkpoint slab every device list is
    reordered first; with both slabs the rounds after the first replay the step-down lists, dealing from
    their own counters, and every round but the last lets small-tier documents step down."""
    order = "ordered" if ckpt else "none"
    steps = [step("micro", key(), src, "microUp")]
    n = rounds if ckpt and desc else 1
    for r in range(n):
        last = r + 1 == n
        to_compact, to_small = ("microUp", "compactUp") if r == 0 else (f"round({r},0)", f"round({r},1)")
        deals = ("compact", "small") if r == 0 else (f"round({r},0)", f"round({r},1)")
        steps.append(step("compact", key(), to_compact, to_small, order=order, deal=deals[0], descend=not last))
        steps.append(step("small", key(), to_small, "toLarge", down="none" if last else f"round({r + 1},0)", order=order,
                          deal=deals[1], descend=not last))
    return steps


def booleans(tiers_ckpt, large_ckpt, resumes_small, huge_ckpt, local):
    return dict(tiers_ckpt=tiers_ckpt, large_ckpt=large_ckpt, large_resumes_small=resumes_small, large_huge_ckpt=huge_ckpt,
                large_local=local)


def expected(name, ckpt, desc):
    """(steps, out-slab booleans, large variant, launches without the large and huge passes) by hand."""
    if name in ("plain", "huge"):
        return (plain_steps(ckpt, desc, "caller" if name == "huge" else "every"), booleans(ckpt, False, True, True, False),
                key(), 2)
    if name == "ob":  # starts compact; its overflow list reordered when there are checkpoints; the large pass
        # reads the live-obliterate table of the slots
        return ([step("compact", key(ob=True), "every", "compactUp"),
                 step("small", key(ob=True), "compactUp", "toLarge", order="ordered" if ckpt else "none")],
                booleans(ckpt, ckpt, True, True, False), key(ob=True), 2)
    if name == "ob_rm":  # remove order: the small tier alone, no checkpoint slab whatever the caller says
        return ([step("small", key(ob=True, rm=True), "every", "toLarge")], booleans(False, False, False, True, False),
                key(ob=True, rm=True), 1)
    if name == "rm":
        return ([step("small", key(rm=True), "every", "toLarge")], booleans(False, False, False, True, False), key(rm=True), 1)
    if name == "adjust":  # small tier first, the Ob variant, no checkpoints
        return ([step("small", key(ob=True, adj=True), "every", "toLarge")], booleans(False, False, True, True, False),
                key(ob=True, adj=True), 2)
    if name == "adjust_rm":
        return ([step("small", key(ob=True, rm=True, adj=True), "every", "toLarge")], booleans(False, False, False, True, False),
                key(ob=True, rm=True, adj=True), 1)
    if name == "local":  # FMT_LOCAL_PATH 1: the small tier's local variant (the views carry the slab, unused)
        return ([step("small", key(loc=True), "every", "toLarge")], booleans(ckpt, False, True, False, True), key(loc=True), 2)
    if name == "local_adjust":
        return ([step("small", key(adj=True, loc=True), "every", "toLarge")], booleans(False, False, True, False, True),
                key(adj=True, loc=True), 2)
    raise KeyError(name)


SPECS = {"plain": PLAIN, "ob": OB, "ob_rm": OB_RM, "rm": RM, "adjust": ADJUST, "adjust_rm": ADJUST_RM, "local": LOCAL,
         "local_adjust": LOCAL_ADJUST, "huge": HUGE}


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "nodesc"])
@pytest.mark.parametrize("ckpt", [True, False], ids=["ckpt", "nockpt"])
@pytest.mark.parametrize("name", list(SPECS))
def test_route_equals_the_hand_written_table(name, ckpt, desc):
    r = route_of(SPECS[name], ckpt, desc)
    steps, flags, large, base = expected(name, ckpt, desc)
    assert r.steps == steps
    assert {k: getattr(r, k) for k in flags} == flags
    assert r.large == large
    assert r.nominal_launches == {(False, False): base, (True, False): base + 1, (False, True): base + 1, (True, True): base + 2}
    assert r.rounds == (2 if name in ("plain", "huge") and ckpt and desc else 1)
    for s in r.steps:
        assert (s["tier"], s["variant"]) in r.kernels, s
    assert ("large", r.large) in r.kernels


def test_the_kernel_table_is_the_twenty_instantiations():
    k = route_of(PLAIN).kernels
    assert k == ({("micro", key())} | {("compact", v) for v in (key(), key(ob=True), key(loc=True))} |
                 {(t, v) for t in ("small", "large")
                  for v in (key(), key(ob=True), key(rm=True), key(ob=True, rm=True), key(ob=True, adj=True),
                            key(ob=True, rm=True, adj=True), key(loc=True), key(adj=True, loc=True))})


def test_local_paths():
    loc = key(loc=True)
    assert route_of(LOCAL, local_path=0).steps == [step("compact", loc, "every", "toLarge")]
    assert route_of(LOCAL, local_path=1).steps == [step("small", loc, "every", "toLarge")]
    assert route_of(LOCAL, local_path=2).steps == [step("compact", loc, "every", "compactUp"),
                                                   step("small", loc, "compactUp", "toLarge")]
    for path in (0, 1, 2):  # annotate-adjust: the small tier first whatever the path
        assert route_of(LOCAL_ADJUST, local_path=path).steps == [step("small", key(adj=True, loc=True), "every", "toLarge")]


def test_the_two_round_plain_route_step_by_step():
    """The five steps of a plain batch with both slabs, written out."""
    k = key()
    assert route_of(PLAIN).steps == [
        {"tier": "micro", "variant": k, "in": "every", "up": "microUp", "down": "none", "order_into": "none",
         "deal": "micro", "descend": False},
        {"tier": "compact", "variant": k, "in": "microUp", "up": "compactUp", "down": "none", "order_into": "ordered",
         "deal": "compact", "descend": True},
        {"tier": "small", "variant": k, "in": "compactUp", "up": "toLarge", "down": "round(1,0)", "order_into": "ordered",
         "deal": "small", "descend": True},
        {"tier": "compact", "variant": k, "in": "round(1,0)", "up": "round(1,1)", "down": "none", "order_into": "ordered",
         "deal": "round(1,0)", "descend": False},
        {"tier": "small", "variant": k, "in": "round(1,1)", "up": "toLarge", "down": "none", "order_into": "ordered",
         "deal": "round(1,1)", "descend": False}]


def test_rounds_override():
    assert route_of(PLAIN, rounds=3).steps == plain_steps(True, True, rounds=3)
    assert route_of(PLAIN, rounds=1).steps == plain_steps(True, True, rounds=1)
    assert route_of(PLAIN, desc=False, rounds=3).steps == plain_steps(True, False)


def test_the_emulation_library_plans_the_same_route():
    from fluidframework_amd import workloads
    from micro_cascade import route

    batch = workloads.conflict_farm(3, n_clients=2, ops_per_doc=20, seed=1)
    for ckpt, desc in ((True, True), (True, False), (False, True)):
        a, b = route(batch, ckpt, desc), native.mt_route(batch, ckpt, desc)
        assert a.steps == b.steps == plain_steps(ckpt, desc) and a.kernels == b.kernels


# ------------------------------------------------------------------------- the route under emulation
def test_route_cases_finish_in_the_tiers_they_are_built_for():
    from micro_cascade import COMPACT, LARGE, MICRO, SMALL
    from route_cases import huge_batch, plain_batch, run_route

    cas, large_ran = run_route(plain_batch())
    assert cas.done_in.tolist() == [MICRO, COMPACT, SMALL, LARGE] and large_ran and (cas.hdr["status"] == 0).all()
    batch, huge = huge_batch()
    assert [int(x) for x in native.mt_plan(batch).huge_docs] == [huge] and native.mt_route(batch).steps[0]["in"] == "caller"
    cas, large_ran = run_route(batch, skip=(huge,))
    assert cas.done_in.tolist() == [MICRO, COMPACT, SMALL, LARGE, -1] and large_ran


def test_variant_cases_finish_in_the_tiers_they_are_built_for():
    """The obliterate, remove-order and local batches of the GPU route tests: the kinds the plan sees, and
    (one tier alone, then the register tiers of the route) where each document finishes."""
    from mt_compare import emu_replay, emu_replay_local
    from route_cases import tier_leaves, variant_batch

    ob, rm, loc, adj = (variant_batch(k) for k in ("ob", "rm", "local", "adjust"))
    assert [s["tier"] for s in native.mt_route(adj).steps] == ["small"] and native.mt_plan(adj).any_adjust
    assert (emu_replay(adj, large=0)[0]["status"] == 0).tolist() == [True, False]   # the small tier, its register program
    assert (emu_replay(adj, large=4)[0]["status"] == 0).all()                       # and the large pass
    assert [s["tier"] for s in native.mt_route(ob).steps] == ["compact", "small"] and native.mt_plan(ob).obliterates
    assert [s["tier"] for s in native.mt_route(rm).steps] == ["small"] and native.mt_plan(rm).rm_order_ops > 0
    assert [s["tier"] for s in native.mt_route(loc).steps] == ["small"] and native.mt_plan(loc).local
    assert (emu_replay(ob, large=2)[0]["status"] == 0).tolist() == [True, False, False]   # the compact tier alone
    assert (emu_replay(ob, large=3)[0]["status"] == 0).tolist() == [True, True, False]    # compact -> small
    assert (emu_replay(ob, large=4)[0]["status"] == 0).all()                              # and the large pass
    assert (emu_replay(rm, large=3, cap_rm=512)[0]["status"] == 0).tolist() == [True, False]
    assert (emu_replay(rm, large=4, cap_rm=512)[0]["status"] == 0).all()
    hdr = emu_replay_local(loc)[0]
    assert (hdr["status"] == 0).all()
    small = tier_leaves()[2]
    assert int(hdr["n_leaves"][0]) <= small + 2 < int(hdr["n_leaves"][1])
