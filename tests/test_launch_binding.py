"""The launch binding (csrc/mt_bind.h: bindDoc's resume decision and collectHeader's classification),
queried through the host build the emulations use (tests/emu/mt_emu_tiers.cpp), against tables written
out from the rules:

  * a tier that also saves (the compact one) resumes only over a list; the micro tier never resumes;
  * the Ob variants refuse kCkptDescend, and the compact tier's Ob variant has nothing to resume;
  * a register tier resumes only with the checkpoint slab;
  * the large tier resumes on kCkptEscalate only, and only when the small tier's slabs are given.
"""
import ctypes
import itertools

from micro_cascade import COMPACT, LARGE, MICRO, SMALL, lib

OK, E_CAPACITY, FINAL, CKPT, HUGE, DESC = 0, -3, -33, -34, -35, -36  # include/fmt.h, mt_engine.h, huge_ckpt.h
NONE, UP, DOWN = 0, 1, 2

# (tier, Ob) -> the (over a list, header status, slab) that resume; every other combination does not.
# slab: the checkpoint slab for the register tiers, the small tier's result slabs for the large tier.
RESUMES = {
    (MICRO, 0): set(),
    (MICRO, 1): set(),
    (COMPACT, 0): {(1, CKPT, 1), (1, DESC, 1)},
    (COMPACT, 1): set(),
    (SMALL, 0): {(0, CKPT, 1), (1, CKPT, 1), (0, DESC, 1), (1, DESC, 1)},
    (SMALL, 1): {(0, CKPT, 1), (1, CKPT, 1)},
    (LARGE, 0): {(0, CKPT, 1), (1, CKPT, 1)},
    (LARGE, 1): {(0, CKPT, 1), (1, CKPT, 1)},
}

# header status -> (hand-off, the status the header reports afterwards)
COLLECT = {
    OK: (NONE, OK),
    E_CAPACITY: (UP, E_CAPACITY),
    CKPT: (UP, CKPT),
    DESC: (DOWN, DESC),
    FINAL: (NONE, E_CAPACITY),
    HUGE: (NONE, HUGE),
    -1: (NONE, -1),
}


def test_resume_decision():
    L = lib()
    for (tier, ob), yes in RESUMES.items():
        for over_list, st, ckpt, small in itertools.product((0, 1), (OK, E_CAPACITY, CKPT, DESC), (0, 1), (0, 1)):
            slab = small if tier == LARGE else ckpt  # the other slab must not matter
            got = L.emu_bind_resumes(tier, ob, over_list, st, ckpt, small)
            assert got == int((over_list, st, slab) in yes), (tier, ob, over_list, st, ckpt, small)


def test_collect_classification():
    L = lib()
    for st, (hand_off, reported) in COLLECT.items():
        after = ctypes.c_int32(12345)
        assert L.emu_bind_collect(st, ctypes.byref(after)) == hand_off, st
        assert after.value == reported, st
