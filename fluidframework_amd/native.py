"""ctypes binding of libfmt.so (include/fmt.h), the HIP engine for gfx950.

There is no CPU fallback: if the library or a gfx950 device is missing, every call raises
`EngineUnavailable`. Result dtypes below mirror the C structs byte for byte.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfmt.so")

FMT_OK = 0
FMT_E_USAGE, FMT_E_DATA, FMT_E_CAPACITY, FMT_E_DEVICE, FMT_E_UNSUPPORTED = -1, -2, -3, -4, -5
STATUS_NAMES = {0: "OK", -1: "USAGE", -2: "DATA", -3: "CAPACITY", -4: "DEVICE", -5: "UNSUPPORTED"}

LEAF_DTYPE = np.dtype(
    [
        ("ins_seq", "<i4"),
        ("rm_seq", "<i4"),
        ("rm_clients", "<u8"),
        ("char_off", "<u4"),
        ("len", "<u4"),
        ("ins_client", "<i2"),
        ("props", "<u2"),
        ("block", "<u2"),
        ("pad", "<u2"),
    ]
)
assert LEAF_DTYPE.itemsize == 32

DOC_RESULT_DTYPE = np.dtype(
    [
        ("status", "<i4"),
        ("fail_seq", "<i4"),
        ("cur_seq", "<i4"),
        ("min_seq", "<i4"),
        ("n_leaves", "<u4"),
        ("n_chars", "<u4"),
        ("n_props", "<u4"),
        ("n_blocks", "<u4"),
        ("depth", "<u4"),
        ("visible_len", "<u4"),
        ("n_catchup", "<u4"),
        ("n_rm_order", "<u4"),
    ]
)
assert DOC_RESULT_DTYPE.itemsize == 48

# fmt_mt_remove_order: a later remove stamp of a leaf (leaf index, client, seq, kind 0 = setRemove /
# 1 = sliceRemove); FMT_MT_LEAF_GONE leaf
RM_ORDER_DTYPE = np.dtype([("leaf", "<u4"), ("client", "<i4"), ("seq", "<i4"), ("kind", "<u4")])
LEAF_GONE = 0xFFFFFFFF

# fmt_kernels::SumV1Seg (csrc/kernels.h): one SnapshotV1 summary segment as the bulk kernel writes it
V1_SEG_DTYPE = np.dtype([("len", "<u4"), ("props", "<u2"), ("flags", "<u2"), ("leaf", "<u4"), ("ins_seq", "<i4"),
                         ("ins_client", "<i4"), ("rm_client", "<i4"), ("rm_seq", "<i4"), ("rm_kind", "<u4")])
assert V1_SEG_DTYPE.itemsize == 32
V1_MARKER, V1_SOLO, V1_REMOVED = 1, 2, 4  # SumV1Seg.flags

CATCHUP_DTYPE = np.dtype([("op", "<u4"), ("pos1", "<i4"), ("pos2", "<i4"), ("type", "<u4")])
# include/fmt_runs.h fmt_mt_prop_run
PROP_RUN_DTYPE = np.dtype([("start", "<u4"), ("len", "<u4"), ("first_leaf", "<u4"), ("props", "<u2"), ("flags", "<u2")])
assert PROP_RUN_DTYPE.itemsize == 16
RUN_MARKER = 1  # fmt_runs.h FMT_MT_RUN_MARKER
# include/fmt_pos.h fmt_mt_pos_query / fmt_mt_pos_hit
POS_QUERY_DTYPE = np.dtype([("pos", "<u4"), ("ref_seq", "<i4"), ("client", "<i4"), ("pad", "<u4")])
POS_HIT_DTYPE = np.dtype([("leaf", "<u4"), ("offset", "<u4"), ("leaf_start", "<u4"), ("leaf_len", "<u4"), ("local_pos", "<u4"),
                          ("props", "<u2"), ("unit", "<u2"), ("status", "<i4"), ("flags", "<u4")])
assert POS_QUERY_DTYPE.itemsize == 16 and POS_HIT_DTYPE.itemsize == 32
VIEW_LOCAL = 0x7FFFFFFF  # fmt_pos.h FMT_MT_VIEW_LOCAL
POS_F_MARKER, POS_F_END, POS_F_HIDDEN_LOCALLY = 1, 2, 4  # fmt_pos.h FMT_MT_POS_F_*
# include/fmt_range.h (bulk range reads)
RANGE_QUERY_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("ref_seq", "<i4"), ("client", "<i4")])
RANGE_HIT_DTYPE = np.dtype([("text_off", "<u8"), ("units", "<u4"), ("span", "<u4"), ("status", "<i4"), ("pad", "<u4")])
assert RANGE_QUERY_DTYPE.itemsize == 16 and RANGE_HIT_DTYPE.itemsize == 24
RANGE_TO_END = 0xFFFFFFFF  # fmt_range.h FMT_MT_RANGE_TO_END

from .streams import (NO_MARKER, RELPOS_DTYPE, SNAPSHOT_DOC_DTYPE, SNAPSHOT_INFO_DTYPE, SNAPSHOT_SEG_DTYPE,  # noqa: E402
                      STAMP_DTYPE)  # (include/fmt.h layouts)

PROPS_MAX = 8        # fmt.h FMT_MT_PROPS_MAX: entries per prop-set record
PROPS_KEYS_MAX = 128  # fmt.h FMT_MT_PROPS_KEYS_MAX: entries per prop set
PROPS_CONT = 0xFFFFFFFF  # fmt.h FMT_MT_PROPS_CONT: n of a continuation record
MAP_PENDING_MAX_EVENTS = 16384  # fmt.h FMT_MAP_PENDING_MAX_EVENTS: local events per document
PROPSET_DTYPE = np.dtype([("n", "<u4"), ("kv", "<u4", (PROPS_MAX,))])


def propset_entries(table, pid: int) -> tuple:
    """The (key << 16 | value) entries of the prop set whose first record is table[pid]; a set wider
    than PROPS_MAX continues in the following records (fmt.h fmt_mt_propset)."""
    n = int(table[pid]["n"])
    if n <= PROPS_MAX:
        return tuple(int(x) for x in table[pid]["kv"][:n])
    rec = table[pid : pid + (n + PROPS_MAX - 1) // PROPS_MAX]["kv"].reshape(-1)
    return tuple(int(x) for x in rec[:n])
assert PROPSET_DTYPE.itemsize == 36

MAP_SLOT_DTYPE = np.dtype([("value", "<u4"), ("birth_seq", "<u4")])
MAP_ENTRY_DTYPE = np.dtype([("key", "<u4"), ("value", "<u4"), ("birth_seq", "<u4")])  # fmt_map_entry


class FmtMtBatch(ctypes.Structure):
    _fields_ = [
        ("ops", ctypes.c_void_p),
        ("n_ops", ctypes.c_uint64),
        ("doc_op_offsets", ctypes.c_void_p),
        ("n_docs", ctypes.c_uint32),
        ("text", ctypes.c_void_p),
        ("text_len", ctypes.c_uint64),
        ("doc_init", ctypes.c_void_p),
        ("props_off", ctypes.c_void_p),
        ("n_props_ops", ctypes.c_uint32),
        ("props_kv", ctypes.c_void_p),
        ("snapshots", ctypes.c_void_p),
        ("snapshot_segs", ctypes.c_void_p),
        ("n_snapshot_segs", ctypes.c_uint64),
        ("relpos", ctypes.c_void_p),
        ("n_relpos", ctypes.c_uint32),
        ("marker_id_key", ctypes.c_uint32),
        ("snapshot_info", ctypes.c_void_p),
        ("snapshot_stamps", ctypes.c_void_p),
        ("n_snapshot_stamps", ctypes.c_uint64),
        ("adjusts", ctypes.c_void_p),
        ("n_adjusts", ctypes.c_uint32),
        ("n_values", ctypes.c_uint32),
        ("value_num", ctypes.c_void_p),
        ("doc_value_base", ctypes.c_void_p),
    ]


from .streams import ADJUST_DTYPE  # noqa: E402  (include/fmt.h fmt_mt_adjust, 32 bytes)

assert ADJUST_DTYPE.itemsize == 32


class FmtStats(ctypes.Structure):
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("ops", ctypes.c_uint64),
        ("docs", ctypes.c_uint64),
        ("bytes_read", ctypes.c_uint64),
        ("bytes_written", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
    ]


class FmtConfig(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("stream", ctypes.c_void_p),
        ("reserved", ctypes.c_uint32 * 4),
    ]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def batch_struct(batch):
    """Build an fmt_mt_batch over a MergeTreeBatch's numpy arrays; returns (struct, keepalive)."""
    keep = [
        np.ascontiguousarray(batch.ops),
        np.ascontiguousarray(batch.doc_op_offsets, dtype=np.uint64),
        np.ascontiguousarray(batch.text, dtype="<u2"),
        np.ascontiguousarray(batch.doc_init, dtype=np.uint32),
        np.ascontiguousarray(batch.props_off, dtype=np.uint32),
        np.ascontiguousarray(batch.props_kv, dtype=np.uint32) if len(batch.props_kv) else np.zeros(1, np.uint32),
    ]
    snaps = getattr(batch, "snapshots", None)
    segs = getattr(batch, "snapshot_segs", None)
    if snaps is not None:
        keep.append(np.ascontiguousarray(snaps, dtype=SNAPSHOT_DOC_DTYPE))
        keep.append(np.ascontiguousarray(segs, dtype=SNAPSHOT_SEG_DTYPE) if len(segs) else
                    np.zeros(1, dtype=SNAPSHOT_SEG_DTYPE))
    relpos = getattr(batch, "relpos", None)
    rel = np.ascontiguousarray(relpos, dtype=RELPOS_DTYPE) if relpos is not None and len(relpos) else None
    b = FmtMtBatch(
        _ptr(keep[0]), len(keep[0]), _ptr(keep[1]), len(keep[1]) - 1, _ptr(keep[2]), len(keep[2]),
        _ptr(keep[3]), _ptr(keep[4]), len(keep[4]) - 1, _ptr(keep[5]),
        _ptr(keep[6]) if snaps is not None else None, _ptr(keep[7]) if snaps is not None else None,
        len(segs) if snaps is not None else 0,
        _ptr(rel) if rel is not None else None, len(rel) if rel is not None else 0,
        int(getattr(batch, "marker_id_key", NO_MARKER)),
    )
    if rel is not None:
        keep.append(rel)
    info = getattr(batch, "snapshot_info", None)
    if snaps is not None and info is not None:
        inf = np.ascontiguousarray(info, dtype=SNAPSHOT_INFO_DTYPE)
        st = getattr(batch, "snapshot_stamps", None)
        stp = np.ascontiguousarray(st, dtype=STAMP_DTYPE) if st is not None and len(st) else np.zeros(1, STAMP_DTYPE)
        b.snapshot_info, b.snapshot_stamps = _ptr(inf), _ptr(stp)
        b.n_snapshot_stamps = 0 if st is None else len(st)
        keep += [inf, stp]
    adj = getattr(batch, "adjusts", None)
    if adj is not None and len(adj):
        a = np.ascontiguousarray(adj, dtype=ADJUST_DTYPE)
        vn = np.ascontiguousarray(batch.value_num, dtype=np.float64)
        b.adjusts, b.n_adjusts, b.value_num, b.n_values = _ptr(a), len(a), _ptr(vn), len(vn)
        keep += [a, vn]
    vb = getattr(batch, "value_base", None)
    if vb is not None:
        vba = np.ascontiguousarray(vb, dtype=np.uint32)
        b.doc_value_base = _ptr(vba)
        keep.append(vba)
    return b, keep


class EngineUnavailable(RuntimeError):
    """libfmt.so is missing or no gfx950 device is usable. There is deliberately no fallback."""


class FmtSummaryTiming(ctypes.Structure):  # fmt_summary_timing
    _fields_ = [("kernel_ms", ctypes.c_double), ("fetch_ms", ctypes.c_double), ("format_ms", ctypes.c_double),
                ("bytes", ctypes.c_uint64), ("threads", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class FmtMapSummaryTiming(ctypes.Structure):  # fmt_map_summary_timing (include/fmt_map_summary.h)
    _fields_ = [("kernel_ms", ctypes.c_double), ("fetch_ms", ctypes.c_double), ("format_ms", ctypes.c_double),
                ("bytes", ctypes.c_uint64), ("threads", ctypes.c_uint32), ("host_ordered_docs", ctypes.c_uint32)]


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fmt error {STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


_libs = {}


def lib(path: str | None = None) -> ctypes.CDLL:
    """The engine library (default: the in-tree libfmt.so; `path` selects an experimental build)."""
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise EngineUnavailable(f"{path} not built (run __graft_entry__.build())")
        L = ctypes.CDLL(path)
        P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.fmt_open.argtypes = [ctypes.POINTER(FmtConfig), ctypes.POINTER(P)]
        L.fmt_close.argtypes = [P]
        L.fmt_last_error.argtypes = [P]
        L.fmt_last_error.restype = ctypes.c_char_p
        L.fmt_sync.argtypes = [P]
        L.fmt_get_stats.argtypes = [P, ctypes.POINTER(FmtStats)]
        L.fmt_device_info.argtypes = [P, ctypes.c_char_p, ctypes.c_size_t]
        L.fmt_map_load.argtypes = [P, P, U64, P, U32, U32]
        L.fmt_map_run.argtypes = [P]
        L.fmt_map_fetch.argtypes = [P, P]
        L.fmt_map_replay_device.argtypes = [P, P, P, U32, U32, P]
        L.fmt_map_check.argtypes = [P]
        L.fmt_map_load_sparse.argtypes = [P, P, U64, P, U32, U32]
        L.fmt_mt_summarize_legacy.argtypes = [P, P, U32, P, U32, U32, U32, ctypes.POINTER(FmtSummaryTiming)]
        L.fmt_mt_summary_blobs.argtypes = [P, U32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
                                           ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t)]
        L.fmt_map_run_sparse.argtypes = [P]
        L.fmt_map_fetch_sparse.argtypes = [P, P, P, U64, ctypes.POINTER(U64)]
        L.fmt_mt_load.argtypes = [P, ctypes.POINTER(FmtMtBatch)]
        L.fmt_mt_run.argtypes = [P]
        L.fmt_mt_fetch_headers.argtypes = [P, P]
        L.fmt_mt_fetch_doc.argtypes = [P, U32, P, U32, P, U32, P, U32]
        L.fmt_mt_fetch_catchup.argtypes = [P, U32, P, U32]
        L.fmt_mt_fetch_catchup_all.argtypes = [P, P, P, U64]
        L.fmt_mt_fetch_remove_order.argtypes = [P, U32, P, U32]
        L.fmt_mt_fetch_numbers.argtypes = [P, U32, P, U32, ctypes.POINTER(U32)]
        L.fmt_mt_capacity.argtypes = [ctypes.POINTER(U32)] * 3
        for name, args in (("fmt_mt_state_digest", [P, P]), ("fmt_mt_fetch_legacy_props", [P, U32, P, U32]),
                           ("fmt_mt_fetch_rm_clients_hi", [P, U32, P, U32]),
                           ("fmt_mt_fetch_rm_clients_hi2", [P, U32, P, U32]),
                           ("fmt_map_pending_run", [P, P, U64, P]),
                           ("fmt_map_run_sparse_tiered", [P]),
                           ("fmt_mt_fetch_regen", [P, U32, P, U32, P, U32, ctypes.POINTER(U32), ctypes.POINTER(U32)]),
                           ("fmt_map_pending_fetch", [P, P, P, P, U64, ctypes.POINTER(U64)]),
                           ("fmt_mt_summarize_v1", [P, P, U32, P, U32, P, P, U32, U32, ctypes.POINTER(FmtSummaryTiming)]),
                           ("fmt_mt_summary_v1_blobs", [P, U32, ctypes.POINTER(ctypes.c_char_p),
                                                        ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(U32)]),
                           ("fmt_mt_summary_v1_body", [P, U32, U32, ctypes.POINTER(ctypes.c_char_p),
                                                       ctypes.POINTER(ctypes.c_size_t)]),
                           ("fmt_map_summarize", [P, P, U32, P, U32, U32, ctypes.POINTER(FmtMapSummaryTiming)]),
                           ("fmt_map_summary_blobs", [P, U32, ctypes.POINTER(ctypes.c_char_p),
                                                      ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(U32)]),
                           ("fmt_map_summary_blob", [P, U32, U32, ctypes.POINTER(ctypes.c_char_p),
                                                     ctypes.POINTER(ctypes.c_size_t)]),
                           ("fmt_mt_fetch_text_all", [P, ctypes.c_uint16, P, P, U64]),
                           ("fmt_mt_text_tile_leaves", []),
                           ("fmt_internal_text_plan", [P, U32, U32, P, ctypes.POINTER(P), ctypes.POINTER(U64)]),
                           ("fmt_mt_fetch_prop_runs_all", [P, P, P, U64]),
                           ("fmt_mt_fetch_props_all", [P, P, P, U64]),
                           ("fmt_internal_runs_plan", [P, U32, U32, P, U64, ctypes.POINTER(P), ctypes.POINTER(U64)]),
                           ("fmt_mt_query_positions", [P, P, P, U64, P]),
                           ("fmt_internal_pos_plan", [P, U32, U32, U32, P, P, U64, P, U64, P, ctypes.POINTER(P),
                                                      ctypes.POINTER(U64)]),
                           ("fmt_mt_fetch_text_ranges", [P, ctypes.c_uint16, P, P, U64, P, P, P, U64]),
                           ("fmt_internal_range_plan", [P, U32, U32, U32, U32, P, P, U64, P, U64, P, U64, P, ctypes.POINTER(U64),
                                                        ctypes.POINTER(P), ctypes.POINTER(U64)]),
                           ("fmt_internal_map_summary_arrays", [P, P, P, P, U64]),
                           ("fmt_internal_map_summary_host_only", [P, ctypes.c_int])):
            if path == LIB_PATH or hasattr(L, name):  # (older experimental builds may lack them)
                getattr(L, name).argtypes = args
        if hasattr(L, "fmt_mt_text_tile_leaves"):
            L.fmt_mt_text_tile_leaves.restype = U32
        _libs[path] = L
    return _libs[path]


EXPORTED_SYMBOLS = [
    "fmt_open", "fmt_close", "fmt_last_error", "fmt_sync", "fmt_get_stats", "fmt_device_info",
    "fmt_map_load", "fmt_map_run", "fmt_map_fetch", "fmt_map_replay_device", "fmt_map_check",
    "fmt_map_load_sparse", "fmt_map_run_sparse", "fmt_map_fetch_sparse",
    "fmt_mt_summarize_legacy", "fmt_mt_summary_blobs",
    "fmt_mt_load", "fmt_mt_run", "fmt_mt_fetch_headers", "fmt_mt_fetch_doc", "fmt_mt_fetch_catchup",
    "fmt_mt_fetch_catchup_all", "fmt_mt_fetch_remove_order", "fmt_mt_fetch_numbers", "fmt_mt_capacity",
    "fmt_mt_state_digest", "fmt_mt_fetch_legacy_props", "fmt_map_pending_run", "fmt_map_pending_fetch",
    "fmt_mt_fetch_regen", "fmt_mt_fetch_rm_clients_hi", "fmt_mt_fetch_rm_clients_hi2",
]


# include/fmt_v1.h (bulk SnapshotV1 summaries)
EXPORTED_SYMBOLS_V1 = ["fmt_mt_summarize_v1", "fmt_mt_summary_v1_blobs", "fmt_mt_summary_v1_body"]
# include/fmt_map_tiered.h (the sparse map path with its HBM tier)
EXPORTED_SYMBOLS_MAP_TIERED = ["fmt_map_run_sparse_tiered"]
# include/fmt_map_summary.h (bulk SharedMap summaries of the sparse path)
EXPORTED_SYMBOLS_MAP_SUMMARY = ["fmt_map_summarize", "fmt_map_summary_blobs", "fmt_map_summary_blob"]
# include/fmt_text.h (bulk getText)
EXPORTED_SYMBOLS_TEXT = ["fmt_mt_fetch_text_all", "fmt_mt_text_tile_leaves"]
# include/fmt_runs.h (bulk property runs)
EXPORTED_SYMBOLS_RUNS = ["fmt_mt_fetch_prop_runs_all", "fmt_mt_fetch_props_all"]
# include/fmt_pos.h (bulk position queries)
EXPORTED_SYMBOLS_POS = ["fmt_mt_query_positions"]
# include/fmt_range.h (bulk range reads)
EXPORTED_SYMBOLS_RANGE = ["fmt_mt_fetch_text_ranges"]
MAP_SUMMARY_CONTENT = 0xFFFFFFFF    # tag of an ordered entry that stays in the header's "content"
MAP_SUMMARY_DEVICE_MAX = 2048       # live entries per document the device tier orders (csrc/map_sum_plan.h)


def _c_strings(strs):
    enc = [x.encode("utf-8") for x in strs]
    return (ctypes.c_char_p * max(len(enc), 1))(*enc), len(enc)


def v1_format(segs, text, propsets, rm_order, keys, values, client_names, min_seq, cur_seq, chunk=10000, numbers=None):
    """fmt_internal_v1_format: the bulk SnapshotV1 path's host formatter over one document's segment
    records (V1_SEG_DTYPE, summary.v1_segment_records), no device needed. Returns (header, [bodies])."""
    from .streams import js_quote

    segs = np.ascontiguousarray(segs, dtype=V1_SEG_DTYPE)
    text = np.ascontiguousarray(text, dtype="<u2")
    propsets = np.ascontiguousarray(propsets, dtype=PROPSET_DTYPE)
    rm_order = np.ascontiguousarray(rm_order, dtype=RM_ORDER_DTYPE)
    nums = None if numbers is None or len(numbers) == 0 else np.ascontiguousarray(numbers, dtype=np.float64)
    ka, nk = _c_strings(js_quote(k) for k in keys)
    va, nv = _c_strings(values)
    na, nn = _c_strings(js_quote(c) for c in client_names)
    P, U32, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    f = lib().fmt_internal_v1_format
    f.argtypes = [P, U32, P, P, U32, P, U32, P, U32, P, U32, P, U32, P, U32, I32, I32, U32, ctypes.POINTER(P),
                  ctypes.POINTER(P), ctypes.POINTER(U32)]
    out, ends, n = P(), P(), U32()
    rc = f(_ptr(segs), len(segs), _ptr(text), _ptr(propsets), len(propsets), _ptr(rm_order), len(rm_order),
           None if nums is None else _ptr(nums), 0 if nums is None else len(nums), ka, nk, va, nv, na, nn, min_seq, cur_seq,
           chunk, ctypes.byref(out), ctypes.byref(ends), ctypes.byref(n))
    if rc != FMT_OK:
        raise EngineError(rc, "fmt_internal_v1_format")
    e = [0] + list((ctypes.c_uint64 * n.value).from_address(ends.value))
    blobs = [ctypes.string_at(out.value + e[k], e[k + 1] - e[k]).decode("utf-8") for k in range(n.value)]
    return blobs[0], blobs[1:]


RUN_DTYPE = np.dtype([("len", "<u4"), ("props", "<u2"), ("flags", "<u2")])  # fmt_kernels::SumRun (csrc/kernels.h)
assert RUN_DTYPE.itemsize == 8


def legacy_format(runs, text, propsets, keys, values, min_seq, chunk=10000, numbers=None):
    """fmt_internal_legacy_format: the bulk legacy path's host formatter over one document's runs
    (RUN_DTYPE, summary.legacy_run_records), no device needed. Returns (header, body or None)."""
    from .streams import js_quote

    runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
    text = np.ascontiguousarray(text, dtype="<u2")
    propsets = np.ascontiguousarray(propsets, dtype=PROPSET_DTYPE)
    nums = None if numbers is None or len(numbers) == 0 else np.ascontiguousarray(numbers, dtype=np.float64)
    ka, nk = _c_strings(js_quote(k) for k in keys)
    va, nv = _c_strings(values)
    P, U32, I32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    f = lib().fmt_internal_legacy_format
    f.argtypes = [P, U32, P, P, U32, P, U32, P, U32, P, U32, I32, U32, ctypes.POINTER(P), ctypes.POINTER(P),
                  ctypes.POINTER(U32)]
    out, ends, n = P(), P(), U32()
    rc = f(_ptr(runs), len(runs), _ptr(text), _ptr(propsets), len(propsets), None if nums is None else _ptr(nums),
           0 if nums is None else len(nums), ka, nk, va, nv, min_seq, chunk, ctypes.byref(out), ctypes.byref(ends),
           ctypes.byref(n))
    if rc != FMT_OK:
        raise EngineError(rc, "fmt_internal_legacy_format")
    e = [0] + list((ctypes.c_uint64 * n.value).from_address(ends.value))
    blobs = [ctypes.string_at(out.value + e[k], e[k + 1] - e[k]).decode("utf-8") for k in range(n.value)]
    return blobs[0], (blobs[1] if len(blobs) > 1 else None)


def _map_summary_host(counts, entries, keys, values, threads):
    from .streams import js_quote

    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    entries = np.ascontiguousarray(entries, dtype=MAP_ENTRY_DTYPE)
    n = int(counts.sum(dtype=np.uint64))
    if len(entries) < n:
        raise ValueError("fewer entries than counts name")
    ka, nk = _c_strings(js_quote(k) for k in keys)
    va, nv = _c_strings(values)
    ordered = np.zeros(max(n, 1), dtype=MAP_ENTRY_DTYPE)
    tags = np.zeros(max(n, 1), dtype=np.uint32)
    n_blobs = np.zeros(max(len(counts), 1), dtype=np.uint32)
    status = np.zeros(max(len(counts), 1), dtype=np.int32)
    P, U32 = ctypes.c_void_p, ctypes.c_uint32
    f = lib().fmt_internal_map_summary_format
    f.argtypes = [P, P, U32, P, U32, P, U32, U32, P, P, P, P, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P)]
    docs, piece_at, ends = P(), P(), P()
    rc = f(_ptr(counts), _ptr(entries), len(counts), ka, nk, va, nv, threads, _ptr(ordered), _ptr(tags), _ptr(n_blobs),
           _ptr(status), ctypes.byref(docs), ctypes.byref(piece_at), ctypes.byref(ends))
    if rc != FMT_OK:
        raise EngineError(rc, "fmt_internal_map_summary_format")
    nd = len(counts)
    out = []
    if nd:
        at = np.ctypeslib.as_array(ctypes.cast(piece_at, ctypes.POINTER(ctypes.c_uint64)), (nd + 1,))
        ptrs = np.ctypeslib.as_array(ctypes.cast(docs, ctypes.POINTER(ctypes.c_uint64)), (nd,))
        e = np.ctypeslib.as_array(ctypes.cast(ends, ctypes.POINTER(ctypes.c_uint64)), (max(int(at[nd]), 1),))
        for d in range(nd):
            if status[d] != FMT_OK:
                out.append(EngineError(int(status[d]), f"document {d}: a key or value id outside the tables"))
                continue
            cut = [0] + [int(x) for x in e[int(at[d]) : int(at[d + 1])]]
            pieces = [ctypes.string_at(int(ptrs[d]) + cut[k], cut[k + 1] - cut[k]).decode("utf-8") for k in range(len(cut) - 1)]
            out.append((pieces[0], pieces[1:]))
    return out, ordered[:n], tags[:n], n_blobs[:nd], status[:nd]


def map_summary_format(counts, entries, keys, values, threads: int = 0):
    """fmt_internal_map_summary_format: fmt_map_summarize's host half (csrc/map_sum_plan.h: tables, JS
    object order, blob scan, formatter) over fetched sparse entries (Engine.map_fetch_sparse's counts and
    birth-ordered entries), no device needed. Returns one item per document: (header, [blob0, ...]), or
    an EngineError (not raised) for a document with a key or value id outside `keys` / `values`."""
    return _map_summary_host(counts, entries, keys, values, threads)[0]


def map_summary_order(counts, entries, keys, values, threads: int = 0):
    """The same hook's arrays: (ordered entries, tags, n_blobs[n_docs], status[n_docs]), the entries of
    all documents packed in document order, each document's in summary order; tags[i] is the blob the
    entry lands in, MAP_SUMMARY_CONTENT for the header. What Engine.map_summary_arrays is compared to."""
    return _map_summary_host(counts, entries, keys, values, threads)[1:]


class MtPlanResult:
    """What mt_plan read back: `status`, `message` (None: FMT_OK) and the plan of csrc/mt_plan.h MtPlan
    as attributes (numpy arrays and Python scalars; loc_offs as (6, n_docs + 1) or empty)."""


def mt_plan(batch, struct=None) -> MtPlanResult:
    """fmt_internal_mt_plan: fmt_mt_load's host half over `batch` (validation, slab sizing, routing), no
    device needed. A refused batch reports its status and message beside the plan of the calling
    thread's last valid batch. struct: an fmt_mt_batch to plan instead of batch_struct(batch)."""
    b, keep = (struct, None) if struct is not None else batch_struct(batch)
    P = ctypes.c_void_p
    f = lib().fmt_internal_mt_plan
    f.argtypes = [ctypes.POINTER(FmtMtBatch), ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(P),
                  ctypes.POINTER(ctypes.c_uint64)]
    err, out, n = ctypes.c_char_p(), P(), ctypes.c_uint64()
    r = MtPlanResult()
    r.status = f(ctypes.byref(b), ctypes.byref(err), ctypes.byref(out), ctypes.byref(n))
    r.message = err.value.decode() if err.value else None
    w = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64)), (n.value,)).copy()
    r.insert_chars, r.init_chars, r.catchup_ops, r.rm_order_ops, flags, r.n_docs = (int(x) for x in w[:6])
    r.obliterates, r.local, r.hi_clients, r.any_adjust = (bool(flags & k) for k in (1, 2, 4, 8))
    at = 6
    for name in ("cu_offs", "rm_offs", "num_offs", "pm_offs", "loc_offs", "num_sorted", "num_sorted_id",
                 "num_sorted_offs", "load_segs", "seg_props", "doc_chars", "start_seg", "huge_docs", "refused"):
        width = {"start_seg": 3, "refused": 5}.get(name, 1)
        cnt = int(w[at]) * width
        setattr(r, name, w[at + 1 : at + 1 + cnt])
        at += 1 + cnt
    assert at == len(w)
    r.num_sorted = r.num_sorted.view(np.float64)
    r.loc_offs = r.loc_offs.reshape(6, -1) if len(r.loc_offs) else r.loc_offs
    r.start_seg = r.start_seg.reshape(-1, 3)
    r.refused = r.refused.view(np.int64).reshape(-1, 5)  # doc, status, fail_seq, cur_seq, min_seq
    return r


MT_TIERS = ("micro", "compact", "small", "large")  # csrc/mt_route.h MtTier
MT_LIST_KINDS = ("none", "every", "caller", "microUp", "compactUp", "toLarge", "ordered", "round")  # MtListKind
MT_DEAL_KINDS = ("compact", "small", "large", "micro", "round")  # MtDealKind


def mt_variant_key(ob=False, rm=False, adj=False, loc=False) -> int:
    """csrc/mt_route.h MtVariant::key"""
    return int(ob) | int(rm) << 1 | int(adj) << 2 | int(loc) << 3


class MtRouteResult:
    """A route read back (csrc/mt_route.h routeWords): the five out-slab booleans (`tiers_ckpt`, `large_ckpt`,
    `large_resumes_small`, `large_huge_ckpt`, `large_local`), `large` (the large pass's variant key), `rounds`,
    `nominal_launches` ({(large_ran, grew): launches}), `steps` (dicts: tier, variant, in / up / down /
    order_into as names with "round(r,k)" for the step-down lists, deal likewise, descend) and `kernels`
    (the (tier, variant key) pairs that exist as kernels)."""


def parse_mt_route(words) -> MtRouteResult:
    w = [int(x) for x in words]
    r = MtRouteResult()
    r.tiers_ckpt, r.large_ckpt, r.large_resumes_small, r.large_huge_ckpt, r.large_local = (bool(x) for x in w[:5])
    r.large, r.rounds = w[5], w[6]
    r.nominal_launches = {(False, False): w[7], (True, False): w[8], (False, True): w[9], (True, True): w[10]}

    def name(kinds, kind, rr, k):
        return f"round({rr},{k})" if kinds[kind] == "round" else kinds[kind]

    at, r.steps = 12, []
    for _ in range(w[11]):
        s = w[at:at + 16]
        r.steps.append({"tier": MT_TIERS[s[0]], "variant": s[1], "in": name(MT_LIST_KINDS, *s[2:5]),
                        "up": name(MT_LIST_KINDS, *s[5:8]), "down": name(MT_LIST_KINDS, *s[8:11]),
                        "order_into": MT_LIST_KINDS[s[11]], "deal": name(MT_DEAL_KINDS, *s[12:15]), "descend": bool(s[15])})
        at += 16
    r.kernels = {(MT_TIERS[w[at + 1 + 2 * i]], w[at + 2 + 2 * i]) for i in range(w[at])}
    assert at + 1 + 2 * w[at] == len(w)
    return r


def mt_route(batch, ckpt_slab=True, desc_slab=True, rounds=0, local_path=-1, struct=None) -> MtRouteResult:
    """fmt_internal_mt_route: the route fmt_mt_load plans for `batch` when the checkpoint / step-down slabs
    are (not) allocated, no device needed. rounds / local_path: other than the build's. Raises EngineError
    for a batch fmt_mt_load refuses."""
    b, keep = (struct, None) if struct is not None else batch_struct(batch)
    P = ctypes.c_void_p
    f = lib().fmt_internal_mt_route
    f.argtypes = [ctypes.POINTER(FmtMtBatch)] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(P),
                                                                     ctypes.POINTER(ctypes.c_uint64)]
    err, out, n = ctypes.c_char_p(), P(), ctypes.c_uint64()
    rc = f(ctypes.byref(b), int(ckpt_slab), int(desc_slab), rounds, local_path, ctypes.byref(err), ctypes.byref(out),
           ctypes.byref(n))
    if rc != FMT_OK:
        raise EngineError(rc, err.value.decode() if err.value else "fmt_internal_mt_route")
    return parse_mt_route(np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint32)), (n.value,)).copy())


MT_VALUE_COMPUTED = 0x8000  # fmt.h FMT_MT_VALUE_COMPUTED: value ids at or above it index the document's numbers


def _computed(x):
    x = float(x)
    return int(x) if x.is_integer() else x


class TextPlanResult:
    """What text_plan read back (csrc/text_plan.h): `items` ((n, 3): doc, first leaf, leaves), `doc_first`
    (n_docs + 1: each document's first item) and, when tile units were given, `offsets` (n_docs + 1) and
    `tile_base` (one per item)."""


def text_tile_leaves() -> int:
    """fmt_mt_text_tile_leaves: leaves per work item of the bulk text kernels."""
    return int(lib().fmt_mt_text_tile_leaves())


def text_plan(headers, tile_leaves: int = 0, tile_units=None) -> TextPlanResult:
    """fmt_internal_text_plan: fmt_mt_fetch_text_all's host half over result headers (DOC_RESULT_DTYPE),
    no device needed. tile_leaves 0: the kernels' tile. tile_units (one per work item): also the offsets
    and tile bases their exclusive prefix gives."""
    hdr = np.ascontiguousarray(headers, dtype=DOC_RESULT_DTYPE)
    units = None if tile_units is None else np.ascontiguousarray(tile_units, dtype=np.uint64)
    P = ctypes.c_void_p
    out, n = P(), ctypes.c_uint64()
    f = lib().fmt_internal_text_plan

    def call(u):
        rc = f(_ptr(hdr) if len(hdr) else None, len(hdr), tile_leaves, u, ctypes.byref(out), ctypes.byref(n))
        if rc != FMT_OK:
            raise EngineError(rc, "fmt_internal_text_plan")
        return np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64)), (n.value,)).copy()

    w = call(None)
    ni = int(w[0])
    if units is not None:
        if len(units) != ni:
            raise ValueError(f"{len(units)} tile units for {ni} work items")
        w = call(_ptr(units) if ni else _ptr(np.zeros(1, np.uint64)))
    r = TextPlanResult()
    r.items = w[1 : 1 + 3 * ni].reshape(ni, 3)
    at = 1 + 3 * ni
    r.doc_first = w[at : at + len(hdr) + 1]
    at += len(hdr) + 1
    r.offsets = r.tile_base = None
    if units is not None:
        r.offsets = w[at : at + len(hdr) + 1]
        at += len(hdr) + 1
        r.tile_base = w[at : at + ni]
        at += ni
    assert at == len(w)
    return r


RUN_END_MARKER, RUN_END_HAS = 1 << 16, 1 << 17  # csrc/runs_plan.h RunTile.first / last
RUN_CONTINUES, RUN_CLOSES = 1, 2                # csrc/runs_plan.h RunTileBase.flags
RUN_TILE_DTYPE = np.dtype([("units", "<u4"), ("heads", "<u4"), ("tail", "<u4"), ("first", "<u4"), ("last", "<u4")])


class RunsPlanResult:
    """What runs_plan read back (csrc/runs_plan.h stitchRuns): `offsets` (n_docs + 1: each document's first
    run) and per work item `run_base`, `pos_base`, `open_start`, `flags` (RUN_CONTINUES | RUN_CLOSES)."""


def runs_plan(headers, tiles, tile_leaves: int = 0) -> RunsPlanResult:
    """fmt_internal_runs_plan: fmt_mt_fetch_prop_runs_all's host half over result headers (DOC_RESULT_DTYPE)
    and one pass-1 report (RUN_TILE_DTYPE) per work item of text_plan(headers, tile_leaves), no device
    needed."""
    hdr = np.ascontiguousarray(headers, dtype=DOC_RESULT_DTYPE)
    t = np.ascontiguousarray(tiles, dtype=RUN_TILE_DTYPE)
    P = ctypes.c_void_p
    out, n = P(), ctypes.c_uint64()
    rc = lib().fmt_internal_runs_plan(_ptr(hdr) if len(hdr) else None, len(hdr), tile_leaves, _ptr(t) if len(t) else None,
                                      len(t), ctypes.byref(out), ctypes.byref(n))
    if rc != FMT_OK:
        raise EngineError(rc, "fmt_internal_runs_plan")
    w = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64)), (n.value,)).copy()
    ni = int(w[0])
    r = RunsPlanResult()
    r.offsets = w[1 : 2 + len(hdr)]
    per = w[2 + len(hdr) :].reshape(ni, 4)
    r.run_base, r.pos_base, r.open_start, r.flags = (per[:, k].copy() for k in range(4))
    return r


class PosPlanResult:
    """What pos_plan read back (csrc/pos_plan.h): `hits` (POS_HIT_DTYPE, one per query, as the host leaves
    them: statuses, ends, and FMT_E_DATA where the device is to write), `views` ((n, 4) int64: doc, ref_seq,
    client, first item), `items` ((n, 4): doc, first leaf, leaves, view) and, when tile units were given,
    `dev` ((n, 9) int64: doc, first leaf, leaves, pos within the tile, ref_seq, client, view base, local
    base, index of the query's record)."""


def pos_plan(headers, queries, q_offsets, tile_units=None, obliterates: bool = False, tile_leaves: int = 0) -> PosPlanResult:
    """fmt_internal_pos_plan: fmt_mt_query_positions' host half over result headers (DOC_RESULT_DTYPE), no
    device needed. tile_leaves 0: the kernels' tile. tile_units ((n_items, 2): units in the view, units in
    the local view): also the tile lookup of every query. Raises EngineError(FMT_E_USAGE) for malformed
    q_offsets."""
    hdr = np.ascontiguousarray(headers, dtype=DOC_RESULT_DTYPE)
    q = np.ascontiguousarray(queries, dtype=POS_QUERY_DTYPE)
    offs = np.ascontiguousarray(q_offsets, dtype=np.uint64)
    if len(offs) != len(hdr) + 1:
        raise EngineError(FMT_E_USAGE, f"{len(offs)} q_offsets for {len(hdr)} documents")
    units = None if tile_units is None else np.ascontiguousarray(tile_units, dtype=np.uint64).reshape(-1, 2)
    hits = np.zeros(max(len(q), 1), dtype=POS_HIT_DTYPE)
    P = ctypes.c_void_p
    out, n = P(), ctypes.c_uint64()
    rc = lib().fmt_internal_pos_plan(_ptr(hdr) if len(hdr) else None, len(hdr), 1 if obliterates else 0, tile_leaves, _ptr(offs),
                                     _ptr(q) if len(q) else None, len(q),
                                     None if units is None else _ptr(units if len(units) else np.zeros(2, np.uint64)),
                                     0 if units is None else len(units), _ptr(hits), ctypes.byref(out), ctypes.byref(n))
    if rc != FMT_OK:
        raise EngineError(rc, "fmt_internal_pos_plan")
    w = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64)), (n.value,)).copy().view(np.int64)
    r = PosPlanResult()
    r.hits = hits[: len(q)]
    nv = int(w[0])
    r.views = w[1 : 1 + 4 * nv].reshape(nv, 4)
    at = 1 + 4 * nv
    ni = int(w[at])
    r.items = w[at + 1 : at + 1 + 4 * ni].reshape(ni, 4)
    at += 1 + 4 * ni
    r.dev = None
    if units is not None:
        ndev = int(w[at])
        r.dev = w[at + 1 : at + 1 + 9 * ndev].reshape(ndev, 9)
        at += 1 + 9 * ndev
    assert at == len(w)
    return r


class RangePlanResult:
    """What range_plan read back (csrc/range_plan.h): `hits` (RANGE_HIT_DTYPE, one per query, as the host
    leaves them), `views` ((n, 4) int64: doc, ref_seq, client, first item), `view_items` ((n, 4): doc, first
    leaf, leaves, view: the sizing pass's work items); when tile units were given, `items` ((n, 8) int64: doc,
    first leaf, leaves, lo, hi, ref_seq, client, query); and, when item units were given or there is a
    placeholder, `item_base` (each item's first unit in the packed text) and `total`."""


def range_plan(headers, queries, q_offsets, tile_units=None, item_units=None, placeholder: int = 0, obliterates: bool = False,
               tile_leaves: int = 0) -> RangePlanResult:
    """fmt_internal_range_plan: fmt_mt_fetch_text_ranges' host half over result headers (DOC_RESULT_DTYPE), no
    device needed. tile_leaves 0: the kernels' tile. tile_units ((n_view_items, 2): units in the view, units
    in the local view): also the cut of every range into items. item_units (one per item: its text units;
    not needed with a placeholder): also the offsets. Raises EngineError(FMT_E_USAGE) for malformed
    q_offsets."""
    hdr = np.ascontiguousarray(headers, dtype=DOC_RESULT_DTYPE)
    q = np.ascontiguousarray(queries, dtype=RANGE_QUERY_DTYPE)
    offs = np.ascontiguousarray(q_offsets, dtype=np.uint64)
    if len(offs) != len(hdr) + 1:
        raise EngineError(FMT_E_USAGE, f"{len(offs)} q_offsets for {len(hdr)} documents")
    units = None if tile_units is None else np.ascontiguousarray(tile_units, dtype=np.uint64).reshape(-1, 2)
    iunits = None if item_units is None else np.ascontiguousarray(item_units, dtype=np.uint64).reshape(-1)
    hits = np.zeros(max(len(q), 1), dtype=RANGE_HIT_DTYPE)
    P = ctypes.c_void_p
    out, n, total = P(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib().fmt_internal_range_plan(_ptr(hdr) if len(hdr) else None, len(hdr), 1 if obliterates else 0, tile_leaves, placeholder,
                                       _ptr(offs), _ptr(q) if len(q) else None, len(q),
                                       None if units is None else _ptr(units if len(units) else np.zeros(2, np.uint64)),
                                       0 if units is None else len(units),
                                       None if iunits is None else _ptr(iunits if len(iunits) else np.zeros(1, np.uint64)),
                                       0 if iunits is None else len(iunits), _ptr(hits), ctypes.byref(total), ctypes.byref(out),
                                       ctypes.byref(n))
    if rc != FMT_OK:
        raise EngineError(rc, "fmt_internal_range_plan")
    w = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64)), (n.value,)).copy().view(np.int64)
    r = RangePlanResult()
    r.hits = hits[: len(q)]
    nv = int(w[0])
    r.views = w[1 : 1 + 4 * nv].reshape(nv, 4)
    at = 1 + 4 * nv
    ni = int(w[at])
    r.view_items = w[at + 1 : at + 1 + 4 * ni].reshape(ni, 4)
    at += 1 + 4 * ni
    r.items = r.item_base = r.total = None
    if units is not None:
        nr = int(w[at])
        r.items = w[at + 1 : at + 1 + 8 * nr].reshape(nr, 8)
        at += 1 + 8 * nr
        if placeholder != 0 or iunits is not None:
            r.item_base = w[at : at + nr]
            at += nr
            r.total = int(total.value)
    assert at == len(w)
    return r


class MapLargePlanResult:
    """What map_large_plan read back (csrc/map_plan.h MapLargePlan): `status`, `message` (None: FMT_OK),
    `tile`, `scratch_bytes`, `slots`, `ops`, `regions` (name -> first 32-bit word: key, first, del, last,
    value, op_slot, tile_count, clear), `docs` (one row per overflowing document: doc, n_ops, slots,
    table_off, op_slot_off, first_tile, n_tiles, shift), `tile_doc` (index into docs) and `tile_first`."""


MAP_LARGE_REGIONS = ("key", "first", "del", "last", "value", "op_slot", "tile_count", "clear")
MAP_LARGE_DOC_FIELDS = ("doc", "n_ops", "slots", "table_off", "op_slot_off", "first_tile", "n_tiles", "shift")


def map_large_plan(op_counts, overflow_docs) -> MapLargePlanResult:
    """fmt_internal_map_large_plan: the host half of the sparse map path's HBM tier over a batch of
    documents with `op_counts` ops each, of which `overflow_docs` (ascending) overflowed the LDS tier.
    No device needed."""
    offs = np.zeros(len(op_counts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.asarray(op_counts, dtype=np.uint64))
    ovf = np.ascontiguousarray(overflow_docs, dtype=np.uint32)
    P = ctypes.c_void_p
    f = lib().fmt_internal_map_large_plan
    f.argtypes = [P, ctypes.c_uint32, P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(P),
                  ctypes.POINTER(ctypes.c_uint64)]
    err, out, n = ctypes.c_char_p(), P(), ctypes.c_uint64()
    r = MapLargePlanResult()
    r.status = f(_ptr(offs), len(op_counts), _ptr(ovf) if len(ovf) else None, len(ovf), ctypes.byref(err),
                 ctypes.byref(out), ctypes.byref(n))
    r.message = err.value.decode() if err.value else None
    w = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64)), (n.value,)).copy()
    r.tile, r.scratch_bytes, r.slots, r.ops = (int(x) for x in w[:4])
    r.regions = {name: int(x) for name, x in zip(MAP_LARGE_REGIONS, w[4:12])}
    at = 12
    got = []
    for width in (len(MAP_LARGE_DOC_FIELDS), 1, 1):
        cnt = int(w[at]) * width
        got.append(w[at + 1 : at + 1 + cnt])
        at += 1 + cnt
    assert at == len(w)
    r.docs = got[0].reshape(-1, len(MAP_LARGE_DOC_FIELDS))
    r.tile_doc, r.tile_first = got[1], got[2]
    return r


def capacity():
    a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    lib().fmt_mt_capacity(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


class Engine:
    """One fmt_ctx bound to one HIP device (one per process/rank)."""

    def __init__(self, device: int = 0, stream: int | None = None, lib_path: str | None = None):
        self.L = L = lib(lib_path)
        cfg = FmtConfig(device, 0, stream, (ctypes.c_uint32 * 4)())
        h = ctypes.c_void_p()
        rc = L.fmt_open(ctypes.byref(cfg), ctypes.byref(h))
        if rc != FMT_OK:
            msg = L.fmt_last_error(h).decode() if h.value else "fmt_open failed"
            if h.value:
                L.fmt_close(h)
            raise EngineUnavailable(msg)
        self.h = h
        self._keep = None

    def close(self):
        if self.h:
            self.L.fmt_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != FMT_OK:
            raise EngineError(rc, self.L.fmt_last_error(self.h).decode())

    def sync(self):
        self._check(self.L.fmt_sync(self.h))

    def stats(self) -> FmtStats:
        s = FmtStats()
        self._check(self.L.fmt_get_stats(self.h, ctypes.byref(s)))
        return s

    def device_info(self) -> str:
        buf = ctypes.create_string_buffer(256)
        self.L.fmt_device_info(self.h, buf, 256)
        return buf.value.decode()

    # ---- SharedMap
    def map_load(self, batch):
        ops = np.ascontiguousarray(batch.ops)
        offs = np.ascontiguousarray(batch.doc_op_offsets, dtype=np.uint64)
        self._check(self.L.fmt_map_load(self.h, _ptr(ops), len(ops), _ptr(offs), batch.n_docs, batch.key_bound))
        self._map_shape = (batch.n_docs, batch.key_bound)

    def map_run(self):
        self._check(self.L.fmt_map_run(self.h))

    def map_replay_device(self, d_ops: int, d_offsets: int, n_docs: int, key_bound: int, d_out: int):
        """fmt_map_replay_device on caller-owned device pointers (e.g. torch tensors' data_ptr())."""
        self._check(self.L.fmt_map_replay_device(self.h, d_ops, d_offsets, n_docs, key_bound, d_out))

    def map_check(self):
        """Raises EngineError(FMT_E_DATA) when the last map run saw a key id >= key_bound."""
        self._check(self.L.fmt_map_check(self.h))

    def map_fetch(self) -> np.ndarray:
        out = np.zeros(self._map_shape[0] * self._map_shape[1], dtype=MAP_SLOT_DTYPE)
        self._check(self.L.fmt_map_fetch(self.h, _ptr(out)))
        return out.reshape(self._map_shape)

    # sparse path (key pools of any size): one entry per live key, per document in birth order
    def map_load_sparse(self, batch):
        ops = np.ascontiguousarray(batch.ops)
        offs = np.ascontiguousarray(batch.doc_op_offsets, dtype=np.uint64)
        self._check(self.L.fmt_map_load_sparse(self.h, _ptr(ops), len(ops), _ptr(offs), batch.n_docs, batch.key_bound))
        self._map_shape = (batch.n_docs, batch.key_bound)
        self._map_nops = len(ops)

    def map_run_sparse(self):
        self._check(self.L.fmt_map_run_sparse(self.h))

    def map_run_sparse_tiered(self):
        """fmt_map_run_sparse_tiered: the LDS tier, then the HBM tier for the documents it refused."""
        self._check(self.L.fmt_map_run_sparse_tiered(self.h))

    def map_fetch_sparse(self):
        """(counts[n_docs], entries[sum(counts)]) with MAP_ENTRY_DTYPE, documents in order."""
        counts = np.zeros(self._map_shape[0], dtype=np.uint32)
        n = ctypes.c_uint64()
        self._check(self.L.fmt_map_fetch_sparse(self.h, _ptr(counts), None, 0, ctypes.byref(n)))
        entries = np.zeros(max(n.value, 1), dtype=MAP_ENTRY_DTYPE)
        self._check(self.L.fmt_map_fetch_sparse(self.h, _ptr(counts), _ptr(entries), n.value, ctypes.byref(n)))
        return counts, entries[: n.value]

    def map_pending(self, batch):
        """fmt_map_pending_run + fetch over the last sparse run: the local client's optimistic view of
        every document of `batch` (its local_ops / local_offsets, streams.MapStreamBuilder.local_*).
        Returns (counts[n_docs], status[n_docs], entries[sum(counts)]) with MAP_ENTRY_DTYPE."""
        ev = np.ascontiguousarray(batch.local_ops)
        eo = np.ascontiguousarray(batch.local_offsets, dtype=np.uint64)
        self._check(self.L.fmt_map_pending_run(self.h, _ptr(ev), len(ev), _ptr(eo)))
        counts = np.zeros(self._map_shape[0], dtype=np.uint32)
        status = np.zeros(self._map_shape[0], dtype=np.int32)
        n = ctypes.c_uint64()
        self._check(self.L.fmt_map_pending_fetch(self.h, _ptr(counts), _ptr(status), None, 0, ctypes.byref(n)))
        entries = np.zeros(max(n.value, 1), dtype=MAP_ENTRY_DTYPE)
        self._check(self.L.fmt_map_pending_fetch(self.h, _ptr(counts), _ptr(status), _ptr(entries), n.value,
                                                 ctypes.byref(n)))
        return counts, status, entries[: n.value]

    # ---- bulk summaries of the last sparse map run (include/fmt_map_summary.h)
    def map_summarize(self, keys, values, threads: int = 0) -> dict:
        """fmt_map_summarize: every document's SharedMap summary from the sequenced entries of the last
        map_run_sparse / map_run_sparse_tiered (device ordering and blob split, host JSON); keys / values:
        MapBatch.keys / .values. Returns the timing. Blobs: map_summary_doc(doc)."""
        from .streams import js_quote

        ka, nk = _c_strings(js_quote(k) for k in keys)
        va, nv = _c_strings(values)
        t = FmtMapSummaryTiming()
        self._check(self.L.fmt_map_summarize(self.h, ka, nk, va, nv, threads, ctypes.byref(t)))
        return {"kernel_ms": t.kernel_ms, "fetch_ms": t.fetch_ms, "format_ms": t.format_ms, "bytes": int(t.bytes),
                "threads": int(t.threads), "host_ordered_docs": int(t.host_ordered_docs)}

    def map_summary_doc(self, doc: int):
        """(header, [blob0, ...]) of document `doc` from the last map_summarize; EngineError with the
        document's status when it has none."""
        h, hl, n = ctypes.c_char_p(), ctypes.c_size_t(), ctypes.c_uint32()
        self._check(self.L.fmt_map_summary_blobs(self.h, doc, ctypes.byref(h), ctypes.byref(hl), ctypes.byref(n)))
        head = ctypes.string_at(h, hl.value).decode("utf-8")
        blobs = []
        for k in range(n.value):
            b, bl = ctypes.c_char_p(), ctypes.c_size_t()
            self._check(self.L.fmt_map_summary_blob(self.h, doc, k, ctypes.byref(b), ctypes.byref(bl)))
            blobs.append(ctypes.string_at(b, bl.value).decode("utf-8"))
        return head, blobs

    def map_summary_arrays(self, n_entries: int):
        """Test hook: (ordered entries, tags, n_blobs) of the last map_summarize as fetched from the device,
        the layout of native.map_summary_order; n_entries: the batch's live entries (sum of the counts)."""
        ordered = np.zeros(max(n_entries, 1), dtype=MAP_ENTRY_DTYPE)
        tags = np.zeros(max(n_entries, 1), dtype=np.uint32)
        n_blobs = np.zeros(max(self._map_shape[0], 1), dtype=np.uint32)
        self._check(self.L.fmt_internal_map_summary_arrays(self.h, _ptr(ordered), _ptr(tags), _ptr(n_blobs), n_entries))
        return ordered[:n_entries], tags[:n_entries], n_blobs[: self._map_shape[0]]

    def map_summary_host_only(self, on: bool):
        """Measurement switch (tools/bench_map_summary.py): map_summarize orders every document on the host."""
        self._check(self.L.fmt_internal_map_summary_host_only(self.h, int(on)))

    # ---- bulk legacy summaries of the last merge-tree run
    def mt_summarize_legacy(self, keys, values, chunk: int = 10000, threads: int = 0) -> dict:
        """fmt_mt_summarize_legacy: every document's legacy summary blobs (device merge + host JSON);
        returns the timing. Blobs: mt_summary(doc)."""
        from .streams import js_quote

        kq = [js_quote(k).encode("utf-8") for k in keys]
        vq = [v.encode("utf-8") for v in values]
        ka = (ctypes.c_char_p * max(len(kq), 1))(*kq)
        va = (ctypes.c_char_p * max(len(vq), 1))(*vq)
        t = FmtSummaryTiming()
        self._check(self.L.fmt_mt_summarize_legacy(self.h, ka, len(kq), va, len(vq), chunk, threads, ctypes.byref(t)))
        return {"kernel_ms": t.kernel_ms, "fetch_ms": t.fetch_ms, "format_ms": t.format_ms, "bytes": int(t.bytes),
                "threads": int(t.threads)}

    def mt_summary(self, doc: int):
        """(header, body or None) of document `doc` from the last mt_summarize_legacy."""
        h, b = ctypes.c_char_p(), ctypes.c_char_p()
        hl, bl = ctypes.c_size_t(), ctypes.c_size_t()
        self._check(self.L.fmt_mt_summary_blobs(self.h, doc, ctypes.byref(h), ctypes.byref(hl), ctypes.byref(b), ctypes.byref(bl)))
        head = ctypes.string_at(h, hl.value).decode("utf-8")
        body = ctypes.string_at(b, bl.value).decode("utf-8") if bl.value else None
        return head, body

    # ---- bulk SnapshotV1 summaries of the last merge-tree run (include/fmt_v1.h)
    def mt_summarize_v1(self, keys, values, clients, chunk: int = 10000, threads: int = 0) -> dict:
        """fmt_mt_summarize_v1: every document's SnapshotV1 blobs (device segmentation and first removers,
        host JSON); clients[d][k]: the long id of document d's short client k (MergeTreeBatch.clients).
        Returns the timing. Blobs: mt_summary_v1(doc)."""
        from .streams import js_quote

        ka, nk = _c_strings(js_quote(k) for k in keys)
        va, nv = _c_strings(values)
        offs = np.zeros(len(clients) + 1, dtype=np.uint64)
        np.cumsum([len(c) for c in clients], out=offs[1:])
        quoted = {}  # (each distinct name quoted once: batches repeat a few names over many documents)
        flat = [quoted.setdefault(name, js_quote(name).encode("utf-8")) for c in clients for name in c]
        ca = (ctypes.c_char_p * max(len(flat), 1))(*flat)
        t = FmtSummaryTiming()
        self._check(self.L.fmt_mt_summarize_v1(self.h, ka, nk, va, nv, ca, _ptr(offs), chunk, threads, ctypes.byref(t)))
        return {"kernel_ms": t.kernel_ms, "fetch_ms": t.fetch_ms, "format_ms": t.format_ms, "bytes": int(t.bytes),
                "threads": int(t.threads)}

    def mt_summary_v1(self, doc: int):
        """(header, [body_0, ...]) of document `doc` from the last mt_summarize_v1; EngineError with the
        document's V1 status when it has none."""
        h, hl, n = ctypes.c_char_p(), ctypes.c_size_t(), ctypes.c_uint32()
        self._check(self.L.fmt_mt_summary_v1_blobs(self.h, doc, ctypes.byref(h), ctypes.byref(hl), ctypes.byref(n)))
        head = ctypes.string_at(h, hl.value).decode("utf-8")
        bodies = []
        for k in range(n.value):
            b, bl = ctypes.c_char_p(), ctypes.c_size_t()
            self._check(self.L.fmt_mt_summary_v1_body(self.h, doc, k, ctypes.byref(b), ctypes.byref(bl)))
            bodies.append(ctypes.string_at(b, bl.value).decode("utf-8"))
        return head, bodies

    # ---- merge-tree
    def mt_load(self, batch):
        b, keep = batch_struct(batch)
        self._check(self.L.fmt_mt_load(self.h, ctypes.byref(b)))
        self._mt_docs = batch.n_docs

    def mt_run(self):
        self._check(self.L.fmt_mt_run(self.h))

    def mt_headers(self, raise_on_failed_docs: bool = True) -> np.ndarray:
        """Every document's result header; by default raises EngineError when a document failed
        (fmt_mt_fetch_headers returns the first failure), else returns them all."""
        out = np.zeros(self._mt_docs, dtype=DOC_RESULT_DTYPE)
        rc = self.L.fmt_mt_fetch_headers(self.h, _ptr(out))
        if raise_on_failed_docs or rc not in (FMT_OK, FMT_E_USAGE, FMT_E_DATA, FMT_E_CAPACITY, FMT_E_UNSUPPORTED):
            self._check(rc)
        return out

    def mt_doc(self, doc: int, hdr=None):
        if hdr is None:
            hdr = self.mt_headers()[doc]
        nl, nc, npp = int(hdr["n_leaves"]), int(hdr["n_chars"]), int(hdr["n_props"])
        leaves = np.zeros(max(nl, 1), dtype=LEAF_DTYPE)
        chars = np.zeros(max(nc, 1), dtype="<u2")
        props = np.zeros(max(npp, 1), dtype=PROPSET_DTYPE)
        self._check(self.L.fmt_mt_fetch_doc(self.h, doc, _ptr(leaves), nl, _ptr(chars), nc, _ptr(props), npp))
        return leaves[:nl], chars[:nc], props[:npp]

    # ---- bulk getText of the last merge-tree run (include/fmt_text.h)
    def mt_texts(self, placeholder: int = 0):
        """fmt_mt_fetch_text_all: every document's text from the local perspective in one device pass:
        (offsets uint64[n_docs + 1], units uint16[total]), document d's units at
        units[offsets[d]:offsets[d + 1]] (none for a document that failed). placeholder 0: getText();
        otherwise getTextWithPlaceholders() with that UTF-16 unit for every Marker."""
        offs = np.zeros(self._mt_docs + 1, dtype=np.uint64)
        self._check(self.L.fmt_mt_fetch_text_all(self.h, placeholder, _ptr(offs), None, 0))
        total = int(offs[-1])
        units = np.zeros(max(total, 1), dtype="<u2")
        self._check(self.L.fmt_mt_fetch_text_all(self.h, placeholder, _ptr(offs), _ptr(units), total))
        return offs, units[:total]

    def mt_text_strings(self, placeholder: int = 0) -> list:
        """mt_texts as one str per document (lone surrogates kept: utf-16-le, surrogatepass)."""
        offs, units = self.mt_texts(placeholder)
        raw = units.tobytes()
        return [raw[2 * int(a) : 2 * int(b)].decode("utf-16-le", "surrogatepass") for a, b in zip(offs[:-1], offs[1:])]

    # ---- bulk property runs of the last merge-tree run (include/fmt_runs.h)
    def _bulk(self, fn, dtype):
        offs = np.zeros(self._mt_docs + 1, dtype=np.uint64)
        self._check(fn(self.h, _ptr(offs), None, 0))
        total = int(offs[-1])
        out = np.zeros(max(total, 1), dtype=dtype)
        self._check(fn(self.h, _ptr(offs), _ptr(out), total))
        return offs, out[:total]

    def mt_prop_runs(self):
        """fmt_mt_fetch_prop_runs_all: every document's property runs from the local perspective in one
        device pass: (offsets uint64[n_docs + 1], runs PROP_RUN_DTYPE[total]), document d's runs at
        runs[offsets[d]:offsets[d + 1]] (none for a document that failed)."""
        return self._bulk(self.L.fmt_mt_fetch_prop_runs_all, PROP_RUN_DTYPE)

    def mt_props_all(self):
        """fmt_mt_fetch_props_all: every document's prop-set table in one copy: (offsets uint64[n_docs + 1],
        records PROPSET_DTYPE[total]); a run's `props` names a first record of its document's span."""
        return self._bulk(self.L.fmt_mt_fetch_props_all, PROPSET_DTYPE)

    def mt_formatted(self, keys, values, placeholder: int = 0) -> list:
        """Every document as rich text: per document a list of (text, props dict or None, is_marker), one
        entry per property run, from mt_prop_runs, mt_props_all and mt_texts(placeholder); no per-document
        fetch except mt_numbers for a document whose sets hold computed values. A Marker's text is the
        placeholder, or "" without one. A document that failed gives None."""
        import json

        status = self.mt_headers(raise_on_failed_docs=False)["status"]
        roffs, runs = self.mt_prop_runs()
        poffs, props = self.mt_props_all()
        toffs, units = self.mt_texts(placeholder)
        raw = units.tobytes()
        out = []
        for d in range(self._mt_docs):
            if int(status[d]) != FMT_OK:
                out.append(None)
                continue
            table = props[int(poffs[d]) : int(poffs[d + 1])]
            numbers = None
            dicts = {}
            at = int(toffs[d])
            doc = []
            for r in runs[int(roffs[d]) : int(roffs[d + 1])]:
                pid, marker = int(r["props"]), bool(int(r["flags"]) & RUN_MARKER)
                if pid != 0xFFFF and pid not in dicts:
                    kv = propset_entries(table, pid)
                    if numbers is None and any((e & 0xFFFF) >= MT_VALUE_COMPUTED for e in kv):
                        numbers = self.mt_numbers(d)
                    dicts[pid] = {keys[e >> 16]: (_computed(numbers[(e & 0xFFFF) - MT_VALUE_COMPUTED])
                                                  if (e & 0xFFFF) >= MT_VALUE_COMPUTED else json.loads(values[e & 0xFFFF]))
                                  for e in kv if e & 0xFFFF}  # (value id 0: null, the key is absent)
                n = (1 if placeholder else 0) if marker else int(r["len"])
                doc.append((raw[2 * at : 2 * (at + n)].decode("utf-16-le", "surrogatepass"),
                            None if pid == 0xFFFF else dicts[pid], marker))
                at += n
            assert at == int(toffs[d + 1]), f"document {d}: runs cover {at - int(toffs[d])} units of {int(toffs[d + 1] - toffs[d])}"
            out.append(doc)
        return out

    # ---- bulk position queries of the last merge-tree run (include/fmt_pos.h)
    def mt_positions(self, queries, q_offsets) -> np.ndarray:
        """fmt_mt_query_positions: every query of every document answered in one device pass. queries:
        POS_QUERY_DTYPE (pos, ref_seq, client; ref_seq VIEW_LOCAL: the local view), packed per document;
        q_offsets: n_docs + 1 offsets, ascending from 0 to len(queries). Returns POS_HIT_DTYPE[len(queries)],
        hit i answering query i; a query that could not be answered carries its own status, the call raises
        only for misuse (bad offsets, no completed run)."""
        q = np.ascontiguousarray(queries, dtype=POS_QUERY_DTYPE)
        offs = np.ascontiguousarray(q_offsets, dtype=np.uint64)
        if len(offs) != self._mt_docs + 1:
            raise EngineError(FMT_E_USAGE, f"mt_positions: {len(offs)} q_offsets for {self._mt_docs} documents")
        out = np.zeros(max(len(q), 1), dtype=POS_HIT_DTYPE)
        self._check(self.L.fmt_mt_query_positions(self.h, _ptr(offs), _ptr(q) if len(q) else None, len(q), _ptr(out)))
        return out[: len(q)]

    # ---- bulk range reads of the last merge-tree run (include/fmt_range.h)
    def mt_text_ranges(self, queries, q_offsets, placeholder: int = 0):
        """fmt_mt_fetch_text_ranges: the text of every range of every document in one device pass. queries:
        RANGE_QUERY_DTYPE (start, end, ref_seq, client; end RANGE_TO_END: the view's length; ref_seq
        VIEW_LOCAL: the local view), packed per document; q_offsets: n_docs + 1 offsets, ascending from 0 to
        len(queries). placeholder as in mt_texts. Returns (hits RANGE_HIT_DTYPE[len(queries)], units
        uint16[total]): range i's units at units[text_off : text_off + units] of hit i; a range that could
        not be read carries its own status, the call raises only for misuse."""
        q = np.ascontiguousarray(queries, dtype=RANGE_QUERY_DTYPE)
        offs = np.ascontiguousarray(q_offsets, dtype=np.uint64)
        if len(offs) != self._mt_docs + 1:
            raise EngineError(FMT_E_USAGE, f"mt_text_ranges: {len(offs)} q_offsets for {self._mt_docs} documents")
        hits = np.zeros(max(len(q), 1), dtype=RANGE_HIT_DTYPE)
        total = ctypes.c_uint64()
        args = (self.h, placeholder, _ptr(offs), _ptr(q) if len(q) else None, len(q), _ptr(hits), ctypes.byref(total))
        self._check(self.L.fmt_mt_fetch_text_ranges(*args, None, 0))
        units = np.zeros(max(int(total.value), 1), dtype="<u2")
        self._check(self.L.fmt_mt_fetch_text_ranges(*args, _ptr(units), int(total.value)))
        return hits[: len(q)], units[: int(total.value)]

    def mt_range_strings(self, queries, q_offsets, placeholder: int = 0) -> list:
        """mt_text_ranges as one str per query (lone surrogates kept), None for a query that failed."""
        hits, units = self.mt_text_ranges(queries, q_offsets, placeholder)
        raw = units.tobytes()
        return [raw[2 * int(h["text_off"]) : 2 * (int(h["text_off"]) + int(h["units"]))].decode("utf-16-le", "surrogatepass")
                if int(h["status"]) == FMT_OK else None for h in hits]

    def mt_positions_local(self, doc_ids, positions) -> np.ndarray:
        """mt_positions for local-view queries given as parallel arrays in any order: hit i answers
        (doc_ids[i], positions[i])."""
        docs = np.asarray(doc_ids, dtype=np.int64)
        pos = np.asarray(positions, dtype=np.uint32)
        if docs.shape != pos.shape or docs.ndim != 1:
            raise EngineError(FMT_E_USAGE, "mt_positions_local: doc_ids and positions must be parallel 1-d arrays")
        if len(docs) and (int(docs.min()) < 0 or int(docs.max()) >= self._mt_docs):
            raise EngineError(FMT_E_USAGE, "mt_positions_local: a document id outside the loaded batch")
        order = np.argsort(docs, kind="stable")
        q = np.zeros(len(docs), dtype=POS_QUERY_DTYPE)
        q["pos"] = pos[order]
        q["ref_seq"] = VIEW_LOCAL
        offs = np.zeros(self._mt_docs + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(np.bincount(docs, minlength=self._mt_docs), dtype=np.uint64)
        out = np.zeros(len(docs), dtype=POS_HIT_DTYPE)
        out[order] = self.mt_positions(q, offs)
        return out

    def mt_digests(self) -> np.ndarray:
        """fmt_mt_state_digest: every document's 64-bit content digest."""
        out = np.zeros(self._mt_docs, dtype=np.uint64)
        self._check(self.L.fmt_mt_state_digest(self.h, _ptr(out)))
        return out

    def huge_profile(self, doc: int):
        """Diagnostics: shader-clock totals per phase of a huge document's last replay
        (inclusive; nested phases overlap)."""
        out = np.zeros(25, dtype=np.uint64)
        f = self.L.fmt_internal_huge_profile
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        self._check(f(self.h, doc, _ptr(out)))
        names = ["replay", "window_groups", "window_slots", "zamboni", "graduate", "load", "output", "find",
                 "scour", "pack_leaf_parent", "slot_shift", "heap", "insert", "range", "split", "pack_interior",
                 "n_group_passes", "n_slot_passes", "sum_window_entries", "sum_groups", "window_share_w0", "group_scan",
                 "text_compactions", "merge_units_in_use", "resumed_at"]
        return dict(zip(names, (int(x) for x in out)))

    def mt_remove_order(self, doc: int, hdr=None) -> np.ndarray:
        """The document's remove-order entries (fmt_mt_remove_order) of its FMT_MT_F_RMORDER ops."""
        if hdr is None:
            hdr = self.mt_headers()[doc]
        n = int(hdr["n_rm_order"])
        out = np.zeros(max(n, 1), dtype=RM_ORDER_DTYPE)
        self._check(self.L.fmt_mt_fetch_remove_order(self.h, doc, _ptr(out), n))
        return out[:n]

    def mt_legacy_props(self, doc: int, hdr=None) -> np.ndarray:
        """Per leaf, the prop-set id of getAtSeq(properties, minSeq) (what the legacy summary reads)."""
        if hdr is None:
            hdr = self.mt_headers(raise_on_failed_docs=False)[doc]
        n = int(hdr["n_leaves"])
        out = np.zeros(max(n, 1), dtype=np.uint16)
        self._check(self.L.fmt_mt_fetch_legacy_props(self.h, doc, _ptr(out), n))
        return out[:n]

    def mt_rm_clients_hi(self, doc: int, hdr=None) -> np.ndarray:
        """Per leaf, its remove clients with short ids 64..127 (bit c - 64; zero for most documents)."""
        if hdr is None:
            hdr = self.mt_headers(raise_on_failed_docs=False)[doc]
        n = int(hdr["n_leaves"])
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self.L.fmt_mt_fetch_rm_clients_hi(self.h, doc, _ptr(out), n))
        return out[:n]

    def mt_rm_clients_hi2(self, doc: int, hdr=None) -> np.ndarray:
        """Per leaf, its remove clients with short ids 128..191 and 192..253 ((n, 2): bit c - 128, c - 192)."""
        if hdr is None:
            hdr = self.mt_headers(raise_on_failed_docs=False)[doc]
        n = int(hdr["n_leaves"])
        out = np.zeros(max(2 * n, 2), dtype=np.uint64)
        self._check(self.L.fmt_mt_fetch_rm_clients_hi2(self.h, doc, _ptr(out), 2 * n))
        return out[: 2 * n].reshape(n, 2)

    def mt_numbers(self, doc: int) -> np.ndarray:
        """The document's computed annotate-adjust numbers (value ids FMT_MT_VALUE_COMPUTED + index)."""
        n = ctypes.c_uint32(0)
        self._check(self.L.fmt_mt_fetch_numbers(self.h, doc, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.float64)
        if n.value:
            self._check(self.L.fmt_mt_fetch_numbers(self.h, doc, _ptr(out), n.value, ctypes.byref(n)))
        return out[: n.value]

    def mt_regen(self, doc: int):
        """f4: the document's regenerated ops (MT_OP_DTYPE) and their text after the last run
        (fmt_mt_fetch_regen; regeneratePendingOp at each reconnect record, client.ts:1452-1542)."""
        from .streams import MT_OP_DTYPE

        n, nt = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self.L.fmt_mt_fetch_regen(self.h, doc, None, 0, None, 0, ctypes.byref(n), ctypes.byref(nt)))
        ops = np.zeros(max(n.value, 1), dtype=MT_OP_DTYPE)
        text = np.zeros(max(nt.value, 1), dtype="<u2")
        if n.value or nt.value:
            self._check(self.L.fmt_mt_fetch_regen(self.h, doc, _ptr(ops), n.value, _ptr(text), nt.value, ctypes.byref(n),
                                                  ctypes.byref(nt)))
        return ops[: n.value], text[: nt.value]

    def mt_catchup(self, doc: int, hdr=None) -> np.ndarray:
        """The document's catch-up ranges (fmt_mt_catchup_range) of its FMT_MT_F_CATCHUP ops."""
        if hdr is None:
            hdr = self.mt_headers()[doc]
        n = int(hdr["n_catchup"])
        out = np.zeros(max(n, 1), dtype=CATCHUP_DTYPE)
        self._check(self.L.fmt_mt_fetch_catchup(self.h, doc, _ptr(out), n))
        return out[:n]

    def mt_catchup_all(self):
        """Every document's catch-up ranges in one copy (fmt_mt_fetch_catchup_all): (offsets[n_docs + 1],
        ranges), document d's at ranges[offsets[d]:offsets[d + 1]]."""
        offs = np.zeros(self._mt_docs + 1, dtype=np.uint64)
        self._check(self.L.fmt_mt_fetch_catchup_all(self.h, _ptr(offs), None, 0))
        out = np.zeros(max(int(offs[-1]), 1), dtype=CATCHUP_DTYPE)
        self._check(self.L.fmt_mt_fetch_catchup_all(self.h, _ptr(offs), _ptr(out), int(offs[-1])))
        return offs, out[: int(offs[-1])]
