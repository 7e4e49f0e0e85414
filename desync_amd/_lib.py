"""ctypes binding of libdsx.so (the C ABI declared in include/dsx.h).

This is the same binding a Go maintainer writes with cgo;
here it backs the Python mirror of desync's Chunker / IndexFromFile API.  There
is deliberately no CPU fallback: if the HIP library is missing or no GPU is
visible, calls raise.
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSX_LIB_PATH") or os.path.join(HERE, "libdsx.so")  # (A/B runs)

DSX_OUT_HOST = 0
DSX_OUT_DEVICE = 1
DSX_NO_SYNC = 2
DSX_TIMED = 16
DSX_SEAM_MAX_CANDS = 1024
DSX_SEAM_MAX_CUTS = 1024

# error codes (include/dsx.h)
DSX_OK = 0
DSX_E_MIN_TOO_SMALL = -1
DSX_E_MIN_GT_MAX = -2
DSX_E_MIN_GT_AVG = -3
DSX_E_AVG_GT_MAX = -4
DSX_E_AVG_RANGE = -5
DSX_E_INVAL = -6
DSX_E_CAPACITY = -7
DSX_E_HIP = -8
DSX_E_NOMEM = -9
DSX_E_INTERRUPTED = -10
DSX_E_IO = -11
DSX_E_STATE = -12
DSX_E_INTERNAL = -13
DSX_E_RESYNC = -14
DSX_E_PEER = -15
DSX_STREAM_EOF = 1
DSX_STREAM_SYNC = 2
DSX_SEAM_DEVICE = 8
DSX_SEAM_LAST = 1
DSX_SEAM_REWALKED = 2
DSX_SEAM_ERROR = 4
DSX_SEAM_REDO = 16

# every symbol include/dsx.h declares (tests check the library exports them)
EXPORTS = (
    "dsx_params_init", "dsx_strerror", "dsx_abi_version", "dsx_ctx_create", "dsx_ctx_destroy",
    "dsx_last_error", "dsx_cancel", "dsx_cut_device", "dsx_sync", "dsx_result", "dsx_cut_host",
    "dsx_cut_fd", "dsx_stream_begin", "dsx_stream_push", "dsx_stream_pop", "dsx_stream_advance",
    "dsx_stream_done", "dsx_stream_end", "dsx_stream_chunk_data", "dsx_stream_buffer",
    "dsx_stream_commit", "dsx_stream_flush", "dsx_stream_ids", "dsx_stream_chunk_id",
    "dsx_stream_pop_many", "dsx_stream_window", "dsx_stream_unpop", "dsx_shard_local", "dsx_shard_resolve",
    "dsx_selftest_boundary", "dsx_gen_uniform", "dsx_gen_dedup", "dsx_chunk_ids",
    "dsx_get_stats", "dsx_debug_trace", "dsx_index_fd", "dsx_index_host", "dsx_copy",
    "dsx_ids_fd", "dsx_ids_host", "dsx_progress", "dsx_shard_resolve_async", "dsx_shard_collect",
    "dsx_ctx_stream", "dsx_stamps_begin", "dsx_stamps_end", "dsx_host_copy",
    "dsx_host_sha512_256", "dsx_idset_create", "dsx_idset_destroy", "dsx_idset_count", "dsx_dedup",
    "dsx_plan_walk", "dsx_seed_plan", "dsx_assemble", "dsx_store_create", "dsx_store_destroy",
    "dsx_store_count", "dsx_store_put", "dsx_store_locate", "dsx_store_arena", "dsx_store_entries",
    "dsx_store_resolve", "dsx_store_verify", "dsx_store_prune", "dsx_store_copy",
    "dsx_aead_seal", "dsx_aead_open", "dsx_selftest_poly1305", "dsx_cut_device_many",
    "dsx_inplace_plan", "dsx_assemble_inplace", "dsx_chunk_keep", "dsx_read_ranges", "dsx_read_plan",
    "dsx_chunk_ids_known", "dsx_store_track", "dsx_store_touch", "dsx_store_stamps", "dsx_store_evict",
)
DSX_DIGEST_SHA512_256 = 0
DSX_DIGEST_SHA256 = 1
DSX_ENDS_DEVICE = 4
DSX_HOST_SHA_SCALAR = 1
DSX_IDS_DEVICE = 32
DSX_SIZES = 64
DSX_POS_NONE = 0xFFFFFFFF  # seed_pos of an ID the seed does not hold
DSX_SRC_NULL = -1          # dsx_plan_seg_t.source: the null seed
DSX_SRC_STORE = -2         # ... the packed store buffer
DSX_SRC_SELF = -3          # ... the buffer's own old content (dsx_assemble_inplace)
DSX_SRC_STASH = -4         # ... the stash (in a schedule's launch tables only)
DSX_STORE_DEVICE = 128
DSX_ASSEMBLE_UNALIGNED = 256
DSX_PRUNE_REMOVE = 512
DSX_COPY_ALL = 1024
DSX_EVICT_DRY = 8192       # dsx_store_evict: select and report, change nothing
DSX_STAMP_NOW = 0          # dsx_store_touch: the store's next clock value
DSX_INPLACE_ASCENDING = 2048
DSX_INPLACE_DESCENDING = 4096
DSX_INPLACE_SAVE = 0       # dsx_inplace_launch_t.kind
DSX_INPLACE_WRITE = 1
DSX_ASSEMBLE_TILE = 65536
DSX_AEAD_XCHACHA20_POLY1305 = 0
DSX_AEAD_NONCE = 24
DSX_AEAD_OVERHEAD = 40     # nonce + tag
DSX_AEAD_TILE = 262144     # plaintext bytes one workgroup of the seal / open main pass owns
DSX_KNOWN_TILE = 65536     # pair bytes one workgroup of dsx_chunk_ids_known's compare owns
DSX_KNOWN_TRIES = 4        # entries compared with one chunk at most
DSX_KNOWN_PROBES = 64      # table slots an insert or a probe visits at most
DSX_OFF_NONE = 0xFFFFFFFFFFFFFFFF  # known_off / dsx_store_locate: the store lacks the ID


class Params(ctypes.Structure):
    """dsx_params_t (mirrors the Chunker fields of chunker.go:108-131)."""

    _fields_ = [
        ("min", ctypes.c_uint64), ("avg", ctypes.c_uint64), ("max", ctypes.c_uint64),
        ("discriminator", ctypes.c_uint32), ("inverse_odd", ctypes.c_uint32),
        ("qmax", ctypes.c_uint32), ("qbias", ctypes.c_uint32), ("rot", ctypes.c_int32),
        ("reserved", ctypes.c_uint32),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("chunks", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("pieces", ctypes.c_uint64),
        ("repaired_segments", ctypes.c_uint64), ("dense_fallbacks", ctypes.c_uint64),
        ("scan_ms", ctypes.c_float), ("stitch_ms", ctypes.c_float),
        ("chunks_discarded", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("host_tail_chunks", ctypes.c_uint64),
    ]


class DedupTotals(ctypes.Structure):
    """dsx_dedup_totals_t: the counters of info.go:135-185."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("total", "unique", "in_seed", "size", "size_not_in_seed")]


class PlanSeg(ctypes.Structure):
    """dsx_plan_seg_t: one plan entry (a SeedSegmentCandidate, sequencer.go:21-25)."""

    _fields_ = [
        ("dst_off", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("src_off", ctypes.c_uint64),
        ("first", ctypes.c_uint32), ("count", ctypes.c_uint32),
        ("source", ctypes.c_int32), ("seed_first", ctypes.c_uint32),
    ]


class PlanTotals(ctypes.Structure):
    """dsx_plan_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("segments", "seed_chunks", "seed_bytes", "null_chunks", "null_bytes",
                 "store_chunks", "store_bytes", "store_unique", "store_len")]


class InplaceLaunch(ctypes.Structure):
    """dsx_inplace_launch_t: one launch of an in-place schedule."""

    _fields_ = [("window", ctypes.c_uint64), ("seg0", ctypes.c_uint64), ("nsegs", ctypes.c_uint64),
                ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64), ("kind", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class InplaceTotals(ctypes.Structure):
    """dsx_inplace_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("windows", "launches", "segments", "kept_chunks", "kept_bytes", "written_bytes",
                 "stash_bytes", "stash_peak")] + [("direction", ctypes.c_uint32),
                                                  ("reserved", ctypes.c_uint32)]


class StoreCounts(ctypes.Structure):
    """dsx_store_counts_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in ("chunks", "bytes", "max_chunks", "arena_bytes")]


class StorePutTotals(ctypes.Structure):
    """dsx_store_put_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("total", "stored", "stored_bytes", "present", "repeats")]


class StorePruneTotals(ctypes.Structure):
    """dsx_store_prune_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("entries", "kept", "kept_bytes", "removed", "removed_bytes", "moved", "moved_bytes",
                 "unmatched")]


class StoreCopyTotals(ctypes.Structure):
    """dsx_store_copy_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("total", "copied", "copied_bytes", "present", "repeats", "missing", "first_missing",
                 "reserved")]


class StoreEvictTotals(ctypes.Structure):
    """dsx_store_evict_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("entries", "evicted", "evicted_bytes", "kept", "kept_bytes", "moved", "moved_bytes",
                 "pinned", "evictable", "evictable_bytes", "cutoff")] + [("reserved", ctypes.c_uint64 * 2)]


class Range(ctypes.Structure):
    """dsx_range_t: bytes [off, off + len) of the blob go to the output at dst_off."""

    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("dst_off", ctypes.c_uint64)]


class ReadTotals(ctypes.Structure):
    """dsx_read_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("ranges", "bytes", "pieces", "store_bytes", "null_bytes", "missing", "wrong_size",
                 "beyond")] + [("first_bad_range", ctypes.c_uint32),
                               ("first_bad_chunk", ctypes.c_uint32)]


class ReadPiece(ctypes.Structure):
    """dsx_read_piece_t: one (range, chunk) pair of dsx_read_plan."""

    _fields_ = [("chunk_off", ctypes.c_uint64), ("dst_off", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64), ("range", ctypes.c_uint32), ("chunk", ctypes.c_uint32)]


class KnownTotals(ctypes.Structure):
    """dsx_known_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("chunks", "recognised", "recognised_bytes", "hashed", "hashed_bytes", "pairs",
                 "compared_bytes", "fp_false", "untried", "reserved")]


class ManyOpts(ctypes.Structure):
    """dsx_many_opts_t: 0 in a field is the library's default."""

    _fields_ = [("big_blob", ctypes.c_uint64), ("group_bytes", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64 * 2)]


class ManyTotals(ctypes.Structure):
    """dsx_many_totals_t."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("blobs", "empty_blobs", "chunks", "groups", "batched_blobs", "single_blobs",
                 "redone_blobs", "reserved")]


class PlanSeed(ctypes.Structure):
    """dsx_plan_seed_t: one seed of dsx_plan_walk, as classes."""

    _fields_ = [("tclass", ctypes.c_void_p), ("sclass", ctypes.c_void_p),
                ("ends", ctypes.c_void_p), ("m", ctypes.c_uint64)]


class ScanStamp(ctypes.Structure):
    """dsx_scan_stamp_t: one scan launch timed from inside the kernel."""

    _fields_ = [(n, ctypes.c_uint64) for n in
                ("seq", "bytes", "t_first", "t_last", "wave_cycles", "wave_ticks", "waves", "reserved")]

    @property
    def ms(self):
        return (self.t_last - self.t_first) / 1e5  # s_memrealtime: 100 MHz

    @property
    def mhz(self):
        return 100.0 * self.wave_cycles / self.wave_ticks if self.wave_ticks else 0.0

    @property
    def busy(self):
        """Mean fraction of the launch its waves were running (1 - the
        wave-end spread and start skew)."""
        span = self.t_last - self.t_first
        return self.wave_ticks / (self.waves * span) if self.waves and span else 0.0


class Seam(ctypes.Structure):
    _fields_ = [
        ("shard_start", ctypes.c_uint64), ("shard_len", ctypes.c_uint64), ("total", ctypes.c_uint64),
        ("first_cand_beyond", ctypes.c_uint64), ("exit_cut", ctypes.c_uint64),
        ("window_end", ctypes.c_uint64), ("entry", ctypes.c_uint64),
        ("ncands", ctypes.c_uint32), ("ncuts", ctypes.c_uint32),
        ("flags", ctypes.c_uint32), ("pad", ctypes.c_uint32),
        ("cands", ctypes.c_uint64 * DSX_SEAM_MAX_CANDS),
        ("cuts", ctypes.c_uint64 * DSX_SEAM_MAX_CUTS),
    ]


_lib = None
_lock = threading.RLock()  # (re-entrant: a Chunker's __del__ may return its context to the pool)


def _share_torch_hip_runtime():
    """A process can drive the GPU through ONE HIP runtime.  PyTorch-ROCm ships
    its own libamdhip64.so (SONAME libamdhip64.so.7, the same as ROCm's); load
    it before libdsx.so so that libdsx binds to it and device pointers, streams
    and RCCL from torch interoperate with the library.  Without torch the
    system ROCm runtime (/opt/rocm/lib, libdsx's RUNPATH) is used."""
    try:
        import torch
    except ImportError:
        return
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(path):
        ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


# The DSX_* settings the product library reads (INTEGRATION.md,
# "Environment"; tests/test_abi.py checks the library's strings against it).
PRODUCT_ENV = ("DSX_TAIL_SPLIT", "DSX_LANE_TARGET", "DSX_SEG_FLOOR", "DSX_SCAN_NT", "DSX_SCAN_ROTF",
               "DSX_DIGEST_PC", "DSX_DIGEST_LPT", "DSX_INDEX_WINDOW", "DSX_INDEX_SLOT",
               "DSX_INDEX_READERS", "DSX_INDEX_HOST_TAIL", "DSX_HOST_THREADS")
# Settings only libdsx_diag.so reads (scan ablations, other geometries,
# rejected experiments), with the value the product library behaves as (None:
# no such value).  Set to anything else with the product library they would
# be silently ignored, so loading it refuses them.
DIAG_ENV = {"DSX_SCAN_VARIANT": "0", "DSX_SCAN_CFG": "0", "DSX_FUSE": "0", "DSX_TEST_MODE": None,
            "DSX_DIGEST_PC_CHUNKS": "2", "DSX_PREFETCH": "0", "DSX_REGIONS_PER_SLOT": "1",
            "DSX_SCAN_LINE": "1", "DSX_SCAN_TRACE": "0", "DSX_WAVE_MAJOR": "1",
            "DSX_FIXUP_FAST": "1", "DSX_FINISH": "1", "DSX_SEG_MAX": "4", "DSX_SEG_TARGET": "4096",
            "DSX_DIGEST_PF": "1", "DSX_TAIL_MULT": "1", "DSX_LANE_BYTES": None,
            "DSX_STITCH_CUS": "0", "DSX_SCAN_MASK": "0", "DSX_SCAN_PRIO": None,
            "DSX_STREAM_BATCH": None, "DSX_NOOP_BEFORE_SCAN": None, "DSX_WALK_WGS": "2",
            "DSX_WALK_NT": "576", "DSX_TAIL_LOG": None, "DSX_FEED_THREADS": None, "DSX_FEED_MULTI": None,
            "DSX_FEED_MID": None, "DSX_SIDE_PRIO": "1",
            "DSX_FEED_CUT_END": None, "DSX_SHARE_NS": "45", "DSX_SHARE_PC": "1", "DSX_SHARE_SLACK": "0", "DSX_CTX_PRIO": "1", "DSX_FEED_EXTRA": None, "DSX_SHARE_MULTI": "1", "DSX_FINE_TAIL": "33554432", "DSX_FINE_DIV": "4"}


def lib():
    """Load libdsx.so; raises ImportError if it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(make -C desync_amd/csrc). desync_amd has no CPU fallback.")
        diag_env = [k for k, dflt in DIAG_ENV.items() if os.environ.get(k, "") not in ("", dflt)]
        if diag_env and not os.path.basename(LIB_PATH).startswith("libdsx_diag"):
            raise ImportError(
                f"{', '.join(diag_env)} selects a diagnostic path (scan ablations, other "
                "geometries, rejected experiments), which only the diagnostic build reads: "
                "make -C desync_amd/csrc diag and set "
                "DSX_LIB_PATH=desync_amd/libdsx_diag.so")
        _share_torch_hip_runtime()
        L = ctypes.CDLL(LIB_PATH)
        u64, u32, i32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
        P = ctypes.POINTER
        sig = {
            "dsx_params_init": (i32, [u64, u64, u64, P(Params)]),
            "dsx_strerror": (ctypes.c_char_p, [i32]),
            "dsx_abi_version": (i32, []),
            "dsx_ctx_create": (i32, [i32, P(vp)]),
            "dsx_ctx_destroy": (i32, [vp]),
            "dsx_last_error": (ctypes.c_char_p, [vp]),
            "dsx_cancel": (i32, [vp]),
            "dsx_progress": (i32, [vp, P(u64)]),
            "dsx_cut_device": (i32, [vp, vp, u64, P(Params), vp, u64, P(u64), u32]),
            "dsx_cut_device_many": (i32, [vp, vp, u64, vp, u64, P(Params), vp, u64, P(u64), vp,
                                          P(ManyOpts), P(ManyTotals), u32]),
            "dsx_sync": (i32, [vp]),
            "dsx_result": (i32, [vp, P(u64)]),
            "dsx_cut_host": (i32, [vp, vp, u64, P(Params), vp, u64, P(u64)]),
            "dsx_cut_fd": (i32, [vp, i32, u64, u64, P(Params), vp, u64, P(u64)]),
            "dsx_stream_begin": (i32, [vp, P(Params)]),
            "dsx_stream_push": (i32, [vp, vp, u64, i32]),
            "dsx_stream_pop": (i32, [vp, P(u64), P(u64)]),
            "dsx_stream_advance": (i32, [vp, u64]),
            "dsx_stream_done": (i32, [vp]),
            "dsx_stream_end": (i32, [vp]),
            "dsx_stream_buffer": (i32, [vp, u64, P(vp)]),
            "dsx_stream_commit": (i32, [vp, u64, i32]),
            "dsx_stream_flush": (i32, [vp, P(u64), P(u64)]),
            "dsx_stream_ids": (i32, [vp, i32]),
            "dsx_stream_chunk_id": (vp, [vp]),
            "dsx_stream_pop_many": (i32, [vp, vp, vp, u64, P(u64), P(u64)]),
            "dsx_stream_window": (i32, [vp, P(vp), P(u64), P(u64)]),
            "dsx_stream_unpop": (i32, [vp, u64]),
            "dsx_stream_chunk_data": (vp, [vp]),
            "dsx_shard_local": (i32, [vp, vp, u64, u64, u64, u64, P(Params), vp, u32]),
            "dsx_shard_resolve": (i32, [vp, vp, i32, i32, vp, vp, u64, P(u64), u32]),
            "dsx_shard_resolve_async": (i32, [vp, vp, i32, i32, vp, u64, vp]),
            "dsx_shard_collect": (i32, [vp, vp, vp, P(ctypes.c_int32), P(u64)]),
            "dsx_ctx_stream": (i32, [vp, P(vp)]),
            "dsx_selftest_boundary": (i32, [vp, P(Params), i32, u64, u64, P(u64)]),
            "dsx_gen_uniform": (i32, [vp, vp, u64, u64, u64]),
            "dsx_gen_dedup": (i32, [vp, vp, u64, u64, u64, ctypes.c_double]),
            "dsx_chunk_ids": (i32, [vp, vp, u64, u64, vp, u64, vp, u32, i32]),
            "dsx_get_stats": (i32, [vp, P(Stats)]),
            "dsx_copy": (i32, [vp, vp, vp, u64]),
            "dsx_index_fd": (i32, [vp, i32, u64, u64, P(Params), i32, vp, vp, u64, P(u64)]),
            "dsx_index_host": (i32, [vp, vp, u64, P(Params), i32, vp, vp, u64, P(u64)]),
            "dsx_debug_trace": (i32, [vp, vp, u64, P(u64), P(u64)]),
            "dsx_ids_fd": (i32, [vp, i32, u64, u64, u64, vp, u64, i32, vp]),
            "dsx_ids_host": (i32, [vp, vp, u64, u64, vp, u64, i32, vp]),
            "dsx_stamps_begin": (i32, [vp, u64]),
            "dsx_stamps_end": (i32, [vp, vp, u64, P(u64)]),
            "dsx_host_copy": (i32, [vp, vp, u64, i32]),
            "dsx_host_sha512_256": (i32, [vp, vp, u64, vp, i32, i32]),
            "dsx_idset_create": (i32, [vp, vp, u64, u32, P(vp)]),
            "dsx_idset_destroy": (i32, [vp, vp]),
            "dsx_idset_count": (i32, [vp, P(u64), P(u64)]),
            "dsx_dedup": (i32, [vp, vp, vp, u64, u64, vp, vp, vp, P(DedupTotals), u32]),
            "dsx_plan_walk": (i32, [vp, u64, u64, vp, vp, vp, u32, u32, vp, u64, vp, u64,
                                    P(PlanTotals)]),
            "dsx_seed_plan": (i32, [vp, vp, vp, u64, u64, vp, vp, vp, u32, vp, u32, vp, u64, vp, u64,
                                    P(PlanTotals), u32]),
            "dsx_assemble": (i32, [vp, vp, u64, vp, vp, u32, vp, u64, vp, u64, u32]),
            "dsx_inplace_plan": (i32, [vp, u64, vp, u64, vp, u64, u64, u64, u64, u64, u64, u32, vp,
                                       u64, vp, u64, P(InplaceTotals)]),
            "dsx_assemble_inplace": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, u32, vp, u64, vp, u64,
                                           u64, u64, u64, u64, u32, P(InplaceTotals)]),
            "dsx_chunk_keep": (i32, [vp, vp, u64, vp, u64, vp, i32, vp, P(u64), u32]),
            "dsx_store_create": (i32, [vp, u64, u64, P(vp)]),
            "dsx_store_destroy": (i32, [vp, vp]),
            "dsx_store_count": (i32, [vp, P(StoreCounts)]),
            "dsx_store_put": (i32, [vp, vp, vp, u64, vp, vp, u64, u64, P(StorePutTotals), u32]),
            "dsx_store_locate": (i32, [vp, vp, vp, u64, vp, vp, P(u64), u32]),
            "dsx_store_arena": (i32, [vp, P(vp), P(u64)]),
            "dsx_store_entries": (i32, [vp, vp, u64, u64, vp, vp, u32]),
            "dsx_store_resolve": (i32, [vp, vp, vp, u64, vp, u64, P(u64), P(u64), P(u32), u32]),
            "dsx_store_verify": (i32, [vp, vp, i32, vp, u64, P(u64)]),
            "dsx_store_prune": (i32, [vp, vp, vp, u64, u64, P(StorePruneTotals), u32]),
            "dsx_store_copy": (i32, [vp, vp, vp, vp, u64, P(StoreCopyTotals), u32]),
            "dsx_store_track": (i32, [vp, vp]),
            "dsx_store_touch": (i32, [vp, vp, vp, u64, u64, P(u64), u32]),
            "dsx_store_stamps": (i32, [vp, vp, u64, u64, vp, P(u64), u32]),
            "dsx_store_evict": (i32, [vp, vp, u64, u64, vp, u64, vp, u64, u64, P(StoreEvictTotals), u32]),
            "dsx_read_ranges": (i32, [vp, vp, vp, vp, u64, u64, vp, u64, vp, u64, vp, u64,
                                      P(ReadTotals), u32]),
            "dsx_read_plan": (i32, [vp, u64, u64, vp, u64, vp, u64, P(u64)]),
            "dsx_chunk_ids_known": (i32, [vp, vp, vp, u64, u64, vp, u64, i32, vp, vp,
                                          P(KnownTotals), u32]),
            "dsx_aead_seal": (i32, [vp, i32, vp, vp, u64, vp, u64, u64, vp, vp, u64, vp, u32]),
            "dsx_aead_open": (i32, [vp, i32, vp, vp, u64, vp, u64, u64, vp, u64, vp, vp, u64,
                                    P(u64), u32]),
            "dsx_selftest_poly1305": (i32, [vp, vp, vp, u64, vp]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
        return L


class DsxError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = lib().dsx_strerror(code).decode()
        super().__init__(f"{msg}" + (f": {detail}" if detail else ""))


def check(rc, ctx=None):
    if rc < 0:
        detail = ""
        if ctx is not None and rc in (DSX_E_HIP, DSX_E_INTERNAL, DSX_E_NOMEM):
            d = lib().dsx_last_error(ctx)
            detail = d.decode() if d else ""
        raise DsxError(rc, detail)
    return rc


class Context:
    """One dsx_ctx (HIP streams + device scratch) on a GPU; not thread-safe."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        rc = lib().dsx_ctx_create(int(device), ctypes.byref(h))
        if rc != DSX_OK:
            why = lib().dsx_last_error(None)
            raise DsxError(rc, f"cannot create a dsx context on HIP device {device}"
                           + (f" ({why.decode()})" if why else ""))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            lib().dsx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        s = Stats()
        check(lib().dsx_get_stats(self.h, ctypes.byref(s)), self.h)
        return s

    def stamps_begin(self, max_launches):
        """Time the next max_launches scan launches from inside the kernel."""
        check(lib().dsx_stamps_begin(self.h, int(max_launches)), self.h)
        self._stamp_cap = int(max_launches)

    def stamps_end(self):
        """The stamped launches' ScanStamp records, in launch order."""
        cap = getattr(self, "_stamp_cap", 0)
        buf = (ScanStamp * max(1, cap))()
        n = ctypes.c_uint64()
        check(lib().dsx_stamps_end(self.h, buf, cap, ctypes.byref(n)), self.h)
        return list(buf[:min(cap, n.value)])


_default = {}
_pool = {}  # (device, DSX_* env) -> idle contexts (IndexFromFile is re-entrant, a context is not)


def default_context(device=0):
    ctx = _default.get(device)
    if ctx is None:
        ctx = Context(device)
        _default[device] = ctx
    return ctx


_POOL_IDLE = 4  # idle contexts kept per device (each holds its pipeline buffers)


def _env_key(device):
    # a context reads its DSX_* settings from the environment when created:
    # it is handed out again only under the same settings
    return (device, tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("DSX_"))))


def acquire_context(device=0):
    """A context no other thread uses until release_context(): an idle pooled
    one (its pinned and device buffers already sized by earlier calls) or a
    new one.  A new context costs ~0.2 s of allocations once its pipelines
    run; a pooled one costs nothing."""
    key = _env_key(device)
    ctx = None
    with _lock:
        # idle contexts made under other settings are not handed out again
        # while these hold: close them rather than keep their buffers
        stale = [c for k in list(_pool) if k[0] == device and k != key for c in _pool.pop(k)]
        idle = _pool.setdefault(key, [])
        while idle and ctx is None:
            ctx = idle.pop()
            ctx = ctx if ctx.h else None  # (closed meanwhile: reset_context_pool)
    for c in stale:
        c.close()
    if ctx is None:
        ctx = Context(device)
        ctx._pool_key = key
    return ctx


def release_context(ctx):
    """Returns a context from acquire_context() to its pool (closed instead
    when the pool is full or the context is closed)."""
    if ctx is None or not ctx.h:
        return
    key = getattr(ctx, "_pool_key", None) or _env_key(ctx.device)
    with _lock:
        idle = _pool.setdefault(key, [])
        if len(idle) < _POOL_IDLE:
            idle.append(ctx)
            return
    ctx.close()


class pooled_context:
    """``with pooled_context(dev) as ctx``: a context no other thread uses
    meanwhile (created on demand, returned to a per-device pool afterwards;
    the pipeline buffers a context holds are reused by the next call)."""

    def __init__(self, device=0):
        self.device = device
        self.ctx = None

    def __enter__(self):
        self.ctx = acquire_context(self.device)
        return self.ctx

    def __exit__(self, *exc):
        release_context(self.ctx)
        self.ctx = None
        return False


def reset_context_pool():
    """Closes the idle pooled contexts (settings such as DSX_INDEX_WINDOW are
    read from the environment when a context is created)."""
    with _lock:
        idle = [c for cs in _pool.values() for c in cs]
        _pool.clear()
    for c in idle:
        c.close()
