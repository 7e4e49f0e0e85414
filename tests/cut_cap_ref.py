"""The cut list's capacity contract (include/dsx.h: dsx_cut_device, dsx_result,
dsx_cut_device_many, dsx_shard_resolve, dsx_shard_resolve_async /
dsx_shard_collect): a fenced output, the checks, the capacities a case sweeps,
a restatement of the stitch geometry and the seeded inputs of every case.

With a cap below the count a call returns DSX_E_CAPACITY, sets *n_out to the
count it needs and writes nothing at or past out_ends[cap].  The writers are
kernels that store into the caller's memory, one per stitch back-end, each
with its own comparison; the call's geometry picks the back-end.  A FencedOut
puts sentinels around and inside the caller's buffer, so that a writer which
forgets cap lands in memory the test owns and fails an assertion.

Host code: nothing here touches the GPU unless a FencedOut is asked for
device memory.
"""
import ctypes
import functools

import numpy as np

from oracle import oracle as o

KiB, MiB = 1024, 1 << 20
DFLT = (16 * KiB, 64 * KiB, 256 * KiB)
TINY = (48, 192, 768)
SENTINEL = 0xA5A5A5A5A5A5A5A5  # no offset: above any length a blob can have
SEAM_MAX_CUTS = 1024           # DSX_SEAM_MAX_CUTS

DSX_OK, DSX_E_CAPACITY = 0, -7


# --------------------------------------------------------------------- fence
class FencedOut:
    """guard + upper + guard uint64 entries, all SENTINEL; the library gets
    the address of entry `guard` and `cap`.  upper is the call's documented
    upper bound and guard >= upper, so a writer that ignores cap (it writes at
    most `upper` entries from the pointer on) stays inside the allocation.
    where: "device" (one torch allocation in HBM) or "host" (numpy).
    untouched_on_failure: whether check() lets a failing call write below cap
    (default: a device output may be, a host output is not)."""

    def __init__(self, upper, cap, where, untouched_on_failure=None):
        assert where in ("device", "host") and 0 <= cap <= upper
        self.upper, self.cap, self.where = int(upper), int(cap), where
        self.guard = max(self.upper, 64)
        size = 2 * self.guard + self.upper
        if where == "device":
            import torch
            self.mem = torch.full((size,), SENTINEL - (1 << 64), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()  # (the library's streams do not wait for torch's)
            self.base = self.mem.data_ptr()
        else:
            self.mem = np.full(size, SENTINEL, dtype=np.uint64)
            self.base = self.mem.ctypes.data
        # a failed call leaves a host output untouched (and a shard's device output)
        self.host_rule = where == "host" if untouched_on_failure is None else untouched_on_failure

    @property
    def ptr(self):
        """out_ends: the address of entry `guard`."""
        return ctypes.c_void_p(self.base + 8 * self.guard)

    @property
    def ptr_or_null(self):
        """out_ends of a counting call: NULL when cap is 0."""
        return self.ptr if self.cap else None

    def read(self):
        """The whole allocation as uint64 (a copy for device memory)."""
        if self.where == "device":
            import torch
            torch.cuda.synchronize()
            return self.mem.cpu().numpy().view(np.uint64)
        return self.mem


def _clean(a, lo, hi, what):
    bad = np.flatnonzero(a[lo:hi] != np.uint64(SENTINEL))
    assert bad.size == 0, (f"{what}: entry {int(bad[0]) + lo} of the allocation was written "
                           f"({int(a[lo + int(bad[0])]):#x}), {bad.size} in all")


def check(fenced, rc, n_out, want, tag=""):
    """The contract, for a call that got fenced.ptr and fenced.cap and whose
    true list is `want`.  Below cap after a failure nothing is asserted for
    device output (earlier pieces and a dense retry's first attempt may have
    written there); a host output is not touched at all by a failing call."""
    want = np.asarray(want, dtype=np.uint64)
    n, g, cap = int(want.size), fenced.guard, fenced.cap
    a = fenced.read()
    tag = f"{tag} cap={cap} n={n} ({fenced.where})"
    _clean(a, 0, g, tag + " front guard")
    if cap >= n:
        assert rc == DSX_OK, (tag, rc)
        assert int(n_out) == n, (tag, int(n_out))
        got = a[g:g + n]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (tag, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
        _clean(a, g + n, a.size, tag + " behind the list")
    else:
        assert rc == DSX_E_CAPACITY, (tag, rc)
        assert int(n_out) == n, (tag, int(n_out))
        _clean(a, g + cap, a.size, tag + " at or past cap")
        if fenced.host_rule:
            _clean(a, g, g + cap, tag + " host output of a failed call")


def check_untouched(fenced, tag=""):
    """No entry of the allocation was written (blob_first of a failed call)."""
    a = fenced.read()
    _clean(a, 0, a.size, f"{tag} ({fenced.where}) untouched")


def check_fences(fenced, most, tag=""):
    """Nothing outside [0, min(most, cap)) was written: for a call whose
    list's content the contract leaves open (a rank that answers DSX_E_PEER
    or DSX_E_RESYNC)."""
    a = fenced.read()
    g = fenced.guard
    _clean(a, 0, g, f"{tag} front guard")
    _clean(a, g + min(int(most), fenced.cap), a.size, f"{tag} behind the list")


def caps(n, upper):
    """The capacities a case sweeps for a list of n cuts: the counting call,
    one entry, a third, both sides of the edge of <=, and the documented bound."""
    assert 2 <= n and n + 1 <= upper, (n, upper)
    return sorted({0, 1, n // 3, n - 1, n, n + 1, upper})


def upper_cut(length, mn):
    return length // mn + 2


def upper_shard(length, mn):
    return length // mn + 2 + 4 + SEAM_MAX_CUTS


def upper_many(length, mn, nblobs):
    return length // mn + nblobs


# ------------------------------------------------------- the stitch geometry
def stitch_seg(n, mx, seg_floor=1 << 20, seg_mult=4, seg_target=4096):
    """dsx_engine.cpp stitch_seg: the segment of a span of n bytes."""
    seg = max(seg_mult * mx, seg_floor)
    if seg_target:
        while (n + seg - 1) // seg > seg_target + 1 and seg < (1 << 26):
            seg <<= 1
    return seg


def piece_nseg(P, n, L, mx, seg_floor=1 << 20, origin=0):
    """launch_stitch: the segments of the piece [P, P + n) of a blob of L
    bytes (its span starts max bytes before a piece that is not the first)."""
    anchor = P - mx if P > origin + mx else origin
    end = L if P + n >= L else P + n
    if end <= anchor:
        return 1
    seg = stitch_seg(end - anchor, mx, seg_floor)
    return (end - anchor + seg - 1) // seg


def nseg(L, mx, seg_floor=1 << 20):
    """A blob of at most 8 GiB on the ordinary path: one piece."""
    assert L <= 8 << 30
    return piece_nseg(0, L, L, mx, seg_floor)


def backend(ns, finish=True, fixup_fast=True):
    """launch_stitch: which kernels end a piece of ns segments."""
    if finish and ns <= 2048:
        return "finish"
    return "fixup_fast+gather" if fixup_fast and ns <= 9 * 1024 else "fixup+gather"


DENSE_PIECE = 32 * MiB  # kDensePiece: the dense retry's pieces
PIECE_MAX = 8 << 30     # kPieceMax: bytes per scan launch
TWO_PIECES_LEN = PIECE_MAX + 64 * MiB + 321  # an 8 GiB piece and a 65-segment one


def piece_cut_caps(want, n, upper, bounds):
    """caps() plus the oracle's cut count at each piece end, one above and one
    below -> (caps, counts)."""
    at = [int(np.searchsorted(want, np.uint64(b), side="right")) for b in bounds]
    return sorted(set(caps(n, upper)) | {c + d for c in at for d in (-1, 0, 1)}), at


def cuts_per_segment(want, seg):
    return np.bincount(((np.asarray(want, dtype=np.uint64) - np.uint64(1)) // np.uint64(seg)).astype(np.int64))


# ------------------------------------------------------------------- inputs
class Case:
    def __init__(self, data, params, seg_floor=None, want=None, length=None):
        """want, length: the oracle's list and the length of a blob that lives
        on the device only."""
        self.data, self.params, self.seg_floor = data, params, seg_floor
        self.length = int(data.size if length is None else length)
        self.want = o.chunk_stream(data, *params) if want is None else want
        self.n = int(self.want.size)
        self.upper = upper_cut(self.length, params[0])
        # (one piece up to 8 GiB; piece_nseg for the pieces of a longer blob)
        self.nseg = nseg(self.length, params[2], seg_floor or (1 << 20)) if self.length <= PIECE_MAX else None


@functools.lru_cache(maxsize=None)
def fast_short():
    return Case(o.synth_uniform(71, 0, 8 * MiB), DFLT)


@functools.lru_cache(maxsize=None)
def fast_long():
    return Case(o.synth_uniform(72, 0, 8 * MiB), TINY, 65536)


@functools.lru_cache(maxsize=None)
def zero_runs():
    """test_stitch_many_workgroups_and_repairs' composition: a random head of
    odd length puts the true chain inside the zero runs off the segment grid."""
    mx = DFLT[2]
    rng = np.random.default_rng(11)
    null = np.zeros(4 * mx, np.uint8)
    r1 = rng.integers(0, 256, 4 * mx, dtype=np.uint8)
    return Case(np.concatenate([r1[:12345], null, null, null, r1, null, r1]), DFLT)


GATHER_LEN = 129 * MiB + 77  # just over 2048 segments of 64 KiB
ZEROS_AT, ZEROS_LEN = 40 * MiB + 12345, 6 * MiB


@functools.lru_cache(maxsize=None)
def gather_clean():
    return Case(o.synth_uniform(73, 0, GATHER_LEN), TINY, 65536)


@functools.lru_cache(maxsize=None)
def gather_suspect():
    """gather_clean's bytes with 6 MiB of zeros inside, entered from random
    bytes (off the max lattice from any segment start)."""
    data = gather_clean().data.copy()
    data[ZEROS_AT:ZEROS_AT + ZEROS_LEN] = 0
    return Case(data, TINY, 65536)


@functools.lru_cache(maxsize=None)
def dense_block():
    """A 48-byte period whose window hash is a candidate at the default
    parameters (test_periodic_dense_candidates, test_gpu_seam_record.dense_tile)."""
    P = o.params(*DFLT)
    rng = np.random.default_rng(1)
    while True:
        blk = rng.integers(0, 256, 48, dtype=np.uint8)
        if o.window_hash(bytes(blk)) % P.d == P.d - 1:
            return blk


DENSE_LEN = 70 * MiB  # three dense pieces: 32 + 32 + 6 MiB


@functools.lru_cache(maxsize=None)
def dense_pieces():
    return Case(np.tile(dense_block(), DENSE_LEN // 48), DFLT)


@functools.lru_cache(maxsize=None)
def dense_small():
    """The 3 MiB tile: one dense piece (a queued call's redo in dsx_result)."""
    return Case(np.tile(dense_block(), (3 * MiB) // 48), DFLT)


def dense_caps(case):
    """caps() plus the oracle's cut counts at the ends of the first and the
    second 32 MiB piece, one above and one below each."""
    return piece_cut_caps(case.want, case.n, case.upper, [DENSE_PIECE, 2 * DENSE_PIECE])


@functools.lru_cache(maxsize=None)
def queued_blobs():
    """Eight queued calls: (case, short?) in queue order, short calls between
    fitting ones; the zero-run composition and the dense tile are short."""
    u = [Case(o.synth_uniform(80 + i, 0, 3 * MiB + 1000 * i), DFLT) for i in range(5)]
    return ((u[0], False), (u[1], True), (u[2], False), (zero_runs(), True), (u[3], False),
            (dense_small(), True), (u[4], True), (fast_short(), False))


def many_expected(data, blob_ends, params):
    """The per-blob oracle of dsx_cut_device_many -> (ends, first)."""
    ends, first, b0 = [], [0], 0
    for b1 in (int(x) for x in blob_ends):
        e = o.chunk_stream(data[b0:b1], *params) + np.uint64(b0) if b1 > b0 else np.empty(0, np.uint64)
        ends.append(e)
        first.append(first[-1] + e.size)
        b0 = b1
    return (np.concatenate(ends) if ends else np.empty(0, np.uint64)), np.array(first, dtype=np.uint64)


class ManyCase:
    def __init__(self, data, blob_ends, params):
        self.data, self.blob_ends, self.params = data, blob_ends, params
        self.want, self.first = many_expected(data, blob_ends, params)
        self.n = int(self.want.size)
        self.upper = upper_many(data.size, params[0], blob_ends.size)


@functools.lru_cache(maxsize=None)
def many_plan():
    """The first 400 blobs of test_gpu_many.py's small_set(): the batched path."""
    rng = np.random.default_rng(3)
    lens = np.exp(rng.uniform(0.0, np.log(256 * KiB), 3000)).astype(np.uint64)
    be = np.cumsum(np.clip(lens, 1, 256 * KiB)).astype(np.uint64)[:400]
    return ManyCase(o.synth_uniform(3, 0, int(be[-1])), be, (2 * KiB, 8 * KiB, 32 * KiB))


@functools.lru_cache(maxsize=None)
def many_fallback():
    """test_fallback_dense_blob's input: the dense tile between random blobs."""
    rng = np.random.default_rng(1)
    blk = dense_block()
    parts = [rng.integers(0, 256, 200_001, dtype=np.uint8), np.tile(blk, (3 * MiB) // 48),
             rng.integers(0, 256, 300_007, dtype=np.uint8)]
    be = np.cumsum([p.size for p in parts]).astype(np.uint64)
    return ManyCase(np.concatenate(parts), be, DFLT)


class ShardCase:
    """world ranks over equal spans (the last takes the rest), as
    test_gpu_parity.py's _shard_protocol; want[r] = the true chain's cuts in
    (start, start + len]."""

    def __init__(self, data, params, world):
        self.data, self.params, self.world = data, params, world
        span = data.size // world
        self.geo = [(r * span, span if r < world - 1 else data.size - r * span) for r in range(world)]
        whole = o.chunk_stream(data, *params)
        self.want = [whole[(whole > np.uint64(s)) & (whole <= np.uint64(s + n))] for s, n in self.geo]
        self.upper = [upper_shard(n, params[0]) for _, n in self.geo]


@functools.lru_cache(maxsize=None)
def shards_uniform():
    return ShardCase(o.synth_uniform(74, 0, 6 * MiB), DFLT, 3)


@functools.lru_cache(maxsize=None)
def shards_zero_run():
    """test_gpu_parity.py's _compose_shard("seam-zero-run"): a zero run far
    longer than the 32 * max seam window across the shard boundaries, entered
    off the max grid, so an owner re-walks (DSX_E_RESYNC)."""
    mx = DFLT[2]
    r2 = o.synth_uniform(23, 0, 4 * mx)
    head = o.synth_uniform(24, 0, 3 * mx + 12345)
    return ShardCase(np.concatenate([head, np.zeros(100 * mx, np.uint8), r2]), DFLT, 3)
