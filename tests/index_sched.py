"""run_index's schedule (dsx_index.cpp index_schedule) as the diagnostic
library exports it (dsx_diag_index_schedule), for the tests: the invariants a
schedule must keep so that every chunk ID of a one-window IndexFromFile call
is hashed by exactly one of the GPU's shares, the tail feeder and the digest
after the read (tests/test_host_logic.py sweeps them without a GPU), and the
count of chunks the host hashes under a schedule (tests/test_gpu_index_shares.py
checks stats.host_tail_chunks against it).  Not a test module."""
import ctypes
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(REPO, "desync_amd", "libdsx_diag.so")
MAX = 256 << 10
NONE = (1 << 64) - 1  # a segment without a feeder


def diag_lib(path=DIAG):
    """libdsx_diag.so with the plan / pieces / schedule exports typed (no GPU
    is touched by loading it or calling them); None if it is not built."""
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    u64, u64p, i32 = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int
    lib.dsx_diag_index_plan.argtypes = [u64, u64, i32, u64p, u64p, u64p, u64p, i32]
    lib.dsx_diag_index_plan.restype = i32
    lib.dsx_diag_index_pieces.argtypes = [u64] * 4 + [i32, u64p, u64p, u64]
    lib.dsx_diag_index_pieces.restype = u64
    lib.dsx_diag_index_schedule.argtypes = [u64, u64, u64, u64, i32, ctypes.c_int64, u64p, u64, u64p,
                                            u64p, u64p, u64p, i32, u64p, i32, ctypes.POINTER(i32), u64p]
    lib.dsx_diag_index_schedule.restype = i32
    return lib


def schedule(lib, length, slot, window, threads, host_tail=-1, max_chunk=MAX):
    """{scan: [...], shares: [(at, cut, fire or 0)], segs: [(from, to,
    feed_cut, skip_above)], last_ws, side0, fcut, fcut_end, sides}."""
    cap = 1024
    while True:
        scan = (ctypes.c_uint64 * cap)()
        n_scan, n_seg = ctypes.c_uint64(), ctypes.c_int()
        at, cut, fire = ((ctypes.c_uint64 * 8)() for _ in range(3))
        seg, info = (ctypes.c_uint64 * 36)(), (ctypes.c_uint64 * 5)()
        n = lib.dsx_diag_index_schedule(length, max_chunk, slot, window, threads, host_tail, scan, cap,
                                        ctypes.byref(n_scan), at, cut, fire, 8, seg, 9,
                                        ctypes.byref(n_seg), info)
        assert 0 <= n <= 8 and 0 < n_seg.value <= 9, (n, n_seg.value)
        if n_scan.value <= cap:
            break
        cap = n_scan.value
    return {"scan": list(scan[:n_scan.value]),
            "shares": [(at[k], cut[k], fire[k]) for k in range(n)],
            "segs": [tuple(seg[4 * j:4 * j + 4]) for j in range(n_seg.value)],
            "last_ws": info[0], "side0": info[1], "fcut": info[2], "fcut_end": info[3],
            "sides": info[4]}


def pieces(lib, length, slot, window, feeds=1, max_chunk=MAX):
    cap = 1024
    while True:
        off, size = (ctypes.c_uint64 * cap)(), (ctypes.c_uint64 * cap)()
        n = lib.dsx_diag_index_pieces(length, max_chunk, slot, window, feeds, off, size, cap)
        if n <= cap:
            return [(off[k], size[k]) for k in range(n)]
        cap = n


def violations(s, length, max_chunk=MAX):
    """The invariants of a schedule `s` of a `length`-byte call; the list of
    those it breaks (empty: none)."""
    bad = []
    scan, segs, shares = s["scan"], s["segs"], s["shares"]
    last_ws = s["last_ws"]
    # the scan points rise to the end of the file
    if not scan or scan[-1] != length or any(a >= b for a, b in zip(scan, scan[1:])):
        bad.append("scan points do not rise to len")
    # 1. the segments tile the last window
    pos = last_ws
    for f, t, _, _ in segs:
        if f != pos or t <= f:
            bad.append(f"segments do not tile: [{f}, {t}) after {pos}")
        pos = t
    if pos != length or not 0 <= last_ws < length:
        bad.append(f"segments end at {pos}, not len")
    # 2. one cut per segment: the feeder takes what the GPU skips
    for j, (f, t, feed, skip) in enumerate(segs):
        if not (feed == skip or (feed >= max_chunk and skip == 0)):
            bad.append(f"segment {j} [{f}, {t}): the feeder takes chunks above {feed}, "
                       f"the GPU skips those above {skip}")
    # 3. every planned share fires below len at or after its point, or the
    # feeder never heard of it
    fired = [(at, cut, fire) for at, cut, fire in shares if fire]
    feeder_cuts = [seg[2] for seg in segs[:-1]]
    for k, (at, cut, fire) in enumerate(shares):
        if fire and not (fire in scan and at <= fire < length):
            bad.append(f"share {k} due at {at} fires at {fire}")
    if feeder_cuts != [cut for _, cut, _ in fired]:
        bad.append(f"the feeder's segment cuts {feeder_cuts} are not the fired shares' "
                   f"{[c for _, c, _ in fired]}")
    if not fired and shares and segs[-1][2] != s["fcut"]:
        bad.append("no share fired, yet the last cut is not the feeder's usual one")
    # 4. fired in order, one scan point and one side stream each
    fires = [fire for _, _, fire in fired]
    if fires != sorted(set(fires)) or [k for k, sh in enumerate(shares) if sh[2]] != list(range(len(fired))):
        bad.append(f"shares fire out of order: {fires}")
    if len(fired) > s["sides"] - s["side0"] or s["side0"] != (1 if last_ws else 0):
        bad.append(f"{len(fired)} shares on {s['sides']} side streams from {s['side0']}")
    # 5. the digest after the read starts at the last fired share's snapshot
    # (the window's start without one), and each share at the one before it
    starts = [last_ws] + fires
    if [seg[0] for seg in segs] != starts:
        bad.append(f"segments start at {[seg[0] for seg in segs]}, the snapshots are at {starts}")
    return bad


def host_chunks(s, ends, max_chunk=MAX):
    """How many chunks of the chain `ends` (the reference's) the feeder hashes
    under schedule `s`: those of the last window (ending past its start) that
    are longer than the feeder's cut of the segment their end lies in, (from,
    to].  None if a chunk ends exactly on a segment boundary inside the file,
    where the count would depend on which side the snapshot puts it."""
    ends = np.asarray(ends, np.int64)
    lens = np.diff(np.concatenate([[0], ends]))
    inner = [t for _, t, _, _ in s["segs"][:-1]]
    if np.isin(inner, ends).any():
        return None
    n = 0
    for f, t, feed, _ in s["segs"]:
        if feed == NONE:
            continue
        n += int(np.sum((ends > f) & (ends <= t) & (lens > feed)))
    return n
