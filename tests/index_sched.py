"""run_index's and run_ids's schedules (dsx_index_plan.h index_schedule,
ids_schedule) as the diagnostic library exports them (dsx_diag_index_schedule,
dsx_diag_ids_schedule), for the tests: the invariants a schedule must keep so
that every chunk ID of an IndexFromFile or VerifyIndex call is hashed by
exactly one of the GPU's shares, the host and the digest after the read
(tests/test_host_logic.py sweeps them without a GPU), and the count of chunks
the host hashes under a schedule (tests/test_gpu_index_shares.py checks
stats.host_tail_chunks against it).  Not a test module."""
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
    lib.dsx_diag_ids_schedule.argtypes = [u64, u64p, u64, u64, u64, i32, ctypes.c_int64, i32, i32,
                                          ctypes.c_double, u64p, u64, u64p, u64p, i32, u64p, i32,
                                          ctypes.POINTER(i32), u64p]
    lib.dsx_diag_ids_schedule.restype = i32
    lib.dsx_diag_host_ns_per_byte.argtypes = []
    lib.dsx_diag_host_ns_per_byte.restype = ctypes.c_double
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


# ------------------------------------------------ run_ids's schedule (ids_schedule)
READ_BYTES_PER_NS = 45.0  # dsx_index_plan.h kReadBytesPerNs


def feed_cut_for(host_tail, threads):
    """The host's usual cut (dsx_index_plan.h feed_cut_for), restated."""
    if host_tail > 0:
        return host_tail
    cut = (28 << 10) * 28 // max(1, threads)
    return min(128 << 10, max(28 << 10, (cut + 2047) & ~4095))


def ids_schedule(lib, start, ends, slot, window, threads, host_tail=-1, tail_on=None, host_ns=0.38, sides=4):
    """run_ids's schedule for the list start, ends (dsx_diag_ids_schedule):
    {pre, piece, W, nwin, L, maxc, i_last, early_cut, end_cut, win_i1: [...],
    shares: [(landed, cut, i1)], segs: [(i_from, i_to, feed_cut, skip_above)]}.
    tail_on None: on unless host_tail is 0 (SHA-512/256 on an AVX-512 host)."""
    ends = np.ascontiguousarray(ends, np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    tail_on = host_tail != 0 if tail_on is None else tail_on
    cap = 64
    while True:
        win, n_win, n_seg = (ctypes.c_uint64 * cap)(), ctypes.c_uint64(), ctypes.c_int()
        share, seg, info = (ctypes.c_uint64 * 24)(), (ctypes.c_uint64 * 36)(), (ctypes.c_uint64 * 8)()
        k = lib.dsx_diag_ids_schedule(start, ends.ctypes.data_as(u64p), ends.size, slot, window, threads,
                                      host_tail, sides, int(tail_on), host_ns, win, cap,
                                      ctypes.byref(n_win), share, 8, seg, 9, ctypes.byref(n_seg), info)
        assert 0 <= k <= 8 and 0 < n_seg.value <= 9, (k, n_seg.value)
        if n_win.value <= cap:
            break
        cap = n_win.value
    out = dict(zip(("pre", "piece", "W", "L", "maxc", "i_last", "early_cut", "end_cut"), info))
    out.update(nwin=n_win.value, win_i1=list(win[:n_win.value]),
               shares=[tuple(share[3 * j:3 * j + 3]) for j in range(k)],
               segs=[tuple(seg[4 * j:4 * j + 4]) for j in range(n_seg.value)])
    return out


def _rel_lens(start, ends):
    rel = np.asarray(ends, np.uint64).astype(np.int64) - int(start)
    return rel, np.diff(np.concatenate([[0], rel]))


def ids_violations(s, start, ends, threads, host_tail=-1, tail_on=None, host_ns=0.38, sides=4):
    """The invariants of run_ids's schedule `s` for the list start, ends; the
    list of those it breaks (empty: none)."""
    bad = []
    tail_on = host_tail != 0 if tail_on is None else tail_on
    rel, lens = _rel_lens(start, ends)
    n = rel.size
    pre, piece, W, nwin, L, maxc = (s[k] for k in ("pre", "piece", "W", "nwin", "L", "maxc"))
    # the windows: whole pieces, the longest chunk kept, at least one
    if L != (int(rel[-1]) if n else 0) or maxc != (int(lens.max()) if n else 0):
        bad.append(f"L {L}, longest chunk {maxc}")
    if (pre < maxc or pre % 128 or piece < 4096 or piece % 4096 or W < piece or W % piece
            or nwin != max(1, -(-L // W)) or (nwin > 1 and W < 2 * pre)):
        bad.append(f"windows: pre {pre} piece {piece} W {W} x {nwin}")
    # 1. the window ranges tile [0, n): a chunk ends in its window's (ws, ws +
    # wl] (window 0 also at 0, the last window takes the rest) and starts at or
    # after ws - pre
    win = s["win_i1"]
    last_ws = (nwin - 1) * W
    if len(win) != nwin or win[-1] != n or any(a > b for a, b in zip(win, win[1:])):
        bad.append(f"{len(win)} window ranges up to {win[-1:]} for {nwin} windows of {n} chunks")
    else:
        i0 = 0
        for w, i1 in enumerate(win):
            ws, we = w * W, min(L, (w + 1) * W)
            e = rel[i0:i1]
            if e.size and (e.max() > we or (w and e.min() <= ws) or (e - lens[i0:i1] + pre).min() < ws):
                bad.append(f"window {w}: chunks [{i0}, {i1}) do not end in ({ws}, {we}] with their bytes kept")
            if i1 < n and rel[i1] <= we:
                bad.append(f"window {w} leaves chunk {i1}")
            i0 = i1
        if s["i_last"] != (win[-2] if nwin > 1 else 0):
            bad.append(f"the last window starts at chunk {s['i_last']}")
    # 2. the segments tile [i_last, n) in order, one cut each
    segs, shares = s["segs"], s["shares"]
    pos = s["i_last"]
    for j, (a, b, feed, skip) in enumerate(segs):
        if a != pos or b < a:
            bad.append(f"segments do not tile: [{a}, {b}) after {pos}")
        pos = b
        ok = (feed == skip or (feed >= maxc and skip == 0)) if tail_on else (feed == NONE and skip == 0)
        if not ok:
            bad.append(f"segment {j}: the host takes chunks above {feed}, the GPU skips those above {skip}")
    if pos != n or len(segs) != len(shares) + 1:
        bad.append(f"{len(segs)} segments end at {pos}, {len(shares)} shares, {n} chunks")
        return bad
    # 3. the shares: whole pieces landed, rising, below L; their chunks end by then
    if len(shares) > sides or (shares and not (tail_on and host_tail < 0)):
        bad.append(f"{len(shares)} shares on {sides} side streams, host tail {host_tail}")
    prev = last_ws
    for k, (landed, cut, i1) in enumerate(shares):
        a = segs[k][0]
        # (two shares may land with the same piece of a large slot: the later one is empty)
        if landed % piece or landed >= L or landed < prev or (landed == prev and (k == 0 or i1 != a)):
            bad.append(f"share {k} lands at {landed} after {prev}")
        if segs[k][1] != i1 or segs[k][2] != cut:
            bad.append(f"share {k} {(landed, cut, i1)} is not segment {segs[k]}")
        if i1 > a and rel[a:i1].max() > landed:
            bad.append(f"a chunk of share {k} ends after {landed}")
        prev = landed
    # 5. every chunk of the last window is taken by exactly one party
    for j, (a, b, feed, skip) in enumerate(segs):
        ln = lens[a:b]
        host = ln > feed
        gpu = (ln <= skip) if skip else np.ones(ln.size, bool)
        if (host == gpu).any():
            i = a + int(np.flatnonzero(host == gpu)[0])
            bad.append(f"chunk {i} of {int(lens[i])} bytes in segment {j} has {int(host[i - a]) + int(gpu[i - a])} takers")
    # 4. the cuts: the host's usual one, and with shares the lowest multiple of
    # 4096 up to it whose host bytes fit 3/4 of the read (by brute force)
    early = feed_cut_for(host_tail, threads)
    if s["early_cut"] != early:
        bad.append(f"early cut {s['early_cut']}, not {early}")
    if tail_on and not shares and (s["end_cut"], segs[-1][2]) != (early, early):
        bad.append(f"no shares: end cut {s['end_cut']}, last segment {segs[-1]}")
    if tail_on and shares:
        fixed = sum(int(lens[a:b][lens[a:b] > feed].sum()) for a, b, feed, _ in segs[:-1])
        last = lens[segs[-1][0]:n]
        budget = 0.75 * float(L) / READ_BYTES_PER_NS * threads / host_ns
        want = next((c for c in range(4096, early + 1, 4096)
                     if float(fixed + int(last[last > c].sum())) <= budget), early)
        got = s["end_cut"]
        if got != want or segs[-1][2] != got or got % 4096 or not 4096 <= got <= early:
            bad.append(f"end cut {got} (last segment {segs[-1]}), brute force {want} of {early}")
    return bad


def ids_host_chunks(s, start, ends):
    """How many chunks of the list the host hashes under run_ids's schedule
    `s`: each segment's chunks longer than its feed_cut.  None if a chunk ends
    exactly on a share's `landed`."""
    rel, lens = _rel_lens(start, ends)
    if np.isin([landed for landed, _, _ in s["shares"]], rel).any():
        return None
    return sum(int(np.sum(lens[a:b] > feed)) for a, b, feed, _ in s["segs"] if feed != NONE)
