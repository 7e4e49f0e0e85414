"""A numpy executor of an in-place schedule (dsx_inplace_plan's launch list),
written from the contract in include/dsx.h, not from the planner.

Bytes are replaced by identities, so that repeated content cannot hide a wrong
source: old byte x of the buffer is the number x, byte o of seed k, of the
store and a zero byte have numbers of their own.  ``expected`` is what the
original plan asks for at every target byte; the executor runs the launches in
order and asserts, per launch,

  * the table ascends in dst_off, its entries overlap no other and lie in
    [lo, hi);
  * SAVE reads only its window of the buffer, and only old bytes nobody has
    written; it writes only stash ranges (inside the reported peak);
  * WRITE writes only its window, inside [0, new_len); the buffer ranges it
    reads lie outside that window, hold old bytes nobody has written, and
    overlap nothing it writes; a stash byte it reads holds exactly the old
    byte the target wants there (a stash range reused while still needed
    shows here), and was saved before;

and at the end: the buffer equals the target over [0, new_len), bytes nobody
was to write (kept chunks, gaps, everything beyond new_len) were never
written, and every saved byte was read.  ``totals`` are recomputed from the
launch list alone.
"""
import ctypes

import numpy as np

from desync_amd import _lib

SELF, STASH, NULL, STORE = _lib.DSX_SRC_SELF, _lib.DSX_SRC_STASH, _lib.DSX_SRC_NULL, _lib.DSX_SRC_STORE
SAVE, WRITE = _lib.DSX_INPLACE_SAVE, _lib.DSX_INPLACE_WRITE
ASC, DESC = _lib.DSX_INPLACE_ASCENDING, _lib.DSX_INPLACE_DESCENDING
SEG_DTYPE = np.dtype([("dst_off", "<u8"), ("bytes", "<u8"), ("src_off", "<u8"), ("first", "<u4"),
                      ("count", "<u4"), ("source", "<i4"), ("seed_first", "<u4")])
LAUNCH_DTYPE = np.dtype([("window", "<u8"), ("seg0", "<u8"), ("nsegs", "<u8"), ("lo", "<u8"),
                         ("hi", "<u8"), ("kind", "<u4"), ("reserved", "<u4")])
assert SEG_DTYPE.itemsize == ctypes.sizeof(_lib.PlanSeg)
assert LAUNCH_DTYPE.itemsize == ctypes.sizeof(_lib.InplaceLaunch)
TOTAL_KEYS = ("windows", "launches", "segments", "kept_chunks", "kept_bytes", "written_bytes",
              "stash_bytes", "stash_peak", "direction")
ZERO_ID = -1
GARBAGE_ID = -2          # buffer bytes beyond have_len
STORE_BASE = 1 << 40     # store byte o is STORE_BASE + o, seed k's (k + 2) * STORE_BASE + o


def make_segs(rows):
    """rows of (dst_off, bytes, src_off, first, count, source) -> dsx_plan_seg_t array."""
    a = np.zeros(len(rows), dtype=SEG_DTYPE)
    for i, r in enumerate(rows):
        a[i] = (r[0], r[1], r[2], r[3], r[4], r[5], 0xFFFFFFFF)
    return a


def schedule(segs, ends, keep, have_len, new_len, skew, tile, window, stash_cap, flags=0):
    """dsx_inplace_plan through ctypes -> (rc, launches, tables, totals dict).
    Asks once for the counts and once for the lists."""
    L = _lib.lib()
    segs = np.ascontiguousarray(segs, dtype=SEG_DTYPE)
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    tot = _lib.InplaceTotals()

    def call(la, sg):
        return L.dsx_inplace_plan(
            ctypes.c_void_p(segs.ctypes.data if segs.size else None), segs.size,
            ctypes.c_void_p(ends.ctypes.data if ends.size else None), ends.size,
            ctypes.c_void_p(kp.ctypes.data) if kp is not None and kp.size else None,
            have_len, new_len, skew, tile, window, stash_cap, flags,
            ctypes.c_void_p(la.ctypes.data if la.size else None), la.size,
            ctypes.c_void_p(sg.ctypes.data if sg.size else None), sg.size, ctypes.byref(tot))

    la, sg = np.zeros(0, dtype=LAUNCH_DTYPE), np.zeros(0, dtype=SEG_DTYPE)
    rc = call(la, sg)
    if rc == _lib.DSX_E_CAPACITY and tot.stash_peak <= stash_cap:
        la = np.zeros(tot.launches, dtype=LAUNCH_DTYPE)
        sg = np.zeros(tot.segments, dtype=SEG_DTYPE)
        rc = call(la, sg)
    return rc, la, sg, {k: int(getattr(tot, k)) for k in TOTAL_KEYS}


def dropped_chunks(segs, ends, keep):
    """The chunks nobody writes: keep[i] set, or named by a SELF segment with
    src_off == dst_off."""
    n = len(ends)
    out = np.zeros(n, dtype=bool)
    if keep is not None:
        out |= np.asarray(keep, dtype=bool)
    for g in segs:
        if int(g["source"]) == SELF and int(g["src_off"]) == int(g["dst_off"]):
            out[int(g["first"]):int(g["first"]) + int(g["count"])] = True
    return out


def expected_ids(segs, ends, keep, cap, have_len):
    """-> (identity wanted at every byte of the buffer, mask of the bytes that
    must never be written)."""
    want = np.arange(cap, dtype=np.int64)
    want[have_len:] = GARBAGE_ID
    untouched = np.ones(cap, dtype=bool)
    drop = dropped_chunks(segs, ends, keep)
    starts = np.concatenate([[0], np.asarray(ends, dtype=np.int64)[:-1]]) if len(ends) else []
    for g in segs:
        src, so, d0 = int(g["source"]), int(g["src_off"]), int(g["dst_off"])
        for k in range(int(g["first"]), int(g["first"]) + int(g["count"])):
            if drop[k]:
                continue
            s, e = int(starts[k]), int(ends[k])
            o = so + (s - d0)
            if src == NULL:
                want[s:e] = ZERO_ID
            else:
                base = 0 if src == SELF else STORE_BASE if src == STORE else (src + 2) * STORE_BASE
                want[s:e] = base + o + np.arange(e - s, dtype=np.int64)
            untouched[s:e] = False
    return want, untouched


def execute(launches, tables, segs, ends, keep, have_len, new_len, skew, window, stash_peak,
            cap=None):
    """Runs the launch list on identities with every assertion of the module
    docstring; returns the totals recomputed from the list (direction None
    when fewer than two windows were visited)."""
    cap = max(have_len, new_len) if cap is None else cap
    want, untouched = expected_ids(segs, ends, keep, cap, have_len)
    buf = np.arange(cap, dtype=np.int64)
    buf[have_len:] = GARBAGE_ID
    written = np.zeros(cap, dtype=bool)
    stash = np.full(max(1, stash_peak), GARBAGE_ID, dtype=np.int64)
    unread = np.zeros(max(1, stash_peak), dtype=bool)   # saved, not yet read
    live_from = np.full(max(1, stash_peak), -1, dtype=np.int64)
    intervals = []  # (save launch, last reading launch, bytes)
    last_read = np.full(max(1, stash_peak), -1, dtype=np.int64)
    saved = written_bytes = 0

    def close(a, b):  # the bytes [a, b) of the stash are saved anew: their old life ends
        for j in np.unique(live_from[a:b]):
            if j < 0:
                continue
            m = live_from[a:b] == j
            assert not unread[a:b][m].any(), "a saved byte was overwritten before any launch read it"
            for lr in np.unique(last_read[a:b][m]):
                intervals.append((int(j), int(lr), int((last_read[a:b][m] == lr).sum())))

    for li, l in enumerate(launches):
        w, kind, lo, hi = int(l["window"]), int(l["kind"]), int(l["lo"]), int(l["hi"])
        tab = tables[int(l["seg0"]):int(l["seg0"]) + int(l["nsegs"])]
        assert len(tab) > 0, "a launch without segments"
        w0, w1 = max(0, w * window - skew), (w + 1) * window - skew
        d0 = tab["dst_off"].astype(np.int64)
        d1 = d0 + tab["bytes"].astype(np.int64)
        assert (tab["bytes"] > 0).all()
        assert (d0[1:] >= d1[:-1]).all(), "the table does not ascend in dst_off"
        assert lo <= d0[0] and d1[-1] <= hi
        if kind == SAVE:
            assert d1[-1] <= stash_peak, "a stash range beyond the reported peak"
            for g, a, b in zip(tab, d0.tolist(), d1.tolist()):
                x0 = int(g["src_off"])
                x1 = x0 + (b - a)
                assert int(g["source"]) == SELF
                assert w0 <= x0 and x1 <= min(w1, have_len), "SAVE reads outside its window"
                assert not written[x0:x1].any(), "SAVE reads a byte that was already written"
                close(a, b)
                stash[a:b] = buf[x0:x1]
                unread[a:b] = True
                live_from[a:b] = li
                last_read[a:b] = li
                saved += b - a
            continue
        assert kind == WRITE
        assert w0 <= d0[0] and d1[-1] <= min(w1, new_len), "WRITE writes outside its window"
        vals = []
        for g, a, b in zip(tab, d0.tolist(), d1.tolist()):
            src, so = int(g["source"]), int(g["src_off"])
            if src == SELF:
                assert so + (b - a) <= have_len
                assert so + (b - a) <= w0 or so >= min(w1, new_len), "WRITE reads the buffer inside its window"
                assert not written[so:so + b - a].any(), "WRITE reads a byte that was already written"
                vals.append(buf[so:so + b - a].copy())
            elif src == STASH:
                assert so + (b - a) <= stash_peak
                assert (live_from[so:so + b - a] >= 0).all(), "a stash byte read before it was saved"
                v = stash[so:so + b - a].copy()
                assert (v == want[a:b]).all(), "the stash does not hold what the target wants here"
                unread[so:so + b - a] = False
                last_read[so:so + b - a] = li
                vals.append(v)
            elif src == NULL:
                vals.append(np.full(b - a, ZERO_ID, dtype=np.int64))
            else:
                assert src == STORE or src >= 0
                base = STORE_BASE if src == STORE else (src + 2) * STORE_BASE
                vals.append(base + so + np.arange(b - a, dtype=np.int64))
        for v, a, b in zip(vals, d0.tolist(), d1.tolist()):  # every read came before the first write
            assert not written[a:b].any(), "a byte is written twice"
            assert not untouched[a:b].any(), "a byte nobody was to write is written"
            buf[a:b] = v
            written[a:b] = True
            written_bytes += b - a
    close(0, len(stash))
    assert (buf[:new_len] == want[:new_len]).all(), "the buffer is not the target"
    assert not written[new_len:].any() and not written[untouched].any()
    assert (written[:new_len] | untouched[:new_len]).all(), "a byte of the target was left out"

    peak = 0
    if intervals:
        ev = np.zeros(len(launches) + 1, dtype=np.int64)
        for j, lr, nbytes in intervals:
            ev[j] += nbytes
            ev[lr + 1] -= nbytes
        # a range is free for the SAVE after its last reader, not for that reader's own window
        live = np.cumsum(ev)[:-1]
        peak = int(max(live[i] for i, l in enumerate(launches) if int(l["kind"]) == SAVE))
    wins = [int(l["window"]) for l in launches]
    order = [w for i, w in enumerate(wins) if i == 0 or wins[i - 1] != w]
    direction = None
    if len(order) > 1:
        inc = all(a < b for a, b in zip(order, order[1:]))
        dec = all(a > b for a, b in zip(order, order[1:]))
        assert inc or dec, "the windows are visited in no one direction"
        direction = ASC if inc else DESC
    drop = dropped_chunks(segs, ends, keep)
    sizes = np.diff(np.asarray(ends, dtype=np.int64), prepend=0) if len(ends) else np.zeros(0, np.int64)
    named = np.zeros(len(ends), dtype=bool)
    for g in segs:
        named[int(g["first"]):int(g["first"]) + int(g["count"])] = True
    drop &= named
    return {"windows": len(set(wins)), "launches": len(launches), "segments": int(len(tables)),
            "kept_chunks": int(drop.sum()), "kept_bytes": int(sizes[drop].sum()),
            "written_bytes": written_bytes, "stash_bytes": saved, "stash_peak": peak,
            "direction": direction}


def same_totals(got, ref):
    """The planner's totals against the executor's (direction: only when the
    executor could tell)."""
    for k in TOTAL_KEYS:
        if k == "direction" and ref[k] is None:
            continue
        assert got[k] == ref[k], (k, got[k], ref[k])
