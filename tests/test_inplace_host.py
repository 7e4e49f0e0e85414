"""dsx_inplace_plan (the schedule of an in-place assembly, host code) through
ctypes with windows of a few dozen bytes: a seeded sweep and crafted cases,
every schedule run by the numpy executor of inplace_ref.py.  No GPU."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import inplace_ref as ref
from desync_amd import _lib

TILE = 16
ASC, DESC = ref.ASC, ref.DESC
SELF, NULL, STORE = ref.SELF, ref.NULL, ref.STORE
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(segs, ends, keep, have_len, new_len, window, flags=0, skew=0, stash_cap=None):
    """Plans, executes and compares the totals; -> (totals, launches, tables)."""
    segs = ref.make_segs(segs) if not isinstance(segs, np.ndarray) else segs
    cap = have_len if stash_cap is None else stash_cap
    rc, la, sg, tot = ref.schedule(segs, ends, keep, have_len, new_len, skew, TILE, window, cap, flags)
    assert rc == 0, (rc, tot)
    got = ref.execute(la, sg, segs, ends, keep, have_len, new_len, skew, window, tot["stash_peak"])
    ref.same_totals(tot, got)
    assert tot["stash_peak"] <= have_len
    if flags:
        assert tot["direction"] == flags
    return tot, la, sg


# ---- the sweep ------------------------------------------------------------------
def random_case(rng):
    """Old and new versions as strings over an alphabet of 1-4 block symbols
    (so repeats, in-place ties and chunks longer than a window are the rule),
    plus symbols only the new version has (store, seed, zeros)."""
    k = rng.randint(1, 4)
    size = {s: rng.choice((1, 3, 7, 15, 16, 17, 33, 70)) for s in range(k + 3)}
    old = [rng.randrange(k) for _ in range(rng.randint(0, 12))]
    new = [rng.randrange(k + 3) if rng.random() < 0.25 else rng.randrange(k)
           for _ in range(rng.randint(0, 12))]
    if rng.random() < 0.3 and old:  # a shifted copy: insertions, deletions, swaps
        cut = rng.randrange(len(old) + 1)
        new = rng.choice((old[cut:] + old[:cut], old[cut:], [rng.randrange(k + 3)] + old, old + old))
    where, at = {}, 0
    for s in old:
        where.setdefault(s, []).append(at)
        at += size[s]
    have_len = at
    rows, ends, keep, at = [], [], [], 0
    ext = {NULL: 0, STORE: 0, 0: 0, 1: 0}
    for i, s in enumerate(new):
        n = size[s]
        in_place = s < k and at in where.get(s, ())
        keep.append(1 if in_place and rng.random() < 0.5 else 0)
        if s < k and s in where and not (in_place and keep[-1] and rng.random() < 0.5):
            src, off = SELF, (at if in_place and rng.random() < 0.7 else rng.choice(where[s]))
        else:  # (a kept chunk may be planned from anywhere: keep wins)
            src = (NULL, STORE, 0, 1)[s % 4] if s >= k else STORE
            off = ext[src]
            ext[src] += n if src != NULL else 0
        last = rows[-1] if rows else None
        if last and last[5] == src and rng.random() < 0.8 and \
                (src == NULL or last[2] + last[1] == off):
            last[1] += n
            last[4] += 1
        else:
            rows.append([at, n, off, i, 1, src])
        at += n
        ends.append(at)
    if rng.random() < 0.1 and rows:  # a gap: chunks no segment names are never touched
        rows.pop(rng.randrange(len(rows)))
    return rows, ends, (keep if rng.random() < 0.7 else None), have_len, at


def test_sweep():
    rng = random.Random(20261020)
    cases = launches = 0  # (run() asserts rc == 0: with stash_cap = have_len no case is refused)
    dirs = {ASC: 0, DESC: 0}
    for _ in range(2200):
        rows, ends, keep, have_len, new_len = random_case(rng)
        window = rng.choice((16, 64))
        skew = rng.choice((0, 0, 1, 15))
        free = None
        for flags in (0, ASC, DESC):
            tot, la, _ = run(rows, ends, keep, have_len, new_len, window, flags, skew)
            launches += len(la)
            if flags == 0:
                free = tot
                dirs[tot["direction"]] += 1
            else:
                assert free["stash_peak"] <= tot["stash_peak"]
                if flags == free["direction"]:
                    assert free["stash_peak"] == tot["stash_peak"]
        cases += 1
    assert cases >= 2000 and launches > cases
    assert dirs[ASC] and dirs[DESC]


# ---- crafted cases ----------------------------------------------------------------
def chunks(total, size):
    ends = list(range(size, total, size)) + [total]
    return ends


def shift_plan(ends, delta):
    """Every chunk of the target is old content delta bytes further on
    (delta < 0: an insertion of -delta bytes in front, from the store)."""
    if delta >= 0:
        return [[0, ends[-1], delta, 0, len(ends), SELF]]
    k = next(i for i, e in enumerate(ends) if e >= -delta)
    assert ends[k] == -delta
    return [[0, -delta, 0, 0, k + 1, STORE], [-delta, ends[-1] + delta, 0, k + 1, len(ends) - k - 1, SELF]]


def test_identity_has_no_launch():
    ends = chunks(300, 20)
    for keep in (None, [1] * len(ends)):
        for segs in ([[0, 300, 0, 0, len(ends), SELF]],
                     [[e - 20, 20, e - 20, i, 1, SELF] for i, e in enumerate(ends)]):
            tot, la, sg = run(segs, ends, keep, 300, 300, 64)
            assert len(la) == 0 and len(sg) == 0
            assert tot["launches"] == 0 and tot["windows"] == 0 and tot["written_bytes"] == 0
            assert tot["kept_chunks"] == len(ends) and tot["kept_bytes"] == 300
    # keep wins over whatever the plan chose
    tot, la, _ = run([[0, 300, 0, 0, len(ends), STORE]], ends, [1] * len(ends), 300, 300, 64)
    assert len(la) == 0 and tot["kept_chunks"] == len(ends)


@pytest.mark.parametrize("window", (16, 64))
@pytest.mark.parametrize("factor", ("1", "tile-1", "window", "3*window+5"))
def test_insertion_and_deletion(window, factor):
    """delta bytes inserted in front: everything moves right, so descending a
    window reads below itself; deleted: everything moves left, the mirror.
    With delta >= window no window reads itself and the stash stays empty.  A
    smaller shift has a window read its own old bytes, which no launch may do
    while it writes them (a launch that reads what it writes is the hazard the
    schedule exists to exclude), so window - delta bytes bounce through the
    stash in the good direction and window + delta in the other."""
    delta = {"1": 1, "tile-1": TILE - 1, "window": window, "3*window+5": 3 * window + 5}[factor]
    body = 10 * window
    # insertion: the new version is delta store bytes, then the old one
    ends = [delta] + [delta + e for e in chunks(body, 24)]
    ins = shift_plan(ends, -delta)
    # deletion: the old version without its first delta bytes
    dele = shift_plan(chunks(body, 24), delta)
    for segs, e, have, new, good in ((ins, ends, body, body + delta, DESC),
                                     (dele, chunks(body, 24), body + delta, body, ASC)):
        peaks = {}
        for flags in (0, ASC, DESC):
            tot, _, _ = run(segs, e, None, have, new, window, flags)
            peaks[flags] = tot["stash_peak"]
            assert tot["written_bytes"] == new and tot["kept_chunks"] == 0
            if flags == 0:
                assert tot["direction"] == good
        assert peaks[0] == peaks[good] == min(peaks.values())
        if delta >= window:
            assert peaks[good] == 0
        else:
            assert peaks[good] == window - delta
            assert peaks[good] < peaks[ASC + DESC - good] <= window + delta


def test_swapped_halves():
    half = 160
    ends = chunks(2 * half, 20)
    n = len(ends)
    segs = [[0, half, half, 0, n // 2, SELF], [half, half, 0, n // 2, n // 2, SELF]]
    for flags in (0, ASC, DESC):
        tot, _, _ = run(segs, ends, None, 2 * half, 2 * half, 64, flags)
        assert tot["stash_peak"] == half and tot["stash_bytes"] == half
    rc, la, sg, tot = ref.schedule(ref.make_segs(segs), ends, None, 2 * half, 2 * half, 0, TILE, 64,
                                   half - 1)
    assert rc == _lib.DSX_E_CAPACITY and tot["stash_peak"] == half and len(la) == 0


def test_self_source_straddles_a_window_edge():
    # target chunk [64, 96) comes from old [50, 82): the source crosses the edge at 64
    ends = [64, 96, 128]
    segs = [[64, 32, 50, 1, 1, SELF]]
    for flags in (ASC, DESC):
        tot, la, sg = run(segs, ends, None, 128, 128, 64, flags)
        w = sg[la[-1]["seg0"]:la[-1]["seg0"] + la[-1]["nsegs"]]
        assert len(w) == 2 and int(w[0]["bytes"]) == 14 and int(w[1]["bytes"]) == 18
        assert tot["written_bytes"] == 32
    tot, la, sg = run(segs, ends, None, 128, 128, 64, ASC)
    # ascending, window 0 is never written: [50, 64) is read where it lies, [64, 82) is saved
    assert tot["stash_bytes"] == 18 and [int(k) for k in la["kind"]] == [ref.SAVE, ref.WRITE]


def test_segment_spanning_five_windows():
    ends = chunks(5 * 64 + 40, 90)
    segs = [[0, ends[-1], 7, 0, len(ends), SELF]]
    tot, la, sg = run(segs, ends, None, ends[-1] + 7, ends[-1], 64, ASC, skew=3)
    assert tot["windows"] == 6 and sum(int(l["kind"]) == ref.WRITE for l in la) == 6
    tot, la, sg = run([[0, ends[-1], 0, 0, len(ends), NULL]], ends, None, 0, ends[-1], 64)
    assert tot["windows"] == 6 and tot["launches"] == 6 and tot["stash_peak"] == 0


def test_growth_from_nothing_and_shrink_to_nothing():
    ends = chunks(100, 30)
    tot, la, _ = run([[0, 100, 0, 0, len(ends), STORE]], ends, None, 0, 100, 16)
    assert tot["written_bytes"] == 100 and tot["stash_peak"] == 0
    tot, la, _ = run([], [], None, 100, 0, 16)
    assert len(la) == 0


# ---- refusals ---------------------------------------------------------------------
def plan_rc(rows, ends, keep=None, have_len=100, new_len=100, skew=0, tile=TILE, window=16,
            stash_cap=1 << 20, flags=0):
    return ref.schedule(ref.make_segs(rows), ends, keep, have_len, new_len, skew, tile, window,
                        stash_cap, flags)[0]


def test_validation_refusals():
    ends = [40, 100]
    good = [[0, 40, 60, 0, 1, SELF], [40, 60, 0, 1, 1, STORE]]
    assert plan_rc(good, ends) == 0
    INVAL = _lib.DSX_E_INVAL
    assert plan_rc(good[::-1], ends) == INVAL                                   # descending
    assert plan_rc([[0, 40, 60, 0, 1, SELF], [30, 70, 0, 1, 1, STORE]], ends) == INVAL  # overlap
    assert plan_rc(good, ends, new_len=99) == INVAL                             # beyond new_len
    assert plan_rc([[0, 40, 61, 0, 1, SELF]], ends) == INVAL                    # SELF beyond have_len
    assert plan_rc([[0, 40, 2 ** 64 - 8, 0, 1, SELF]], ends) == INVAL           # ... with a wrap
    assert plan_rc([[0, 40, 0, 0, 1, SELF]], ends, have_len=39) == INVAL
    assert plan_rc([[40, 60, 0, 1, 2, STORE]], ends) == INVAL                   # first + count > n
    assert plan_rc([[40, 60, 0, 0xFFFFFFFF, 0xFFFFFFFF, STORE]], ends) == INVAL
    assert plan_rc([[40, 60, 0, 2, 0, STORE]], ends) == INVAL                   # bytes without chunks
    assert plan_rc([[0, 41, 0, 0, 1, STORE]], ends) == INVAL                    # bytes != chunk sizes
    assert plan_rc([[1, 40, 0, 0, 1, STORE]], ends) == INVAL                    # dst_off != chunk start
    assert plan_rc([[0, 40, 0, 0, 1, -5]], ends) == INVAL                       # unknown source
    assert plan_rc(good, [100, 40]) == INVAL                                    # ends decrease
    assert plan_rc(good, [40, 101]) == INVAL                                    # ends beyond new_len
    for window in (0, 8, 24):
        assert plan_rc(good, ends, window=window) == INVAL                      # no multiple of tile
    assert plan_rc(good, ends, tile=0) == INVAL
    assert plan_rc(good, ends, skew=TILE) == INVAL
    for flags in (1, 128, 256, ASC | DESC, 1 << 31):
        assert plan_rc(good, ends, flags=flags) == INVAL                        # unknown flag bits
    # descending, [60, 100) is overwritten before [0, 40) reads it: 40 bytes through the stash
    assert plan_rc(good, ends, stash_cap=39, flags=DESC) == _lib.DSX_E_CAPACITY
    assert plan_rc(good, ends, stash_cap=40, flags=DESC) == 0
    assert plan_rc(good, ends, stash_cap=0) == 0                                # (ascending: none)


def test_output_capacity_reports_the_counts():
    ends = chunks(200, 20)
    segs = ref.make_segs([[0, 200, 0, 0, len(ends), STORE]])
    e = np.asarray(ends, dtype=np.uint64)
    tot = _lib.InplaceTotals()
    la = np.zeros(1, dtype=ref.LAUNCH_DTYPE)
    sg = np.zeros(1, dtype=ref.SEG_DTYPE)
    rc = _lib.lib().dsx_inplace_plan(segs.ctypes.data, 1, e.ctypes.data, e.size, None, 0, 200, 0, TILE,
                                     16, 0, 0, la.ctypes.data, 1, sg.ctypes.data, 1, ctypes.byref(tot))
    assert rc == _lib.DSX_E_CAPACITY and tot.stash_peak == 0
    assert tot.launches == 13 and tot.segments == 13
    assert not la["nsegs"].any()  # nothing was listed


# ---- ABI and binding -----------------------------------------------------------------
def test_abi_and_binding():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "dsx.h")).read()
    for name in ("dsx_inplace_plan", "dsx_assemble_inplace", "dsx_chunk_keep"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, hdr)
    assert L.dsx_abi_version() == 5
    tot = _lib.InplaceTotals()
    assert L.dsx_inplace_plan(None, 0, None, 0, None, 0, 0, 0, TILE, 16, 0, 0, None, 0, None, 0,
                              None) == _lib.DSX_E_INVAL
    assert L.dsx_inplace_plan(None, 1, None, 0, None, 0, 0, 0, TILE, 16, 0, 0, None, 0, None, 0,
                              ctypes.byref(tot)) == _lib.DSX_E_INVAL
    assert L.dsx_inplace_plan(None, 0, None, 1, None, 0, 0, 0, TILE, 16, 0, 0, None, 0, None, 0,
                              ctypes.byref(tot)) == _lib.DSX_E_INVAL
    assert L.dsx_inplace_plan(None, 0, None, 0, None, 0, 0, 0, TILE, 16, 0, 0, None, 5, None, 0,
                              ctypes.byref(tot)) == _lib.DSX_E_INVAL
    assert L.dsx_inplace_plan(None, 0, None, 0, None, 0, 0, 0, TILE, 16, 0, 0, None, 0, None, 0,
                              ctypes.byref(tot)) == 0
    assert L.dsx_assemble_inplace(None, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, 0, 0,
                                  0, 0, 0, None) == _lib.DSX_E_INVAL
    assert L.dsx_chunk_keep(None, None, 0, None, 0, None, 0, None, None, 0) == _lib.DSX_E_INVAL
    assert ctypes.sizeof(_lib.InplaceLaunch) == 48 and ctypes.sizeof(_lib.InplaceTotals) == 72


def test_replay_program_builds_and_runs_without_hip(tmp_path):
    """dsx_inplace_plan.h includes nothing of HIP: a plain C++ compiler builds
    tests/inplace_replay.cpp (the program meant for
    -fsanitize=address,undefined) against it, and its own brute-force executor
    agrees with every schedule of its sweep."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "inplace_replay")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "inplace_replay.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, (r.stdout, r.stderr)
