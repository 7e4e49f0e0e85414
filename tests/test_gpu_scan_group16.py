"""The 16-byte test groups of scanl_kernel<ROTF>: a candidate
at every place of a group, at the seams between groups, trips, lane segments
and regions, and two candidates in one group, against the oracle and against
the kernel without the rotating frame (DSX_SCAN_ROTF=0), which tests 8 bytes
at a time.

The rotating-frame kernel pairs the 8-byte subgroups (2j, 2j+1): one compare
and branch per 16 bytes, one hit entry {16 hit bits << 16 | offset of the
group} per lane and group.  A candidate depends only on the 48 bytes before it,
so the test finds one 48-byte window with h % d == d - 1 on the CPU (the first
candidate of a seeded buffer, by the oracle) and plants copies of it in a
seeded uniform blob so that the candidate falls on a chosen byte y of a chosen
lane segment (entry group y // 16, bit y % 16):

  bits    every bit 0..15 of a group, in 16 lanes and 16 different groups
  edge    the last byte of one group, the first byte of the next
  end     the last position of a lane segment (offset S), and offsets 1, 2,
          16, 17, 32, 33, 47, 48 of the next one, which the lane before tests
          in its handoff extension (S + 1 .. S + 48); the same behind a region
          border, where lane 0 takes its window from the warm-up line
  trip    the last byte of a trip, the first byte and a middle byte of the next
  spill   six candidates in six groups of one lane: more entries than kHitRegs
  pairs   two candidates k <= 3 bytes apart (the window plus k searched bytes
          whose window is a candidate too: 2^24 trials for k = 3): both in one
          group, across a group border, in the handoff extension, across a
          lane border

Cases, all in ONE child process with a DSX_SCAN_ROTF=1 and a =0 context:
  rec64   8 MiB + 777 B at 16K/64K/256K (odd d, lane segments of 384 B): the
          candidates through dsx_shard_local's record, whose cands[] is the
          scan's own list (tests/test_gpu_seam_record.py), so the second
          candidate of a pair shows although the chain never cuts there
  rec16   the same at 4K/16K/64K: d = 12318 is even, the rotate form of the
          rare path over 16 values (its window is 2 MiB; the plants lie in the
          first 600 KB)
  cuts    a blob just large enough for lane segments of 768 B (two trips) at
          48/64K/256K: with min = 48 every planted candidate is a cut
          (asserted on the oracle's list before the GPU runs), pairs left out
  two     4 GiB - 999 B at the default parameters: the two-size instantiation
          with tail regions (tests/test_gpu_variants.py's shape), no plants
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("rec64", "rec16", "cuts", "two")
D64 = (16 << 10, 64 << 10, 256 << 10)
D16 = (4 << 10, 16 << 10, 64 << 10)
CUT = (48, 64 << 10, 256 << 10)
NREC = (8 << 20) + 777
NCAP = 1024


def _library():
    from desync_amd import _lib
    if "DSX_SCAN_ROTF" in _lib.PRODUCT_ENV:
        return os.path.join(REPO, "desync_amd", "libdsx.so")
    assert "DSX_SCAN_ROTF" in _lib.DIAG_ENV
    return os.path.join(REPO, "desync_amd", "libdsx_diag.so")


def test_group16_candidates_equal_oracle_and_parent():
    path = _library()
    assert os.path.exists(path), path + " missing: __graft_entry__.build() makes it"
    env = dict(os.environ, DSX_LIB_PATH=path, PYTHONPATH=REPO)
    env.pop("DSX_SCAN_ROTF", None)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for name in CASES:
        assert f"case {name} ok" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------ the plants
def find_window(prm, seed):
    """The 48 bytes before the first candidate of a seeded buffer."""
    from oracle import oracle as o
    buf = o.synth_uniform(seed, 0, 4 << 20)
    c = o.candidates(buf, *prm)
    assert c.size, "no candidate in 4 MiB"
    p = int(c[0])
    w = buf[p - 48:p].copy()
    d = o.discriminator(prm[1])
    assert o.window_hash(bytes(w)) % d == d - 1
    return w


def find_pair(w, d):
    """(k, x): k <= 3 bytes x after the window w so that the window ending k
    bytes later, w[k:] + x, is a candidate too; the smallest k that has one."""
    from oracle import oracle as o
    T = np.asarray(o.T, dtype=np.uint32)

    def rot(a, r):
        r &= 31
        return a if r == 0 else ((a << np.uint32(r)) | (a >> np.uint32(32 - r)))

    for k in (1, 2, 3):
        base = 0
        for j in range(48 - k):  # byte w[k + j] is byte j of the later window
            base ^= o.rotl32(int(T[int(w[k + j])]), 47 - j)
        h = np.full((1,) * k, base, np.uint32)
        for m in range(k):  # x[m] is byte 48 - k + m of it
            shape = [1] * k
            shape[m] = 256
            h = h ^ rot(T, k - 1 - m).reshape(shape)
        hit = np.argwhere(h % np.uint32(d) == np.uint32(d - 1))
        if hit.size:
            x = np.array(hit[0], np.uint8)
            assert o.window_hash(bytes(w[k:]) + bytes(x)) % d == d - 1
            return k, x
    raise AssertionError("no pair within 3 bytes")


def plant_spots(S, k):
    """(lane, byte y in the lane segment, pair?) of every plant: the candidate
    is the cut after byte y, offset y + 1, entry group y // 16, bit y % 16."""
    lane = lambda r, l: 64 * r + l
    spots = []
    for b in range(16):  # bits
        spots.append((lane(2, 3 + 3 * b), 16 * ((5 + b) % 24) + b, False))
    spots += [(lane(3, 5), 16 * 7 + 15, False), (lane(3, 9), 16 * 8, False)]  # edge
    spots.append((lane(4, 10), S - 1, False))  # end: offset S
    for i, off in enumerate((1, 2, 16, 17, 32, 33, 47, 48)):  # ... and the handoff extension
        spots.append((lane(4, 20 + 4 * i), off - 1, False))
    spots += [(lane(5, 0), 0, False), (lane(6, 0), 47, False), (lane(7, 0), 19, False)]  # region border
    spots.append((lane(5, 40), S - 1, False))
    spots += [(lane(8, 7), 384 + 16 * 3 + 5, False), (lane(8, 20), 383, False), (lane(8, 30), 384, False)]  # trip
    spots += [(lane(8, 44), S - 384 + 16 * 11 + 9, False)]  # (the last trip of a region)
    spots += [(lane(9, 17), 63 + 64 * i, False) for i in range(5)] + [(lane(9, 17), 376, False)]  # spill
    spots += [(lane(10, 11), 16 * 4 + 2, True),          # both in one group
              (lane(10, 30), 16 * 9 + 16 - k, True),     # bit 16 - k, bit 0 of the next group
              (lane(10, 50), 16 * 12 + 15 - k, True),    # ..., bit 15
              (lane(11, 5), 9, True),                    # in the handoff extension of lane 4
              (lane(11, 25), S - 1, True),               # offset S, offset k of the next lane
              (lane(11, 40), 16 * 22 + 16 - k, True)]    # into the last group of a trip
    return spots


def plant(blob, S, w, k, x, pairs):
    """Plants into blob (delta 0: the grid starts at the blob); returns the
    sorted candidate positions planted."""
    want = []
    for ln, y, pair in plant_spots(S, k):
        if pair and not pairs:
            continue
        p = ln * S + y + 1
        assert p >= 48 + 1 and p + 4 < blob.size
        blob[p - 48:p] = w
        want.append(p)
        if pair:
            blob[p:p + k] = x
            want.append(p + k)
    assert len(set(want)) == len(want)
    return sorted(want)


def lane_bytes(n, lanes):
    """S of the line scan over a piece of n bytes from a line-aligned pointer
    (dsx_scan_geom.h under the context's defaults, as _geometry of
    tests/test_gpu_seam_record.py restates it)."""
    assert n <= 2 * 384 * lanes
    return 768 if n > 384 * lanes else 384


def rec_case(prm, seed, lanes):
    """(blob, planted positions, the oracle's record) of a record case."""
    from oracle import oracle as o
    from oracle import seam as oseam
    d = o.discriminator(prm[1])
    w = find_window(prm, seed)
    k, x = find_pair(w, d)
    blob = o.synth_uniform(seed + 100, 0, NREC).copy()
    planted = plant(blob, lane_bytes(NREC, lanes), w, k, x, True)
    exp = oseam.shard_local(blob, 0, NREC, NREC, *prm)[0]
    cands = exp["cands"]
    assert 48 not in cands and len(cands) < NCAP and len(exp["cuts"]) < NCAP
    assert exp["window_end"] == min(NREC, 32 * prm[2])
    missing = [p for p in planted if p not in set(cands)]
    assert not missing, f"planted positions that are no candidates: {missing}"
    return blob, planted, exp, k


def cuts_case(lanes):
    from oracle import oracle as o
    n = 384 * lanes + NREC
    S = lane_bytes(n, lanes)
    assert S == 768
    w = find_window(CUT, 31)
    blob = o.synth_uniform(131, 0, n).copy()
    planted = plant(blob, S, w, 0, None, False)
    want = o.chunk_stream(blob, *CUT)
    missing = sorted(set(planted) - set(want.tolist()))
    assert not missing, f"planted candidates that are no cuts: {missing}"
    return blob, planted, want


def _main():
    import torch

    import desync_amd
    from desync_amd import _lib, shard
    from oracle import oracle as o
    L = _lib.lib()
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 64

    ctxs = {}
    for rotf in ("1", "0"):
        os.environ["DSX_SCAN_ROTF"] = rotf
        ctxs[rotf] = _lib.Context(0)
    os.environ.pop("DSX_SCAN_ROTF", None)

    def dev(blob):
        t = torch.from_numpy(blob).to("cuda")
        torch.cuda.synchronize()
        assert t.data_ptr() % 128 == 0  # delta 0: plant() places by it
        return t

    def record(c, t, n, prm):
        rec = _lib.Seam()
        p = desync_amd.Params(*prm)
        _lib.check(L.dsx_shard_local(c.h, ctypes.c_void_p(t.data_ptr()), 0, 0, n, n, ctypes.byref(p.c),
                                     ctypes.c_void_p(ctypes.addressof(rec)), 0), c.h)
        assert rec.ncands <= NCAP and rec.ncuts <= NCAP
        return rec

    try:
        for name, prm, seed in (("rec64", D64, 41), ("rec16", D16, 43)):
            blob, planted, exp, k = rec_case(prm, seed, lanes)
            t = dev(blob)
            pieces = {r: c.stats().pieces for r, c in ctxs.items()}
            got = {r: record(c, t, NREC, prm) for r, c in ctxs.items()}
            for r, rec in got.items():
                cands, cuts = list(rec.cands[:rec.ncands]), list(rec.cuts[:rec.ncuts])
                miss = sorted(set(exp["cands"]) - set(cands))
                extra = sorted(set(cands) - set(exp["cands"]))
                assert cands == exp["cands"], (f"{name} DSX_SCAN_ROTF={r}: candidates missing {miss[:8]}, "
                                               f"spurious {extra[:8]} (planted: {[p for p in miss if p in planted]})")
                assert cuts == exp["cuts"], f"{name} DSX_SCAN_ROTF={r}: cuts differ"
                assert (rec.window_end, rec.exit_cut) == (exp["window_end"], exp["exit_cut"])
                assert ctxs[r].stats().pieces - pieces[r] == 1 and ctxs[r].stats().dense_fallbacks == 0
            print(f"case {name} ok ({len(exp['cands'])} candidates, {len(planted)} planted, pairs {k} apart)",
                  flush=True)
            del t

        blob, planted, want = cuts_case(lanes)
        t = dev(blob)
        got = {r: np.asarray(desync_amd.cut_device(t.data_ptr(), blob.size, *CUT, ctx=c), dtype=np.uint64)
               for r, c in ctxs.items()}
        assert np.array_equal(got["1"], want), "cuts: the rotating frame differs from the oracle"
        assert np.array_equal(got["0"], got["1"]), "cuts: the two kernels differ"
        print(f"case cuts ok ({want.size} cuts, {len(planted)} planted)", flush=True)
        del t, blob

        n = (4 << 30) - 999
        t = torch.empty(n, dtype=torch.uint8, device="cuda")
        _lib.check(L.dsx_gen_uniform(ctxs["0"].h, ctypes.c_void_p(t.data_ptr()), 0, n, 7), ctxs["0"].h)
        torch.cuda.synchronize()
        host = t.cpu().numpy()
        want = o.chunk_parallel(host, *D64, o.default_threads())
        before = {r: c.stats().pieces for r, c in ctxs.items()}
        got = {r: np.asarray(desync_amd.cut_device(t.data_ptr(), n, *D64, ctx=c), dtype=np.uint64)
               for r, c in ctxs.items()}
        assert np.array_equal(got["1"], want), "two: the rotating frame differs from the oracle"
        assert np.array_equal(got["0"], got["1"]), "two: the two kernels differ"
        for r, c in ctxs.items():  # (one piece: the two-size region geometry)
            assert c.stats().pieces - before[r] == 1
        print(f"case two ok ({want.size} cuts)", flush=True)
    finally:
        for c in ctxs.values():
            c.close()


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    _main()
