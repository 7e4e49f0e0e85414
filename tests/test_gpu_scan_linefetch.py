"""The line fetch and the hit path of scanl_kernel against the
oracle and against the kernel without the rotating frame (DSX_SCAN_ROTF=0).

fetch() treats a line by where it stands: the SIMD partner's progress is
exchanged once per trip, at the trip's first line, and only a region's lines 0
and 1 carry the trace's test; the last line of a region runs the region-end
arm (the successor region and its first line).  What can go wrong there shows
at the first and last lines of a region, at a piece's end, and where a wave
changes its lane geometry.  The `halves` case pins the rare path of a 16-byte
group whose two 8-byte halves are hit in different lanes of a wave.

Cases, all in ONE child process with a DSX_SCAN_ROTF=1 and a =0 context:
  one     8 MiB + 777, 778, 779 and 780 B at 16K/64K/256K: lane segments of
          384 B, one trip, so every line is a region's first or last; the four
          lengths put the piece end on every byte of a dword; a window is
          planted so that the piece's last position and the one 100 before it
          are candidates.  Candidates through dsx_shard_local's record
          (tests/test_gpu_scan_group16.py: the scan's own list, up to 32 * max
          = 8 MiB) and, for the piece's end, cuts at 48/64K/256K
  trips   the smallest blob with lane segments of 768 B (two trips) at
          48/64K/256K, with that file's plants: cuts against the oracle
  two     the smallest piece that has two region sizes under
          DSX_LANE_TARGET=768 DSX_TAIL_SPLIT=2 (tests/scan_two_size.cpp finds it
          from scan_geom on the CPU: about 300 MB, S = 768 and S2 = 384): a wave
          crosses from the big regions to the tail ones and issues the first
          line of a region with the other geometry.  Cuts against
          oracle.chunk_parallel and against DSX_SCAN_ROTF=0
  halves  the `one` shape with candidates at byte 3 of a 16-byte group in one
          lane and at byte 12 of the same group in another lane of the same
          region (both halves must run), a group with byte 3 only and one with
          byte 12 only; at 16K/64K/256K (odd d) and at 4K/16K/64K (d = 12318,
          even: the rotate form).  That no other lane of the region has a
          candidate in those groups is asserted on the oracle's list
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("one", "trips", "two", "halves")
D64 = (16 << 10, 64 << 10, 256 << 10)
D16 = (4 << 10, 16 << 10, 64 << 10)
NREC = (8 << 20) + 777
NCAP = 1024
TWO_ENV = {"DSX_LANE_TARGET": "768", "DSX_TAIL_SPLIT": "2"}


def _library():
    from desync_amd import _lib
    if "DSX_SCAN_ROTF" in _lib.PRODUCT_ENV:
        return os.path.join(REPO, "desync_amd", "libdsx.so")
    assert "DSX_SCAN_ROTF" in _lib.DIAG_ENV
    return os.path.join(REPO, "desync_amd", "libdsx_diag.so")


def test_linefetch_candidates_equal_oracle_and_parent():
    path = _library()
    assert os.path.exists(path), path + " missing: __graft_entry__.build() makes it"
    env = dict(os.environ, DSX_LIB_PATH=path, PYTHONPATH=REPO)
    for k in ("DSX_SCAN_ROTF",) + tuple(TWO_ENV):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for name in CASES:
        assert f"case {name} ok" in r.stdout, r.stdout[-3000:]


def two_size_piece(ncu, tmp):
    """(len, S, S2, nbig, nregions) of the smallest two-size piece, by scan_geom."""
    import shutil
    cxx = next((p for p in map(shutil.which, ("g++", "c++", "clang++")) if p), "/opt/rocm/llvm/bin/clang++")
    exe = os.path.join(tmp, "scan_two_size")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                    "-I" + os.path.join(REPO, "desync_amd", "csrc"),
                    os.path.join(REPO, "tests", "scan_two_size.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe, str(ncu)], check=True, capture_output=True, text=True, timeout=60).stdout
    return tuple(int(x) for x in out.split())


def halves_spots(S):
    """(lane, byte y) of the planted candidates: groups 5 (both halves, in lanes
    9 and 41 of region 3), 9 (byte 3 only) and 14 (byte 12 only) of region 3."""
    assert S == 384
    return [(64 * 3 + 9, 16 * 5 + 3), (64 * 3 + 41, 16 * 5 + 12), (64 * 3 + 20, 16 * 9 + 3),
            (64 * 3 + 50, 16 * 14 + 12)]


def _main():
    import tempfile

    import torch

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import test_gpu_scan_group16 as g16

    import desync_amd
    from desync_amd import _lib
    from oracle import oracle as o
    from oracle import seam as oseam
    L = _lib.lib()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = ncu * 8 * 64

    def contexts(extra):
        cs = {}
        os.environ.update(extra)
        for rotf in ("1", "0"):
            os.environ["DSX_SCAN_ROTF"] = rotf
            cs[rotf] = _lib.Context(0)
        for k in ("DSX_SCAN_ROTF",) + tuple(extra):
            os.environ.pop(k, None)
        return cs

    ctxs = contexts({})
    ctxs2 = contexts(TWO_ENV)

    def dev(blob):
        t = torch.from_numpy(blob).to("cuda")
        torch.cuda.synchronize()
        assert t.data_ptr() % 128 == 0  # delta 0: the plants are placed by it
        return t

    def record(c, t, n, prm):
        rec = _lib.Seam()
        p = desync_amd.Params(*prm)
        _lib.check(L.dsx_shard_local(c.h, ctypes.c_void_p(t.data_ptr()), 0, 0, n, n, ctypes.byref(p.c),
                                     ctypes.c_void_p(ctypes.addressof(rec)), 0), c.h)
        assert rec.ncands <= NCAP and rec.ncuts <= NCAP
        return rec

    def check_record(name, blob, n, prm, exp):
        t = dev(blob)
        for r, c in ctxs.items():
            before = c.stats().pieces
            rec = record(c, t, n, prm)
            cands, cuts = list(rec.cands[:rec.ncands]), list(rec.cuts[:rec.ncuts])
            miss = sorted(set(exp["cands"]) - set(cands))
            extra = sorted(set(cands) - set(exp["cands"]))
            assert cands == exp["cands"], (f"{name} n={n} DSX_SCAN_ROTF={r}: candidates missing {miss[:8]}, "
                                           f"spurious {extra[:8]}")
            assert cuts == exp["cuts"], f"{name} n={n} DSX_SCAN_ROTF={r}: cuts differ"
            assert (rec.window_end, rec.exit_cut) == (exp["window_end"], exp["exit_cut"])
            assert c.stats().pieces - before == 1 and c.stats().dense_fallbacks == 0
        del t

    def oracle_record(blob, n, prm):
        exp = oseam.shard_local(blob, 0, n, n, *prm)[0]
        assert 48 not in exp["cands"] and len(exp["cands"]) < NCAP and len(exp["cuts"]) < NCAP
        return exp

    try:
        # ---- one: M = 1, the piece end on every byte of a dword
        w = g16.find_window(D64, 41)
        k, x = g16.find_pair(w, o.discriminator(D64[1]))
        base = o.synth_uniform(141, 0, NREC + 3)
        total = ncuts = 0
        for extra in range(4):
            n = NREC + extra
            assert g16.lane_bytes(n, lanes) == 384 and n % 4 == (1 + extra) % 4
            blob = base[:n].copy()
            if extra == 0:
                g16.plant(blob, 384, w, k, x, True)
            blob[n - 48:n] = w          # the piece's last position
            blob[n - 148:n - 100] = w   # ... and the one 100 before it
            exp = oracle_record(blob, n, D64)
            total += len(exp["cands"])
            check_record("one", blob, n, D64, exp)
            # (the record's window ends at 32 * max = 8 MiB, before the piece's
            # end: the last positions show in the cuts at min = 48, where every
            # candidate 48 bytes behind a cut is a cut)
            want = o.chunk_stream(blob, *g16.CUT)
            assert n - 100 in set(want.tolist()), "the planted position is no cut"
            t = dev(blob)
            for r, c in ctxs.items():
                got = np.asarray(desync_amd.cut_device(t.data_ptr(), n, *g16.CUT, ctx=c), dtype=np.uint64)
                assert np.array_equal(got, want), f"one n={n} DSX_SCAN_ROTF={r}: cuts differ from the oracle"
            ncuts += want.size
            del t
        print(f"case one ok ({total} candidates, {ncuts} cuts over 4 lengths)", flush=True)

        # ---- trips: two trips per lane segment
        blob, planted, want = g16.cuts_case(lanes)
        t = dev(blob)
        got = {r: np.asarray(desync_amd.cut_device(t.data_ptr(), blob.size, *g16.CUT, ctx=c), dtype=np.uint64)
               for r, c in ctxs.items()}
        assert np.array_equal(got["1"], want), "trips: the rotating frame differs from the oracle"
        assert np.array_equal(got["0"], got["1"]), "trips: the two kernels differ"
        print(f"case trips ok ({want.size} cuts, {len(planted)} planted)", flush=True)
        del t, blob

        # ---- two: the smallest piece with two region sizes
        with tempfile.TemporaryDirectory() as tmp:
            n, S, S2, nbig, nregions = two_size_piece(ncu, tmp)
        assert S2 != 0 and (S, S2) == (768, 384) and 0 < nbig < nregions, (n, S, S2, nbig, nregions)
        assert n < (1 << 29), n
        t = torch.empty(n, dtype=torch.uint8, device="cuda")
        _lib.check(L.dsx_gen_uniform(ctxs2["0"].h, ctypes.c_void_p(t.data_ptr()), 0, n, 11), ctxs2["0"].h)
        torch.cuda.synchronize()
        assert t.data_ptr() % 128 == 0
        want = o.chunk_parallel(t.cpu().numpy(), *D64, o.default_threads())
        before = {r: c.stats().pieces for r, c in ctxs2.items()}
        got = {r: np.asarray(desync_amd.cut_device(t.data_ptr(), n, *D64, ctx=c), dtype=np.uint64)
               for r, c in ctxs2.items()}
        assert np.array_equal(got["1"], want), "two: the rotating frame differs from the oracle"
        assert np.array_equal(got["0"], got["1"]), "two: the two kernels differ"
        for r, c in ctxs2.items():
            assert c.stats().pieces - before[r] == 1 and c.stats().dense_fallbacks == 0
        print(f"case two ok ({n} bytes, {nbig} big regions of {nregions}, {want.size} cuts)", flush=True)
        del t

        # ---- halves: the two halves of a group hit in different lanes
        for prm, seed in ((D64, 41), (D16, 43)):
            w = g16.find_window(prm, seed)
            blob = o.synth_uniform(seed + 200, 0, NREC).copy()
            S = g16.lane_bytes(NREC, lanes)
            spots = halves_spots(S)
            for ln, y in spots:
                p = ln * S + y + 1
                blob[p - 48:p] = w
            exp = oracle_record(blob, NREC, prm)
            where = {}  # (region, group) -> [(lane, byte of the group)] of every candidate in the main loop
            for c in exp["cands"]:
                ln, y = divmod(c - 1, S)
                where.setdefault((ln // 64, y // 16), []).append((ln, y % 16))
            assert sorted(where[(3, 5)]) == [(64 * 3 + 9, 3), (64 * 3 + 41, 12)], where[(3, 5)]
            assert where[(3, 9)] == [(64 * 3 + 20, 3)] and where[(3, 14)] == [(64 * 3 + 50, 12)]
            check_record("halves", blob, NREC, prm, exp)
        print("case halves ok (odd and even d)", flush=True)
    finally:
        for c in list(ctxs.values()) + list(ctxs2.values()):
            c.close()


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    _main()
