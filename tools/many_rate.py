#!/usr/bin/env python3
"""dsx_cut_device_many's rate, on one MI355X.

4 GiB of the seed-3 uniform stream (dsx_gen_uniform) cut at 16/64/256 KiB, as
three packed shapes:

  64k      65,536 blobs of 64 KiB;
  1m       4,096 blobs of 1 MiB;
  loguni   seeded log-uniform lengths from 4 KiB to 64 MiB.

For each shape, alternating in one process:

  many     one dsx_cut_device_many call (device output);
  loop     what the library offered before: a loop of synchronous
           dsx_cut_device calls, one per blob (device output, blob-relative);
  whole    one dsx_cut_device over the whole buffer: the floor, and another
           result (no cut at the blob boundaries).

and a sweep of one blob of 1 MiB .. 1 GiB through the batched walk (big_blob
at its maximum) and through the one-blob path (big_blob = 1): the crossing is
where one blob alone is better off on the one-blob path.  A shape that has
blobs of that length or more is also timed with big_blob set to the crossing
(many_big_blob_at_crossing): in a batch a single blob costs a host round trip
of its own, a long chain in the batched walk runs beside the others.

Every call is synchronous (it ends in a wait for the context's stream), so the
host clock around it times the device work and the round trips.  Each figure
is the median [min-max] of REPS rounds after 2 warm-up rounds.  Every timed
many result is compared on the device with the loop's result, every timed loop
and whole result with its first one, and the loop's result of the blobs in the
first --oracle-mib MiB with the CPU oracle.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/many_rate.json).  Run on the GPU box: python tools/many_rate.py
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import desync_amd  # noqa: E402
from desync_amd import _lib  # noqa: E402
from oracle import oracle as o  # noqa: E402

REPS = 10
WARM = 2
PARAMS = (16 * 1024, 64 * 1024, 256 * 1024)
vp = ctypes.c_void_p
KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30


def summary(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4),
            "ms_max": round(float(a.max()), 4), "n": int(a.size)}


def shapes(size):
    rng = np.random.default_rng(3)
    lens, total = [], 0
    while total < size:
        n = int(np.exp(rng.uniform(np.log(4 * KiB), np.log(64 * MiB))))
        n = min(n, size - total)
        lens.append(n)
        total += n
    return {"64k": np.full(size // (64 * KiB), 64 * KiB, dtype=np.uint64),
            "1m": np.full(size // MiB, MiB, dtype=np.uint64),
            "loguni": np.array(lens, dtype=np.uint64)}


class Bench:
    def __init__(self, size):
        self.ctx = _lib.default_context(0)
        self.L = _lib.lib()
        self.p = desync_amd.Params(*PARAMS)
        self.size = size
        self.blob = torch.empty(size, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        _lib.check(self.L.dsx_gen_uniform(self.ctx.h, vp(self.blob.data_ptr()), 0, size, 3), self.ctx.h)
        _lib.check(self.L.dsx_sync(self.ctx.h), self.ctx.h)
        self.cap = size // PARAMS[0] + 70000
        self.out = {k: torch.zeros(self.cap, dtype=torch.int64, device="cuda:0") for k in ("many", "loop", "whole")}
        torch.cuda.synchronize()

    def many(self, be, first, big_blob=0, group_bytes=0, length=None):
        opts = _lib.ManyOpts(big_blob, group_bytes)
        tot = _lib.ManyTotals()
        n = ctypes.c_uint64()
        _lib.check(self.L.dsx_cut_device_many(
            self.ctx.h, vp(self.blob.data_ptr()), int(be[-1]) if length is None else length, vp(be.ctypes.data),
            be.size, ctypes.byref(self.p.c), vp(self.out["many"].data_ptr()), self.cap, ctypes.byref(n),
            vp(first.ctypes.data), ctypes.byref(opts), ctypes.byref(tot), _lib.DSX_OUT_DEVICE), self.ctx.h)
        return n.value, {k: getattr(tot, k) for k, _ in _lib.ManyTotals._fields_ if k != "reserved"}

    def loop(self, be, first):
        """dsx_cut_device per blob; blob i's blob-relative cuts at out[first[i]:first[i+1]]"""
        base, optr, b0, at = self.blob.data_ptr(), self.out["loop"].data_ptr(), 0, 0
        n = ctypes.c_uint64()
        cut, h, pc, nref = self.L.dsx_cut_device, self.ctx.h, ctypes.byref(self.p.c), ctypes.byref(n)
        first[0] = 0
        for i, b1 in enumerate(be.tolist()):
            if b1 > b0:
                rc = cut(h, vp(base + b0), b1 - b0, pc, vp(optr + 8 * at), self.cap - at, nref, _lib.DSX_OUT_DEVICE)
                if rc:
                    _lib.check(rc, h)
                at += n.value
            first[i + 1] = at
            b0 = b1
        return at

    def whole(self, length):
        n = ctypes.c_uint64()
        _lib.check(self.L.dsx_cut_device(self.ctx.h, vp(self.blob.data_ptr()), length, ctypes.byref(self.p.c),
                                         vp(self.out["whole"].data_ptr()), self.cap, ctypes.byref(n),
                                         _lib.DSX_OUT_DEVICE), self.ctx.h)
        return n.value


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def run_shape(b, name, lens, oracle_bytes, cross):
    be = np.cumsum(lens).astype(np.uint64)
    length = int(be[-1])
    starts = np.concatenate([np.zeros(1, np.uint64), be[:-1]])
    f_many, f_loop = np.zeros(be.size + 1, np.uint64), np.zeros(be.size + 1, np.uint64)
    # the reference results: the loop's (absolute), checked against the oracle on a prefix
    n_loop = b.loop(be, f_loop)
    rel = b.out["loop"][:n_loop].clone()
    torch.cuda.synchronize()  # (torch's stream, not the context's)
    counts = np.diff(f_loop.astype(np.int64))
    add = torch.from_numpy(np.repeat(starts.astype(np.int64), counts)).to("cuda:0")
    want = rel + add
    nb = int(np.searchsorted(be, oracle_bytes, side="right"))
    if nb:
        host = b.blob[:int(be[nb - 1])].cpu().numpy()
        rel_h = rel[:int(f_loop[nb])].cpu().numpy().view(np.uint64)
        for i in range(nb):
            e = o.chunk_stream(host[int(starts[i]):int(be[i])], *PARAMS)
            if not np.array_equal(e, rel_h[int(f_loop[i]):int(f_loop[i + 1])]):
                raise SystemExit(f"{name}: the loop's blob {i} differs from the oracle")
    n_whole = b.whole(length)
    whole0 = b.out["whole"][:n_whole].clone()
    torch.cuda.synchronize()
    ms = {"many": [], "loop": [], "whole": []}
    # blobs at least as long as the sweep's crossing on the one-blob path
    at_cross = cross is not None and bool((lens >= cross).any())
    if at_cross:
        ms["many_big_blob_at_crossing"] = []
    totals = totals_cross = None
    for rep in range(WARM + REPS):
        t, (n, totals) = timed(lambda: b.many(be, f_many))
        if n != n_loop or not torch.equal(b.out["many"][:n], want) or not np.array_equal(f_many, f_loop):
            raise SystemExit(f"{name}: the many-blob result differs from the loop's")
        if rep >= WARM:
            ms["many"].append(t)
        if at_cross:
            t, (n, totals_cross) = timed(lambda: b.many(be, f_many, big_blob=cross))
            if n != n_loop or not torch.equal(b.out["many"][:n], want) or not np.array_equal(f_many, f_loop):
                raise SystemExit(f"{name}: the many-blob result with big_blob differs from the loop's")
            if rep >= WARM:
                ms["many_big_blob_at_crossing"].append(t)
        t, n = timed(lambda: b.loop(be, f_loop))
        if n != n_loop or not torch.equal(b.out["loop"][:n], rel):
            raise SystemExit(f"{name}: the loop's result changed")
        if rep >= WARM:
            ms["loop"].append(t)
        t, n = timed(lambda: b.whole(length))
        if n != n_whole or not torch.equal(b.out["whole"][:n], whole0):
            raise SystemExit(f"{name}: the whole-buffer result changed")
        if rep >= WARM:
            ms["whole"].append(t)
    row = {"blobs": int(be.size), "bytes": length, "chunks": int(n_loop), "whole_chunks": int(n_whole),
           "oracle_checked_blobs": nb, "totals": totals}
    if at_cross:
        row["totals_big_blob_at_crossing"] = totals_cross
    for k, v in ms.items():
        row[k] = summary(v)
        row[k]["GiBps_median"] = round(length / GiB / (row[k]["ms_median"] * 1e-3), 1)
    row["loop_over_many"] = round(row["loop"]["ms_median"] / row["many"]["ms_median"], 2)
    row["many_over_whole"] = round(row["many"]["ms_median"] / row["whole"]["ms_median"], 2)
    return row


def run_sweep(b):
    rows = []
    first = np.zeros(2, np.uint64)
    for length in [MiB << k for k in range(11) if (MiB << k) <= b.size]:
        be = np.array([length], dtype=np.uint64)
        n_ref = b.whole(length)
        ref = b.out["whole"][:n_ref].clone()
        torch.cuda.synchronize()
        ms = {"batched": [], "single": []}
        tot = {}
        for rep in range(WARM + REPS):
            for k, big in (("batched", 1 << 62), ("single", 1)):
                t, (n, tot[k]) = timed(lambda: b.many(be, first, big_blob=big, length=length))
                if n != n_ref or not torch.equal(b.out["many"][:n], ref):
                    raise SystemExit(f"sweep {length} {k}: differs from dsx_cut_device")
                if rep >= WARM:
                    ms[k].append(t)
        rows.append({"bytes": length, "chunks": int(n_ref), "batched": summary(ms["batched"]),
                     "single": summary(ms["single"]), "batched_redone": tot["batched"]["redone_blobs"],
                     "batched_was_single": tot["batched"]["single_blobs"]})
    cross = next((r["bytes"] for r in rows if r["single"]["ms_median"] <= r["batched"]["ms_median"]), None)
    return rows, cross


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--oracle-mib", type=int, default=256)
    ap.add_argument("--shapes", default="64k,1m,loguni")
    args = ap.parse_args()
    size = int(args.gib * GiB) // MiB * MiB
    b = Bench(size)
    res = {"params": PARAMS, "bytes": size, "reps": REPS, "warmup": WARM,
           "default_big_blob": (4096 - 8) * b.p.discriminator, "shapes": {}}
    res["sweep"], res["sweep_crossing_bytes"] = run_sweep(b)
    for name, lens in shapes(size).items():
        if name in args.shapes.split(","):
            res["shapes"][name] = run_shape(b, name, lens, args.oracle_mib * MiB, res["sweep_crossing_bytes"])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
