#!/usr/bin/env python3
"""dsx_chunk_ids_known's rate, on one MI355X, on the store of
tools/store_rate.py: a window of the dsx_gen_dedup stream (p = 0.5) cut at
16/64/256 KiB and put into an empty store; the window's ends in HBM, the IDs
and offsets written to HBM.  Windows of 1, 4 and 16 GiB, each three ways:

  all_known     the window itself against the store that holds it;
  every_100th   every 100th chunk changed by one byte, a third of the way into
                the chunk (outside the fingerprint's windows: the fingerprint
                passes, the compare finds the byte, the chunk is hashed);
  none_known    the same blob against an empty store;

and, in the same process and alternating with the call,

  ids_locate    what the library offered before: dsx_chunk_ids(DSX_OUT_DEVICE)
                followed by dsx_store_locate on those IDs;
  memcpy_d2d    hipMemcpyAsync device to device of the blob's bytes.

Before the timed rounds every case is checked: the call's IDs and offsets must
equal the old path's.  Each row is the median [min-max] of REPS rounds after 2
warm-up rounds, timed with device events on the context's stream around the
synchronous calls and by the host clock.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/known_rate.json).  Run on the GPU box: python tools/known_rate.py
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import desync_amd  # noqa: E402
from assemble_rate import HIP_D2D, Timer, hip_runtime, summary  # noqa: E402
from desync_amd import _lib  # noqa: E402
from store_rate import Window, put  # noqa: E402

REPS = 10
ALGO = _lib.DSX_DIGEST_SHA512_256
vp = ctypes.c_void_p


def window_rates(ctx, stream, sp, hip, size):
    L = _lib.lib()
    w = Window(ctx, 8 * size, size)
    n = w.n
    out = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    ids_new = torch.empty(n * 32, dtype=torch.uint8, device="cuda:0")
    ids_old = torch.empty(n * 32, dtype=torch.uint8, device="cuda:0")
    off_new = torch.empty(n, dtype=torch.int64, device="cuda:0")
    off_old = torch.empty(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    full = desync_amd.DeviceStore(size, n, ctx=ctx)
    tot_put = put(ctx, full, w)
    empty = desync_amd.DeviceStore(4096, 16, ctx=ctx)
    dev = _lib.DSX_OUT_DEVICE | _lib.DSX_ENDS_DEVICE
    last = {}

    def known(store):
        tot = _lib.KnownTotals()
        rc = L.dsx_chunk_ids_known(ctx.h, store.h, vp(w.blob.data_ptr()), size, 0, vp(w.d_ends.data_ptr()),
                                   n, ALGO, vp(ids_new.data_ptr()), vp(off_new.data_ptr()),
                                   ctypes.byref(tot), dev)
        if rc:
            raise _lib.DsxError(rc, (L.dsx_last_error(ctx.h) or b"").decode())
        last["totals"] = {k: getattr(tot, k) for k, _ in _lib.KnownTotals._fields_ if k != "reserved"}

    def ids_locate(store):
        _lib.check(L.dsx_chunk_ids(ctx.h, vp(w.blob.data_ptr()), size, 0, vp(w.d_ends.data_ptr()), n,
                                   vp(ids_old.data_ptr()), dev, ALGO), ctx.h)
        nm = ctypes.c_uint64()
        _lib.check(L.dsx_store_locate(ctx.h, store.h, vp(ids_old.data_ptr()), n, vp(off_old.data_ptr()),
                                      None, ctypes.byref(nm), _lib.DSX_IDS_DEVICE | _lib.DSX_OUT_DEVICE),
                   ctx.h)

    def memcpy():
        hip.hipMemcpyAsync(out.data_ptr(), w.blob.data_ptr(), size, HIP_D2D, sp)

    def edit():
        """One byte of every 100th chunk, a third of the way in."""
        starts = np.concatenate(([0], w.ends[:-1])).astype(np.int64)
        sizes = w.ends.astype(np.int64) - starts
        at = torch.from_numpy((starts + sizes // 3)[::100].copy()).to("cuda:0")
        w.blob[at] ^= 1
        torch.cuda.synchronize()
        return int(at.numel())

    cases = {}
    for name, store in (("all_known", full), ("every_100th", full), ("none_known", empty)):
        edited = edit() if name == "every_100th" else None
        known(store)
        ids_locate(store)
        if not (torch.equal(ids_new, ids_old) and torch.equal(off_new, off_old)):
            raise SystemExit(f"{name} at {size}: the call differs from dsx_chunk_ids + dsx_store_locate")
        totals = dict(last["totals"])
        want = {"all_known": 0, "every_100th": edited, "none_known": n}[name]
        if totals["hashed"] != want:
            raise SystemExit(f"{name} at {size}: {totals['hashed']} chunks hashed, not {want}")
        timers = {k: Timer(stream) for k in ("known", "ids_locate", "memcpy_d2d")}
        for rep in range(2 + REPS):
            rec = rep >= 2
            timers["known"].run(lambda: known(store), record=rec)
            timers["ids_locate"].run(lambda: ids_locate(store), record=rec)
            timers["memcpy_d2d"].run(memcpy, record=rec)
        rows = {k: {"device": summary(t.dev), "host_clock": summary(t.host)} for k, t in timers.items()}
        ms, old, d2d = (rows[k]["device"]["ms_median"] for k in ("known", "ids_locate", "memcpy_d2d"))
        cases[name] = {"totals": totals, "rows": rows, "ms_median": ms,
                       "time_over_ids_locate": round(ms / old, 4),
                       "time_over_memcpy_d2d": round(ms / d2d, 3),
                       "GiBps_blob": round(size / (ms * 1e-3) / (1 << 30), 1)}
    full.close()
    empty.close()
    return {"window_bytes": size, "chunks": n, "put": tot_put, "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--gib", type=float, nargs="+", default=[4.0, 1.0, 16.0])
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    sp = vp()
    _lib.check(_lib.lib().dsx_ctx_stream(ctx.h, ctypes.byref(sp)), ctx.h)
    stream = torch.cuda.ExternalStream(sp.value, device="cuda:0")
    hip = hip_runtime()
    res = {"reps": REPS, "ratios_are_of": "device-event medians around the synchronous calls", "windows": {}}
    for gib in args.gib:
        size = int(gib * (1 << 30)) // (1 << 20) * (1 << 20)
        res["windows"][f"{gib:g}GiB"] = window_rates(ctx, stream, sp, hip, size)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
