#!/usr/bin/env python3
"""dsx_store_copy's rate, on one MI355X, on the store of
tools/store_rate.py: a 4 GiB window of the dsx_gen_dedup stream (p = 0.5) cut at
16/64/256 KiB and put into an empty store, the source.  Cases, by which of the
source's entries are named (the IDs in HBM, in entry order), each copied into
an empty store:

  all            every entry;
  every_second   every second entry;
  all_flag       every entry by DSX_COPY_ALL (no ID list, no table of the call's);

and, in the same process and alternating with them,

  memcpy_d2d     hipMemcpyAsync device to device of the case's copied_bytes;
  composition    what the library needed for the same result before it had a
                 copy: dsx_store_locate of the IDs in the source, the offsets
                 and sizes read back, a segment list built on the host (numpy),
                 dsx_assemble out of the source's arena into a temporary blob
                 and dsx_store_put of that blob (that every ID is new to the
                 destination is given to it for nothing);
  put            dsx_store_put of the window itself into an empty store with its
                 own memcpy_d2d: the ratio the copy's is compared with.

Each is the median of REPS rounds after 2 warm-up rounds, timed with device
events on the context's stream around the synchronous call and by the host
clock.  Every timed call gets a fresh empty destination; creating it is outside
the timed region.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/copy_rate.json).  Run on the GPU box: python tools/copy_rate.py
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
from desync_amd import _lib, extract  # noqa: E402
from store_rate import Window, put  # noqa: E402

REPS = 10
vp = ctypes.c_void_p


def copy(ctx, dst, src, d_ids, n):
    """d_ids None: DSX_COPY_ALL"""
    tot = _lib.StoreCopyTotals()
    if d_ids is None:
        rc = _lib.lib().dsx_store_copy(ctx.h, dst.h, src.h, None, 0, ctypes.byref(tot), _lib.DSX_COPY_ALL)
    else:
        rc = _lib.lib().dsx_store_copy(ctx.h, dst.h, src.h, vp(d_ids.data_ptr()), n, ctypes.byref(tot),
                                       _lib.DSX_IDS_DEVICE)
    if rc:
        raise _lib.DsxError(rc, (_lib.lib().dsx_last_error(ctx.h) or b"").decode())
    return {k: getattr(tot, k) for k, _ in _lib.StoreCopyTotals._fields_}


def composition(ctx, dst, src, d_ids, n, packed):
    """locate -> D2H -> host segment list -> dsx_assemble into `packed` -> dsx_store_put."""
    L = _lib.lib()
    offs, sizes = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
    miss = ctypes.c_uint64()
    _lib.check(L.dsx_store_locate(ctx.h, src.h, vp(d_ids.data_ptr()), n, vp(offs.ctypes.data),
                                  vp(sizes.ctypes.data), ctypes.byref(miss), _lib.DSX_IDS_DEVICE), ctx.h)
    if miss.value:
        raise SystemExit("the source does not hold its own IDs")
    ends = np.cumsum(sizes).astype(np.uint64)
    segs = np.zeros(n, dtype=extract.SEG_DTYPE)
    segs["dst_off"] = ends - sizes
    segs["bytes"] = sizes
    segs["src_off"] = offs
    segs["first"] = np.arange(n, dtype=np.uint32)
    segs["count"] = 1
    segs["source"] = _lib.DSX_SRC_STORE
    segs["seed_first"] = 0xFFFFFFFF
    total = int(ends[-1]) if n else 0
    base, used = src.arena()
    _lib.check(L.dsx_assemble(ctx.h, vp(segs.ctypes.data), n, None, None, 0, vp(base), used,
                              vp(packed.data_ptr()), total, _lib.DSX_STORE_DEVICE), ctx.h)
    tot = _lib.StorePutTotals()
    rc = L.dsx_store_put(ctx.h, dst.h, vp(packed.data_ptr()), total, vp(d_ids.data_ptr()), vp(ends.ctypes.data),
                         0, n, ctypes.byref(tot), _lib.DSX_IDS_DEVICE)
    if rc:
        raise _lib.DsxError(rc, (L.dsx_last_error(ctx.h) or b"").decode())
    return tot.stored, tot.stored_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--gib", type=float, default=4.0)
    args = ap.parse_args()
    size = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    ctx = _lib.default_context(0)
    L = _lib.lib()
    sp = vp()
    _lib.check(L.dsx_ctx_stream(ctx.h, ctypes.byref(sp)), ctx.h)
    stream = torch.cuda.ExternalStream(sp.value, device="cuda:0")
    hip = hip_runtime()

    target = Window(ctx, 8 * size, size)
    packed = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    src = desync_amd.DeviceStore(size, target.n, ctx=ctx)
    tot_put = put(ctx, src, target)
    ids, ends = src.entries()
    filled = src.counts()
    n = len(ends)
    picks = {"all": np.arange(n), "every_second": np.arange(0, n, 2)}
    d_ids = {k: torch.from_numpy(np.ascontiguousarray(ids[p]).reshape(-1).copy()).to("cuda:0")
             for k, p in picks.items()}
    d_ids["all_flag"] = None
    picks["all_flag"] = picks["all"]
    torch.cuda.synchronize()

    def fresh():
        return desync_amd.DeviceStore(size, target.n, ctx=ctx)

    # every case once, checked: the totals, the entries, the verify, and the composition's store
    totals = {}
    for k, p in picks.items():
        dst = fresh()
        t = totals[k] = copy(ctx, dst, src, d_ids[k], len(p))
        got_ids, got_ends = dst.entries()
        starts = np.concatenate(([0], ends[:-1])).astype(np.uint64)
        want_ends = np.cumsum((ends - starts)[p]).astype(np.uint64)
        if (t["copied"], t["present"], t["repeats"], t["missing"]) != (len(p), 0, 0, 0) \
                or not np.array_equal(got_ids, ids[p]) or not np.array_equal(got_ends, want_ends) or dst.Verify():
            raise SystemExit(f"{k}: the copied store is wrong")
        dst.close()
        if d_ids[k] is not None:
            dst = fresh()
            if composition(ctx, dst, src, d_ids[k], len(p), packed) != (t["copied"], t["copied_bytes"]) \
                    or not np.array_equal(dst.entries()[1], want_ends):
                raise SystemExit(f"{k}: the composition gives another store")
            dst.close()

    names = [f"{what}_{k}" for k in picks for what in ("copy", "memcpy_d2d")]
    names += [f"composition_{k}" for k in picks if d_ids[k] is not None] + ["put", "memcpy_d2d_put"]
    timers = {k: Timer(stream) for k in names}
    for rep in range(2 + REPS):
        rec = rep >= 2
        for k, p in picks.items():
            dst = fresh()
            timers[f"copy_{k}"].run(lambda: copy(ctx, dst, src, d_ids[k], len(p)), record=rec)
            dst.close()
            if d_ids[k] is not None:
                dst = fresh()
                timers[f"composition_{k}"].run(lambda: composition(ctx, dst, src, d_ids[k], len(p), packed),
                                               record=rec)
                dst.close()
            nbytes = totals[k]["copied_bytes"]
            timers[f"memcpy_d2d_{k}"].run(
                lambda: hip.hipMemcpyAsync(packed.data_ptr(), target.blob.data_ptr(), nbytes, HIP_D2D, sp),
                record=rec)
        dst = fresh()
        timers["put"].run(lambda: put(ctx, dst, target), record=rec)
        dst.close()
        timers["memcpy_d2d_put"].run(
            lambda: hip.hipMemcpyAsync(packed.data_ptr(), target.blob.data_ptr(), tot_put["stored_bytes"], HIP_D2D,
                                       sp), record=rec)

    rows = {k: {"device": summary(t.dev), "host_clock": summary(t.host)} for k, t in timers.items()}
    put_ratio = rows["put"]["device"]["ms_median"] / rows["memcpy_d2d_put"]["device"]["ms_median"]
    cases = {}
    for k in picks:
        ms = rows[f"copy_{k}"]["device"]["ms_median"]
        d2d = rows[f"memcpy_d2d_{k}"]["device"]["ms_median"]
        c = {"totals": totals[k], "ms_median": ms, "time_over_memcpy_d2d": round(ms / d2d, 3),
             "memcpy_d2d_over_time": round(d2d / ms, 3),
             "TBps_read_plus_written": round(2 * totals[k]["copied_bytes"] / (ms * 1e-3) / 1e12, 3)}
        if f"composition_{k}" in rows:
            comp = rows[f"composition_{k}"]
            c["time_over_composition"] = round(ms / comp["device"]["ms_median"], 3)
            c["host_time_over_composition"] = round(rows[f"copy_{k}"]["host_clock"]["ms_median"] /
                                                    comp["host_clock"]["ms_median"], 3)
        cases[k] = c
    res = {"window_bytes": size, "chunks": target.n, "store": filled, "reps": REPS, "cases": cases,
           "put": {"totals": tot_put, "time_over_memcpy_d2d": round(put_ratio, 3),
                   "memcpy_d2d_over_time": round(1 / put_ratio, 3)},
           "rows": rows}
    src.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
