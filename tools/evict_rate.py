#!/usr/bin/env python3
"""dsx_store_evict's and dsx_store_touch's cost (Eviction), on one
MI355X, on the store of tools/store_rate.py: a 4 GiB window of the dsx_gen_dedup
stream (p = 0.5) cut at 16/64/256 KiB and put into a store, the source.  Every
timed call gets a fresh tracked store filled by one DSX_COPY_ALL copy of the
source (outside the timed region).  Cases:

  evict_half     every second entry touched, then an eviction for half of the
                 used bytes: victims and survivors interleave, the arena moves;
  evict_oldest   nothing touched, an eviction for 5 % of the used bytes: the
                 victims are the first entries, everything behind them moves;
  dry_half       evict_half's selection with DSX_EVICT_DRY: nothing moves;
  touch_host, touch_device   dsx_store_touch of every ID, from host memory and
                 from HBM;

and, in the same process and alternating with them, the yardstick that is not
the code under test:

  prune_half, prune_oldest   dsx_store_prune(DSX_PRUNE_REMOVE) of an untracked
                 copy of the same store given the same victims as an ID list in
                 HBM: what a caller runs today after choosing the victims on the
                 host, and the same compaction.  evict minus prune is the price
                 of the selection and of carrying the stamps.

Each is the median of REPS rounds after 2 warm-up rounds, timed with device
events on the context's stream around the synchronous call and by the host
clock.  The evicted store is checked once per case against the pruned one:
entries, ends and arena bytes.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/evict_rate.json).  Run on the GPU box: python tools/evict_rate.py
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
from assemble_rate import Timer, summary  # noqa: E402
from desync_amd import _lib  # noqa: E402
from desync_amd.encrypt import _download  # noqa: E402
from store_rate import Window, put  # noqa: E402

REPS = 10
vp = ctypes.c_void_p


def evict(ctx, s, need_bytes, dry=False, ids_out=None):
    tot = _lib.StoreEvictTotals()
    cap = 0 if ids_out is None else len(ids_out)
    rc = _lib.lib().dsx_store_evict(ctx.h, s.h, need_bytes, 0, None, 0,
                                    None if ids_out is None else ids_out.ctypes.data, cap, 0, ctypes.byref(tot),
                                    _lib.DSX_EVICT_DRY if dry else 0)
    if rc:
        raise _lib.DsxError(rc, (_lib.lib().dsx_last_error(ctx.h) or b"").decode())
    return {k: getattr(tot, k) for k, _ in _lib.StoreEvictTotals._fields_ if k != "reserved"}


def prune_remove(ctx, s, d_ids, n):
    tot = _lib.StorePruneTotals()
    rc = _lib.lib().dsx_store_prune(ctx.h, s.h, vp(d_ids.data_ptr()), n, 0, ctypes.byref(tot),
                                    _lib.DSX_IDS_DEVICE | _lib.DSX_PRUNE_REMOVE)
    if rc:
        raise _lib.DsxError(rc, (_lib.lib().dsx_last_error(ctx.h) or b"").decode())
    return {k: getattr(tot, k) for k, _ in _lib.StorePruneTotals._fields_}


def touch(ctx, s, ptr, n, device):
    miss = ctypes.c_uint64()
    rc = _lib.lib().dsx_store_touch(ctx.h, s.h, vp(ptr), n, _lib.DSX_STAMP_NOW, ctypes.byref(miss),
                                    _lib.DSX_IDS_DEVICE if device else 0)
    if rc or miss.value:
        raise SystemExit(f"touch: rc {rc}, {miss.value} missing")


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

    target = Window(ctx, 8 * size, size)
    src = desync_amd.DeviceStore(size, target.n, ctx=ctx)
    put(ctx, src, target)
    ids, ends = src.entries()
    filled = src.counts()
    n = len(ends)
    d_all = torch.from_numpy(ids.reshape(-1).copy()).to("cuda:0")
    d_second = torch.from_numpy(np.ascontiguousarray(ids[1::2]).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    needs = {"half": size - filled["bytes"] + filled["bytes"] // 2,
             "oldest": size - filled["bytes"] + filled["bytes"] // 20}

    def fresh(track, case=None):
        s = desync_amd.DeviceStore(size, target.n, ctx=ctx, track=track)
        s.CopyFrom(src)
        if track and case == "half":
            touch(ctx, s, d_second.data_ptr(), len(ids[1::2]), True)
        return s

    # every case once, checked against the prune of the same victims
    totals, victims = {}, {}
    for case, need in needs.items():
        s = fresh(True, case)
        out = np.empty((n, 32), dtype=np.uint8)
        dry = evict(ctx, s, need, dry=True, ids_out=out)
        t = totals[case] = evict(ctx, s, need, ids_out=out)
        if dry != t:
            raise SystemExit(f"{case}: the dry run's totals differ")
        victims[case] = torch.from_numpy(out[:t["evicted"]].reshape(-1).copy()).to("cuda:0")
        torch.cuda.synchronize()
        twin = fresh(False)
        p = prune_remove(ctx, twin, victims[case], t["evicted"])
        a, b = s.entries(), twin.entries()
        (pa, ua), (pb, ub) = s.arena(), twin.arena()
        same = ua == ub and np.array_equal(_download(ctx, pa, ua), _download(ctx, pb, ub))
        if not (same and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                and (p["removed"], p["moved"], p["moved_bytes"]) == (t["evicted"], t["moved"], t["moved_bytes"])
                and not s.Verify()):
            raise SystemExit(f"{case}: the evicted store is not the pruned one")
        s.close()
        twin.close()

    names = [f"{what}_{case}" for case in needs for what in ("evict", "prune")] + ["dry_half", "touch_host",
                                                                                   "touch_device"]
    timers = {k: Timer(stream) for k in names}
    for rep in range(2 + REPS):
        rec = rep >= 2
        for case, need in needs.items():
            s = fresh(True, case)
            if case == "half":
                timers["dry_half"].run(lambda: evict(ctx, s, need, dry=True), record=rec)
            timers[f"evict_{case}"].run(lambda: evict(ctx, s, need), record=rec)
            s.close()
            twin = fresh(False)
            timers[f"prune_{case}"].run(lambda: prune_remove(ctx, twin, victims[case], totals[case]["evicted"]),
                                        record=rec)
            twin.close()
        s = fresh(True)
        timers["touch_host"].run(lambda: touch(ctx, s, ids.ctypes.data, n, False), record=rec)
        timers["touch_device"].run(lambda: touch(ctx, s, d_all.data_ptr(), n, True), record=rec)
        s.close()

    rows = {k: {"device": summary(t.dev), "host_clock": summary(t.host)} for k, t in timers.items()}
    cases = {}
    for case in needs:
        ev, pr = rows[f"evict_{case}"], rows[f"prune_{case}"]
        cases[case] = {"totals": totals[case], "evict_ms_median": ev["device"]["ms_median"],
                       "prune_ms_median": pr["device"]["ms_median"],
                       "selection_ms": round(ev["device"]["ms_median"] - pr["device"]["ms_median"], 4),
                       "evict_over_prune": round(ev["device"]["ms_median"] / pr["device"]["ms_median"], 3),
                       "host_evict_over_prune": round(ev["host_clock"]["ms_median"] / pr["host_clock"]["ms_median"], 3)}
    res = {"window_bytes": size, "chunks": target.n, "store": filled, "reps": REPS, "cases": cases,
           "dry_half_ms_median": rows["dry_half"]["device"]["ms_median"],
           "touch_ms_median": {"host": rows["touch_host"]["device"]["ms_median"],
                               "device": rows["touch_device"]["device"]["ms_median"]},
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
