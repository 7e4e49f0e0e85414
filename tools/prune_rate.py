#!/usr/bin/env python3
"""dsx_store_prune's rate, on one MI355X, on the store of
tools/store_rate.py: a 4 GiB window of the dsx_gen_dedup stream (p = 0.5) cut at
16/64/256 KiB and put into an empty store.  Cases, by which entries go:

  every_second   every second entry;
  one_in_ten     one entry in ten;
  first_only     entry 0 alone: everything behind it moves by one chunk;
  nothing        none: the early return after the selection;

each pruned with a window of 64, 128 and 256 MiB, and, in the same process and
alternating with them,

  memcpy_d2d     hipMemcpyAsync device to device of the case's moved_bytes;
  parent         what the library needed for the same store before it had a
                 prune: the entries read back, the survivors gathered into a
                 packed buffer by dsx_assemble, the store destroyed, a new one
                 created and the packed buffer put into it (which entries
                 survive is given to it for nothing).

Each is the median of REPS rounds after 2 warm-up rounds, timed with device
events on the context's stream around the synchronous call and by the host
clock.  Every timed prune gets a freshly filled store; creating and filling it
is outside the timed region.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/prune_rate.json).  Run on the GPU box: python tools/prune_rate.py
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
WINDOWS_MIB = (64, 128, 256)
vp = ctypes.c_void_p


def prune(ctx, store, d_keep, n, window):
    tot = _lib.StorePruneTotals()
    rc = _lib.lib().dsx_store_prune(ctx.h, store.h, vp(d_keep.data_ptr()), n, window, ctypes.byref(tot),
                                    _lib.DSX_IDS_DEVICE)
    if rc:
        raise _lib.DsxError(rc, (_lib.lib().dsx_last_error(ctx.h) or b"").decode())
    return {k: getattr(tot, k) for k, _ in _lib.StorePruneTotals._fields_}


def parent_composition(ctx, store, mask, packed, size, max_chunks):
    """The survivors into a packed buffer, then a new store filled from it.
    -> the new store (the old one is destroyed)"""
    ids, ends = store.entries()
    starts = np.concatenate(([0], ends[:-1])).astype(np.uint64)
    pos = np.flatnonzero(mask)
    sizes = (ends - starts)[pos]
    new_ends = np.cumsum(sizes).astype(np.uint64)
    segs = np.zeros(len(pos), dtype=extract.SEG_DTYPE)
    segs["dst_off"] = new_ends - sizes
    segs["bytes"] = sizes
    segs["src_off"] = starts[pos]
    segs["first"] = pos
    segs["count"] = 1
    segs["source"] = _lib.DSX_SRC_STORE
    segs["seed_first"] = 0xFFFFFFFF
    total = int(new_ends[-1]) if len(pos) else 0
    base, used = store.arena()
    _lib.check(_lib.lib().dsx_assemble(ctx.h, vp(segs.ctypes.data), len(segs), None, None, 0, vp(base), used,
                                       vp(packed.data_ptr()), total, _lib.DSX_STORE_DEVICE), ctx.h)
    store.close()
    new = desync_amd.DeviceStore(size, max_chunks, ctx=ctx)
    new.put((packed.data_ptr(), total), np.ascontiguousarray(ids[pos]), new_ends)
    return new


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

    def fresh():
        s = desync_amd.DeviceStore(size, target.n, ctx=ctx)
        put(ctx, s, target)
        return s

    probe = fresh()
    ids, ends = probe.entries()
    filled = probe.counts()
    probe.close()
    n = len(ends)
    masks = {"every_second": np.arange(n) % 2 == 0, "one_in_ten": np.arange(n) % 10 != 5,
             "first_only": np.arange(n) != 0, "nothing": np.ones(n, dtype=bool)}
    keep = {}
    for k, m in masks.items():
        keep[k] = torch.from_numpy(np.ascontiguousarray(ids[m]).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()

    # every case once, checked: the totals, the verify, and the parent's store holding the same
    totals = {}
    for k, m in masks.items():
        s = fresh()
        totals[k] = prune(ctx, s, keep[k], int(m.sum()), 0)
        if totals[k]["kept"] != int(m.sum()) or totals[k]["unmatched"] or s.Verify():
            raise SystemExit(f"{k}: the pruned store is wrong")
        mine = (s.entries()[0].tobytes(), s.entries()[1].tobytes())
        s.close()
        p = parent_composition(ctx, fresh(), m, packed, size, target.n)
        if (p.entries()[0].tobytes(), p.entries()[1].tobytes()) != mine:
            raise SystemExit(f"{k}: the parent's composition gives another store")
        p.close()

    names = [f"prune_{k}_w{w}" for k in masks for w in WINDOWS_MIB]
    names += [f"parent_{k}" for k in masks] + [f"memcpy_d2d_{k}" for k in masks]
    timers = {k: Timer(stream) for k in names}
    state = {}
    for rep in range(2 + REPS):
        rec = rep >= 2
        for k, m in masks.items():
            kept = int(m.sum())
            for w in WINDOWS_MIB:
                state["s"] = fresh()
                timers[f"prune_{k}_w{w}"].run(lambda: prune(ctx, state["s"], keep[k], kept, w << 20), record=rec)
                state.pop("s").close()
            state["s"] = fresh()
            timers[f"parent_{k}"].run(
                lambda: state.__setitem__("s", parent_composition(ctx, state["s"], m, packed, size, target.n)),
                record=rec)
            state.pop("s").close()
            nbytes = totals[k]["moved_bytes"]
            if nbytes:
                timers[f"memcpy_d2d_{k}"].run(
                    lambda: hip.hipMemcpyAsync(packed.data_ptr(), target.blob.data_ptr(), nbytes, HIP_D2D, sp),
                    record=rec)

    rows = {k: {"device": summary(t.dev), "host_clock": summary(t.host)} for k, t in timers.items() if t.dev}
    cases = {}
    for k in masks:
        c = {"totals": totals[k]}
        parent = rows[f"parent_{k}"]["device"]["ms_median"]
        d2d = rows.get(f"memcpy_d2d_{k}", {}).get("device", {}).get("ms_median")
        for w in WINDOWS_MIB:
            ms = rows[f"prune_{k}_w{w}"]["device"]["ms_median"]
            c[f"w{w}"] = {"ms_median": ms, "time_over_parent": round(ms / parent, 3),
                          "host_time_over_parent": round(rows[f"prune_{k}_w{w}"]["host_clock"]["ms_median"] /
                                                         rows[f"parent_{k}"]["host_clock"]["ms_median"], 3),
                          "time_over_memcpy_d2d": round(ms / d2d, 3) if d2d else None,
                          "TBps_moved_read_plus_written": round(
                              2 * totals[k]["moved_bytes"] / (ms * 1e-3) / 1e12, 3)}
        cases[k] = c
    res = {"window_bytes": size, "chunks": target.n, "store": filled, "reps": REPS,
           "windows_mib": WINDOWS_MIB, "cases": cases, "rows": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
