#!/usr/bin/env python3
"""dsx_read_ranges' rate, on one MI355X, on the store of
tools/store_rate.py: a 4 GiB window of the dsx_gen_dedup stream (p = 0.5) cut at
16/64/256 KiB and put into an empty store; the index's IDs and ends in HBM (a
DeviceIndex).  Shapes, each into a preallocated output:

  whole        one range, the whole blob;
  mib_4096     4,096 ranges of 1 MiB at random unaligned offsets, packed;
  kib4_65536   65,536 ranges of 4 KiB likewise;
  kib4_1       one range of 4 KiB: the latency of a single Read;

and, in the same process and alternating with them,

  memcpy_d2d_<shape>   hipMemcpyAsync device to device of the bytes read;
  assemble_blob        AssembleBlob(index, store) of the whole blob, the public call
                       (plan, resolve, gather, and the read-back hash of 4 GiB);
  assemble_no_check    its plan, dsx_store_resolve and dsx_assemble alone: what the
                       whole-blob read is compared with, and, plus a copy of the
                       bytes (memcpy_d2d_<shape>, the least a slicing costs), the
                       best the API offered for the other shapes before this call.

With --parent-lib PATH (a libdsx.so built from the parent commit) the two
assemble rows run in that library, on a context and a store of its own filled
from the same window; without it they run in this build, whose code on that
path is the same files.  Each row is the median of REPS rounds after 2 warm-up
rounds, timed with device events on the context's stream around the synchronous
call and by the host clock.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/read_rate.json).  Run on the GPU box: python tools/read_rate.py
"""
import argparse
import contextlib
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
from desync_amd.readseeker import DeviceIndex, ranges_array, read_ranges_raw  # noqa: E402
from store_rate import Window, put  # noqa: E402

REPS = 10
vp = ctypes.c_void_p


def load_parent(path):
    """A second libdsx.so, bound with this build's signatures for the entry
    points it has."""
    cur = _lib.lib()
    lib = ctypes.CDLL(path)
    for name in _lib.EXPORTS:
        if hasattr(lib, name):
            f, g = getattr(lib, name), getattr(cur, name)
            f.restype, f.argtypes = g.restype, g.argtypes
    return lib


@contextlib.contextmanager
def using(lib):
    """Calls of the package go to `lib` inside the block."""
    old, _lib._lib = _lib._lib, lib
    try:
        yield
    finally:
        _lib._lib = old


def stream_of(ctx):
    sp = vp()
    _lib.check(_lib.lib().dsx_ctx_stream(ctx.h, ctypes.byref(sp)), ctx.h)
    return sp, torch.cuda.ExternalStream(sp.value, device="cuda:0")


def shapes(size, rng):
    def packed(count, ln):
        offs = rng.integers(0, size - ln, count, dtype=np.int64) | 1  # unaligned
        return ranges_array([(int(o), ln) for o in offs])
    return {"whole": ranges_array([(0, size)]), "mib_4096": packed(4096, 1 << 20),
            "kib4_65536": packed(65536, 4096), "kib4_1": packed(1, 4096)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--parent-lib")
    args = ap.parse_args()
    size = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    ctx = _lib.default_context(0)
    cur = _lib.lib()
    sp, stream = stream_of(ctx)
    hip = hip_runtime()

    target = Window(ctx, 8 * size, size)
    out = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    store = desync_amd.DeviceStore(size, target.n, ctx=ctx)
    tot_put = put(ctx, store, target)
    di = DeviceIndex(target.index, ctx)
    rgs = shapes(size, np.random.default_rng(29))

    def read(rg):
        return read_ranges_raw(store, di.d_ids.data_ptr(), di.d_ends.data_ptr(), rg, out, 0, di.null.ID,
                               len(di.null.Data), n=di.n)

    # every shape once, checked against the window itself
    totals = {}
    for k, rg in rgs.items():
        out.zero_()
        torch.cuda.synchronize()
        t = totals[k] = read(rg)
        if t["missing"] or t["wrong_size"] or t["beyond"] or t["bytes"] != int(rg[:, 1].sum()):
            raise SystemExit(f"{k}: the read is refused: {t}")
        for off, ln, dst in rg[:: max(1, len(rg) // 64)].tolist():
            if not torch.equal(out[dst:dst + ln], target.blob[off:off + ln]):
                raise SystemExit(f"{k}: range at {off} differs from the blob")

    # the yardstick's library: the parent's, with a context and a store of its own
    plib = load_parent(args.parent_lib) if args.parent_lib else cur
    with using(plib):
        pctx = _lib.Context(0) if args.parent_lib else ctx
        _psp, pstream = stream_of(pctx)
        pstore = desync_amd.DeviceStore(size, target.n, ctx=pctx) if args.parent_lib else store
        if args.parent_lib:
            put(pctx, pstore, target)
        sq = desync_amd.NewSeedSequencer(target.index, null_seed=True, ctx=pctx)

    def assemble_blob():
        with using(plib):
            got, _stats = desync_amd.AssembleBlob(target.index, pstore, ctx=pctx)
        return got

    def assemble_no_check():
        with using(plib):
            plan = sq.Plan()
            miss, wrong, _bad = pstore.resolve(sq.ids, plan.segs)
            if miss or wrong:
                raise SystemExit("the store does not hold the window")
            extract.assemble(plan, out, pstore.arena(), ctx=pctx)

    if not torch.equal(assemble_blob(), target.blob):
        raise SystemExit("AssembleBlob differs from the blob")
    out.zero_()
    assemble_no_check()
    if not torch.equal(out, target.blob):
        raise SystemExit("the plan's gather differs from the blob")

    timers = {f"{what}_{k}": Timer(stream) for k in rgs for what in ("read", "memcpy_d2d")}
    timers["assemble_blob"], timers["assemble_no_check"] = Timer(pstream), Timer(pstream)
    for rep in range(2 + REPS):
        rec = rep >= 2
        for k, rg in rgs.items():
            timers[f"read_{k}"].run(lambda: read(rg), record=rec)
            if k == "whole":
                timers["assemble_no_check"].run(assemble_no_check, record=rec)
                timers["assemble_blob"].run(assemble_blob, record=rec)
            nbytes = totals[k]["bytes"]
            timers[f"memcpy_d2d_{k}"].run(
                lambda: hip.hipMemcpyAsync(out.data_ptr(), target.blob.data_ptr(), nbytes, HIP_D2D, sp),
                record=rec)

    rows = {k: {"device": summary(t.dev), "host_clock": summary(t.host)} for k, t in timers.items()}
    asm = rows["assemble_no_check"]["device"]["ms_median"]
    full = rows["assemble_blob"]["device"]["ms_median"]
    cases = {}
    for k, rg in rgs.items():
        ms = rows[f"read_{k}"]["device"]["ms_median"]
        d2d = rows[f"memcpy_d2d_{k}"]["device"]["ms_median"]
        before = asm if k == "whole" else asm + d2d
        cases[k] = {"totals": totals[k], "ranges": len(rg), "ms_median": ms,
                    "host_clock_ms_median": rows[f"read_{k}"]["host_clock"]["ms_median"],
                    "time_over_memcpy_d2d": round(ms / d2d, 3),
                    "GBps_read": round(totals[k]["bytes"] / (ms * 1e-3) / 1e9, 2),
                    "time_over_assemble_no_check" + ("" if k == "whole" else "_plus_copy"): round(ms / before, 4),
                    "time_over_assemble_blob" + ("" if k == "whole" else "_plus_copy"):
                        round(ms / (full if k == "whole" else full + d2d), 4)}
    res = {"window_bytes": size, "chunks": target.n, "store": store.counts(), "put": tot_put, "reps": REPS,
           "assemble_library": "parent commit" if args.parent_lib else "this build",
           "ratios_are_of": "device-event medians around the synchronous calls", "cases": cases, "rows": rows}
    with using(plib):
        if args.parent_lib:
            pstore.close()
            pctx.close()
    store.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
