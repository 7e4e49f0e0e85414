#!/usr/bin/env python3
"""Chunk-store rates, on one MI355X, for a resident 4 GiB window
of the dsx_gen_dedup stream (p = 0.5) cut at 16/64/256 KiB, its IDs and chunk
ends in HBM:

  put_empty        dsx_store_put of the window into an empty store;
  put_after_other  the same put into a store that already holds another window;
  locate           dsx_store_locate of every chunk ID of the window;
  resolve          dsx_store_resolve of the window's plan (no seed: every segment
                   is a store segment);
  assemble_arena   dsx_assemble of the resolved plan, reading the arena in place;

and, in the same process and alternating with them, what the library needed for
the same result before it had a store:

  parent_empty / parent_after_other
                   dsx_idset_create of the IDs the store holds + dsx_dedup of the
                   window against that set + a segment list built on the host
                   (numpy) + dsx_assemble of the new chunks into a packed buffer;
  memcpy_d2d       hipMemcpyAsync device to device of the put's stored_bytes.

Each is the median of REPS rounds after 2 warm-up rounds, timed with device
events on the context's stream around the synchronous call and by the host
clock.  A put needs a fresh store each round (nothing removes chunks): creating
and filling it is outside the timed region.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/store_rate.json).  Run on the GPU box: python tools/store_rate.py
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
from desync_amd.index import ChunkArray, FormatIndex, Index  # noqa: E402

REPS = 10
MIN, AVG, MAX = 16384, 65536, 262144
vp = ctypes.c_void_p


class Window:
    """A window of the stream in HBM with its cut list and IDs there too."""

    def __init__(self, ctx, offset, length, seed=5, p=0.5):
        L = _lib.lib()
        self.length = length
        self.blob = torch.empty(length, dtype=torch.uint8, device="cuda:0")
        cap = length // MIN + 2
        self.d_ends = torch.empty(cap, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        _lib.check(L.dsx_gen_dedup(ctx.h, vp(self.blob.data_ptr()), offset, length, seed, p), ctx.h)
        self.n = desync_amd.cut_device(self.blob.data_ptr(), length, MIN, AVG, MAX, ctx=ctx,
                                       out_ptr=self.d_ends.data_ptr(), out_cap=cap)
        self.d_ids = torch.empty(self.n * 32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        _lib.check(L.dsx_chunk_ids(ctx.h, vp(self.blob.data_ptr()), length, 0, vp(self.d_ends.data_ptr()),
                                   self.n, vp(self.d_ids.data_ptr()),
                                   _lib.DSX_OUT_DEVICE | _lib.DSX_ENDS_DEVICE, _lib.DSX_DIGEST_SHA512_256),
                   ctx.h)
        self.ends = self.d_ends[:self.n].cpu().numpy().astype(np.uint64)
        self.ids = self.d_ids.cpu().numpy().reshape(-1, 32)
        self.index = Index(FormatIndex(0, MIN, AVG, MAX), ChunkArray(self.ends, self.ids.tobytes()))


def put(ctx, store, w):
    tot = _lib.StorePutTotals()
    rc = _lib.lib().dsx_store_put(ctx.h, store.h, vp(w.blob.data_ptr()), w.length, vp(w.d_ids.data_ptr()),
                                  vp(w.d_ends.data_ptr()), 0, w.n, ctypes.byref(tot),
                                  _lib.DSX_IDS_DEVICE | _lib.DSX_ENDS_DEVICE)
    if rc:
        raise _lib.DsxError(rc, (_lib.lib().dsx_last_error(ctx.h) or b"").decode())
    return {k: getattr(tot, k) for k, _ in _lib.StorePutTotals._fields_}


def parent_composition(ctx, w, held_ids, packed):
    """What the library needed before it had a store, for the result of one
    put: which chunks are new (a set of the IDs already held + dsx_dedup), a
    segment list built on the host, one gather into a packed buffer.
    -> (new chunks, new bytes)"""
    seed = desync_amd.IDSet(held_ids, ctx=ctx) if held_ids is not None else None
    first, seedp, _ = desync_amd.dedup(w.d_ids, w.d_ends.data_ptr(), seed=seed, ctx=ctx, n=w.n)
    new = first == np.arange(w.n, dtype=np.uint32)
    if seedp is not None:
        new &= seedp == _lib.DSX_POS_NONE
    pos = np.flatnonzero(new)
    starts = np.concatenate(([0], w.ends[:-1])).astype(np.uint64)
    sizes = (w.ends - starts)[pos]
    segs = np.zeros(len(pos), dtype=extract.SEG_DTYPE)
    segs["dst_off"] = np.cumsum(sizes) - sizes
    segs["bytes"] = sizes
    segs["src_off"] = starts[pos]
    segs["first"] = pos
    segs["count"] = 1
    segs["seed_first"] = pos
    ptrs = (vp * 1)(w.blob.data_ptr())
    lens = (ctypes.c_uint64 * 1)(w.length)
    total = int(sizes.sum())
    _lib.check(_lib.lib().dsx_assemble(ctx.h, vp(segs.ctypes.data), len(segs), ptrs, lens, 1, None, 0,
                                       vp(packed.data_ptr()), total, 0), ctx.h)
    if seed is not None:
        seed.close()
    return len(pos), total


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
    other = Window(ctx, size // 2 + 12345, size)
    packed = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.empty(target.n, dtype=torch.int64, device="cuda:0")
    d_sizes = torch.empty(target.n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    # the stores the read side is measured on, and the figures of the two puts
    full = desync_amd.DeviceStore(2 * size, target.n + other.n, ctx=ctx)
    tot_other = put(ctx, full, other)
    other_ids = full.entries()[0].copy()
    d_other_ids = torch.from_numpy(other_ids.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    tot_after = put(ctx, full, target)
    probe = desync_amd.DeviceStore(size, target.n, ctx=ctx)
    tot_empty = put(ctx, probe, target)
    probe.close()
    if full.Verify():
        raise SystemExit("the store does not verify")
    plan = desync_amd.NewSeedSequencer(target.index, null_seed=False, ctx=ctx).Plan()
    segs0 = np.ascontiguousarray(plan.segs)
    segs = segs0.copy()

    def resolve():
        segs[:] = segs0
        nm, nw, fb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        _lib.check(L.dsx_store_resolve(ctx.h, full.h, vp(target.d_ids.data_ptr()), target.n,
                                       vp(segs.ctypes.data), len(segs), ctypes.byref(nm), ctypes.byref(nw),
                                       ctypes.byref(fb), _lib.DSX_IDS_DEVICE), ctx.h)
        if nm.value or nw.value:
            raise SystemExit("the store does not hold the window")

    def locate():
        nm = ctypes.c_uint64()
        _lib.check(L.dsx_store_locate(ctx.h, full.h, vp(target.d_ids.data_ptr()), target.n,
                                      vp(d_offs.data_ptr()), vp(d_sizes.data_ptr()), ctypes.byref(nm),
                                      _lib.DSX_IDS_DEVICE | _lib.DSX_OUT_DEVICE), ctx.h)

    def assemble_arena():
        ap_, used = full.arena()
        _lib.check(L.dsx_assemble(ctx.h, vp(segs.ctypes.data), len(segs), None, None, 0, vp(ap_), used,
                                  vp(out.data_ptr()), size, _lib.DSX_STORE_DEVICE), ctx.h)

    resolve()
    out.zero_()
    torch.cuda.synchronize()
    assemble_arena()
    if not torch.equal(out, target.blob):
        raise SystemExit("the window assembled from the arena differs from the window")
    # the parent's composition gives the put's figures
    if parent_composition(ctx, target, None, packed) != (tot_empty["stored"], tot_empty["stored_bytes"]):
        raise SystemExit("parent composition (empty) disagrees with the put")
    if parent_composition(ctx, target, d_other_ids, packed) != (tot_after["stored"], tot_after["stored_bytes"]):
        raise SystemExit("parent composition (after the other window) disagrees with the put")

    state = {}

    def fresh(preload):
        s = desync_amd.DeviceStore(2 * size if preload else size, target.n + other.n, ctx=ctx)
        if preload:
            put(ctx, s, other)
        state["s"] = s

    names = ("put_empty", "put_after_other", "parent_empty", "parent_after_other", "memcpy_d2d_empty",
             "memcpy_d2d_after_other", "locate", "resolve", "assemble_arena")
    timers = {k: Timer(stream) for k in names}
    for rep in range(2 + REPS):
        rec = rep >= 2
        for preload, tag in ((False, "empty"), (True, "after_other")):
            fresh(preload)
            timers["put_" + tag].run(lambda: put(ctx, state["s"], target), record=rec)
            state.pop("s").close()
            held = d_other_ids if preload else None
            timers["parent_" + tag].run(lambda: parent_composition(ctx, target, held, packed), record=rec)
            nbytes = (tot_after if preload else tot_empty)["stored_bytes"]
            timers["memcpy_d2d_" + tag].run(
                lambda: hip.hipMemcpyAsync(packed.data_ptr(), target.blob.data_ptr(), nbytes, HIP_D2D, sp),
                record=rec)
        timers["locate"].run(locate, record=rec)
        timers["resolve"].run(resolve, record=rec)
        timers["assemble_arena"].run(assemble_arena, record=rec)

    rows = {k: {"device": summary(t.dev), "host_clock": summary(t.host)} for k, t in timers.items()}
    for tag, tot in (("empty", tot_empty), ("after_other", tot_after)):
        p = rows["put_" + tag]
        p["totals"] = tot
        ms = p["device"]["ms_median"]
        p["TBps_read_plus_written"] = round(2 * tot["stored_bytes"] / (ms * 1e-3) / 1e12, 3)
        p["time_over_memcpy_d2d"] = round(ms / rows["memcpy_d2d_" + tag]["device"]["ms_median"], 3)
        p["time_over_parent_composition"] = round(ms / rows["parent_" + tag]["device"]["ms_median"], 3)
        p["host_time_over_parent_composition"] = round(
            p["host_clock"]["ms_median"] / rows["parent_" + tag]["host_clock"]["ms_median"], 3)
    rows["assemble_arena"]["TBps_read_plus_written"] = round(
        2 * size / (rows["assemble_arena"]["device"]["ms_median"] * 1e-3) / 1e12, 3)
    res = {"window_bytes": size, "chunks": target.n, "other_window": tot_other,
           "plan_segments": len(segs0), "reps": REPS, "rows": rows}
    full.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
