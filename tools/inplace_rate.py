#!/usr/bin/env python3
"""dsx_assemble_inplace's rate ("In place"), on one MI355X, on a
4 GiB window of the dsx_gen_dedup stream (p = 0.5) cut at 16/64/256 KiB: the
version the buffer holds.  Shapes, by what the next version is:

  insert_front   4 KiB from the store in front of the old version: every byte
                 moves;
  scattered      64 chunks at scattered places replaced out of a store arena in
                 HBM: everything else is kept;
  swap           the two halves swapped (at a chunk boundary): first with a
                 stash of one window, which must be refused, then with enough.

insert_front and swap run with windows of 64, 128 and 256 MiB and, in the same
process and alternating with them,

  parent         dsx_assemble of the same plan into a second buffer, the old
                 version as a seed: what the library offered before;
  memcpy_d2d     hipMemcpyAsync device to device of the bytes written.

Each is the median of REPS rounds after 2 warm-up rounds, timed with device
events on the context's stream around the synchronous call and by the host
clock.  The schedule moves bytes whatever they are, so the rounds run on the
buffer as the round before left it; each shape's result is compared with the
second buffer's once, from the old version, before anything is timed.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/inplace_rate.json).  Run on the GPU box: python tools/inplace_rate.py
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

from assemble_rate import HIP_D2D, Timer, hip_runtime, summary  # noqa: E402
from desync_amd import _lib, extract  # noqa: E402
from store_rate import Window  # noqa: E402

REPS = 10
WINDOWS_MIB = (64, 128, 256)
vp = ctypes.c_void_p
SELF, STORE = _lib.DSX_SRC_SELF, _lib.DSX_SRC_STORE


def segs_of(rows):
    a = np.zeros(len(rows), dtype=extract.SEG_DTYPE)
    for i, (dst, nbytes, src, first, count, source) in enumerate(rows):
        a[i] = (dst, nbytes, src, first, count, source, 0xFFFFFFFF)
    return a


def inplace(ctx, segs, ends, keep, store, buf, have_len, new_len, window, stash):
    """-> (rc, totals)"""
    tot = _lib.InplaceTotals()
    rc = _lib.lib().dsx_assemble_inplace(
        ctx.h, vp(segs.ctypes.data), len(segs), vp(ends.ctypes.data), ends.size,
        vp(keep.ctypes.data) if keep is not None else None, None, None, 0,
        vp(store.data_ptr()) if store is not None else None, store.numel() if store is not None else 0,
        vp(buf.data_ptr()), buf.numel(), have_len, new_len, window, stash, _lib.DSX_STORE_DEVICE,
        ctypes.byref(tot))
    return rc, {k: getattr(tot, k) for k, _ in _lib.InplaceTotals._fields_ if k != "reserved"}


def parent(ctx, segs, keep, old, store, out, new_len):
    """The same plan out of place: SELF becomes seed 0, the old version."""
    s = segs.copy()
    s["source"] = np.where(s["source"] == SELF, 0, s["source"])
    ptrs = (ctypes.c_void_p * 1)(old.data_ptr())
    lens = (ctypes.c_uint64 * 1)(old.numel())
    rc = _lib.lib().dsx_assemble(ctx.h, vp(s.ctypes.data), len(s), ptrs, lens, 1,
                                 vp(store.data_ptr()) if store is not None else None,
                                 store.numel() if store is not None else 0, vp(out.data_ptr()), new_len,
                                 _lib.DSX_STORE_DEVICE)
    if rc:
        raise _lib.DsxError(rc, (_lib.lib().dsx_last_error(ctx.h) or b"").decode())


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

    old = Window(ctx, 8 * size, size)          # the old version, kept as it is
    n, ends = old.n, old.ends
    starts = np.concatenate(([0], ends[:-1])).astype(np.uint64)
    ins = 4096
    buf = torch.empty(size + ins, dtype=torch.uint8, device="cuda:0")   # the buffer updated in place
    out = torch.empty(size + ins, dtype=torch.uint8, device="cuda:0")   # the parent's second buffer
    torch.cuda.synchronize()

    # ---- the three shapes: segments, chunk ends, keep mask, store bytes, lengths ----
    shapes = {}
    front = torch.randint(0, 256, (ins,), dtype=torch.uint8, device="cuda:0")
    shapes["insert_front"] = dict(
        segs=segs_of([(0, ins, 0, 0, 1, STORE), (ins, size, 0, 1, n, SELF)]),
        ends=np.concatenate(([ins], ends + np.uint64(ins))).astype(np.uint64), keep=None, store=front,
        new_len=size + ins)
    which = np.linspace(n // 130, n - n // 130, 64).astype(np.int64)   # 64 chunks, scattered
    sizes = (ends - starts)[which]
    packed = torch.cat([old.blob[(p * 7919) % (size - (1 << 20)):][:int(s)].bitwise_xor(0x5A)
                        for p, s in zip(which.tolist(), sizes.tolist())])
    rows, at, soff = [], 0, 0
    for p, s in zip(which.tolist(), sizes.tolist()):
        if p > at:
            rows.append((int(starts[at]), int(starts[p] - starts[at]), int(starts[at]), at, p - at, SELF))
        rows.append((int(starts[p]), int(s), soff, p, 1, STORE))
        soff += int(s)
        at = p + 1
    rows.append((int(starts[at]), int(ends[-1] - starts[at]), int(starts[at]), at, n - at, SELF))
    shapes["scattered"] = dict(segs=segs_of(rows), ends=ends, keep=None, store=packed, new_len=size)
    h = n // 2
    half = int(ends[h - 1])
    shapes["swap"] = dict(
        segs=segs_of([(0, size - half, half, 0, n - h, SELF), (size - half, half, 0, n - h, h, SELF)]),
        ends=np.concatenate((ends[h:] - np.uint64(half), ends[:h] + np.uint64(size - half))).astype(np.uint64),
        keep=None, store=None, new_len=size)
    torch.cuda.synchronize()

    def reset():
        buf[:size].copy_(old.blob)
        torch.cuda.synchronize()   # (torch's stream is not the context's)

    # ---- every shape once, checked against the parent's second buffer ----------------
    res = {"window_bytes": size, "chunks": n, "reps": REPS, "windows_mib": WINDOWS_MIB, "shapes": {}}
    totals = {}
    for name, s in shapes.items():
        parent(ctx, s["segs"], s["keep"], old.blob, s["store"], out, s["new_len"])
        for w in WINDOWS_MIB:
            reset()
            rc, tot = inplace(ctx, s["segs"], s["ends"], s["keep"], s["store"], buf, size, s["new_len"],
                              w << 20, size)
            if rc or not torch.equal(buf[:s["new_len"]], out[:s["new_len"]]):
                raise SystemExit(f"{name} w{w}: rc {rc}, or the buffer is not the target")
            totals[name, w] = tot
    reset()
    s = shapes["swap"]
    before = buf.clone()
    rc, tot = inplace(ctx, s["segs"], s["ends"], None, None, buf, size, size, 128 << 20, 128 << 20)
    torch.cuda.synchronize()
    res["swap_refusal"] = {"stash_cap": 128 << 20, "rc": rc, "needed": tot["stash_peak"],
                           "buffer_unchanged": bool(torch.equal(buf, before))}
    del before
    if rc != _lib.DSX_E_CAPACITY or not res["swap_refusal"]["buffer_unchanged"]:
        raise SystemExit(f"swap with a stash of one window: rc {rc}, expected the refusal")

    def copy(nbytes):
        if hip.hipMemcpyAsync(out.data_ptr(), buf.data_ptr(), nbytes, HIP_D2D, sp):
            raise SystemExit(f"hipMemcpyAsync of {nbytes} bytes failed")

    # ---- timed ----------------------------------------------------------------------------
    names = [f"{k}_w{w}" for k in shapes for w in WINDOWS_MIB]
    names += [f"parent_{k}" for k in shapes] + [f"memcpy_d2d_{k}" for k in shapes]
    timers = {k: Timer(stream) for k in names}
    for rep in range(2 + REPS):
        rec = rep >= 2
        for k, s in shapes.items():
            for w in WINDOWS_MIB:
                timers[f"{k}_w{w}"].run(
                    lambda: inplace(ctx, s["segs"], s["ends"], s["keep"], s["store"], buf, size, s["new_len"],
                                    w << 20, size), record=rec)
            timers[f"parent_{k}"].run(
                lambda: parent(ctx, s["segs"], s["keep"], old.blob, s["store"], out, s["new_len"]), record=rec)
            nbytes = totals[k, WINDOWS_MIB[0]]["written_bytes"]
            # (out of the buffer itself: the old version is 4 KiB shorter than insert_front's target)
            timers[f"memcpy_d2d_{k}"].run(lambda: copy(nbytes), record=rec)

    rows = {k: {"device": summary(t.dev), "host_clock": summary(t.host)} for k, t in timers.items()}
    for k in shapes:
        par = rows[f"parent_{k}"]["device"]["ms_median"]
        d2d = rows[f"memcpy_d2d_{k}"]["device"]["ms_median"]
        c = {"parent_ms_median": par, "memcpy_d2d_ms_median": d2d}
        for w in WINDOWS_MIB:
            ms = rows[f"{k}_w{w}"]["device"]["ms_median"]
            tot = totals[k, w]
            c[f"w{w}"] = {"totals": tot, "ms_median": ms, "time_over_parent": round(ms / par, 3),
                          "time_over_memcpy_d2d": round(ms / d2d, 3),
                          "TBps_read_plus_written": round(
                              2 * (tot["written_bytes"] + tot["stash_bytes"]) / (ms * 1e-3) / 1e12, 3)}
        res["shapes"][k] = c
    res["rows"] = rows
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
