#!/usr/bin/env python3
"""Seal / open rates of the AEAD store converter, on one MI355X,
for three shapes resident in HBM:

  store     the 4.7 store shape: a 4 GiB window of the dsx_gen_dedup stream
            (p = 0.5) cut at 16/64/256 KiB, about 60 K chunks;
  one       one chunk of 1 GiB;
  small     1 M chunks of 4 KiB.

For each: dsx_aead_seal (host ends, given nonces, so that drawing them is not
in the figure) and dsx_aead_open of its output, and in the same process,
alternating with them, hipMemcpyAsync device to device of the same plaintext
bytes: the project's usual yardstick.  Each is the median [min-max] of REPS
rounds after 2 warm-up rounds, timed with device events on the context's stream
around the synchronous call and by the host clock.  The opened bytes are
compared with the source once per shape.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/aead_rate.json).  Run on the GPU box: python tools/aead_rate.py
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

REPS = 10
MIN, AVG, MAX = 16384, 65536, 262144
KEY = bytes.fromhex("6368616e676520746869732070617373776f726420746f206120736563726574")
vp = ctypes.c_void_p


def shapes(ctx, gib, only):
    size = int(gib * (1 << 30)) // (1 << 20) * (1 << 20)
    blob = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().dsx_gen_dedup(ctx.h, vp(blob.data_ptr()), 8 * size, size, 5, 0.5), ctx.h)
    out = {}
    if "store" in only:
        out["store"] = np.asarray(desync_amd.cut_device(blob.data_ptr(), size, MIN, AVG, MAX, ctx=ctx), dtype=np.uint64)
    if "one" in only:
        out["one"] = np.array([min(size, 1 << 30)], dtype=np.uint64)
    if "small" in only:
        out["small"] = (np.arange(1, min(size >> 12, 1 << 20) + 1, dtype=np.uint64) << np.uint64(12))
    return blob, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--shapes", default="store,one,small")
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    L = _lib.lib()
    sp = vp()
    _lib.check(L.dsx_ctx_stream(ctx.h, ctypes.byref(sp)), ctx.h)
    stream = torch.cuda.ExternalStream(sp.value, device="cuda:0")
    hip = hip_runtime()
    blob, cases = shapes(ctx, args.gib, args.shapes.split(","))
    rng = np.random.default_rng(1)
    rows = {}
    for name, ends in cases.items():
        n, total = len(ends), int(ends[-1])
        nonces = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
        cap = total + _lib.DSX_AEAD_OVERHEAD * n
        rec = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        back = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        rec_ends = np.empty(n, dtype=np.uint64)
        out_ends = np.empty(n, dtype=np.uint64)
        bad = np.empty(1, dtype=np.uint32)
        n_bad = ctypes.c_uint64()
        torch.cuda.synchronize()

        def seal():
            _lib.check(L.dsx_aead_seal(ctx.h, 0, KEY, vp(blob.data_ptr()), total, vp(ends.ctypes.data), 0, n,
                                       nonces, vp(rec.data_ptr()), cap, vp(rec_ends.ctypes.data), 0), ctx.h)

        def open_():
            _lib.check(L.dsx_aead_open(ctx.h, 0, KEY, vp(rec.data_ptr()), cap, vp(rec_ends.ctypes.data), 0, n,
                                       vp(back.data_ptr()), total, vp(out_ends.ctypes.data),
                                       vp(bad.ctypes.data), 1, ctypes.byref(n_bad), 0), ctx.h)

        def copy():
            hip.hipMemcpyAsync(back.data_ptr(), blob.data_ptr(), total, HIP_D2D, sp)

        timers = {k: Timer(stream) for k in ("seal", "open", "memcpy_d2d")}
        for rep in range(2 + REPS):
            timers["seal"].run(seal, record=rep >= 2)
            timers["memcpy_d2d"].run(copy, record=rep >= 2)
            back.zero_()
            torch.cuda.synchronize()
            timers["open"].run(open_, record=rep >= 2)
            if rep == 0 and (n_bad.value or not torch.equal(back, blob[:total])):
                raise SystemExit(f"{name}: the opened bytes differ from the source")
        row = {"chunks": n, "plaintext_bytes": total}
        for k, t in timers.items():
            row[k] = {"device": summary(t.dev), "host_clock": summary(t.host)}
            ms = row[k]["device"]["ms_median"]
            row[k]["GBps_plaintext"] = round(total / (ms * 1e-3) / 1e9, 1)
        for k in ("seal", "open"):
            row[k]["time_over_memcpy_d2d"] = round(
                row[k]["device"]["ms_median"] / row["memcpy_d2d"]["device"]["ms_median"], 2)
        rows[name] = row
        del rec, back
        torch.cuda.empty_cache()
    res = {"tile_bytes": _lib.DSX_AEAD_TILE, "reps": REPS, "rows": rows,
           "device_bytes_after": ctx.stats().device_bytes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
