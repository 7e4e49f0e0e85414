#!/usr/bin/env python3
"""Chunk-ID set rate: dsx_dedup over 524,384 IDs already in
HBM -- the headline job's chunk count -- for three inputs (all distinct, about
half duplicated from a pool, all equal), each without and with a seed set of
the same size, and dsx_idset_create of that seed.  Each call is timed with
device events on the context's stream around the (synchronous) call, and by
the host clock; after a warm-up, the median of REPS calls with min and max.

Beside it the same answer on the host from host-resident IDs, labelled as
what it is: a Python dict loop over 32-byte keys, np.unique over a 32-byte
void view, and the device-to-host copy of the IDs that either needs first.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/idset_rate.json).  Run on the GPU box: python tools/idset_rate.py
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import desync_amd  # noqa: E402
from desync_amd import _lib  # noqa: E402

N = 524384
REPS = 25
HOST_REPS = 3


def summary(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
            "ms_max": round(max(ts), 4), "reps": len(ts)}


def timed(stream, fn, reps=REPS, warmup=3):
    """fn() `reps` times: device events on `stream` around each call, and the host clock."""
    for _ in range(warmup):
        fn()
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return {"device": summary(dev), "host_clock": summary(host)}


def host_dict(ids):
    """info.go's loop as Python: first position per ID, by dict."""
    first = {}
    out = np.empty(len(ids), np.uint32)
    for i, k in enumerate(ids.view("V32").ravel().tolist()):
        out[i] = first.setdefault(k, i)
    return out


def host_unique(ids):
    _, first, inv = np.unique(ids.view("V32").ravel(), return_index=True, return_inverse=True)
    return first[inv].astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--n", type=int, default=N)
    args = ap.parse_args()
    n = args.n
    ctx = _lib.default_context(0)
    sp = ctypes.c_void_p()
    _lib.check(_lib.lib().dsx_ctx_stream(ctx.h, ctypes.byref(sp)), ctx.h)
    stream = torch.cuda.ExternalStream(sp.value, device="cuda:0")
    rng = np.random.default_rng(1)
    distinct = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pool = rng.integers(0, 256, (n // 4, 32), dtype=np.uint8)
    half = distinct.copy()
    dup = rng.random(n) < 0.5
    half[dup] = pool[rng.integers(0, len(pool), int(dup.sum()))]
    inputs = {"all_distinct": distinct, "half_duplicated": half,
              "all_equal": np.tile(distinct[0], (n, 1))}
    sizes = rng.integers(16 << 10, 256 << 10, n).astype(np.uint64)
    d_ends = torch.from_numpy(np.cumsum(sizes).astype(np.int64)).to("cuda:0")
    d_first = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_seedp = torch.empty(n, dtype=torch.int32, device="cuda:0")
    res = {"n": n, "id_bytes": n * 32, "rows": {}}
    for name, ids in inputs.items():
        d_ids = torch.from_numpy(ids).to("cuda:0")
        # a seed of the same size: half of its IDs are the target's
        seed_ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        seed_ids[::2] = ids[rng.integers(0, n, (n + 1) // 2)]
        d_seed_ids = torch.from_numpy(seed_ids).to("cuda:0")
        row = {}
        holder = []

        def create():
            if holder:
                holder.pop().close()
            holder.append(desync_amd.IDSet(d_seed_ids, ctx=ctx))
        row["idset_create"] = timed(stream, create)
        seed = holder[0]
        for label, sd in (("dedup", None), ("dedup_with_seed", seed)):
            def call():
                return desync_amd.dedup(d_ids, d_ends, seed=sd, ctx=ctx,
                                        out=(d_first.data_ptr(), d_seedp.data_ptr()))
            row[label] = timed(stream, call)
            row[label + "_totals"] = call()[2]
        # check against the host's answer once
        want = host_unique(ids)
        got = d_first.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), name
        seed.close()
        # the same question on the host, from host-resident IDs
        ts = []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            host_dict(ids)
            ts.append((time.perf_counter() - t0) * 1e3)
        row["host_python_dict_loop"] = summary(ts)
        ts = []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            host_unique(ids)
            ts.append((time.perf_counter() - t0) * 1e3)
        row["host_np_unique_void32"] = summary(ts)
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_ids.cpu()
            ts.append((time.perf_counter() - t0) * 1e3)
        row["ids_device_to_host_copy"] = summary(ts)
        res["rows"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
