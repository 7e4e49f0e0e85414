#!/usr/bin/env python3
"""Assembly and seed-plan rates, on one MI355X, for a resident
4 GiB target:

  (a) dsx_assemble of one aligned segment (a plain copy through the gather kernel);
  (b) dsx_assemble of a real plan: the target is a window of the dsx_gen_dedup
      stream cut with the default chunk sizes, its seeds two other windows of
      that stream, the rest a packed store buffer in HBM -- tens of thousands
      of segments at arbitrary byte offsets -- with the aligned two-word shift
      body (the product's) and with the unaligned-load body
      (DSX_ASSEMBLE_UNALIGNED);
  (c) hipMemcpyAsync device-to-device of the same bytes on the same stream.

The four alternate inside one process, REPS rounds after a warm-up; each call
is timed with device events on the context's stream and by the host clock
(dsx_assemble is synchronous: its time includes staging the segment table).
Rates count the bytes read plus the bytes written (null segments only write).

Also dsx_seed_plan for 524,384 chunks against a seed of the same size: the
identical index, and one in which each chunk is the seed's with probability
0.5, else new.

Prints one JSON line; with --out FILE also writes it there
(profiles/<tag>/assemble_rate.json).  Run on the GPU box: python tools/assemble_rate.py
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
from desync_amd import _lib, extract  # noqa: E402
from desync_amd.index import ChunkArray, FormatIndex, Index  # noqa: E402

REPS = 10
N_PLAN = 524384
MIN, AVG, MAX = 16384, 65536, 262144
HIP_D2D = 3


def summary(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
            "ms_max": round(max(ts), 4), "reps": len(ts)}


class Timer:
    def __init__(self, stream):
        self.stream, self.dev, self.host = stream, [], []

    def run(self, fn, record=True):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(self.stream)
        fn()
        b.record(self.stream)
        b.synchronize()
        if record:
            self.host.append((time.perf_counter() - t0) * 1e3)
            self.dev.append(a.elapsed_time(b))

    def result(self, traffic):
        r = {"device": summary(self.dev), "host_clock": summary(self.host), "traffic_bytes": traffic}
        r["TBps_device_median"] = round(traffic / (r["device"]["ms_median"] * 1e-3) / 1e12, 3)
        r["TBps_host_clock_median"] = round(traffic / (r["host_clock"]["ms_median"] * 1e-3) / 1e12, 3)
        return r


def hip_runtime():
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(path if os.path.exists(path) else "libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return hip


def window(ctx, offset, length, seed=5, p=0.5):
    t = torch.empty(length, dtype=torch.uint8, device="cuda:0")
    _lib.check(_lib.lib().dsx_gen_dedup(ctx.h, ctypes.c_void_p(t.data_ptr()), offset, length, seed, p), ctx.h)
    ends = desync_amd.cut_device(t.data_ptr(), length, MIN, AVG, MAX, ctx=ctx)
    ids = desync_amd.chunk_ids(t.data_ptr(), length, ends, 0, ctx=ctx)
    return t, Index(FormatIndex(0, MIN, AVG, MAX), ChunkArray(ends, b"".join(ids)))


def seg_rows(rows):
    a = np.zeros(len(rows), dtype=extract.SEG_DTYPE)
    for i, (dst, nbytes, source, src) in enumerate(rows):
        a[i] = (dst, nbytes, src, i, 1, source, 0xFFFFFFFF)
    return a


def raw_assemble(ctx, segs, seeds, store, out, flags):
    ns = len(seeds)
    ptrs = (ctypes.c_void_p * max(1, ns))(*[t.data_ptr() for t in seeds])
    lens = (ctypes.c_uint64 * max(1, ns))(*[t.numel() for t in seeds])
    sp, sl = (store.data_ptr(), store.numel()) if store is not None else (None, 0)
    rc = _lib.lib().dsx_assemble(ctx.h, ctypes.c_void_p(segs.ctypes.data), len(segs), ptrs, lens, ns,
                                 ctypes.c_void_p(sp), sl, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                 flags | _lib.DSX_STORE_DEVICE)
    if rc:
        raise _lib.DsxError(rc, (_lib.lib().dsx_last_error(ctx.h) or b"").decode())


def assemble_rates(ctx, stream, size, res):
    hip = hip_runtime()
    sp = ctypes.c_void_p()
    _lib.check(_lib.lib().dsx_ctx_stream(ctx.h, ctypes.byref(sp)), ctx.h)
    target, tix = window(ctx, 8 * size, size)
    s1, ix1 = window(ctx, size // 2 + 12345, size)
    s2, ix2 = window(ctx, 9 * size - 777 - size // 4, size)
    seeds = [desync_amd.NewIndexSeed(ix1, s1), desync_amd.NewIndexSeed(ix2, s2)]
    sq = desync_amd.NewSeedSequencer(tix, *seeds, null_seed=True, limit=0, ctx=ctx)
    t0 = time.perf_counter()
    plan = sq.Plan()
    plan_ms = (time.perf_counter() - t0) * 1e3
    tot = plan.totals
    # the packed store buffer, gathered out of the target by the same kernel
    ends = sq.ends
    starts = np.concatenate(([0], ends[:-1])).astype(np.uint64)
    pos = plan.store_chunks
    sizes = (ends - starts)[pos]
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64) if len(pos) else np.zeros(0, np.uint64)
    store = torch.empty(max(int(tot["store_len"]), 16), dtype=torch.uint8, device="cuda:0")
    if len(pos):
        raw_assemble(ctx, seg_rows(list(zip(offs.tolist(), sizes.tolist(), [0] * len(pos), starts[pos].tolist()))),
                     [target], None, store, 0)
    out = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    one = seg_rows([(0, size, 0, 0)])
    segs = np.ascontiguousarray(plan.segs)
    blobs = [s1, s2]
    calls = {
        "a_one_aligned_segment": lambda: raw_assemble(ctx, one, blobs, store, out, 0),
        "b_plan_shift_loads": lambda: raw_assemble(ctx, segs, blobs, store, out, 0),
        "b_plan_unaligned_loads": lambda: raw_assemble(ctx, segs, blobs, store, out, _lib.DSX_ASSEMBLE_UNALIGNED),
        "c_hipMemcpyAsync_d2d": lambda: hip.hipMemcpyAsync(out.data_ptr(), s1.data_ptr(), size, HIP_D2D, sp),
    }
    # the plan's result is the target, with either body
    for name in ("b_plan_unaligned_loads", "b_plan_shift_loads"):
        out.zero_()
        torch.cuda.synchronize()  # (torch's stream is not the context's)
        calls[name]()
        if not torch.equal(out, target):
            bad = torch.nonzero(out != target).flatten()
            raise SystemExit(f"{name}: {bad.numel()} wrong bytes, the first at {int(bad[0])}")
    timers = {k: Timer(stream) for k in calls}
    for rep in range(2 + REPS):
        for k, fn in calls.items():
            timers[k].run(fn, record=rep >= 2)
    plan_traffic = 2 * (tot["seed_bytes"] + tot["store_bytes"]) + tot["null_bytes"]
    rows = {k: timers[k].result(plan_traffic if k.startswith("b_") else 2 * size) for k in calls}
    c = rows["c_hipMemcpyAsync_d2d"]["TBps_device_median"]
    for k in rows:
        rows[k]["fraction_of_c"] = round(rows[k]["TBps_device_median"] / c, 3)
        rows[k]["fraction_of_6.29TBps"] = round(rows[k]["TBps_device_median"] / 6.29, 3)
    seg_bytes = plan.segs["bytes"]
    res["assemble"] = {
        "target_bytes": size, "tile": _lib.DSX_ASSEMBLE_TILE, "plan_ms_first_call": round(plan_ms, 2),
        "plan": dict(tot, chunks=len(ends), seg_bytes_median=int(np.median(seg_bytes)),
                     seg_bytes_max=int(seg_bytes.max()),
                     dst_misaligned=int(np.count_nonzero(plan.segs["dst_off"] % 16)),
                     src_misaligned=int(np.count_nonzero(plan.segs["src_off"] % 16))),
        "rows": rows}
    for s in seeds:
        s.close()


def plan_rates(ctx, res):
    rng = np.random.default_rng(3)
    n = N_PLAN
    seed_ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    half = seed_ids.copy()
    fresh = rng.random(n) >= 0.5
    half[fresh] = rng.integers(0, 256, (int(fresh.sum()), 32), dtype=np.uint8)
    sizes = rng.integers(MIN, MAX, n).astype(np.uint64)
    ends = np.cumsum(sizes, dtype=np.uint64)
    fi = FormatIndex(0, MIN, AVG, MAX)
    six = Index(fi, ChunkArray(ends, seed_ids))
    rows = {}
    for name, ids in (("identical", seed_ids), ("half_from_seed", half)):
        seed = desync_amd.NewIndexSeed(six)
        sq = desync_amd.NewSeedSequencer(Index(fi, ChunkArray(ends, ids)), seed, null_seed=True, limit=0, ctx=ctx)
        ts = []
        for rep in range(2 + REPS):
            t0 = time.perf_counter()
            plan = sq.Plan()
            if rep >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        rows[name] = dict(summary(ts), **plan.totals)
        seed.close()
    res["seed_plan"] = {"chunks": n, "seed_chunks": n, "host_clock_of_SeedSequencer.Plan": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--gib", type=float, default=4.0)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    sp = ctypes.c_void_p()
    _lib.check(_lib.lib().dsx_ctx_stream(ctx.h, ctypes.byref(sp)), ctx.h)
    stream = torch.cuda.ExternalStream(sp.value, device="cuda:0")
    res = {}
    assemble_rates(ctx, stream, int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20), res)
    plan_rates(ctx, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
