"""The cut list's capacity contract on every stitch and shard writer.

Every call that returns a cut list takes out_ends and cap; with a cap below
the count it returns DSX_E_CAPACITY, *n_out holds the count, and nothing is
written at or past out_ends[cap] (include/dsx.h).  With DSX_OUT_DEVICE the
writers are kernels, one per stitch back-end, and the call's geometry picks
the back-end.  Each case below reaches one writer (cut_cap_ref.py restates
the geometry rule, tests/test_cut_capacity_host.py checks the claims on the
CPU) and sweeps cut_cap_ref.caps(n): 0 with a NULL pointer, 1, n // 3, n - 1,
n, n + 1 and the documented bound, each call into its own FencedOut.  After a
failing call the same context cuts the same bytes with cap = upper and must
return the oracle's list (no error bit or count survives).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import cut_cap_ref as cc
from cut_cap_ref import FencedOut, caps, check, check_fences, check_untouched

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(REPO, "desync_amd", "libdsx_diag.so")


def dev(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint8)).to("cuda")
    torch.cuda.synchronize()
    return t


def params(prm):
    import desync_amd
    return desync_amd.Params(*prm)


def ctx_with(**env):
    """A context of its own: a context reads its DSX_* settings when created."""
    from desync_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def floor_ctx():
    """64 KiB stitch segments (48/192/768: lists of more than 64 cuts, and
    more than 2048 segments in 129 MiB)."""
    ctx = ctx_with(DSX_SEG_FLOOR=65536)
    yield ctx
    ctx.close()


def cut(ctx, t, p, fenced, flags):
    from desync_amd import _lib
    n = ctypes.c_uint64(0xDEAD)
    rc = _lib.lib().dsx_cut_device(ctx.h, ctypes.c_void_p(t.data_ptr()), t.numel(), ctypes.byref(p.c),
                                   fenced.ptr_or_null, fenced.cap, ctypes.byref(n), flags)
    return rc, n.value


def sweep(ctx, case, where, cap_list=None, after=None, tag="", t=None):
    """One dsx_cut_device per cap, each into a fresh fence; `after(rc)` runs
    after every call (the case's condition on the context's stats)."""
    from desync_amd import _lib
    t, p = dev(case.data) if t is None else t, params(case.params)
    flags = _lib.DSX_OUT_DEVICE if where == "device" else _lib.DSX_OUT_HOST
    failed = 0
    for cap in cap_list or caps(case.n, case.upper):
        f = FencedOut(case.upper, cap, where)
        rc, n = cut(ctx, t, p, f, flags)
        check(f, rc, n, case.want, tag)
        if after:
            after(rc)
        if rc != 0:
            failed += 1
            f = FencedOut(case.upper, case.upper, where)
            rc, n = cut(ctx, t, p, f, flags)
            check(f, rc, n, case.want, tag + " after a failure")
            if after:
                after(rc)
    assert failed >= 4  # caps 0, 1, n // 3 and n - 1


# ------------------------------------------------------------- finish_kernel
@pytest.mark.parametrize("where", ["device", "host"])
def test_fast_short_lists(dctx, where):
    """finish_kernel's fast path, every staged list in its first store loop."""
    case = cc.fast_short()
    assert cc.backend(case.nseg) == "finish" and case.nseg <= 256
    assert cc.cuts_per_segment(case.want, cc.stitch_seg(case.data.size, case.params[2])).max() <= 64

    def after(rc):
        st = dctx.stats()
        assert st.repaired_segments == 0 and st.chunks == case.n

    sweep(dctx, case, where, after=after, tag="fast short")


@pytest.mark.parametrize("where", ["device", "host"])
def test_fast_long_lists(floor_ctx, where):
    """finish_kernel's fast path, the i >= 64 store loop."""
    case = cc.fast_long()
    assert cc.backend(case.nseg) == "finish"
    assert cc.cuts_per_segment(case.want, 65536).max() > 64
    dense = floor_ctx.stats().dense_fallbacks

    def after(rc):
        st = floor_ctx.stats()
        assert st.repaired_segments == 0 and st.dense_fallbacks == dense

    sweep(floor_ctx, case, where, after=after, tag="fast long")


def test_suspect_in_finish(dctx):
    """Workgroup 0's fixup_body and inline gather."""
    case = cc.zero_runs()
    assert cc.backend(case.nseg) == "finish"

    def after(rc):
        assert dctx.stats().repaired_segments > 0

    sweep(dctx, case, "device", after=after, tag="suspect in finish")


# ------------------------------------------------------------- gather_kernel
def test_gather_clean(floor_ctx):
    """fixup_fast_kernel's fast path + gather_kernel: more than 2048 segments."""
    case = cc.gather_clean()
    assert case.nseg > 2048 and cc.backend(case.nseg) == "fixup_fast+gather"
    dense = floor_ctx.stats().dense_fallbacks

    def after(rc):
        st = floor_ctx.stats()
        assert st.repaired_segments == 0 and st.dense_fallbacks == dense

    sweep(floor_ctx, case, "device", after=after, tag="gather clean")


def test_gather_suspect(floor_ctx):
    """fixup_body (from fixup_fast_kernel) + gather_kernel."""
    case = cc.gather_suspect()
    assert case.nseg > 2048 and cc.backend(case.nseg) == "fixup_fast+gather"
    dense = floor_ctx.stats().dense_fallbacks

    def after(rc):
        st = floor_ctx.stats()
        assert st.repaired_segments > 0 and st.dense_fallbacks == dense

    sweep(floor_ctx, case, "device", after=after, tag="gather suspect")


# --------------------------------------------------------------- dense retry
def test_dense_several_pieces(dctx):
    """The dense retry's 32 MiB pieces, the capacity running out in the first,
    the second and the third: earlier pieces are written, the first that does
    not fit and the later ones are not, the count goes on.  Every segment of
    a dense piece is flagged, so each piece ends in finish_kernel's suspect
    path and the rule tested is fixup_body's s_total0 + piece_cuts > out_cap."""
    case = cc.dense_pieces()
    cap_list, at = cc.dense_caps(case)
    assert 0 < at[0] < at[1] < case.n and case.data.size > 2 * cc.DENSE_PIECE
    seen = {"dense": dctx.stats().dense_fallbacks}

    def after(rc):
        now = dctx.stats().dense_fallbacks
        assert now > seen["dense"]
        seen["dense"] = now

    sweep(dctx, case, "device", cap_list=cap_list, after=after, tag="dense pieces")


def test_two_product_pieces(dctx):
    """8 GiB + 64 MiB of uniform bytes: the first piece ends in
    fixup_fast_kernel + gather_kernel (4096 segments), the second in
    finish_kernel's fast path with cuts already counted (base > 0).  The
    capacity runs out in the first piece (the second writes nothing, the
    count goes on) and in the second (the first piece's cuts are written)."""
    import torch
    from desync_amd import _lib
    from oracle import oracle as o
    n, mx = cc.TWO_PIECES_LEN, cc.DFLT[2]
    assert cc.backend(cc.piece_nseg(0, cc.PIECE_MAX, n, mx)) == "fixup_fast+gather"
    assert cc.backend(cc.piece_nseg(cc.PIECE_MAX, n - cc.PIECE_MAX, n, mx)) == "finish"
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().dsx_gen_uniform(dctx.h, ctypes.c_void_p(t.data_ptr()), 0, n, 9), dctx.h)
    host = t.cpu().numpy()
    want = o.chunk_parallel(host, *cc.DFLT, o.default_threads())
    del host
    case = cc.Case(None, cc.DFLT, want=want, length=n)
    cap_list, at = cc.piece_cut_caps(want, case.n, case.upper, [cc.PIECE_MAX])
    assert 0 < at[0] < case.n - 600 and int(want[-1]) == n
    seen = {"pieces": dctx.stats().pieces}

    def after(rc):
        st = dctx.stats()
        assert st.pieces == seen["pieces"] + 2 and st.repaired_segments == 0
        seen["pieces"] = st.pieces

    try:
        sweep(dctx, case, "device", cap_list=cap_list, after=after, tag="two pieces", t=t)
    finally:
        del t
        torch.cuda.empty_cache()


# -------------------------------------------------------------------- queued
def test_queued_calls(dctx):
    """Eight DSX_NO_SYNC calls, short ones between fitting ones: dsx_result
    answers each call's own rc and count, in order; the dense tile's call is
    redone inside dsx_result with the caller's cap."""
    from desync_amd import _lib
    L = _lib.lib()
    jobs = cc.queued_blobs()
    short_caps = iter((1, 0))
    queue = []
    n = ctypes.c_uint64()
    for case, short in jobs:
        cap = case.upper
        if short:
            cap = case.n - 1 if case in (cc.zero_runs(), cc.dense_small()) else next(short_caps)
        t, p, f = dev(case.data), params(case.params), FencedOut(case.upper, cap, "device")
        rc = L.dsx_cut_device(dctx.h, ctypes.c_void_p(t.data_ptr()), t.numel(), ctypes.byref(p.c),
                              f.ptr_or_null, f.cap, ctypes.byref(n),
                              _lib.DSX_OUT_DEVICE | _lib.DSX_NO_SYNC)
        assert rc == 0
        queue.append((case, short, t, p, f))
    dense = dctx.stats().dense_fallbacks
    for i, (case, short, t, p, f) in enumerate(queue):
        n.value = 0xDEAD
        rc = L.dsx_result(dctx.h, ctypes.byref(n))
        assert (rc != 0) == short, (i, rc)
        check(f, rc, n.value, case.want, f"queued call {i}")
        if case is cc.zero_runs():
            assert dctx.stats().repaired_segments > 0
        if case is cc.dense_small():
            assert dctx.stats().dense_fallbacks > dense
    assert L.dsx_result(dctx.h, ctypes.byref(n)) == _lib.DSX_E_STATE
    for i, (case, short, t, p, f) in enumerate(queue):
        if short:
            f = FencedOut(case.upper, case.upper, "device")
            rc, got = cut(dctx, t, p, f, _lib.DSX_OUT_DEVICE)
            check(f, rc, got, case.want, f"queued call {i} again")


# ---------------------------------------------------------------------- many
def _many(ctx, t, case, p, f, first, flags):
    from desync_amd import _lib
    n, totals = ctypes.c_uint64(0xDEAD), _lib.ManyTotals()
    rc = _lib.lib().dsx_cut_device_many(ctx.h, ctypes.c_void_p(t.data_ptr()), t.numel(),
                                        case.blob_ends.ctypes.data, case.blob_ends.size,
                                        ctypes.byref(p.c), f.ptr_or_null, f.cap, ctypes.byref(n),
                                        first.ptr, None, ctypes.byref(totals), flags)
    return rc, n.value, totals


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", ["plan", "fallback"])
def test_many(dctx, name, where):
    """many_gather_kernel behind the batched walk and behind the one-blob
    fallback; blob_first (host, nblobs + 1 entries) is fenced too and is not
    written by a failing call."""
    from desync_amd import _lib
    case = cc.many_plan() if name == "plan" else cc.many_fallback()
    t, p = dev(case.data), params(case.params)
    flags = _lib.DSX_OUT_DEVICE if where == "device" else _lib.DSX_OUT_HOST
    nb = case.blob_ends.size

    def call(cap):
        f, first = FencedOut(case.upper, cap, where), FencedOut(nb + 1, nb + 1, "host")
        rc, n, totals = _many(dctx, t, case, p, f, first, flags)
        check(f, rc, n, case.want, f"many {name}")
        assert totals.chunks == case.n and totals.blobs == nb  # (totals is written either way)
        if name == "fallback":
            assert totals.redone_blobs + totals.single_blobs > 0
        else:
            assert totals.redone_blobs == totals.single_blobs == 0 and totals.groups == 1
        if rc == 0:
            check(first, 0, nb + 1, case.first, f"many {name} blob_first")
        else:
            check_untouched(first, f"many {name} blob_first after DSX_E_CAPACITY")
        return rc

    for cap in caps(case.n, case.upper):
        if call(cap) != 0:
            assert call(case.upper) == 0


# -------------------------------------------------------------------- shards
def _shard_local(case, ctxs, t, p, recs_ptr, flags):
    from desync_amd import _lib
    L = _lib.lib()
    for r, (start, length) in enumerate(case.geo):
        _lib.check(L.dsx_shard_local(ctxs[r].h, ctypes.c_void_p(t.data_ptr() + start), 64 if r else 0,
                                     start, length, case.data.size, ctypes.byref(p.c),
                                     ctypes.c_void_p(recs_ptr[r]), flags), ctxs[r].h)


def _resolve_round(case, ctxs, recs, fences, flags):
    """dsx_shard_resolve on every rank over host records -> [(rc, n)]."""
    from desync_amd import _lib
    L = _lib.lib()
    allrec = (_lib.Seam * case.world)(*recs)
    out = []
    for r in range(case.world):
        n = ctypes.c_uint64(0xDEAD)
        rc = L.dsx_shard_resolve(ctxs[r].h, ctypes.c_void_p(ctypes.addressof(allrec)), case.world, r,
                                 ctypes.c_void_p(ctypes.addressof(recs[r])), fences[r].ptr_or_null,
                                 fences[r].cap, ctypes.byref(n), flags)
        out.append((rc, n.value))
    return out


@pytest.mark.parametrize("where", ["device", "host"])
def test_shards_sync(where):
    """shard_emit_kernel with the caller's cap (device output) and
    shard_outcome's n > cap (host output): rank 1 short, ranks 0 and 2 not."""
    from desync_amd import _lib
    case = cc.shards_uniform()
    t, p = dev(case.data), params(case.params)
    ctxs = [_lib.Context(0) for _ in range(case.world)]
    try:
        recs = [_lib.Seam() for _ in range(case.world)]
        _shard_local(case, ctxs, t, p, [ctypes.addressof(x) for x in recs], 0)
        flags = _lib.DSX_OUT_DEVICE if where == "device" else 0
        failed = 0
        for cap in caps(case.want[1].size, case.upper[1]):
            for c1 in (cap, case.upper[1]):  # (after a failure: the same contexts with cap = upper)
                fences = [FencedOut(case.upper[r], c1 if r == 1 else case.upper[r], where, True)
                          for r in range(case.world)]
                res = _resolve_round(case, ctxs, recs, fences, flags)
                for r, (rc, n) in enumerate(res):
                    check(fences[r], rc, n, case.want[r], f"shards sync rank {r}")
                if res[1][0] == 0:
                    break
                failed += 1
        assert failed >= 4
    finally:
        for c in ctxs:
            c.close()


def test_shards_async():
    """dsx_shard_resolve_async / dsx_shard_collect: a short rank 1 publishes
    code 2; after the MAX, collect answers DSX_E_CAPACITY with the count on
    rank 1 and DSX_E_PEER on the others."""
    import torch
    from desync_amd import _lib, shard
    L = _lib.lib()
    case = cc.shards_uniform()
    W = case.world
    t, p = dev(case.data), params(case.params)
    ctxs = [_lib.Context(0) for _ in range(W)]
    try:
        recs = [torch.zeros(shard.SEAM_BYTES, dtype=torch.uint8, device="cuda") for _ in range(W)]
        torch.cuda.synchronize()
        _shard_local(case, ctxs, t, p, [x.data_ptr() for x in recs],
                     _lib.DSX_SEAM_DEVICE | _lib.DSX_NO_SYNC)
        for c in ctxs:
            _lib.check(L.dsx_sync(c.h), c.h)
        allrec = torch.cat(recs)
        torch.cuda.synchronize()
        n1 = case.want[1].size
        failed = 0
        for cap in caps(n1, case.upper[1]):
            for c1 in (cap, case.upper[1]):
                fences = [FencedOut(case.upper[r], c1 if r == 1 else case.upper[r], "device", True)
                          for r in range(W)]
                codes = torch.full((W,), 0x5A5A, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                for r in range(W):  # (the async call wants a pointer even with cap 0)
                    _lib.check(L.dsx_shard_resolve_async(
                        ctxs[r].h, ctypes.c_void_p(allrec.data_ptr()), W, r, fences[r].ptr, fences[r].cap,
                        ctypes.c_void_p(codes.data_ptr() + 4 * r)), ctxs[r].h)
                for c in ctxs:  # the ranks' all-reduce (MAX) of the code words, by hand
                    _lib.check(L.dsx_sync(c.h), c.h)
                agreed_d = codes.max().reshape(1).contiguous()
                torch.cuda.synchronize()
                short = c1 < n1
                assert codes.cpu().tolist() == [0, 2 if short else 0, 0]
                for r in range(W):
                    agreed, n = ctypes.c_int32(-1), ctypes.c_uint64(0xDEAD)
                    rc = L.dsx_shard_collect(ctxs[r].h, ctypes.c_void_p(recs[r].data_ptr()),
                                             ctypes.c_void_p(agreed_d.data_ptr()), ctypes.byref(agreed),
                                             ctypes.byref(n))
                    assert agreed.value == (2 if short else 0)
                    if short and r != 1:
                        assert rc == _lib.DSX_E_PEER and n.value == 0, (r, rc, n.value)
                        check_fences(fences[r], case.want[r].size, f"shards async rank {r}")
                    else:
                        check(fences[r], rc, n.value, case.want[r], f"shards async rank {r}")
                if not short:
                    break
                failed += 1
        assert failed >= 4
    finally:
        for c in ctxs:
            c.close()


def test_shards_rewalk_then_short():
    """Owners re-walk their shards (DSX_E_RESYNC) and rank 1, short by one,
    then gets DSX_E_CAPACITY from the emit that follows its re-walk; the same
    contexts finish with cap = upper."""
    from desync_amd import _lib
    case = cc.shards_zero_run()
    t, p = dev(case.data), params(case.params)
    ctxs = [_lib.Context(0) for _ in range(case.world)]
    try:
        recs = [_lib.Seam() for _ in range(case.world)]
        _shard_local(case, ctxs, t, p, [ctypes.addressof(x) for x in recs], 0)
        n1 = case.want[1].size
        rounds = 0
        while True:
            rounds += 1
            assert rounds <= case.world
            fences = [FencedOut(case.upper[r], n1 - 1 if r == 1 else case.upper[r], "device", True)
                      for r in range(case.world)]
            res = _resolve_round(case, ctxs, recs, fences, _lib.DSX_OUT_DEVICE)
            if all(rc == _lib.DSX_E_RESYNC for rc, _ in res):
                for r in range(case.world):
                    assert res[r][1] == 0
                    check_fences(fences[r], 0, f"re-walk round {rounds} rank {r}")
                continue
            break
        assert rounds > 1 and recs[1].flags & _lib.DSX_SEAM_REWALKED
        for r, (rc, n) in enumerate(res):
            check(fences[r], rc, n, case.want[r], f"re-walk rank {r}")
        assert res[1][0] == _lib.DSX_E_CAPACITY
        fences = [FencedOut(case.upper[r], case.upper[r], "device") for r in range(case.world)]
        for r, (rc, n) in enumerate(_resolve_round(case, ctxs, recs, fences, _lib.DSX_OUT_DEVICE)):
            check(fences[r], rc, n, case.want[r], f"re-walk rank {r} again")
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------- the diagnostic build, one child process
def test_diag_backends():
    """fixup_fast_kernel + gather_kernel and fixup_kernel + gather_kernel at
    8 MiB (DSX_FINISH=0, DSX_FIXUP_FAST=0) and finish_task (DSX_FUSE=1, queued
    calls): libdsx_diag.so, which the package never loads itself."""
    assert os.path.exists(DIAG), "libdsx_diag.so missing: __graft_entry__.build() makes it"
    env = dict(os.environ, DSX_LIB_PATH=DIAG, PYTHONPATH=REPO)
    for k in ("DSX_FINISH", "DSX_FIXUP_FAST", "DSX_FUSE", "DSX_SEG_FLOOR"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for name in ("fixup_fast+gather", "fixup+gather", "finish_task"):
        assert f"ok: {name}" in r.stdout, r.stdout[-3000:]


def _diag_fused(ctx):
    """Three queued calls per cap, the middle one with the cap under test:
    its stitch runs as tasks inside the next call's scan (finish_task), the
    last call's in the flush of dsx_result."""
    from desync_amd import _lib
    L = _lib.lib()
    case = cc.fast_short()
    t, p = dev(case.data), params(case.params)
    n = ctypes.c_uint64()
    for cap in caps(case.n, case.upper):
        for order in ((case.upper, cap, case.upper), (cap, case.upper, cap)):
            fences = [FencedOut(case.upper, c, "device") for c in order]
            for f in fences:
                assert L.dsx_cut_device(ctx.h, ctypes.c_void_p(t.data_ptr()), t.numel(), ctypes.byref(p.c),
                                        f.ptr_or_null, f.cap, ctypes.byref(n),
                                        _lib.DSX_OUT_DEVICE | _lib.DSX_NO_SYNC | _lib.DSX_TIMED) == 0
            for i, f in enumerate(fences):
                n.value = 0xDEAD
                rc = L.dsx_result(ctx.h, ctypes.byref(n))
                check(f, rc, n.value, case.want, f"fused call {i} of {order}")
                st = ctx.stats()  # (a timed call stitched behind a scan reports no stitch time)
                assert st.scan_ms > 0 and st.stitch_ms == 0, (st.scan_ms, st.stitch_ms)
        f = FencedOut(case.upper, case.upper, "device")
        rc, got = cut(ctx, t, p, f, _lib.DSX_OUT_DEVICE)
        check(f, rc, got, case.want, "fused: a synchronous call after")


def _main():
    from desync_amd import _lib
    assert os.path.basename(_lib.LIB_PATH).startswith("libdsx_diag")
    for name, env in (("fixup_fast+gather", {"DSX_FINISH": 0}),
                      ("fixup+gather", {"DSX_FINISH": 0, "DSX_FIXUP_FAST": 0})):
        ctx = ctx_with(**env)
        try:
            sweep(ctx, cc.fast_short(), "device", tag=name)
            def repaired(rc, ctx=ctx):
                assert ctx.stats().repaired_segments > 0

            sweep(ctx, cc.zero_runs(), "device", tag=name + " suspect", after=repaired)
        finally:
            ctx.close()
        print("ok:", name, flush=True)
    ctx = ctx_with(DSX_FUSE=1)
    try:
        _diag_fused(ctx)
    finally:
        ctx.close()
    print("ok: finish_task", flush=True)


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    _main()
