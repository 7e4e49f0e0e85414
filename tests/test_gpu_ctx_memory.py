"""A context gives back the HBM it took: hipMemGetInfo across whole context
lives.  Every device allocation of the library goes through the context's
ledger (csrc/dsx_devmem.h), dsx_ctx_destroy frees what the ledger still holds,
and stats().device_bytes is the ledger's total; tests/devmem_model.cpp checks
the ledger itself on the CPU, this file that nothing on the device escapes it.

hipMemGetInfo moves in 2 MiB reservations, and torch's caching allocator keeps
what a cycle's tensors took, so every reading is taken after a warm-up cycle
and after torch.cuda.empty_cache()."""
import ctypes
import gc
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIN, AVG, MAX = 4096, 16384, 65536
BLOB = 4 << 20
KEY = bytes(range(32))
MiB = 1 << 20


def _free_hbm():
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_stamp_ring_comes_back():
    """dsx_stamps_begin's ring (max_launches x ncu x 8 waves x 32 B, the largest
    buffer bench.py's timed loop makes) is freed with its context: three
    contexts that each stamped 2048 launches leave less than half a ring
    behind (a ring no destroy frees costs one per cycle, 128 MiB and more on a
    256-CU part; hipMemGetInfo's 2 MiB granularity is far below the bound)."""
    import torch
    from desync_amd import _lib

    def cycle():
        ctx = _lib.Context(0)
        try:
            ctx.stamps_begin(2048)
            ring = ctx.stats().device_bytes
            ctx.stamps_end()
        finally:
            ctx.close()
        return ring

    cycle()  # (the runtime's own code-object and stream memory)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    free0 = _free_hbm()
    rings = [cycle() for _ in range(3)]
    drop = free0 - _free_hbm()
    ring = rings[0]
    print(f"ring {ring} bytes ({ring / MiB:.1f} MiB), ncu {ncu}, drop over 3 cycles {drop} bytes "
          f"({drop / MiB:.1f} MiB)")
    assert rings == [ring] * 3
    assert ring >= 2048 * ncu * 8 * 32
    assert drop < ring // 2, (drop, ring)


class _Inputs:
    """What every cycle reads: 4 MiB of seeded bytes on the device, their cut
    list and chunk IDs, a cut-list buffer (allocated once, so that the cycles
    themselves take nothing from torch but what the library's wrappers do)."""

    def __init__(self):
        import torch

        import desync_amd
        from desync_amd import _lib
        from oracle import oracle as o
        self.host = o.synth_uniform(77, 0, BLOB)
        self.t = torch.from_numpy(self.host.copy()).to("cuda:0")
        self.cap = BLOB // MIN + 4
        self.outs = [torch.empty(self.cap, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        ctx = _lib.Context(0)
        try:
            self.ends = desync_amd.cut_device(self.t.data_ptr(), BLOB, MIN, AVG, MAX, ctx=ctx)
            ids = desync_amd.chunk_ids(self.t.data_ptr(), BLOB, self.ends, 0, ctx=ctx)
        finally:
            ctx.close()
        self.ids = np.frombuffer(b"".join(bytes(i) for i in ids), dtype=np.uint8).reshape(-1, 32).copy()
        self.index = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=MAX),
                                      desync_amd.index.ChunkArray(self.ends, self.ids))
        # four blobs packed in the buffer, for dsx_cut_device_many
        self.blob_ends = np.array([BLOB // 4, BLOB // 2, BLOB // 2 + 12345, BLOB], dtype=np.uint64)
        torch.cuda.synchronize()


def _everything_cycle(inp, close_objects):
    """One context through every call that allocates device memory, then
    closed.  device_bytes never decreases across a call that only allocates."""
    import desync_amd
    from desync_amd import _lib
    from desync_amd.encrypt import aead_open, aead_seal
    L = _lib.lib()
    ptr, n = inp.t.data_ptr(), BLOB
    nchunks = len(inp.ends)
    assert 100 < nchunks < 1000
    ctx = _lib.Context(0)
    objects = []
    try:
        seen = [ctx.stats().device_bytes]
        assert seen[0] > 0  # (the chain state and the queue counters)

        def step(name, fn, strict=False):
            r = fn()
            now = ctx.stats().device_bytes
            assert now >= seen[-1], (name, seen[-1], now)
            if strict:
                assert now > seen[-1], (name, seen[-1], now)
            seen.append(now)
            return r

        # the index pipeline first, on the fresh context: its windows, and the
        # side streams' queue counters, which alone make the total grow
        ends, ids = step("index_host", lambda: desync_amd.make.index_host(inp.host, MIN, AVG, MAX, ctx=ctx),
                         strict=True)
        assert np.array_equal(ends, inp.ends) and np.array_equal(ids, inp.ids)
        got = step("cut_device", lambda: desync_amd.cut_device(ptr, n, MIN, AVG, MAX, ctx=ctx))
        assert np.array_equal(got, inp.ends)

        def queued_pair():
            for o in inp.outs:
                desync_amd.cut_device(ptr, n, MIN, AVG, MAX, ctx=ctx, out_ptr=o.data_ptr(), out_cap=inp.cap,
                                      sync=False)
            return [desync_amd.cut_device_result(ctx) for _ in inp.outs]
        assert step("queued pair", queued_pair) == [nchunks, nchunks]

        def stream():
            c = desync_amd.NewChunker(io.BytesIO(inp.host.tobytes()), MIN, AVG, MAX, ctx=ctx)
            try:
                return desync_amd.ChunkStream(None, c, desync_amd.MemoryStore(), 2)
            finally:
                c.close()
        idx = step("ChunkStream", stream)
        assert len(idx.Chunks) == nchunks and bytes(idx.Chunks[nchunks - 1].ID) == inp.ids[-1].tobytes()

        idset = step("IDSet", lambda: desync_amd.IDSet(inp.ids, ctx=ctx))
        objects.append(idset)
        assert len(idset) == nchunks
        store = step("DeviceStore", lambda: desync_amd.DeviceStore(BLOB + MiB, nchunks + 16, ctx=ctx))
        objects.append(store)
        tot = step("put", lambda: store.put(inp.t, inp.ids, inp.ends))
        assert tot["stored"] == nchunks
        out, rtot = step("read_ranges", lambda: store.read_ranges(inp.index, [(5, 100000), (BLOB - 70000, 70000)]))
        assert out.cpu().numpy().tobytes() == inp.host[5:100005].tobytes() + inp.host[BLOB - 70000:].tobytes()
        del out
        ids2, offs, ktot = step("chunk_ids_known", lambda: desync_amd.chunk_ids_known(store, inp.t, inp.ends))
        assert np.array_equal(ids2, inp.ids) and ktot["chunks"] == nchunks
        second = step("second store", lambda: desync_amd.DeviceStore(BLOB + MiB, nchunks + 16, ctx=ctx))
        objects.append(second)
        assert step("copy", lambda: second.CopyFrom(store))["copied"] == nchunks
        ptot = step("prune", lambda: store.Prune(inp.ids[::2]))  # (every other chunk leaves: the arena moves)
        assert ptot["kept"] == (nchunks + 1) // 2 and ptot["moved"] > 0

        def seal_open():
            rec, rec_ends = aead_seal(KEY, ptr, n, inp.ends, ctx=ctx)
            plain, plain_ends, bad = aead_open(KEY, rec.data_ptr(), int(rec_ends[-1]), rec_ends, ctx=ctx)
            return plain.cpu().numpy(), plain_ends, bad
        plain, plain_ends, bad = step("seal and open", seal_open)
        assert not bad and np.array_equal(plain_ends, inp.ends) and np.array_equal(plain, inp.host)

        mends, first, _mt = step("cut_device_many", lambda: desync_amd.cut_device_many(
            ptr, n, inp.blob_ends, MIN, AVG, MAX, ctx=ctx))
        assert int(mends[-1]) == BLOB and int(first[-1]) == len(mends)

        def shard():
            p = desync_amd.Params(MIN, AVG, MAX)
            rec = _lib.Seam()
            _lib.check(L.dsx_shard_local(ctx.h, ctypes.c_void_p(ptr), 0, 0, n, n, ctypes.byref(p.c),
                                         ctypes.c_void_p(ctypes.addressof(rec)), 0), ctx.h)
            allrec = (_lib.Seam * 1)(rec)
            cuts = np.empty(n // MIN + 4 + 1024, np.uint64)
            cnt = ctypes.c_uint64()
            _lib.check(L.dsx_shard_resolve(ctx.h, ctypes.c_void_p(ctypes.addressof(allrec)), 1, 0,
                                           ctypes.c_void_p(ctypes.addressof(rec)), cuts.ctypes.data, cuts.size,
                                           ctypes.byref(cnt), 0), ctx.h)
            return cuts[:cnt.value]
        assert np.array_equal(step("shard at one rank", shard), inp.ends)

        step("stamps_begin", lambda: ctx.stamps_begin(64), strict=True)
        ctx.stamps_end()

        if close_objects:  # (the other cycles leave them to dsx_ctx_destroy)
            for obj in objects:
                before = ctx.stats().device_bytes
                obj.close()
                assert ctx.stats().device_bytes < before
        return seen[-1]
    finally:
        ctx.close()
        for obj in objects:
            obj.close()  # (of a closed context: forgets the handle only)


def test_context_that_touched_everything_gives_everything_back():
    """Four context lives through every call that allocates (the index
    pipeline, cut lists synchronous, queued and of many blobs, a chunk stream
    with IDs, an ID set, two stores with put, read, recognise, copy and prune,
    the AEAD converter, a one-rank shard, the stamp ring) cost the device at
    most 8 MiB: one 2 MiB reservation per cycle of placement noise.  Half of
    the cycles close their stores and sets themselves, half leave them to the
    context."""
    inp = _Inputs()
    _everything_cycle(inp, True)  # (warm-up: code objects, streams, torch's and the host pool's first use)
    free0 = _free_hbm()
    peaks = [_everything_cycle(inp, i % 2 == 0) for i in range(4)]
    drop = free0 - _free_hbm()
    print(f"device_bytes at the end of a cycle {peaks}, drop over 4 cycles {drop} bytes ({drop / MiB:.1f} MiB)")
    assert len(set(peaks)) == 1, peaks  # (the same calls: the same total)
    assert drop <= 8 * MiB, drop
