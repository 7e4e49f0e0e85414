"""dsx_store_copy on the GPU (desync_amd.copy: Copy, Cache; DeviceStore.CopyFrom,
Grow): dst's arena, entries and totals against the model (store_copy_ref.py)
byte for byte; the scan's edges at every kind of arena residue; missing IDs and
the capacity, both all or nothing; DSX_COPY_ALL; every placement of the IDs;
one ID 70,000 times; every refusal; a pruned source; and the Python layer."""
import ctypes
import functools

import numpy as np
import pytest

import store_copy_ref
import store_ref
from test_gpu_store import RawStore, goldens, last_error, same_as_model, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

U64_MAX = store_copy_ref.U64_MAX
ARENA = 2 << 20


def _torch():
    import torch
    return torch


def _L():
    from desync_amd import _lib
    return _lib


class CopyStore(RawStore):
    def copy_from(self, src, ids=None, n=None, flags=0):
        """ids: a numpy array (host), an integer device pointer or None (NULL).  -> (rc, totals dict)"""
        L = _L()
        tot = L.StoreCopyTotals()
        if ids is None or isinstance(ids, int):
            ip = ids
            n = 0 if n is None else n
        else:
            ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
            ip = ids.ctypes.data
            if n is None:
                n = len(ids)
        rc = L.lib().dsx_store_copy(self.ctx.h, self.h, src.h, ctypes.c_void_p(ip), n, ctypes.byref(tot), flags)
        self.err = last_error(self.ctx)  # (the next call on the context clears it)
        assert tot.reserved == 0
        return rc, {k: getattr(tot, k) for k in store_copy_ref.TOTALS}

    def copy_all(self, src):
        return self.copy_from(src, None, 0, _L().DSX_COPY_ALL)

    def prune(self, ids):
        tot = _L().StorePruneTotals()
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
        rc = _L().lib().dsx_store_prune(self.ctx.h, self.h, ids.ctypes.data, len(ids), 0, ctypes.byref(tot), 0)
        assert rc == 0, last_error(self.ctx)

    def snapshot(self):
        ids, ends = self.entries()
        return self.counts(), self.arena(whole=True).tobytes(), ids.tobytes(), ends.tobytes()


def view(ctx, device_store):
    """A desync_amd.DeviceStore through ctypes."""
    raw = CopyStore.__new__(CopyStore)
    raw.ctx, raw.h = ctx, device_store.h
    return raw


class Pool:
    """`count` distinct IDs with their chunks' bytes in one blob (host and HBM),
    out of which stores and their models are filled."""

    def __init__(self, count, sizes, seed):
        rng = np.random.default_rng(seed)
        self.ids = rng.integers(0, 256, (count, 32), dtype=np.uint8)
        assert len({r.tobytes() for r in self.ids}) == count
        self.ends = np.cumsum(np.asarray(sizes, dtype=np.uint64)).astype(np.uint64)
        self.blob = rng.integers(0, 256, int(self.ends[-1]) + 3, dtype=np.uint8)
        self.ptr, self._keep = to_dev(self.blob)

    def put(self, store, model, lo, hi):
        """Puts the chunks [lo, hi) into the store and its model."""
        if hi <= lo:
            return
        start = int(self.ends[lo - 1]) if lo else 0
        rc, tot = store.put(self.ptr, self.blob.size, self.ids[lo:hi], self.ends[lo:hi], start)
        assert rc == 0 and tot["stored"] == hi - lo, (rc, tot, last_error(store.ctx))
        model.put(self.blob.tobytes(), self.ids[lo:hi], self.ends[lo:hi], start)

    def pair(self, ctx, lo, hi, arena_bytes=ARENA, max_chunks=None):
        max_chunks = len(self.ids) + 8 if max_chunks is None else max_chunks
        s, m = CopyStore(ctx, arena_bytes, max_chunks), store_ref.Store(arena_bytes, max_chunks)
        self.put(s, m, lo, hi)
        return s, m


def check_copy(dst, model, src, src_model, ids, flags=0, n=None, model_ids=None):
    """One copy on the GPU and in the model: the rc, the totals and dst agree."""
    L = _L()
    before = model.counts()
    want = store_copy_ref.copy(model, src_model, ids if model_ids is None else model_ids)
    rc, tot = dst.copy_from(src, ids, n, flags)
    fits = want["missing"] or store_copy_ref.fits(before, want)
    assert rc == (0 if fits else L.DSX_E_CAPACITY), (rc, last_error(dst.ctx))
    assert tot == want
    assert tot["total"] == tot["copied"] + tot["present"] + tot["repeats"] + tot["missing"]
    same_as_model(dst, model)
    return tot


# ---- 1. scan edges ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_case(n):
    """A pool of which src holds about two thirds, [a, count), and dst is preloaded
    with about a third, [0, d), d > a: every ID is in one of the two.  Chunk sizes
    0..49, one of 4,097 and one of 70,001 (it crosses a DSX_ASSEMBLE_TILE edge),
    both in src only; n IDs drawn with duplicates, the two big ones among them
    (from n = 1 and n = 3 on)."""
    rng = np.random.default_rng(3000 + n)
    count = n // 2 + 6
    sizes = rng.integers(0, 50, count)
    sizes[1] = 0
    sizes[count - 1], sizes[count - 2] = 70001, 4097
    pool = Pool(count, sizes, 4000 + n)
    a = count // 3
    d = a + max(1, count // 8)
    assert d <= count - 2
    pick = rng.integers(0, count, n)
    pick[0] = count - 1
    if n > 2:
        pick[n // 2] = count - 2
    return pool, a, d, pool.ids[pick]


def preloaded(dctx, pool, d, residue):
    """dst and its model holding [0, d) and one pad chunk that makes `used` = residue mod 16."""
    dst, model = pool.pair(dctx, 0, d)
    pad = (residue - dst.counts()["bytes"]) % 16
    pad_id = np.full((1, 32), 0xA5, dtype=np.uint8)
    blob = np.arange(16, dtype=np.uint8)
    ptr, _k = to_dev(blob)
    rc, tot = dst.put(ptr, 16, pad_id, np.array([pad], dtype=np.uint64))
    assert rc == 0 and tot["stored"] == 1
    model.put(blob.tobytes(), pad_id, [pad])
    assert dst.counts()["bytes"] % 16 == residue
    return dst, model


# 65,537: one more than the second scan level takes in one pass (256 workgroups of 256 IDs)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 65537])
def test_scan_edges(dctx, n):
    pool, a, d, ids = scan_case(n)
    src, src_model = pool.pair(dctx, a, len(pool.ids))
    src_before = src.snapshot()
    shots = []
    try:
        for residue in (0, 1, 7, 15, 0):
            dst, model = preloaded(dctx, pool, d, residue)
            with dst:
                tot = check_copy(dst, model, src, src_model, ids)
                assert tot["missing"] == 0 and tot["copied"] >= 1 and tot["copied_bytes"] > 65536
                if residue == 0:
                    shots.append(dst.snapshot()[2:] + (dst.arena().tobytes(),))
        assert shots[0] == shots[1]  # two runs into fresh stores: identical bytes
        assert src.snapshot() == src_before
    finally:
        src.close()


# ---- 2. missing ---------------------------------------------------------------------
def test_missing_is_all_or_nothing(dctx):
    pool, a, d, ids = scan_case(513)
    rng = np.random.default_rng(21)
    absent = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    ask = np.concatenate([ids[:40], absent[1:2], ids[40:90], absent[0:1], absent[1:2], ids[90:], absent[2:3]])
    src, src_model = pool.pair(dctx, a, len(pool.ids))
    with src:
        dst, model = preloaded(dctx, pool, d, 7)
        with dst:
            before = dst.snapshot()
            where = dst.locate(pool.ids[:1])
            tot = check_copy(dst, model, src, src_model, ask)
            assert (tot["missing"], tot["first_missing"]) == (3, 40)
            assert dst.snapshot() == before
            got = dst.locate(pool.ids[:1])
            assert got[2] == 0 and all(np.array_equal(x, y) for x, y in zip(got[:2], where[:2]))
            # the same IDs preloaded into dst (src still lacks them): the rest is copied
            blob = rng.integers(0, 256, 30, dtype=np.uint8)
            ptr, _k = to_dev(blob)
            ends = np.array([10, 20, 30], dtype=np.uint64)
            rc, put = dst.put(ptr, 30, absent, ends)
            assert rc == 0 and put == model.put(blob.tobytes(), absent, ends)
            tot = check_copy(dst, model, src, src_model, ask)
            assert tot["missing"] == 0 and tot["first_missing"] == U64_MAX and tot["copied"] > 0
            assert tot["present"] >= 3


# ---- 3. capacity --------------------------------------------------------------------
def test_capacity_is_all_or_nothing(dctx):
    L = _L()
    pool = Pool(300, np.arange(300) % 23, 31)
    src, src_model = pool.pair(dctx, 100, 300)
    with src:
        ask = pool.ids[80:260]  # 20 are in dst already
        need = int(pool.ends[259] - pool.ends[99])
        have = int(pool.ends[99])
        more_id = np.full((1, 32), 0x5A, dtype=np.uint8)
        one = np.zeros(16, dtype=np.uint8)
        optr, _k = to_dev(one)
        for arena_bytes, max_chunks, ok in ((have + need, 100 + 159, False), (have + need - 1, 100 + 160, False),
                                            (have + need, 100 + 160, True)):
            dst, model = pool.pair(dctx, 0, 100, arena_bytes, max_chunks)
            with dst:
                before = dst.snapshot()
                tot = check_copy(dst, model, src, src_model, ask)  # (asserts the rc the model's rule gives)
                assert (tot["copied"], tot["copied_bytes"], tot["present"]) == (160, need, 20)
                if not ok:
                    assert dst.snapshot() == before and "do not fit" in dst.err
                    continue
                assert dst.counts()["chunks"] == max_chunks and dst.counts()["bytes"] == arena_bytes
                # the store is full now: a put is refused as before
                assert dst.put(optr, 16, more_id, np.array([1], dtype=np.uint64))[0] == L.DSX_E_CAPACITY
                assert dst.put(optr, 16, more_id, np.array([0], dtype=np.uint64))[0] == L.DSX_E_CAPACITY
                same_as_model(dst, model)


# ---- 4. DSX_COPY_ALL ----------------------------------------------------------------
def test_copy_all(dctx):
    pool, a, d, _ = scan_case(513)
    src, src_model = pool.pair(dctx, a, len(pool.ids))
    with src:
        src_before = src.snapshot()
        with CopyStore(dctx, ARENA, len(pool.ids)) as dst:
            model = store_ref.Store(ARENA, len(pool.ids))
            tot = check_copy(dst, model, src, src_model, None, _L().DSX_COPY_ALL)
            assert tot["copied"] == tot["total"] == src.counts()["chunks"]
            assert dst.snapshot()[2:] == src.snapshot()[2:]
            assert dst.arena().tobytes() == src.arena().tobytes()
            assert dst.counts()["bytes"] == src.counts()["bytes"]
            # again: everything is present
            tot = check_copy(dst, model, src, src_model, None, _L().DSX_COPY_ALL)
            assert tot["present"] == tot["total"] and tot["copied"] == 0
        dst, model = preloaded(dctx, pool, d, 1)  # half overlapping
        with dst:
            tot = check_copy(dst, model, src, src_model, None, _L().DSX_COPY_ALL)
            assert tot["present"] == d - a and tot["copied"] == len(pool.ids) - d
        # an empty source
        with CopyStore(dctx, 64, 4) as empty, CopyStore(dctx, 64, 4) as dst:
            rc, tot = dst.copy_all(empty)
            assert rc == 0 and tot == dict.fromkeys(store_copy_ref.TOTALS, 0) | {"first_missing": U64_MAX}
        assert src.snapshot() == src_before


def test_copy_all_of_the_goldens_verifies(dctx, goldens):
    b1 = goldens["blob1"]
    with CopyStore(dctx, 2 << 20, 256) as src, CopyStore(dctx, 2 << 20, 256) as dst:
        assert src.put(b1["ptr"], b1["host"].size, b1["ids"], b1["ends"])[0] == 0
        rc, tot = dst.copy_all(src)
        assert rc == 0 and (tot["copied"], tot["copied_bytes"]) == (131, 1114112)
        assert dst.snapshot()[2:] == src.snapshot()[2:] and dst.arena().tobytes() == src.arena().tobytes()
        assert dst.verify(0) == []


# ---- 5. placements ------------------------------------------------------------------
def test_id_placements(dctx):
    L = _L()
    pool, a, d, ids = scan_case(513)
    src, src_model = pool.pair(dctx, a, len(pool.ids))
    shots = []
    with src:
        for where in ("host", "device", "device+1"):
            dst, model = preloaded(dctx, pool, d, 15)
            with dst:
                if where == "host":
                    check_copy(dst, model, src, src_model, ids)
                else:
                    ptr, _k = to_dev(ids, 1 if where.endswith("1") else 0, 16)
                    check_copy(dst, model, src, src_model, ptr, L.DSX_IDS_DEVICE, len(ids), model_ids=ids)
                shots.append(dst.snapshot())
    assert shots[0] == shots[1] == shots[2]


# ---- 6. one ID 70,000 times ---------------------------------------------------------
def test_one_id_many_times(dctx):
    pool = Pool(4, [5, 0, 300, 7], 61)
    src, src_model = pool.pair(dctx, 0, 4)
    with src, CopyStore(dctx, 1 << 12, 8) as dst:
        model = store_ref.Store(1 << 12, 8)
        ask = np.repeat(pool.ids[2:3], 70000, axis=0)
        tot = check_copy(dst, model, src, src_model, ask)
        assert (tot["copied"], tot["repeats"], tot["copied_bytes"]) == (1, 69999, 300)
        tot = check_copy(dst, model, src, src_model, ask)
        assert (tot["copied"], tot["present"], tot["repeats"]) == (0, 1, 69999)


# ---- 7. refusals --------------------------------------------------------------------
def test_refusals(dctx):
    L = _L()
    E = L.DSX_E_INVAL
    pool = Pool(40, np.arange(40) + 1, 71)
    other = L.Context(0)
    try:
        src, src_model = pool.pair(dctx, 10, 40)
        dst, model = pool.pair(dctx, 0, 20)
        with src, dst, CopyStore(other, 1 << 12, 16) as foreign:
            before, src_before = dst.snapshot(), src.snapshot()
            ids = pool.ids[15:30]
            tot = L.StoreCopyTotals()
            call = L.lib().dsx_store_copy

            def refused(rc, text):
                assert rc == E, rc
                assert text in last_error(dctx), last_error(dctx)
                assert dst.snapshot() == before and src.snapshot() == src_before

            refused(call(dctx.h, None, src.h, ids.ctypes.data, 15, ctypes.byref(tot), 0), "missing")
            refused(call(dctx.h, dst.h, None, ids.ctypes.data, 15, ctypes.byref(tot), 0), "missing")
            refused(call(dctx.h, dst.h, src.h, ids.ctypes.data, 15, None, 0), "missing")
            assert call(None, dst.h, src.h, ids.ctypes.data, 15, ctypes.byref(tot), 0) == E
            refused(call(dctx.h, dst.h, dst.h, ids.ctypes.data, 15, ctypes.byref(tot), 0), "same store")
            refused(call(dctx.h, foreign.h, src.h, ids.ctypes.data, 15, ctypes.byref(tot), 0), "another context")
            refused(call(dctx.h, dst.h, foreign.h, ids.ctypes.data, 15, ctypes.byref(tot), 0), "another context")
            refused(dst.copy_from(src, None, 1)[0], "IDs are missing")
            refused(dst.copy_from(src, ids, 15, L.DSX_COPY_ALL)[0], "takes no IDs")
            refused(dst.copy_from(src, None, 3, L.DSX_COPY_ALL)[0], "takes no IDs")
            refused(dst.copy_from(src, ids, 0, L.DSX_COPY_ALL)[0], "takes no IDs")
            refused(dst.copy_from(src, ids, 0xFFFFFFF1)[0], "0xFFFFFFF0")
            for flags in (L.DSX_SIZES, L.DSX_OUT_DEVICE, L.DSX_PRUNE_REMOVE, L.DSX_ENDS_DEVICE, 1 << 20):
                refused(dst.copy_from(src, ids, 15, flags)[0], "flag")
            # n == 0: zero totals, with or without a list
            for arg in (None, ids):
                rc, t = dst.copy_from(src, arg, 0)
                assert rc == 0 and t == dict.fromkeys(store_copy_ref.TOTALS, 0) | {"first_missing": U64_MAX}
                assert dst.snapshot() == before
            # the stores and the context are still usable
            check_copy(dst, model, src, src_model, ids)
    finally:
        other.close()


# ---- 8. a pruned source ---------------------------------------------------------------
def test_after_a_prune_of_the_source(dctx):
    import store_prune_ref
    pool = Pool(600, np.arange(600) % 41, 81)
    src = CopyStore(dctx, ARENA, 600)
    src_model = store_prune_ref.Store(ARENA, 600)
    pool.put(src, src_model, 0, 600)
    with src, CopyStore(dctx, ARENA, 600) as dst:
        keep = pool.ids[np.arange(600) % 3 != 1]
        src.prune(keep)
        src_model.prune(keep)
        same_as_model(src, src_model)
        model = store_ref.Store(ARENA, 600)
        ask = pool.ids[::-1][:400]  # survivors and removed ones, last first: the removed are missing
        tot = check_copy(dst, model, src, src_model, ask)
        assert tot["missing"] > 0 and dst.counts()["chunks"] == 0
        ask = keep[::-1][:300]
        tot = check_copy(dst, model, src, src_model, ask)
        assert tot["copied"] == 300
        for row in ask[:5]:  # the bytes are the survivors'
            e = int(np.flatnonzero((pool.ids == row).all(axis=1))[0])
            lo = int(pool.ends[e - 1]) if e else 0
            assert model.get(row.tobytes()) == pool.blob[lo:int(pool.ends[e])].tobytes()


# ---- 9. the Python layer ---------------------------------------------------------------
def test_python_copy_from_and_copy(dctx, goldens):
    import desync_amd
    b1, b2 = goldens["blob1"], goldens["blob2"]
    with desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as big, \
            desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as small:
        big.put_index((b1["ptr"], b1["host"].size), b1["index"])
        src_model, model = store_ref.Store(4 << 20, 1024), store_ref.Store(4 << 20, 1024)
        src_model.put(b1["host"].tobytes(), b1["ids"], b1["ends"])
        # CopyFrom: a host array, then a device tensor, then everything
        want = store_copy_ref.copy(model, src_model, b1["ids"][:50])
        assert small.CopyFrom(big, b1["ids"][:50]) == want
        d_ids = _torch().from_numpy(b1["ids"][30:90].copy()).to("cuda:0")
        _torch().cuda.synchronize()
        assert small.CopyFrom(big, d_ids) == store_copy_ref.copy(model, src_model, b1["ids"][30:90])
        same_as_model(view(dctx, small), model)
        # Copy: blob2 has seven chunks blob1 lacks
        have = {r.tobytes() for r in b1["ids"]}
        first = next(i for i, r in enumerate(b2["ids"]) if r.tobytes() not in have)
        before = view(dctx, small).snapshot()
        with pytest.raises(desync_amd.ChunkMissing) as e:
            desync_amd.Copy(b2["index"], big, small)
        assert e.value.ID == b2["ids"][first].tobytes()
        assert view(dctx, small).snapshot() == before
        # a capacity error carries the totals
        with desync_amd.DeviceStore(1000, 1024, ctx=dctx) as tiny:
            with pytest.raises(desync_amd._lib.DsxError) as e:
                tiny.CopyFrom(big)
            assert e.value.code == desync_amd._lib.DSX_E_CAPACITY and e.value.totals["copied"] == 131
        desync_amd.Copy(b1["index"], big, small)
        store_copy_ref.copy(model, src_model, b1["ids"])
        same_as_model(view(dctx, small), model)
        tot = small.CopyFrom(big)
        assert tot == store_copy_ref.copy(model, src_model, None) and tot["present"] == 131
        assert len(small) == 131 and small.Verify() == []
        for cid in (b1["ids"][0].tobytes(), b1["ids"][160].tobytes()):
            assert small.GetChunk(cid) == big.GetChunk(cid)
        # a MemoryStore on one side: the reference's loop
        mem = desync_amd.MemoryStore()
        desync_amd.Copy(b1["ids"][:5], small, mem)
        assert mem.chunks[b1["ids"][3].tobytes()] == big.GetChunk(b1["ids"][3].tobytes())
        with desync_amd.DeviceStore(1 << 20, 64, ctx=dctx) as third:
            desync_amd.Copy(b1["ids"][:5], mem, third)
            assert third.GetChunk(b1["ids"][4].tobytes()) == big.GetChunk(b1["ids"][4].tobytes())


def test_python_grow(dctx, goldens):
    import desync_amd
    L = _L()
    b1, b2 = goldens["blob1"], goldens["blob2"]
    with desync_amd.DeviceStore(1114112, 131, ctx=dctx) as store:  # blob1's exact fit
        store.put_index((b1["ptr"], b1["host"].size), b1["index"])
        with pytest.raises(L.DsxError) as e:
            store.put_index((b2["ptr"], b2["host"].size), b2["index"])
        assert e.value.code == L.DSX_E_CAPACITY
        ids, ends = store.entries()
        chunks = {ids[k].tobytes(): store.GetChunk(ids[k].tobytes()) for k in (0, 1, 64, 130)}
        old_arena = view(dctx, store).arena().tobytes()
        tot = store.Grow(2 << 20, 200)
        assert (tot["total"], tot["copied"], tot["copied_bytes"]) == (131, 131, 1114112)
        assert store.counts() == {"chunks": 131, "bytes": 1114112, "max_chunks": 200, "arena_bytes": 2 << 20}
        got_ids, got_ends = store.entries()
        assert np.array_equal(got_ids, ids) and np.array_equal(got_ends, ends)
        assert view(dctx, store).arena().tobytes() == old_arena
        for cid, data in chunks.items():
            assert store.GetChunk(cid) == data
        assert store.put_index((b2["ptr"], b2["host"].size), b2["index"])["stored"] == 7
        assert store.Verify() == []
        # below the fill: refused, and the store stays usable
        with pytest.raises(L.DsxError) as e:
            store.Grow(2 << 20, 137)
        assert e.value.code == L.DSX_E_CAPACITY
        with pytest.raises(L.DsxError):
            store.Grow(1114112, 200)
        assert len(store) == 138 and store.Verify() == []
        for cid, data in chunks.items():
            assert store.GetChunk(cid) == data
        out, _ = desync_amd.AssembleBlob(b2["index"], store, null_seed=False, ctx=dctx)
        assert np.array_equal(out.cpu().numpy(), b2["host"])
        store.Grow(1114112 + 80029, 138)  # shrinking to the exact fill is a Grow too
        assert store.Verify() == [] and store.counts()["arena_bytes"] == 1114112 + 80029


def test_python_assemble_through_a_cache(dctx, goldens):
    import desync_amd
    b1 = goldens["blob1"]
    with desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as big, \
            desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as small:
        big.put_index((b1["ptr"], b1["host"].size), b1["index"])
        cache = desync_amd.Cache(big, small)
        plan = desync_amd.NewSeedSequencer(b1["index"], ctx=dctx).Plan()
        want = b1["ids"][plan.store_chunks]
        assert 0 < len(want) <= 131
        out, stats = desync_amd.AssembleBlob(b1["index"], cache, ctx=dctx)
        assert np.array_equal(out.cpu().numpy(), b1["host"])
        assert stats["chunks-from-store"] == len(want)
        assert np.array_equal(small.entries()[0], want)  # exactly the plan's store chunks, in its order
        assert len(big) == 131
        filled = view(dctx, small).snapshot()
        out, _ = desync_amd.AssembleBlob(b1["index"], cache, ctx=dctx)
        assert np.array_equal(out.cpu().numpy(), b1["host"])
        assert view(dctx, small).snapshot() == filled  # the second call copies nothing
        tot = small.CopyFrom(big, want)
        assert (tot["copied"], tot["present"], tot["missing"]) == (0, len(want), 0)
        # the cache as a store: a chunk small lacks comes from big and stays in small
        rest = [r.tobytes() for r in b1["ids"] if not small.HasChunk(r.tobytes())]
        if rest:
            assert cache.HasChunk(rest[0]) and cache.GetChunk(rest[0]) == big.GetChunk(rest[0])
            assert small.HasChunk(rest[0])
        with pytest.raises(desync_amd.ChunkMissing):
            cache.GetChunk(b"\x01" * 32)


def test_memory_accounting(dctx, goldens):
    import desync_amd
    L = _L()
    b1 = goldens["blob1"]
    ctx = L.Context(0)
    try:
        ptr, _k = to_dev(b1["host"])
        seen = []
        for _ in range(2):
            with desync_amd.DeviceStore(2 << 20, 256, ctx=ctx) as a, desync_amd.DeviceStore(3 << 20, 256, ctx=ctx) as b:
                a.put_index((ptr, b1["host"].size), b1["index"])
                assert b.CopyFrom(a, b1["ids"])["copied"] == 131
                assert ctx.stats().device_bytes >= (5 << 20)
                b.Grow(4 << 20, 512)
                inside = ctx.stats().device_bytes
            seen.append(ctx.stats().device_bytes)  # the scratch stays, the stores are gone
            assert seen[-1] <= inside - (6 << 20)
        assert seen[0] == seen[1]
    finally:
        ctx.close()
