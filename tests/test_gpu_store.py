"""The chunk store in HBM on the GPU (dsx_store_*, desync_amd.store): the
arena, the entries and the totals against the dict-and-bytearray model
(store_ref.py) byte for byte; the scan's edges; crafted IDs; every placement of
the arguments; the all-or-nothing capacity rule; every refusal; locate,
resolve and verify; the Python layer; memory accounting; and make -> chop ->
extract end to end in HBM."""
import ctypes
import os
import threading

import numpy as np
import pytest

import store_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U64_MAX = 0xFFFFFFFFFFFFFFFF


def _torch():
    import torch
    return torch


def _L():
    from desync_amd import _lib
    return _lib


def to_dev(arr, residue=0, word=16):
    """The array's bytes in HBM at an address that is `residue` modulo `word`:
    -> (pointer, tensor to keep alive)."""
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = _torch().zeros(a.size + 2 * word, dtype=_torch().uint8, device="cuda:0")
    off = (residue - t.data_ptr()) % word
    if a.size:
        t[off:off + a.size] = _torch().from_numpy(a.copy())
    _torch().cuda.synchronize()  # (torch's stream is not the context's)
    assert (t.data_ptr() + off) % word == residue
    return t.data_ptr() + off, t


def last_error(ctx):
    m = _L().lib().dsx_last_error(ctx.h)
    return m.decode() if m else ""


class RawStore:
    """dsx_store_* through ctypes."""

    def __init__(self, ctx, arena_bytes, max_chunks):
        self.ctx = ctx
        self.h = ctypes.c_void_p()
        rc = _L().lib().dsx_store_create(ctx.h, arena_bytes, max_chunks, ctypes.byref(self.h))
        assert rc == 0 and self.h.value, rc

    def close(self):
        if self.h:
            assert _L().lib().dsx_store_destroy(self.ctx.h, self.h) == 0
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def put(self, blob_ptr, length, ids, ends, start=0, n=None, flags=0):
        """ids / ends: numpy arrays (host) or integer device pointers.  -> (rc, totals dict)"""
        tot = _L().StorePutTotals()
        ip = ids if isinstance(ids, int) else np.ascontiguousarray(ids).ctypes.data
        ep = ends if isinstance(ends, int) else np.ascontiguousarray(ends, dtype=np.uint64).ctypes.data
        if n is None:
            n = len(ends)
        keep = (ids, ends)  # noqa: F841
        rc = _L().lib().dsx_store_put(self.ctx.h, self.h, ctypes.c_void_p(blob_ptr), length,
                                      ctypes.c_void_p(ip), ctypes.c_void_p(ep), start, n,
                                      ctypes.byref(tot), flags)
        return rc, {k: getattr(tot, k) for k, _ in _L().StorePutTotals._fields_}

    def counts(self):
        c = _L().StoreCounts()
        assert _L().lib().dsx_store_count(self.h, ctypes.byref(c)) == 0
        return {k: getattr(c, k) for k, _ in _L().StoreCounts._fields_}

    def arena_ptr(self):
        p, used = ctypes.c_void_p(), ctypes.c_uint64()
        assert _L().lib().dsx_store_arena(self.h, ctypes.byref(p), ctypes.byref(used)) == 0
        return p.value, used.value

    def arena(self, whole=False):
        """The arena's used bytes (whole: all arena_bytes of it) on the host."""
        p, used = self.arena_ptr()
        n = self.counts()["arena_bytes"] if whole else used
        out = np.empty(n, dtype=np.uint8)
        if n:
            assert _L().lib().dsx_copy(self.ctx.h, out.ctypes.data, ctypes.c_void_p(p), n) == 0
        return out

    def entries(self):
        n = self.counts()["chunks"]
        ids = np.empty((n, 32), dtype=np.uint8)
        ends = np.empty(n, dtype=np.uint64)
        assert _L().lib().dsx_store_entries(self.ctx.h, self.h, 0, n, ids.ctypes.data, ends.ctypes.data,
                                            0) == 0
        return ids, ends

    def locate(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
        n = len(ids)
        offs, sizes = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
        miss = ctypes.c_uint64()
        rc = _L().lib().dsx_store_locate(self.ctx.h, self.h, ids.ctypes.data, n, offs.ctypes.data,
                                         sizes.ctypes.data, ctypes.byref(miss), 0)
        assert rc == 0, rc
        return offs, sizes, miss.value

    def verify(self, algo=0):
        n = self.counts()["chunks"]
        bad = np.zeros(max(1, n), dtype=np.uint32)
        nb = ctypes.c_uint64()
        rc = _L().lib().dsx_store_verify(self.ctx.h, self.h, algo, bad.ctypes.data, n, ctypes.byref(nb))
        assert rc == 0, (rc, last_error(self.ctx))
        return bad[:nb.value].tolist()


def same_as_model(store, model):
    """The counts, the entries, the used arena and every locate answer equal the model's."""
    assert store.counts() == model.counts()
    ids, ends = store.entries()
    mids, mends = model.entries()
    assert np.array_equal(ids, mids) and np.array_equal(ends, mends)
    assert store.arena().tobytes() == bytes(model.arena)
    if len(mids):
        offs, sizes, miss = store.locate(mids)
        moffs, msizes, mmiss = model.locate(mids)
        assert (offs.tolist(), sizes.tolist(), miss) == (moffs, msizes, mmiss)


def load_index(name):
    from desync_amd.index import IndexFromReader
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return IndexFromReader(f)


@pytest.fixture(scope="module")
def goldens():
    """blob1 / blob2: host bytes, device copies, (ids, ends), the Index."""
    from desync_amd.extract import _index_arrays
    out = {}
    for name in ("blob1", "blob2"):
        with open(os.path.join(GOLDEN, name), "rb") as f:
            data = np.frombuffer(f.read(), dtype=np.uint8)
        ix = load_index(name + ".caibx")
        ids, ends = _index_arrays(ix)
        ptr, keep = to_dev(data)
        out[name] = dict(host=data, ptr=ptr, keep=keep, ids=ids, ends=ends, index=ix, n=len(ends))
    return out


# ---- 1. goldens ---------------------------------------------------------------------
def test_goldens_counts_arena_locate_verify(dctx, goldens):
    b1, b2 = goldens["blob1"], goldens["blob2"]
    model = store_ref.Store(4 << 20, 1024)
    with RawStore(dctx, 4 << 20, 1024) as s:
        rc, tot = s.put(b1["ptr"], b1["host"].size, b1["ids"], b1["ends"])
        assert rc == 0, last_error(dctx)
        assert tot == {"total": 161, "stored": 131, "stored_bytes": 1114112, "present": 0, "repeats": 30}
        assert tot == model.put(b1["host"].tobytes(), b1["ids"], b1["ends"])
        same_as_model(s, model)
        rc, tot = s.put(b2["ptr"], b2["host"].size, b2["ids"], b2["ends"])
        assert rc == 0, last_error(dctx)
        assert tot == {"total": 161, "stored": 7, "stored_bytes": 80029, "present": 124, "repeats": 30}
        assert tot == model.put(b2["host"].tobytes(), b2["ids"], b2["ends"])
        same_as_model(s, model)
        arena = s.arena()
        for b in (b1, b2):  # locate of every ID of both indexes finds the right bytes
            offs, sizes, miss = s.locate(b["ids"])
            assert miss == 0
            starts = np.concatenate([[0], b["ends"][:-1]]).astype(np.int64)
            for i in range(b["n"]):
                lo, size = int(offs[i]), int(sizes[i])
                assert size == int(b["ends"][i]) - int(starts[i])
                assert np.array_equal(arena[lo:lo + size], b["host"][starts[i]:starts[i] + size]), i
        assert s.verify(0) == []


def test_goldens_assemble_blob(dctx, goldens):
    import desync_amd
    b1, b2 = goldens["blob1"], goldens["blob2"]
    with desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as store:
        off = b1["ptr"] - b1["keep"].data_ptr()
        assert store.put_index(b1["keep"][off:off + b1["host"].size], b1["index"])["stored"] == 131
        assert store.put_index((b2["ptr"], b2["host"].size), b2["index"])["stored"] == 7
        assert store.Verify() == []
        # no seed at all (the null seed is one: blob2 holds one run of zeros of a whole chunk)
        out, stats = desync_amd.AssembleBlob(b2["index"], store, null_seed=False, ctx=dctx)
        assert np.array_equal(out.cpu().numpy(), b2["host"])
        assert stats["chunks-from-store"] == 131 and stats["seeds"] == 0
        out, stats = desync_amd.AssembleBlob(b2["index"], store, ctx=dctx)
        assert np.array_equal(out.cpu().numpy(), b2["host"])
        assert stats["chunks-from-store"] == 130 and stats["seeds"] == 1
        seed = desync_amd.NewIndexSeed(b1["index"], (b1["ptr"], b1["host"].size))
        out, stats = desync_amd.AssembleBlob(b2["index"], store, seeds=[seed], null_seed=False, ctx=dctx)
        assert np.array_equal(out.cpu().numpy(), b2["host"])
        assert stats["chunks-from-store"] == 7
        seed.close()


# ---- 2. scan edges ------------------------------------------------------------------
def scan_case(n, seed):
    """A random pool of IDs with duplicates, chunk sizes 0..49 and one of 4,097,
    the first chunk starting at `start` != 0."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (n // 2 + 1, 32), dtype=np.uint8)
    pick = rng.integers(0, len(pool), n)
    sizes = rng.integers(0, 50, n).astype(np.uint64)
    sizes[int(rng.integers(0, n))] = 4097
    start = 7
    ends = (start + np.cumsum(sizes)).astype(np.uint64)
    blob = rng.integers(0, 256, int(ends[-1]) + 5, dtype=np.uint8)
    return pool, pool[pick], ends, start, blob


# 65,537: one more than the second scan level takes in one pass (256 workgroups of 256 chunks)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 65537])
def test_scan_edges(dctx, n):
    pool, ids, ends, start, blob = scan_case(n, 1000 + n)
    half = pool[:len(pool) // 2]
    half_sizes = np.arange(len(half), dtype=np.uint64) % 13
    half_ends = np.cumsum(half_sizes).astype(np.uint64)
    half_blob = np.random.default_rng(5).integers(0, 256, int(half_ends[-1]) + 1 if len(half) else 1,
                                                  dtype=np.uint8)
    half_ptr, _k1 = to_dev(half_blob)
    residues = range(16) if n <= 513 else (0, 11)
    first_arena = None
    for preload in (False, True):
        for r in residues:
            ptr, _k2 = to_dev(blob, r)
            model = store_ref.Store(2 << 20, n + len(half))
            with RawStore(dctx, 2 << 20, n + len(half)) as s:
                if preload and len(half):
                    rc, tot = s.put(half_ptr, half_blob.size, half, half_ends)
                    assert rc == 0 and tot == model.put(half_blob.tobytes(), half, half_ends)
                rc, tot = s.put(ptr, blob.size, ids, ends, start)
                assert rc == 0, last_error(dctx)
                assert tot == model.put(blob.tobytes(), ids, ends, start), (n, r, preload)
                same_as_model(s, model)
                if not preload:
                    # a second, identical run into a fresh store gives identical bytes
                    whole = (s.arena().tobytes(), s.entries()[0].tobytes(), s.entries()[1].tobytes())
                    if first_arena is None:
                        first_arena = whole
                    assert whole == first_arena, (n, r)


# ---- 3. one ID 70,000 times ---------------------------------------------------------
def test_one_id_many_times(dctx):
    n = 70000
    ids = np.tile(np.arange(32, dtype=np.uint8), (n, 1))
    ends = (np.arange(1, n + 1, dtype=np.uint64) * 16)
    blob = np.random.default_rng(3).integers(0, 256, n * 16, dtype=np.uint8)
    ptr, _k = to_dev(blob)
    with RawStore(dctx, 1 << 16, 8) as s:
        rc, tot = s.put(ptr, blob.size, ids, ends)
        assert rc == 0 and tot == {"total": n, "stored": 1, "stored_bytes": 16, "present": 0,
                                   "repeats": n - 1}
        before = s.arena(whole=True)
        assert before[:16].tobytes() == blob[:16].tobytes()
        rc, tot = s.put(ptr, blob.size, ids, ends)
        assert rc == 0 and tot == {"total": n, "stored": 0, "stored_bytes": 0, "present": 1,
                                   "repeats": n - 1}
        assert s.counts()["chunks"] == 1 and s.counts()["bytes"] == 16
        assert np.array_equal(s.arena(whole=True), before)


# ---- 4. crafted IDs -----------------------------------------------------------------
def test_crafted_ids(dctx):
    base = np.arange(100, 132, dtype=np.uint8)
    rows = [base.copy()]
    for w in range(8):          # IDs that differ from the base in one 32-bit word only
        for bit in (0, 13, 31):
            r = base.copy().view(np.uint32)
            r[w] ^= np.uint32(1 << bit)
            rows.append(r.view(np.uint8))
    for k in range(1, 65):      # IDs that share the base's 24 leading bytes
        r = base.copy()
        r[24:] = np.frombuffer(int(k * 0x9E3779B97F4A7C15 & U64_MAX).to_bytes(8, "little"), np.uint8)
        rows.append(r)
    ids = np.stack(rows)
    assert len({r.tobytes() for r in ids}) == len(ids)
    n = len(ids)
    ends = np.cumsum(np.arange(1, n + 1, dtype=np.uint64))
    blob = np.random.default_rng(4).integers(0, 256, int(ends[-1]), dtype=np.uint8)
    ptr, _k = to_dev(blob)
    model = store_ref.Store(1 << 20, n)
    with RawStore(dctx, 1 << 20, n) as s:
        rc, tot = s.put(ptr, blob.size, ids, ends)
        assert rc == 0 and tot["stored"] == n and tot == model.put(blob.tobytes(), ids, ends)
        same_as_model(s, model)
        assert s.locate(ids)[2] == 0


# ---- 5. placements ------------------------------------------------------------------
@pytest.mark.parametrize("ids_dev,ends_dev,misaligned", [
    (False, False, False), (True, False, False), (False, True, False), (True, True, False),
    (True, False, True), (False, True, True), (True, True, True)])
def test_placements(dctx, ids_dev, ends_dev, misaligned):
    _, ids, ends, start, blob = scan_case(300, 77)
    ptr, _k = to_dev(blob, 3)
    L = _L()
    flags = 0
    ia, ea = ids, ends
    keep = []
    if ids_dev:
        ia, k = to_dev(ids, 1 if misaligned else 0, 16)
        keep.append(k)
        flags |= L.DSX_IDS_DEVICE
    if ends_dev:
        ea, k = to_dev(ends, 4 if misaligned else 0, 8)
        keep.append(k)
        flags |= L.DSX_ENDS_DEVICE
    model = store_ref.Store(1 << 20, 512)
    with RawStore(dctx, 1 << 20, 512) as s:
        rc, tot = s.put(ptr, blob.size, ia, ea, start, n=len(ends), flags=flags)
        assert rc == 0, last_error(dctx)
        assert tot == model.put(blob.tobytes(), ids, ends, start)
        same_as_model(s, model)


# ---- 6. capacity ---------------------------------------------------------------------
def test_capacity_is_all_or_nothing(dctx):
    pool, ids, ends, start, blob = scan_case(400, 9)
    ptr, _k = to_dev(blob)
    need = store_ref.Store(1 << 30, 1 << 20).put(blob.tobytes(), ids, ends, start)
    chunks, nbytes = need["stored"], need["stored_bytes"]
    # an exact fit in chunks and in bytes succeeds
    model = store_ref.Store(nbytes, chunks)
    with RawStore(dctx, nbytes, chunks) as s:
        rc, tot = s.put(ptr, blob.size, ids, ends, start)
        assert rc == 0 and tot == need
        model.put(blob.tobytes(), ids, ends, start)
        same_as_model(s, model)
        # a store filled to max_chunks still answers locate for absent IDs
        absent = np.random.default_rng(10).integers(0, 256, (50, 32), dtype=np.uint8)
        offs, sizes, miss = s.locate(absent)
        assert miss == 50 and np.all(offs == U64_MAX) and not sizes.any()
    # one chunk or one byte more: refused, with the would-be totals, and nothing changes
    first_ids = np.random.default_rng(11).integers(0, 256, (3, 32), dtype=np.uint8)
    first_ends = np.array([5, 9, 9], dtype=np.uint64)
    first_blob = np.arange(9, dtype=np.uint8)
    fptr, _k2 = to_dev(first_blob)
    for arena_bytes, max_chunks in ((9 + nbytes - 1, 3 + chunks), (9 + nbytes, 3 + chunks - 1)):
        model = store_ref.Store(arena_bytes, max_chunks)
        with RawStore(dctx, arena_bytes, max_chunks) as s:
            assert s.put(fptr, 9, first_ids, first_ends)[0] == 0
            model.put(first_blob.tobytes(), first_ids, first_ends)
            before = s.arena(whole=True)
            rc, tot = s.put(ptr, blob.size, ids, ends, start)
            assert rc == _L().DSX_E_CAPACITY and tot == need, (rc, tot)
            same_as_model(s, model)
            assert np.array_equal(s.arena(whole=True), before)
            assert s.locate(ids)[2] == len(ids)  # no table slot was taken


# ---- 7. refusals ---------------------------------------------------------------------
def test_refusals(dctx):
    L = _L()
    E = L.DSX_E_INVAL
    _, ids, ends, start, blob = scan_case(100, 21)
    ptr, _k = to_dev(blob)
    d_ids, _k1 = to_dev(ids)
    other = L.Context(0)
    try:
        with RawStore(dctx, 1 << 16, 256) as s, RawStore(other, 1 << 12, 16) as foreign:
            model = store_ref.Store(1 << 16, 256)
            assert s.put(ptr, blob.size, ids[:10], ends[:10], start)[0] == 0
            model.put(blob.tobytes(), ids[:10], ends[:10], start)
            before = s.arena(whole=True)

            def refused(rc):
                assert rc == E, rc
                assert last_error(dctx), "no message"
                same_as_model(s, model)
                assert np.array_equal(s.arena(whole=True), before)

            # an unknown flag bit
            refused(s.put(ptr, blob.size, ids, ends, start, flags=L.DSX_SIZES)[0])
            refused(s.put(ptr, blob.size, ids, ends, start, flags=1 << 20)[0])
            # a store of another context
            tot = L.StorePutTotals()
            refused(L.lib().dsx_store_put(dctx.h, foreign.h, ctypes.c_void_p(ptr), blob.size,
                                          ids.ctypes.data, ends.ctypes.data, start, len(ends),
                                          ctypes.byref(tot), 0))
            miss = ctypes.c_uint64()
            refused(L.lib().dsx_store_locate(dctx.h, foreign.h, ids.ctypes.data, 1, None, None,
                                             ctypes.byref(miss), 0))
            refused(L.lib().dsx_store_destroy(dctx.h, foreign.h))
            # a blob overlapping the arena
            ap, used = s.arena_ptr()
            refused(s.put(ap + 8, 64, ids[:2], np.array([10, 20], dtype=np.uint64))[0])
            refused(s.put(ap - 16, 32, ids[:2], np.array([10, 20], dtype=np.uint64))[0])
            # malformed chunk lists, host ends and device ends
            dec = ends.copy()
            dec[50] = dec[49] - 1
            above = ends.copy()
            beyond = ends.copy()
            beyond[-1] = blob.size + 1
            for bad_ends, st in ((dec, start), (above, int(ends[0]) + 1), (beyond, start)):
                refused(s.put(ptr, blob.size, ids, bad_ends, st)[0])
                d_ends, _k2 = to_dev(bad_ends, 0, 8)
                refused(s.put(ptr, blob.size, d_ids, d_ends, st, n=len(ends),
                              flags=L.DSX_IDS_DEVICE | L.DSX_ENDS_DEVICE)[0])
            # n > 0xFFFFFFF0 (refused before a pointer is read)
            refused(s.put(ptr, blob.size, ids, ends, start, n=0xFFFFFFF1)[0])
            # a resolve segment with first + count > n
            from desync_amd.extract import SEG_DTYPE
            segs = np.zeros(2, dtype=SEG_DTYPE)
            segs[0] = (0, 5, 0, 0, 1, L.DSX_SRC_STORE, 0xFFFFFFFF)
            segs[1] = (5, 5, 0, 99, 2, 0, 0)
            nm, nw, fb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
            keep = segs.copy()
            refused(L.lib().dsx_store_resolve(dctx.h, s.h, ids.ctypes.data, 100, segs.ctypes.data, 2,
                                              ctypes.byref(nm), ctypes.byref(nw), ctypes.byref(fb), 0))
            assert segs.tobytes() == keep.tobytes()
            # the context is still usable
            rc, tot = s.put(ptr, blob.size, ids, ends, start)
            assert rc == 0 and tot == model.put(blob.tobytes(), ids, ends, start)
            same_as_model(s, model)
    finally:
        other.close()


# ---- 8. locate / resolve --------------------------------------------------------------
def test_locate_outputs_host_and_device(dctx):
    L = _L()
    pool, ids, ends, start, blob = scan_case(500, 31)
    ptr, _k = to_dev(blob)
    absent = np.random.default_rng(32).integers(0, 256, (37, 32), dtype=np.uint8)
    ask = np.concatenate([ids[:200], absent, ids[200:]])
    model = store_ref.Store(1 << 20, 512)
    with RawStore(dctx, 1 << 20, 512) as s:
        assert s.put(ptr, blob.size, ids, ends, start)[0] == 0
        model.put(blob.tobytes(), ids, ends, start)
        moffs, msizes, mmiss = model.locate(ask)
        assert mmiss == 37
        offs, sizes, miss = s.locate(ask)
        assert (offs.tolist(), sizes.tolist(), miss) == (moffs, msizes, mmiss)
        assert np.all(offs[200:237] == U64_MAX) and not sizes[200:237].any()
        # device IDs and device outputs, aligned and off their alignment (staged)
        for res in (0, 4):
            d_ask, _k1 = to_dev(ask, res and 8, 16)
            d_offs = _torch().zeros(8 * len(ask) + 16, dtype=_torch().uint8, device="cuda:0")
            d_sizes = _torch().zeros(8 * len(ask) + 16, dtype=_torch().uint8, device="cuda:0")
            _torch().cuda.synchronize()
            m = ctypes.c_uint64()
            rc = L.lib().dsx_store_locate(dctx.h, s.h, ctypes.c_void_p(d_ask), len(ask),
                                          ctypes.c_void_p(d_offs.data_ptr() + res),
                                          ctypes.c_void_p(d_sizes.data_ptr() + res), ctypes.byref(m),
                                          L.DSX_IDS_DEVICE | L.DSX_OUT_DEVICE)
            assert rc == 0 and m.value == 37
            go = d_offs.cpu().numpy()[res:res + 8 * len(ask)].view(np.uint64)
            gs = d_sizes.cpu().numpy()[res:res + 8 * len(ask)].view(np.uint64)
            assert go.tolist() == moffs and gs.tolist() == msizes
        # each output may be NULL
        m = ctypes.c_uint64()
        assert L.lib().dsx_store_locate(dctx.h, s.h, ask.ctypes.data, len(ask), None, None,
                                        ctypes.byref(m), 0) == 0 and m.value == 37
        assert L.lib().dsx_store_locate(dctx.h, s.h, ask.ctypes.data, len(ask), offs.ctypes.data, None,
                                        None, 0) == 0 and offs.tolist() == moffs


def test_resolve_and_assemble_from_the_arena(dctx, goldens):
    import desync_amd
    from desync_amd import extract
    b1, b2 = goldens["blob1"], goldens["blob2"]
    seed = desync_amd.NewIndexSeed(b1["index"], (b1["ptr"], b1["host"].size))
    sq = desync_amd.NewSeedSequencer(b2["index"], seed, null_seed=False, ctx=dctx)
    plan = sq.Plan()
    assert plan.totals["store_unique"] == 7
    starts = np.concatenate([[0], b2["ends"][:-1]]).astype(np.int64)
    packed = b"".join(b2["host"][starts[i]:int(b2["ends"][i])].tobytes() for i in plan.store_chunks.tolist())
    torch = _torch()
    want = torch.zeros(b2["host"].size, dtype=torch.uint8, device="cuda:0")
    got = torch.zeros(b2["host"].size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    extract.assemble(plan, want, packed, ctx=dctx)
    with desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as store:
        # other chunks first, so that arena offsets differ from packed-buffer offsets
        store.put((b1["ptr"], b1["host"].size), b1["ids"], b1["ends"])
        store.put((b2["ptr"], b2["host"].size), b2["ids"], b2["ends"])
        model = store_ref.Store(4 << 20, 1024)
        model.put(b1["host"].tobytes(), b1["ids"], b1["ends"])
        model.put(b2["host"].tobytes(), b2["ids"], b2["ends"])
        segs_before = plan.segs.copy()
        msegs = plan.segs.copy()
        assert store.resolve(b2["ids"], plan.segs) == (0, 0, 0xFFFFFFFF) == model.resolve(b2["ids"], msegs)
        assert plan.segs.tobytes() == msegs.tobytes()
        from_store = segs_before["source"] == extract.SRC_STORE
        for f in segs_before.dtype.names:  # only the store segments' src_off changed
            if f != "src_off":
                assert np.array_equal(plan.segs[f], segs_before[f]), f
        assert np.array_equal(plan.segs["src_off"][~from_store], segs_before["src_off"][~from_store])
        assert not np.array_equal(plan.segs["src_off"][from_store], segs_before["src_off"][from_store])
        extract.assemble(plan, got, store.arena(), ctx=dctx)
        assert torch.equal(got, want)
        assert np.array_equal(got.cpu().numpy(), b2["host"])
        # device IDs give the same answer
        d_ids, _k = to_dev(b2["ids"])
        again = segs_before.copy()
        assert store.resolve(d_ids, again, n=b2["n"]) == (0, 0, 0xFFFFFFFF)
        assert again.tobytes() == plan.segs.tobytes()
    seed.close()


def test_resolve_counts_missing_and_wrong_size(dctx, goldens):
    import desync_amd
    b2 = goldens["blob2"]
    sq = desync_amd.NewSeedSequencer(b2["index"], null_seed=False, ctx=dctx)
    plan = sq.Plan()
    sc = plan.store_chunks.tolist()
    assert len(sc) == 131
    gone, short = sc[40], sc[17]  # (the wrong size sits at the lower position)
    starts = np.concatenate([[0], b2["ends"][:-1]]).astype(np.int64)
    parts, ids = [], []
    for i in sc:
        if i == gone:
            continue
        data = b2["host"][starts[i]:int(b2["ends"][i])].tobytes()
        parts.append(data[:-1] if i == short else data)
        ids.append(b2["ids"][i])
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8)
    ends = np.cumsum([len(p) for p in parts]).astype(np.uint64)
    ptr, _k = to_dev(blob)
    with desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as store:
        assert store.put((ptr, blob.size), np.stack(ids), ends)["stored"] == 130
        model = store_ref.Store(4 << 20, 1024)
        model.put(blob.tobytes(), np.stack(ids), ends)
        before = plan.segs.copy()
        assert store.resolve(b2["ids"], plan.segs) == (1, 1, min(gone, short))
        assert model.resolve(b2["ids"], before.copy()) == (1, 1, min(gone, short))
        assert plan.segs.tobytes() == before.tobytes()
        # 10. AssembleBlob reports the lowest of the two: the size error ...
        with pytest.raises(ValueError, match="unexpected size for chunk " + b2["ids"][short].tobytes().hex()):
            desync_amd.AssembleBlob(b2["index"], store, null_seed=False, ctx=dctx)
    # ... and a store without the chunks ChunkMissing
    with desync_amd.DeviceStore(1 << 16, 16, ctx=dctx) as store:
        with pytest.raises(desync_amd.ChunkMissing) as ei:
            desync_amd.AssembleBlob(b2["index"], store, null_seed=False, ctx=dctx)
        assert ei.value.ID == b2["ids"][sc[0]].tobytes()


# ---- 9. verify -----------------------------------------------------------------------
def test_verify_clean_and_flipped(dctx, goldens):
    import desync_amd
    L = _L()
    b1 = goldens["blob1"]
    sha256 = np.frombuffer(b"".join(desync_amd.chunk_ids(b1["ptr"], b1["host"].size, b1["ends"], 0, ctx=dctx,
                                                         algo=L.DSX_DIGEST_SHA256)),
                           dtype=np.uint8).reshape(-1, 32)
    assert not np.array_equal(sha256, b1["ids"])
    for algo, ids in ((L.DSX_DIGEST_SHA512_256, b1["ids"]), (L.DSX_DIGEST_SHA256, sha256)):
        with RawStore(dctx, 2 << 20, 256) as s:
            rc, tot = s.put(b1["ptr"], b1["host"].size, ids, b1["ends"])
            assert rc == 0 and tot["stored"] == 131
            assert s.verify(algo) == []
            assert len(s.verify(1 - algo)) == 131  # (the other digest made none of these IDs)
            _, ends = s.entries()
            ap, used = s.arena_ptr()
            one = np.empty(1, dtype=np.uint8)
            for k in (0, 65, 130):
                lo, hi = (int(ends[k - 1]) if k else 0), int(ends[k])
                assert hi - lo >= 3
                for at in (lo, (lo + hi) // 2, hi - 1):
                    assert L.lib().dsx_copy(dctx.h, one.ctypes.data, ctypes.c_void_p(ap + at), 1) == 0
                    flipped = one ^ np.uint8(0x40)
                    assert L.lib().dsx_copy(dctx.h, ctypes.c_void_p(ap + at), flipped.ctypes.data, 1) == 0
                    assert s.verify(algo) == [k], (k, at)
                    assert L.lib().dsx_copy(dctx.h, ctypes.c_void_p(ap + at), one.ctypes.data, 1) == 0
            assert s.verify(algo) == []
            # cap below the count: the count is still whole
            bad = np.zeros(4, dtype=np.uint32)
            nb = ctypes.c_uint64()
            assert L.lib().dsx_store_verify(dctx.h, s.h, 1 - algo, bad.ctypes.data, 4, ctypes.byref(nb)) == 0
            assert nb.value == 131 and bad.tolist() == [0, 1, 2, 3]


# ---- 10. the Python layer --------------------------------------------------------------
def test_chop_blob(dctx, goldens):
    import desync_amd
    b1 = goldens["blob1"]
    with desync_amd.DeviceStore(2 << 20, 256, ctx=dctx) as store:
        bad = b1["host"].copy()
        raw = [r.tobytes() for r in b1["ids"]]
        k = next(i for i in range(77, len(raw)) if raw[i] not in raw[:i] and raw[i] not in raw[i + 1:])
        at = int(b1["ends"][k]) - 1
        bad[at] ^= 1
        ptr, _k = to_dev(bad)
        with pytest.raises(desync_amd.ChunkInvalid) as ei:
            desync_amd.ChopBlob(b1["index"], (ptr, bad.size), store)
        assert ei.value.ID == b1["ids"][k].tobytes() and ei.value.Sum != ei.value.ID
        assert store.counts()["chunks"] == 0 and store.counts()["bytes"] == 0
        tot = desync_amd.ChopBlob(b1["index"], (b1["ptr"], b1["host"].size), store)
        assert tot == {"total": 161, "stored": 131, "stored_bytes": 1114112, "present": 0, "repeats": 30}
        assert store.Verify() == []
        # GetChunk: the bytes, or ChunkMissing (a KeyError)
        i = 5
        lo = int(b1["ends"][i - 1])
        assert store.GetChunk(b1["ids"][i].tobytes()) == b1["host"][lo:int(b1["ends"][i])].tobytes()
        assert store.HasChunk(b1["ids"][i].tobytes())
        absent = bytes(range(32))
        assert not store.HasChunk(absent)
        with pytest.raises(desync_amd.ChunkMissing, match="chunk " + absent.hex() + " missing from store"):
            store.GetChunk(absent)
        with pytest.raises(KeyError):
            store.GetChunk(absent)
        # without verify the IDs are trusted; Verify() then names the chunk
        with desync_amd.DeviceStore(2 << 20, 256, ctx=dctx) as loose:
            desync_amd.ChopBlob(b1["index"], (ptr, bad.size), loose, verify=False)
            assert loose.Verify() == [b1["ids"][k].tobytes()]


def test_store_chunk_from_four_threads(dctx):
    import desync_amd
    rng = np.random.default_rng(40)
    datas = [rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes() for _ in range(24)]
    datas[3] = b""
    chunks = [desync_amd.Chunk(desync_amd.digest.Digest.Sum(d), d) for d in datas]
    unique = {c.ID(): c.Data() for c in chunks}
    work = chunks * 3
    with desync_amd.DeviceStore(1 << 16, 64, ctx=dctx) as store:
        cs = desync_amd.ChunkStorage(store)
        errors = []

        def run(part):
            try:
                for c in part:
                    cs.StoreChunk(c)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=run, args=(work[k::4],)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert store.counts()["chunks"] == len(unique)
        assert store.counts()["bytes"] == sum(len(d) for d in unique.values())
        for cid, d in unique.items():
            assert store.GetChunk(cid) == d
        assert store.Verify() == []


# ---- 11. memory ------------------------------------------------------------------------
def test_memory_accounting(dctx):
    L = _L()
    arena_bytes, max_chunks = 3 << 20, 1000
    before = dctx.stats().device_bytes
    s = RawStore(dctx, arena_bytes, max_chunks)
    assert dctx.stats().device_bytes - before >= arena_bytes + 40 * max_chunks
    s.close()
    assert dctx.stats().device_bytes == before
    # a context destroyed with a live store frees it: a second cycle finds the memory again
    torch = _torch()
    big = 1 << 30
    free = []
    for _ in range(2):
        ctx = L.Context(0)
        h = ctypes.c_void_p()
        assert L.lib().dsx_store_create(ctx.h, big, 1000, ctypes.byref(h)) == 0
        assert ctx.stats().device_bytes >= big
        ctx.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    assert free[1] >= free[0] - (big >> 2), free


# ---- 12. end to end in HBM -------------------------------------------------------------
def test_make_chop_extract_in_hbm(dctx):
    """64 MiB of dsx_gen_dedup: cut_device -> chunk_ids (device output) -> put
    -> plan with no seed -> resolve -> assemble, the IDs and the ends staying
    in HBM on the write side; the result equals the blob."""
    import desync_amd
    from desync_amd import extract
    from desync_amd.index import ChunkArray, FormatIndex, Index
    L = _L()
    torch = _torch()
    length = 64 << 20
    mn, av, mx = 16 << 10, 64 << 10, 256 << 10
    blob = torch.empty(length, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L.check(L.lib().dsx_gen_dedup(dctx.h, ctypes.c_void_p(blob.data_ptr()), 0, length, 11, 0.5), dctx.h)
    cap = length // mn + 2
    d_ends = torch.empty(cap, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    n = desync_amd.cut_device(blob.data_ptr(), length, mn, av, mx, ctx=dctx, out_ptr=d_ends.data_ptr(),
                              out_cap=cap)
    d_ids = torch.empty(n * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L.check(L.lib().dsx_chunk_ids(dctx.h, ctypes.c_void_p(blob.data_ptr()), length, 0,
                                  ctypes.c_void_p(d_ends.data_ptr()), n, ctypes.c_void_p(d_ids.data_ptr()),
                                  L.DSX_OUT_DEVICE | L.DSX_ENDS_DEVICE, L.DSX_DIGEST_SHA512_256), dctx.h)
    with desync_amd.DeviceStore(length, n, ctx=dctx) as store:
        tot = store.put(blob, d_ids, d_ends.data_ptr(), n=n)
        first, _, dd = desync_amd.dedup(d_ids, d_ends.data_ptr(), n=n, ctx=dctx)
        assert tot["total"] == n and tot["stored"] == dd["unique"] and tot["present"] == 0
        assert tot["stored_bytes"] == dd["size_not_in_seed"] < length  # (the stream repeats blocks)
        assert tot["repeats"] == n - dd["unique"] > 0
        assert store.Verify() == []
        # the read side works from an index: the IDs and ends cross once, 40 bytes a chunk
        ends = d_ends[:n].cpu().numpy().astype(np.uint64)
        ids = d_ids.cpu().numpy().reshape(-1, 32)
        index = Index(FormatIndex(0, mn, av, mx), ChunkArray(ends, ids.tobytes()))
        plan = desync_amd.NewSeedSequencer(index, null_seed=False, ctx=dctx).Plan()
        assert plan.totals["store_unique"] == tot["stored"]
        assert store.resolve(d_ids, plan.segs, n=n) == (0, 0, 0xFFFFFFFF)
        out = torch.zeros(length, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        extract.assemble(plan, out, store.arena(), ctx=dctx)
        assert torch.equal(out, blob)
        # and through the package's front door
        out2, stats = desync_amd.AssembleBlob(index, store, ctx=dctx)
        assert torch.equal(out2, blob) and stats["chunks-from-store"] == tot["stored"]
