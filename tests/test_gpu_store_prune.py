"""dsx_store_prune on the GPU (desync_amd.store: Prune, RemoveChunk,
Verify(repair)): the compacted arena, the entries and the totals against the
dict-and-bytearray model (store_prune_ref.py) byte for byte; the scan's edges
under every keep pattern and in both modes; self-overlapping moves at every
alignment and across the window edges; the early return; every form of the ID
list; the capacity coming back; every refusal; the Python layer; memory
accounting; and make -> chop -> prune -> extract end to end in HBM."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import store_prune_ref
from test_gpu_store import RawStore, U64_MAX, goldens, last_error, same_as_model, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

WINDOW = 65536
TOTALS = ("entries", "kept", "kept_bytes", "removed", "removed_bytes", "moved", "moved_bytes", "unmatched")


def _torch():
    import torch
    return torch


def _L():
    from desync_amd import _lib
    return _lib


class PruneStore(RawStore):
    def prune(self, ids, remove=False, window=0, n=None, flags=0):
        """ids: a numpy array (host), an integer device pointer or None (NULL).  -> (rc, totals dict)"""
        L = _L()
        tot = L.StorePruneTotals()
        if ids is None or isinstance(ids, int):
            ip = ids
        else:
            ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
            ip = ids.ctypes.data
            if n is None:
                n = len(ids)
        if remove:
            flags |= L.DSX_PRUNE_REMOVE
        rc = L.lib().dsx_store_prune(self.ctx.h, self.h, ctypes.c_void_p(ip), n, window, ctypes.byref(tot),
                                     flags)
        return rc, {k: getattr(tot, k) for k in TOTALS}

    def snapshot(self):
        ids, ends = self.entries()
        return self.arena().tobytes(), ids.tobytes(), ends.tobytes()


def filled(ctx, ids, ends, blob, arena_bytes, max_chunks, start=0):
    """A store and its model holding the chunks of one put."""
    ptr, _k = to_dev(blob)
    s = PruneStore(ctx, arena_bytes, max_chunks)
    rc, tot = s.put(ptr, blob.size, ids, ends, start)
    assert rc == 0 and tot["stored"] == len(ends), (rc, tot, last_error(ctx))
    return s


def model_of(ids, ends, blob, arena_bytes, max_chunks, start=0):
    m = store_prune_ref.Store(arena_bytes, max_chunks)
    m.put(blob.tobytes(), ids, ends, start)
    return m


# ---- 1. goldens ---------------------------------------------------------------------
def test_goldens_pruned_to_blob2(dctx, goldens):
    import desync_amd
    b1, b2 = goldens["blob1"], goldens["blob2"]
    model = store_prune_ref.Store(4 << 20, 1024)
    with desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as store:
        raw = PruneStore.__new__(PruneStore)  # the same store through ctypes
        raw.ctx, raw.h = dctx, store.h
        for b in (b1, b2):
            rc, tot = raw.put(b["ptr"], b["host"].size, b["ids"], b["ends"])
            assert rc == 0 and tot == model.put(b["host"].tobytes(), b["ids"], b["ends"])
        assert raw.counts()["chunks"] == 138
        rc, tot = raw.prune(b2["ids"])
        assert rc == 0, last_error(dctx)
        assert tot == model.prune(b2["ids"])
        assert (tot["kept"], tot["removed"], tot["unmatched"]) == (131, 7, 0)
        same_as_model(raw, model)
        assert raw.verify(0) == []
        out, stats = desync_amd.AssembleBlob(b2["index"], store, null_seed=False, ctx=dctx)
        assert np.array_equal(out.cpu().numpy(), b2["host"])
        assert stats["chunks-from-store"] == 131
        with pytest.raises(desync_amd.ChunkMissing):
            desync_amd.AssembleBlob(b1["index"], store, null_seed=False, ctx=dctx)


# ---- 2. scan edges ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prune_case(n):
    """n distinct IDs with test_gpu_store.scan_case's sizes: 0..49 bytes, one
    chunk of 4,097, empty chunks among them; the model after the put."""
    rng = np.random.default_rng(2000 + n)
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    assert len({r.tobytes() for r in ids}) == n
    sizes = rng.integers(0, 50, n).astype(np.uint64)
    if n > 2:
        sizes[1] = 0
    sizes[int(rng.integers(0, n))] = 4097
    start = 7
    ends = (start + np.cumsum(sizes)).astype(np.uint64)
    blob = rng.integers(0, 256, int(ends[-1]) + 5, dtype=np.uint8)
    return ids, ends, start, blob, model_of(ids, ends, blob, 4 << 20, n, start)


def keep_mask(n, pattern):
    m = np.zeros(n, dtype=bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[-1] = True
    elif pattern == "second":
        m[::2] = True
    elif pattern == "random":
        m = np.random.default_rng(n).random(n) < 0.5
    elif pattern == "prefix":
        m[:3 * n // 4] = True
        m[3 * n // 4::2] = True
    else:
        assert pattern == "none"
    return m


# 65,537: one more than the second scan level takes in one pass (256 workgroups of 256 entries)
@pytest.mark.parametrize("pattern", ["none", "all", "first", "last", "second", "random", "prefix"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 65537])
def test_scan_edges(dctx, n, pattern):
    ids, ends, start, blob, base = prune_case(n)
    mask = keep_mask(n, pattern)
    model = copy.deepcopy(base)
    want = model.prune(ids[mask])
    assert want["kept"] == int(mask.sum())
    with filled(dctx, ids, ends, blob, 4 << 20, n, start) as s:
        rc, tot = s.prune(ids[mask])
        assert rc == 0, last_error(dctx)
        assert tot == want, (n, pattern)
        same_as_model(s, model)
        absent = ids[~mask]
        if len(absent):
            offs, sizes, miss = s.locate(absent)
            assert miss == len(absent) and np.all(offs == U64_MAX) and not sizes.any()
        first = s.snapshot()
    # the remove mode with the complement, and a second run: the same store
    for remove in (True, False):
        with filled(dctx, ids, ends, blob, 4 << 20, n, start) as s:
            rc, tot = s.prune(ids[~mask] if remove else ids[mask], remove=remove)
            assert rc == 0 and tot == want, (n, pattern, remove)
            assert s.counts() == model.counts()
            assert s.snapshot() == first, (n, pattern, remove)


# ---- 3. overlap and window edges ------------------------------------------------------
def window_case(gone, prefix):
    """A kept entry of `prefix` bytes (0: none), a removed one of `gone` bytes,
    then kept entries whose new ends lie on, one byte before and one byte after
    a window edge, one of 200,000 bytes that spans four windows, and empty ones."""
    W = WINDOW
    new_ends = [prefix, W - 1, W, W + 1, W + 1, W + 1 + 200000, 5 * W - 1, 5 * W, 5 * W + 1,
                7 * W, 9 * W, 9 * W + 77777, 14 * W - 3, 15 * W + 9, 16 * W - 77]
    kept = np.diff(np.array([prefix] + new_ends)).tolist()
    assert 200000 in kept and min(kept) == 0
    sizes = np.array(([prefix] if prefix else []) + [gone] + kept, dtype=np.uint64)
    n = len(sizes)
    rng = np.random.default_rng(gone)
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ends = np.cumsum(sizes).astype(np.uint64)
    blob = rng.integers(0, 256, int(ends[-1]), dtype=np.uint8)
    return ids, ends, blob


# gone = 1..16: every later byte shifts left by that much, the self-overlap at every
# alignment residue; 300,000: the shift exceeds a window
@pytest.mark.parametrize("prefix", [0, 12345])
@pytest.mark.parametrize("gone", list(range(1, 17)) + [300000])
def test_overlap_and_window_edges(dctx, gone, prefix):
    ids, ends, blob = window_case(gone, prefix)
    n, cap = len(ends), 2 << 20
    at = 1 if prefix else 0  # the removed entry
    model = model_of(ids, ends, blob, cap, n)
    want = model.prune(ids[at:at + 1], remove=True)
    assert want["moved"] == n - 1 - at and want["moved_bytes"] == int(ends[-1]) - prefix - gone
    shots = []
    for window in (WINDOW, 0):
        with filled(dctx, ids, ends, blob, cap, n) as s:
            rc, tot = s.prune(ids[at:at + 1], remove=True, window=window)
            assert rc == 0, last_error(dctx)
            assert tot == want, (gone, window)
            same_as_model(s, model)
            assert s.arena(whole=True)[:prefix].tobytes() == blob[:prefix].tobytes()
            shots.append(s.snapshot())
    assert shots[0] == shots[1]


def test_removed_entries_between_windows(dctx):
    """Many entries, every third dropped, a window of one tile: every window has
    sources in itself and in later windows, and segments straddle every edge."""
    rng = np.random.default_rng(77)
    n = 700
    sizes = rng.integers(1, 3000, n).astype(np.uint64)
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ends = np.cumsum(sizes).astype(np.uint64)
    blob = rng.integers(0, 256, int(ends[-1]), dtype=np.uint8)
    mask = np.arange(n) % 3 != 1
    model = model_of(ids, ends, blob, 2 << 20, n)
    want = model.prune(ids[mask])
    assert want["kept_bytes"] > 8 * WINDOW
    with filled(dctx, ids, ends, blob, 2 << 20, n) as s:
        rc, tot = s.prune(ids[mask], window=1)  # (rounded up to one tile)
        assert rc == 0 and tot == want
        same_as_model(s, model)


# ---- 4. nothing to do ----------------------------------------------------------------
def test_nothing_removed_writes_nothing(dctx):
    ids, ends, start, blob, base = prune_case(513)
    absent = np.random.default_rng(8).integers(0, 256, (40, 32), dtype=np.uint8)
    with filled(dctx, ids, ends, blob, 1 << 20, 600, start) as s:
        model = model_of(ids, ends, blob, 1 << 20, 600, start)
        before = s.arena(whole=True)
        entries = s.snapshot()
        where = s.locate(ids)
        for arg, remove in ((ids, False), (np.concatenate([ids, absent]), False), (absent, True),
                            (np.empty((0, 32), np.uint8), True)):
            rc, tot = s.prune(arg, remove=remove)
            assert rc == 0, last_error(dctx)
            assert tot == model.prune(arg, remove=remove)
            assert (tot["removed"], tot["moved"], tot["moved_bytes"], tot["kept"]) == (0, 0, 0, 513)
            assert np.array_equal(s.arena(whole=True), before)
            assert s.snapshot() == entries
            got = s.locate(ids)
            assert all(np.array_equal(x, y) for x, y in zip(got[:2], where[:2])) and got[2] == 0
        # NULL ids with n == 0 is the empty list
        assert s.prune(None, remove=True, n=0)[0] == 0 and s.snapshot() == entries
        # an empty store
        with PruneStore(dctx, 1 << 12, 16) as empty:
            rc, tot = empty.prune(absent)
            assert rc == 0 and tot == dict.fromkeys(TOTALS, 0) | {"unmatched": 40}
        # and the empty keep list empties the store
        rc, tot = s.prune(None, n=0)
        assert rc == 0 and tot == model.prune(np.empty((0, 32), np.uint8))
        assert tot["removed"] == 513 and s.counts()["chunks"] == 0 and s.counts()["bytes"] == 0
        assert s.locate(ids)[2] == 513
        ptr, _k = to_dev(blob)
        rc, put = s.put(ptr, blob.size, ids, ends, start)
        assert rc == 0 and put == model.put(blob.tobytes(), ids, ends, start)
        same_as_model(s, model)


# ---- 5. list forms -------------------------------------------------------------------
def test_duplicates_unmatched_and_device_ids(dctx):
    L = _L()
    ids, ends, start, blob, base = prune_case(513)
    rng = np.random.default_rng(9)
    absent = rng.integers(0, 256, (33, 32), dtype=np.uint8)
    pick = rng.integers(0, 513, 300)
    ask = np.concatenate([ids[pick], absent, ids[pick[:50]], absent[:5]])
    want_model = copy.deepcopy(base)
    want = want_model.prune(ask)
    assert want["unmatched"] == 33 and want["kept"] == len(set(pick.tolist()))
    shots = []
    for where in ("host", "device", "device+1"):
        with filled(dctx, ids, ends, blob, 4 << 20, 513, start) as s:
            if where == "host":
                rc, tot = s.prune(ask)
            else:
                ptr, _k = to_dev(ask, 1 if where.endswith("1") else 0, 16)
                rc, tot = s.prune(ptr, n=len(ask), flags=L.DSX_IDS_DEVICE)
            assert rc == 0, last_error(dctx)
            assert tot == want, where
            same_as_model(s, want_model)
            shots.append(s.snapshot())
    assert shots[0] == shots[1] == shots[2]
    # the remove mode counts its unmatched IDs the same way
    model = copy.deepcopy(base)
    with filled(dctx, ids, ends, blob, 4 << 20, 513, start) as s:
        rc, tot = s.prune(ask, remove=True)
        assert rc == 0 and tot == model.prune(ask, remove=True) and tot["unmatched"] == 33
        same_as_model(s, model)


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
    n = len(ids)
    assert len({r.tobytes() for r in ids}) == n
    ends = np.cumsum(np.arange(1, n + 1, dtype=np.uint64))
    blob = np.random.default_rng(4).integers(0, 256, int(ends[-1]), dtype=np.uint8)
    model = model_of(ids, ends, blob, 1 << 20, n)
    with filled(dctx, ids, ends, blob, 1 << 20, n) as s:
        rc, tot = s.prune(ids[::2])
        assert rc == 0 and tot == model.prune(ids[::2]) and tot["kept"] == (n + 1) // 2
        same_as_model(s, model)
        assert s.locate(ids[1::2])[2] == n // 2 and s.locate(ids[::2])[2] == 0


# ---- 6. capacity returns ---------------------------------------------------------------
def test_capacity_returns(dctx):
    L = _L()
    ids, ends, start, blob, _ = prune_case(257)
    used = int(ends[-1]) - start
    rng = np.random.default_rng(12)
    more_ids = rng.integers(0, 256, (100, 32), dtype=np.uint8)
    more_ends = np.cumsum(rng.integers(1, 20, 100)).astype(np.uint64)
    more = rng.integers(0, 256, int(more_ends[-1]), dtype=np.uint8)
    mptr, _k = to_dev(more)
    bptr, _k2 = to_dev(blob)
    model = model_of(ids, ends, blob, used, 257, start)
    with filled(dctx, ids, ends, blob, used, 257, start) as s:  # an exact fit
        assert s.put(mptr, more.size, more_ids, more_ends)[0] == L.DSX_E_CAPACITY
        assert s.put(mptr, more.size, more_ids[:1], more_ends[:1])[0] == L.DSX_E_CAPACITY
        same_as_model(s, model)
        rc, tot = s.prune(ids[::2])
        assert rc == 0 and tot == model.prune(ids[::2])
        rc, put = s.put(mptr, more.size, more_ids, more_ends)
        assert rc == 0, last_error(dctx)
        assert put == model.put(more.tobytes(), more_ids, more_ends) and put["stored"] == 100
        same_as_model(s, model)
        gone = ids[1::2]
        offs, sizes, miss = s.locate(gone)
        assert miss == len(gone) and np.all(offs == U64_MAX)
        # put again, the removed chunks are stored anew at the end
        n_before, bytes_before = s.counts()["chunks"], s.counts()["bytes"]
        few = np.array([1, 3, 5])
        sub_ends = np.cumsum((ends - np.concatenate([[start], ends[:-1]]))[few]).astype(np.uint64)
        sub_blob = np.concatenate([blob[int(ends[i - 1]):int(ends[i])] for i in few])
        sptr, _k3 = to_dev(sub_blob) if sub_blob.size else (bptr, None)
        rc, put = s.put(sptr, sub_blob.size, ids[few], sub_ends)
        assert rc == 0 and put == model.put(sub_blob.tobytes(), ids[few], sub_ends) and put["stored"] == 3
        same_as_model(s, model)
        offs, sizes, miss = s.locate(ids[few])
        assert miss == 0 and int(offs[0]) == bytes_before
        assert s.entries()[0][n_before:].tobytes() == ids[few].tobytes()


# ---- 7. refusals -----------------------------------------------------------------------
def test_refusals(dctx):
    L = _L()
    E = L.DSX_E_INVAL
    ids, ends, start, blob, base = prune_case(255)
    other = L.Context(0)
    try:
        with filled(dctx, ids, ends, blob, 1 << 16, 256, start) as s, PruneStore(other, 1 << 12, 16) as foreign:
            model = copy.deepcopy(base)
            model.arena_bytes, model.max_chunks = 1 << 16, 256
            before = s.arena(whole=True)

            def refused(rc):
                assert rc == E, rc
                assert last_error(dctx), "no message"
                same_as_model(s, model)
                assert np.array_equal(s.arena(whole=True), before)

            for remove in (False, True):
                refused(s.prune(ids[:5], remove=remove, flags=L.DSX_SIZES)[0])
                refused(s.prune(ids[:5], remove=remove, flags=1 << 20)[0])
                refused(s.prune(ids[:5], remove=remove, flags=L.DSX_OUT_DEVICE)[0])
                refused(s.prune(ids[:5], remove=remove, n=0xFFFFFFF1)[0])
                refused(s.prune(None, remove=remove, n=1)[0])
                tot = L.StorePruneTotals()
                refused(L.lib().dsx_store_prune(dctx.h, foreign.h, ids.ctypes.data, 5, 0, ctypes.byref(tot),
                                                L.DSX_PRUNE_REMOVE if remove else 0))
            assert L.lib().dsx_store_prune(dctx.h, None, ids.ctypes.data, 5, 0, None, 0) == E
            assert L.lib().dsx_store_prune(None, s.h, ids.ctypes.data, 5, 0, None, 0) == E
            same_as_model(s, model)
            # the store and the context are still usable; totals may be NULL
            assert L.lib().dsx_store_prune(dctx.h, s.h, ids[:200].ctypes.data, 200, 0, None, 0) == 0
            model.prune(ids[:200])
            same_as_model(s, model)
            rc, tot = s.prune(ids[100:150], remove=True)
            assert rc == 0 and tot == model.prune(ids[100:150], remove=True)
            same_as_model(s, model)
    finally:
        other.close()


# ---- 8. the Python layer -----------------------------------------------------------------
def test_python_prune_forms(dctx, goldens):
    import desync_amd
    b1, b2 = goldens["blob1"], goldens["blob2"]

    def both():
        store = desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx)
        store.put_index((b1["ptr"], b1["host"].size), b1["index"])
        store.put_index((b2["ptr"], b2["host"].size), b2["index"])
        assert len(store) == 138
        return store

    model = store_prune_ref.Store(4 << 20, 1024)
    for b in (b1, b2):
        model.put(b["host"].tobytes(), b["ids"], b["ends"])
    want = copy.deepcopy(model).prune(b2["ids"])
    d_ids = _torch().from_numpy(b2["ids"].copy()).to("cuda:0")
    _torch().cuda.synchronize()
    for arg in (b2["index"], b2["ids"], [r.tobytes() for r in b2["ids"]], d_ids):
        with both() as store:
            assert store.Prune(arg) == want
            assert store.Verify() == []
            out, _ = desync_amd.AssembleBlob(b2["index"], store, null_seed=False, ctx=dctx)
            assert np.array_equal(out.cpu().numpy(), b2["host"])
    with both() as store:  # a list of indexes is merged: nothing goes
        tot = store.Prune([b1["index"], b2["index"]])
        assert (tot["kept"], tot["removed"], tot["moved"], tot["unmatched"]) == (138, 0, 0, 0)
        # RemoveChunk, HasChunk, ChunkMissing
        cid = b1["ids"][5].tobytes()
        data = store.GetChunk(b1["ids"][6].tobytes())
        assert store.HasChunk(cid)
        store.RemoveChunk(cid)
        assert not store.HasChunk(cid) and len(store) == 137
        assert store.GetChunk(b1["ids"][6].tobytes()) == data
        with pytest.raises(desync_amd.ChunkMissing, match="chunk " + cid.hex() + " missing from store"):
            store.RemoveChunk(cid)
        assert len(store) == 137 and store.Verify() == []


def test_python_verify_repair(dctx, goldens):
    import desync_amd
    L = _L()
    b1 = goldens["blob1"]
    with desync_amd.DeviceStore(2 << 20, 256, ctx=dctx) as store:
        store.put_index((b1["ptr"], b1["host"].size), b1["index"])
        ids, ends = store.entries()
        base, used = store.arena()
        one = np.empty(1, dtype=np.uint8)
        hit = (0, 65, 130)
        for k in hit:
            at = (int(ends[k - 1]) if k else 0) + 1
            assert L.lib().dsx_copy(dctx.h, one.ctypes.data, ctypes.c_void_p(base + at), 1) == 0
            one ^= np.uint8(0x40)
            assert L.lib().dsx_copy(dctx.h, ctypes.c_void_p(base + at), one.ctypes.data, 1) == 0
        bad = [ids[k].tobytes() for k in hit]
        # without repair the bad store stays as it is
        assert store.Verify() == bad and store.Verify(repair=False) == bad
        assert len(store) == 131 and store.arena() == (base, used)
        chunks = {ids[e].tobytes(): store.GetChunk(ids[e].tobytes()) for e in range(131) if e not in hit}
        assert store.Verify(repair=True) == bad
        assert len(store) == 128 and store.Verify() == [] and store.Verify(repair=True) == []
        assert store.arena()[0] == base
        for cid in bad:
            assert not store.HasChunk(cid)
        for cid, data in chunks.items():
            assert store.GetChunk(cid) == data


# ---- 9. memory ---------------------------------------------------------------------------
def test_memory_accounting(dctx):
    L = _L()
    torch = _torch()
    ids, ends, start, blob, base = prune_case(513)
    ptr, _k = to_dev(blob)
    free = []
    for _ in range(2):
        ctx = L.Context(0)
        s = PruneStore(ctx, 1 << 20, 513)
        assert s.put(ptr, blob.size, ids, ends, start)[0] == 0
        before = ctx.stats().device_bytes
        rc, tot = s.prune(ids[::2], window=WINDOW + 1)
        assert rc == 0 and tot["moved"] > 0
        grown = ctx.stats().device_bytes - before
        assert 0 < grown <= 2 * WINDOW + 40 * 513, grown
        rc, tot = s.prune(ids[::4], window=WINDOW + 1)
        assert rc == 0 and tot["moved"] > 0
        assert ctx.stats().device_bytes == before + grown
        s.close()
        assert ctx.stats().device_bytes < before + grown
        ctx.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    assert free[1] >= free[0] - (1 << 20), free


# ---- 10. end to end in HBM -----------------------------------------------------------------
def test_make_chop_prune_extract_in_hbm(dctx):
    """Two 64 MiB dsx_gen_dedup blobs through cut -> IDs -> put into one store;
    pruned to the second blob's IDs (in HBM) the store holds exactly the second
    blob's distinct chunks, verifies clean and assembles the second blob."""
    import desync_amd
    from desync_amd.index import ChunkArray, FormatIndex, Index
    L = _L()
    torch = _torch()
    length = 64 << 20
    mn, av, mx = 16 << 10, 64 << 10, 256 << 10
    cap = length // mn + 2
    made = []
    for seed in (11, 12):
        blob = torch.empty(length, dtype=torch.uint8, device="cuda:0")
        d_ends = torch.empty(cap, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        L.check(L.lib().dsx_gen_dedup(dctx.h, ctypes.c_void_p(blob.data_ptr()), 0, length, seed, 0.5), dctx.h)
        n = desync_amd.cut_device(blob.data_ptr(), length, mn, av, mx, ctx=dctx, out_ptr=d_ends.data_ptr(),
                                  out_cap=cap)
        d_ids = torch.empty(n * 32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        L.check(L.lib().dsx_chunk_ids(dctx.h, ctypes.c_void_p(blob.data_ptr()), length, 0,
                                      ctypes.c_void_p(d_ends.data_ptr()), n, ctypes.c_void_p(d_ids.data_ptr()),
                                      L.DSX_OUT_DEVICE | L.DSX_ENDS_DEVICE, L.DSX_DIGEST_SHA512_256), dctx.h)
        made.append((blob, d_ends, d_ids, n))
    with desync_amd.DeviceStore(2 * length, made[0][3] + made[1][3], ctx=dctx) as store:
        for blob, d_ends, d_ids, n in made:
            store.put(blob, d_ids, d_ends.data_ptr(), n=n)
        filled_to = store.counts()
        blob, d_ends, d_ids, n = made[1]
        _, _, dd = desync_amd.dedup(d_ids, d_ends.data_ptr(), n=n, ctx=dctx)
        tot = store.Prune(d_ids)
        assert tot["entries"] == filled_to["chunks"] and tot["unmatched"] == 0
        assert tot["kept"] == dd["unique"] and tot["kept_bytes"] == dd["size_not_in_seed"]
        assert tot["removed"] == filled_to["chunks"] - dd["unique"] > 0 and tot["moved"] > 0
        assert store.counts()["chunks"] == dd["unique"] and store.counts()["bytes"] == dd["size_not_in_seed"]
        assert store.Verify() == []
        ends = d_ends[:n].cpu().numpy().astype(np.uint64)
        ids = d_ids.cpu().numpy().reshape(-1, 32)
        index = Index(FormatIndex(0, mn, av, mx), ChunkArray(ends, ids.tobytes()))
        out, stats = desync_amd.AssembleBlob(index, store, null_seed=False, ctx=dctx)
        assert torch.equal(out, blob) and stats["chunks-from-store"] == dd["unique"]
