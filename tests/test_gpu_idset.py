"""Chunk-ID sets on the GPU (dsx_idset_*, dsx_dedup, desync_amd.info) against a
Python dict: first positions, seed positions and info.go's counters, for
random pools, one ID repeated many thousand times, IDs crafted to collide
under a partial hash or compare, and IDs that never leave HBM."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = 0xFFFFFFFF


def _torch():
    import torch
    return torch


def to_dev(arr):
    """The array's bytes in HBM (a uint8 tensor; .data_ptr() is the pointer)."""
    torch = _torch()
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")


def dev_u32(n):
    return _torch().empty(max(4 * n, 4), dtype=_torch().uint8, device="cuda:0")


def from_dev(t, n):
    return t.cpu().numpy().view(np.uint32)[:n].copy()


def dict_ref(ids, sizes, start=0, seed_ids=None):
    """first_pos, seed_pos and the five totals, by dict."""
    n = len(ids)
    rows = [r.tobytes() for r in ids]
    seed_first = {}
    if seed_ids is not None:
        for j, r in enumerate(seed_ids):
            seed_first.setdefault(r.tobytes(), j)
    first, own = np.empty(n, np.uint32), {}
    seedp = np.full(n, NONE, np.uint32)
    tot = {"total": n, "unique": 0, "in_seed": 0, "size": 0, "size_not_in_seed": 0}
    for i, r in enumerate(rows):
        first[i] = own.setdefault(r, i)
        seedp[i] = seed_first.get(r, NONE)
        if first[i] == i:
            tot["unique"] += 1
            if seedp[i] != NONE:
                tot["in_seed"] += 1
            else:
                tot["size_not_in_seed"] += int(sizes[i])
    tot["size"] = (start + int(np.sum(sizes, dtype=np.uint64))) if n else 0
    return first, seedp, tot


def raw_dedup(ctx, ids, ends, start, seed, flags, want_seed=True):
    """dsx_dedup through ctypes with host or device arguments per `flags`;
    returns host copies of the outputs and the totals dict."""
    from desync_amd import _lib
    n = ids.shape[0]
    keep = []
    ip, ep = ids.ctypes.data if n else None, ends.ctypes.data if n else None
    if flags & _lib.DSX_IDS_DEVICE and n:
        keep.append(to_dev(ids))
        ip = keep[-1].data_ptr()
    if flags & _lib.DSX_ENDS_DEVICE and n:
        keep.append(to_dev(ends))
        ep = keep[-1].data_ptr()
    if flags & _lib.DSX_OUT_DEVICE:
        df, ds = dev_u32(n), dev_u32(n)
        fp, sp = df.data_ptr(), ds.data_ptr()
    else:
        hf, hs = np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.uint32)
        fp, sp = hf.ctypes.data, hs.ctypes.data
    tot = _lib.DedupTotals()
    rc = _lib.lib().dsx_dedup(ctx.h, ctypes.c_void_p(ip), ctypes.c_void_p(ep), start, n,
                              seed.h if seed is not None else None, ctypes.c_void_p(fp),
                              ctypes.c_void_p(sp if want_seed else None), ctypes.byref(tot), flags)
    assert rc == 0, (rc, _lib.lib().dsx_last_error(ctx.h))
    if flags & _lib.DSX_OUT_DEVICE:
        first, seedp = from_dev(df, n), from_dev(ds, n)
    else:
        first, seedp = hf[:n], hs[:n]
    return first, seedp, {k: getattr(tot, k) for k, _ in _lib.DedupTotals._fields_}


def pool_draw(rng, pool, n):
    return pool[rng.integers(0, len(pool), n)] if n else np.empty((0, 32), np.uint8)


# ---- 1. goldens ---------------------------------------------------------------
def _index(name):
    from desync_amd.index import IndexFromReader
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return IndexFromReader(f)


@pytest.mark.parametrize("k", range(4))
def test_info_on_the_goldens_equals_the_fixture(dctx, k):
    import desync_amd
    with open(os.path.join(GOLDEN, "info_blob1_blob2.json")) as f:
        case = json.load(f)["cases"][k]
    got = desync_amd.Info(_index(case["index"]), seeds=[_index(s) for s in case["seeds"]], ctx=dctx)
    for key, want in case["expect"].items():
        assert got[key] == want, key
    assert got["in-store"] == 0 and got["in-cache"] == 0
    assert got["dedup-size-not-in-seed-nor-cache-compressed"] == 0


@pytest.mark.parametrize("with_seed", [False, True])
def test_info_with_a_cache(dctx, with_seed):
    import desync_amd
    from test_idset_host import dict_info
    b1, b2 = _index("blob1.caibx"), _index("blob2.caibx")
    cache = desync_amd.MemoryStore()
    uniq = list(dict.fromkeys(bytes(c.ID) for c in b2.Chunks))
    for cid in uniq[3:128:5]:  # 25 of blob2's IDs
        cache.chunks[cid] = b""
    assert len(cache.chunks) == 25
    seeds = [b1] if with_seed else []
    got = desync_amd.Info(b2, seeds=seeds, cache=cache, store=cache, ctx=dctx)
    want = dict_info(b2, seeds, cache)
    assert got["in-cache"] == 25 and got["in-store"] == 25
    want["in-store"] = 25
    assert got == want


def test_info_counts_a_hand_built_list_by_its_sizes(dctx):
    """Non-contiguous chunks: Size is summed, as info.go sums chunk.Size."""
    import desync_amd
    from desync_amd.index import FormatIndex, Index, IndexChunk
    a, b = bytes(range(32)), bytes(range(1, 33))
    ix = Index(FormatIndex(0, 1, 2, 3), [IndexChunk(a, 0, 10), IndexChunk(b, 100, 7),
                                          IndexChunk(a, 500, 10), IndexChunk(b, 900, 7)])
    got = desync_amd.Info(ix, ctx=dctx)
    assert (got["total"], got["unique"], got["size"], got["dedup-size-not-in-seed"]) == (4, 2, 907, 17)
    got = desync_amd.Info(ix, seeds=[[b]], ctx=dctx)
    assert (got["in-seed"], got["dedup-size-not-in-seed"], got["not-in-seed-nor-cache"]) == (1, 10, 1)


# ---- 2. random pools, every argument placement ----------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 4097])
def test_random_pools_all_placements(dctx, n):
    import desync_amd
    from desync_amd import _lib
    rng = np.random.default_rng(1000 + n)
    pool = rng.integers(0, 256, (max(1, n // 3) + 8, 32), dtype=np.uint8)
    ids = pool_draw(rng, pool[:max(1, n // 3)], n)
    # the seed: another draw from an overlapping pool, with its own duplicates
    seed_ids = pool_draw(rng, pool[max(1, n // 3) // 2:], n + 5)
    sizes = rng.integers(1, 70000, n).astype(np.uint64)
    start = 12345
    ends = (start + np.cumsum(sizes, dtype=np.uint64)).astype(np.uint64)
    want_f, want_s, want_t = dict_ref(ids, sizes, start, seed_ids)
    with desync_amd.IDSet(seed_ids, ctx=dctx) as seed:
        assert len(seed) == n + 5
        assert seed.unique == len({r.tobytes() for r in seed_ids})
        for place in itertools.product((0, _lib.DSX_IDS_DEVICE), (0, _lib.DSX_ENDS_DEVICE),
                                       (0, _lib.DSX_OUT_DEVICE)):
            for as_sizes in (False, True):
                flags = sum(place) | (_lib.DSX_SIZES if as_sizes else 0)
                f, s, t = raw_dedup(dctx, ids, sizes if as_sizes else ends, start, seed, flags)
                assert np.array_equal(f, want_f), flags
                assert np.array_equal(s, want_s), flags
                assert t == want_t, flags
        # without a seed: nothing is in it
        f, s, t = raw_dedup(dctx, ids, ends, start, None, 0)
        nf, ns, nt = dict_ref(ids, sizes, start, None)
        assert np.array_equal(f, nf) and np.array_equal(s, ns) and t == nt
    # the Python layer, host arrays and device tensors
    with desync_amd.IDSet(to_dev(seed_ids), ctx=dctx) as seed:
        f, s, t = desync_amd.dedup(ids, ends, start=start, seed=seed, ctx=dctx)
        assert np.array_equal(f, want_f) and np.array_equal(s, want_s) and t == want_t
        if n:
            f, s, t = desync_amd.dedup(to_dev(ids), to_dev(sizes), start=start, seed=seed,
                                       sizes=True, ctx=dctx)
            assert np.array_equal(f, want_f) and np.array_equal(s, want_s) and t == want_t


def test_misaligned_device_arguments_are_staged(dctx):
    """Device pointers below the vector loads' alignment still give the answer."""
    from desync_amd import _lib
    rng = np.random.default_rng(5)
    n = 300
    ids = pool_draw(rng, rng.integers(0, 256, (90, 32), dtype=np.uint8), n)
    sizes = rng.integers(1, 9000, n).astype(np.uint64)
    want_f, _, want_t = dict_ref(ids, sizes, 0, None)
    torch = _torch()
    d_ids = torch.empty(n * 32 + 64, dtype=torch.uint8, device="cuda:0")
    d_ids[4:4 + n * 32] = to_dev(ids)
    d_sz = torch.empty(n * 8 + 64, dtype=torch.uint8, device="cuda:0")
    d_sz[4:4 + n * 8] = to_dev(sizes)
    d_out = dev_u32(n + 4)
    tot = _lib.DedupTotals()
    flags = _lib.DSX_IDS_DEVICE | _lib.DSX_ENDS_DEVICE | _lib.DSX_OUT_DEVICE | _lib.DSX_SIZES
    rc = _lib.lib().dsx_dedup(dctx.h, ctypes.c_void_p(d_ids.data_ptr() + 4),
                              ctypes.c_void_p(d_sz.data_ptr() + 4), 0, n, None,
                              ctypes.c_void_p(d_out.data_ptr() + 2), None, ctypes.byref(tot), flags)
    assert rc == 0
    got = d_out.cpu().numpy()[2:2 + 4 * n].copy().view(np.uint32)
    assert np.array_equal(got, want_f)
    assert {k: getattr(tot, k) for k in want_t} == want_t


# ---- 3. one ID many thousand times ------------------------------------------------
def test_all_equal(dctx):
    import desync_amd
    n = 70000  # 274 workgroups, every wave full but the last
    one = np.random.default_rng(3).integers(0, 256, 32, dtype=np.uint8)
    ids = np.tile(one, (n, 1))
    sizes = np.full(n, 4096, np.uint64)
    with desync_amd.IDSet(ids, ctx=dctx) as seed:
        assert (len(seed), seed.unique) == (n, 1)
        f, s, t = desync_amd.dedup(ids, sizes, sizes=True, seed=seed, ctx=dctx)
    assert not f.any() and not s.any()
    assert t == {"total": n, "unique": 1, "in_seed": 1, "size": 4096 * n, "size_not_in_seed": 0}
    f, s, t = desync_amd.dedup(ids, sizes, sizes=True, ctx=dctx)
    assert not f.any() and s is None
    assert t == {"total": n, "unique": 1, "in_seed": 0, "size": 4096 * n, "size_not_in_seed": 4096}


def test_one_id_at_every_odd_position(dctx):
    """Between distinct IDs the predecessor skip cannot help: 35,000 lanes
    meet in one slot, and atomicMin must leave position 1 there."""
    import desync_amd
    n = 70000
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ids[1::2] = ids[1]
    sizes = rng.integers(1, 5000, n).astype(np.uint64)
    want_f, want_s, want_t = dict_ref(ids, sizes, 0, ids)
    assert want_t["unique"] == n // 2 + 1
    with desync_amd.IDSet(ids, ctx=dctx) as seed:
        assert seed.unique == n // 2 + 1
        f, s, t = desync_amd.dedup(ids, sizes, sizes=True, seed=seed, ctx=dctx)
    assert np.array_equal(f, want_f) and (f[1::2] == 1).all()
    assert np.array_equal(s, want_s)
    assert t == want_t


# ---- 4. crafted IDs ---------------------------------------------------------------
def _crafted(kind):
    n = 4096
    rng = np.random.default_rng(11)
    k = np.arange(n, dtype=np.uint64)
    if kind == "same first 8 bytes":
        ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ids[:, :8] = ids[0, :8]
        ids[:, 8:16] = k.view(np.uint8).reshape(n, 8)  # (distinct for certain)
    elif kind == "same first 31 bytes in groups of 256":
        heads = rng.integers(0, 256, (n // 256, 31), dtype=np.uint8)
        ids = np.empty((n, 32), np.uint8)
        ids[:, :31] = np.repeat(heads, 256, axis=0)
        ids[:, 31] = np.arange(n) % 256
    else:  # differ only in bytes 16-23
        ids = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (n, 1))
        ids[:, 16:24] = (k * np.uint64(0x9E3779B97F4A7C15)).view(np.uint8).reshape(n, 8)
    assert len({r.tobytes() for r in ids}) == n
    return ids


@pytest.mark.parametrize("kind", ["same first 8 bytes", "same first 31 bytes in groups of 256",
                                  "differ only in bytes 16-23"])
def test_crafted_ids_are_all_distinct(dctx, kind):
    import desync_amd
    ids = _crafted(kind)
    n = len(ids)
    sizes = np.full(n, 3, np.uint64)
    perm = np.random.default_rng(12).permutation(n)
    with desync_amd.IDSet(ids[perm], ctx=dctx) as seed:
        assert seed.unique == n
        f, s, t = desync_amd.dedup(ids, sizes, sizes=True, seed=seed, ctx=dctx)
    assert np.array_equal(f, np.arange(n, dtype=np.uint32))
    inv = np.empty(n, np.uint32)
    inv[perm] = np.arange(n, dtype=np.uint32)
    assert np.array_equal(s, inv)
    assert t == {"total": n, "unique": n, "in_seed": n, "size": 3 * n, "size_not_in_seed": 0}


# ---- 5. lowest position, reproducible ---------------------------------------------
def test_lowest_seed_position_and_identical_reruns(dctx):
    import desync_amd
    rng = np.random.default_rng(21)
    m = 3000
    base = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    seed_ids = np.concatenate([base, base, base])[rng.permutation(3 * m)]
    ids = base[rng.integers(0, m, 5000)]
    sizes = rng.integers(1, 100, len(ids)).astype(np.uint64)
    want_f, want_s, want_t = dict_ref(ids, sizes, 0, seed_ids)
    runs = []
    for _ in range(2):
        with desync_amd.IDSet(seed_ids, ctx=dctx) as seed:
            assert (len(seed), seed.unique) == (3 * m, m)
            runs.append(desync_amd.dedup(ids, sizes, sizes=True, seed=seed, ctx=dctx))
    (f0, s0, t0), (f1, s1, t1) = runs
    assert np.array_equal(s0, want_s) and np.array_equal(f0, want_f) and t0 == want_t
    assert f0.tobytes() == f1.tobytes() and s0.tobytes() == s1.tobytes() and t0 == t1


# ---- 6. end to end on the device -----------------------------------------------------
def test_cut_hash_dedup_without_leaving_the_device(dctx):
    import desync_amd
    from desync_amd import _lib
    torch = _torch()
    L = _lib.lib()
    rng = np.random.default_rng(7)
    A, B, C, D = (rng.integers(0, 256, 256 << 10, dtype=np.uint8) for _ in range(4))
    blob = np.concatenate([A, B, A, C, B, A, D, A])
    seed_blob = np.concatenate([B, D, D, A])

    def cut_and_hash(data):
        d = to_dev(data)
        cap = data.size // 2048 + 2
        d_ends = torch.empty(cap * 8, dtype=torch.uint8, device="cuda:0")
        n = desync_amd.cut_device(d.data_ptr(), data.size, 2048, 8192, 32768, ctx=dctx,
                                  out_ptr=d_ends.data_ptr(), out_cap=cap)
        d_ids = torch.empty(n * 32, dtype=torch.uint8, device="cuda:0")
        rc = L.dsx_chunk_ids(dctx.h, ctypes.c_void_p(d.data_ptr()), data.size, 0,
                             ctypes.c_void_p(d_ends.data_ptr()), n,
                             ctypes.c_void_p(d_ids.data_ptr()),
                             _lib.DSX_OUT_DEVICE | _lib.DSX_ENDS_DEVICE, _lib.DSX_DIGEST_SHA512_256)
        assert rc == 0
        return n, d_ends, d_ids

    n, d_ends, d_ids = cut_and_hash(blob)
    sn, _, d_seed_ids = cut_and_hash(seed_blob)
    d_first, d_seedp = dev_u32(n), dev_u32(n)
    with desync_amd.IDSet(d_seed_ids.data_ptr(), ctx=dctx, n=sn) as seed:
        f, s, t = desync_amd.dedup(d_ids.data_ptr(), d_ends.data_ptr(), n=n, seed=seed, ctx=dctx,
                                   out=(d_first.data_ptr(), d_seedp.data_ptr()))
        seed_unique = seed.unique
    assert f is None and s is None
    ids = d_ids.cpu().numpy().reshape(n, 32)
    ends = d_ends.cpu().numpy().view(np.uint64)[:n]
    seed_ids = d_seed_ids.cpu().numpy().reshape(sn, 32)
    sizes = np.diff(ends, prepend=np.uint64(0))
    want_f, want_s, want_t = dict_ref(ids, sizes, 0, seed_ids)
    assert np.array_equal(from_dev(d_first, n), want_f)
    assert np.array_equal(from_dev(d_seedp, n), want_s)
    assert t == want_t and t["size"] == blob.size
    assert t["total"] - t["unique"] >= 100 and t["in_seed"] >= 90
    # the CPU oracle's figures for this input
    assert (t["total"], t["unique"], t["in_seed"]) == (272, 134, 102)
    assert (sn, seed_unique) == (140, 105)


# ---- 7. errors ---------------------------------------------------------------------
def test_errors_leave_the_context_usable(dctx):
    import desync_amd
    from desync_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(31)
    n = 1000
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ends = np.cumsum(rng.integers(1, 100, n)).astype(np.uint64)
    tot = _lib.DedupTotals()
    first = np.empty(n, np.uint32)

    def call(ends_, start=0, seed=None, flags=0, count=n):
        return L.dsx_dedup(dctx.h, ids.ctypes.data, ends_.ctypes.data, start, count,
                           seed, first.ctypes.data, None, ctypes.byref(tot), flags)

    bad = ends.copy()
    bad[500] = bad[499] - 1
    assert call(bad) == _lib.DSX_E_INVAL
    assert b"non-decreasing" in L.dsx_last_error(dctx.h)
    assert call(ends, start=int(ends[0]) + 1) == _lib.DSX_E_INVAL
    assert call(bad, flags=_lib.DSX_SIZES) == 0  # sizes need not be ordered
    for bit in (2, 8, 16, 128, 1 << 31):
        assert call(ends, flags=bit) == _lib.DSX_E_INVAL, bit
    h = ctypes.c_void_p()
    for bit in (1, 4, 64, 128):
        assert L.dsx_idset_create(dctx.h, ids.ctypes.data, n, bit, ctypes.byref(h)) == _lib.DSX_E_INVAL
    assert L.dsx_idset_create(dctx.h, ids.ctypes.data, 0xFFFFFFF1, 0, ctypes.byref(h)) == _lib.DSX_E_INVAL
    assert call(ends, count=0xFFFFFFF1) == _lib.DSX_E_INVAL

    other = _lib.Context(0)
    try:
        before = other.stats().device_bytes
        foreign = desync_amd.IDSet(ids, ctx=other)
        with_set = other.stats().device_bytes
        assert with_set - before >= n * 32 + 2048 * 4  # its IDs and its table
        assert call(ends, seed=foreign.h) == _lib.DSX_E_INVAL
        assert L.dsx_idset_destroy(dctx.h, foreign.h) == _lib.DSX_E_INVAL  # not dctx's set
        # dsx_dedup's scratch lives in the context that runs it, and stays
        f, s, t = desync_amd.dedup(ids, ends, seed=foreign, ctx=other)
        with_scratch = other.stats().device_bytes
        assert with_scratch - with_set >= n * 32 + n * 8 + 2 * n * 4 + 2048 * 4
        assert t["in_seed"] == n == t["unique"]
        foreign.close()
        assert with_scratch - other.stats().device_bytes == n * 32 + 2048 * 4  # the set's bytes
    finally:
        other.close()

    # the session's context still works
    assert call(ends) == 0
    assert np.array_equal(first, np.arange(n, dtype=np.uint32))
    assert (tot.total, tot.unique, tot.in_seed, tot.size) == (n, n, 0, int(ends[-1]))
    # n == 0: zero totals
    tot.total = 99
    assert L.dsx_dedup(dctx.h, None, None, 7, 0, None, None, None, ctypes.byref(tot), 0) == 0
    assert (tot.total, tot.unique, tot.in_seed, tot.size, tot.size_not_in_seed) == (0, 0, 0, 0, 0)
