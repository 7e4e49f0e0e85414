"""dsx_assemble (the gather kernel), dsx_seed_plan and desync_amd.extract on
the GPU: every (source, destination) alignment with neighbours sharing
granules, tile edges, every refusal, the plan from IDs against the host walk,
and round trips through AssembleBlob."""
import ctypes
import os
import random

import numpy as np
import pytest

import seedplan_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAT = 0xA5     # what the output holds before a call
CANARY = 64


def _torch():
    import torch
    return torch


def _lib():
    from desync_amd import _lib
    return _lib


def to_dev(arr):
    a = np.ascontiguousarray(arr)
    t = _torch().from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    _torch().cuda.synchronize()  # (torch's stream is not the context's)
    return t


def seg_array(rows):
    """rows of (dst_off, bytes, source, src_off) -> dsx_plan_seg_t array."""
    from desync_amd.extract import SEG_DTYPE
    a = np.zeros(len(rows), dtype=SEG_DTYPE)
    for i, (dst, nbytes, source, src) in enumerate(rows):
        a[i] = (dst, nbytes, src, i, 1, source, 0xFFFFFFFF)
    return a


def raw_assemble(ctx, segs, seeds, store, out_ptr, out_len, flags=0):
    """dsx_assemble through ctypes; seeds: device tensors; store: host array or
    device tensor (with DSX_STORE_DEVICE in flags).  -> (rc, message)"""
    L = _lib()
    ns = len(seeds)
    ptrs = (ctypes.c_void_p * max(1, ns))(*[t.data_ptr() for t in seeds])
    lens = (ctypes.c_uint64 * max(1, ns))(*[t.numel() for t in seeds])
    if store is None:
        sp, sl = None, 0
    elif isinstance(store, np.ndarray):
        sp, sl = store.ctypes.data, store.size
    else:
        sp, sl = store.data_ptr(), store.numel()
    segs = np.ascontiguousarray(segs)
    rc = L.lib().dsx_assemble(ctx.h, ctypes.c_void_p(segs.ctypes.data if len(segs) else None), len(segs),
                              ptrs, lens, ns, ctypes.c_void_p(sp), sl, ctypes.c_void_p(out_ptr), out_len,
                              flags)
    msg = L.lib().dsx_last_error(ctx.h)
    return rc, (msg.decode() if msg else "")


def gather(rows, sources, out_len):
    """The expected output: PAT where no segment writes."""
    want = np.full(out_len, PAT, np.uint8)
    for dst, nbytes, source, src in rows:
        want[dst:dst + nbytes] = 0 if source == -1 else sources[source][src:src + nbytes]
    return want


@pytest.fixture(scope="module")
def blobs():
    """Two seed blobs and a store buffer of random bytes, on the host and in HBM."""
    rng = np.random.default_rng(7)
    host = [rng.integers(0, 256, 1 << 20, dtype=np.uint8) for _ in range(3)]
    return host, [to_dev(h) for h in host]


def run_case(ctx, rows, blobs, skew, out_len, flags=0, store_device=False):
    """Assembles `rows` into a dirty output at address skew `skew` between two
    canaries and compares every byte, canaries included, with the numpy gather."""
    host, dev = blobs
    L = _lib()
    buf = _torch().full((CANARY + 16 + out_len + CANARY + 16,), PAT, dtype=_torch().uint8, device="cuda:0")
    base = buf.data_ptr()
    off = CANARY + ((-(base + CANARY)) % 16) + skew  # the output's offset in buf: address = skew mod 16
    assert (base + off) % 16 == skew % 16
    sources = {0: host[0], 1: host[1], -2: host[2]}
    store = dev[2] if store_device else host[2]
    _torch().cuda.synchronize()  # the fill above ran on torch's stream, the library has its own
    if store_device:
        flags |= L.DSX_STORE_DEVICE
    rc, msg = raw_assemble(ctx, seg_array(rows), dev[:2], store, base + off, out_len, flags)
    assert rc == 0, (rc, msg)
    got = buf.cpu().numpy()
    want = np.full(got.size, PAT, np.uint8)
    want[off:off + out_len] = gather(rows, sources, out_len)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (skew, flags, "first wrong byte at output offset", int(bad[0]) - off)


# ---- case 1: alignment sweep ------------------------------------------------------
def sweep_rows():
    """For every length 1..49 and 4097 and every source address residue 0..15
    one segment, packed back to back; the sources alternate between the two
    seeds and the store.  With the output at each of the 16 address skews
    every (src mod 16, dst mod 16) pair occurs for every length."""
    rows, dst = [], 0
    at = [0, 0, 0]
    for k, length in enumerate(list(range(1, 50)) + [4097]):
        for s in range(16):
            which = (k + s) % 3
            source = (0, 1, -2)[which]
            src = at[which] + ((s - at[which]) % 16)  # (the blobs' addresses are multiples of 16)
            rows.append((dst, length, source, src))
            at[which] = src + length
            dst += length
    return rows, dst


@pytest.mark.parametrize("unaligned", (False, True))
def test_alignment_sweep(dctx, blobs, unaligned):
    L = _lib()
    assert all(t.data_ptr() % 16 == 0 for t in blobs[1])
    rows, total = sweep_rows()
    for skew in range(16):
        run_case(dctx, rows, blobs, skew, total, flags=L.DSX_ASSEMBLE_UNALIGNED if unaligned else 0,
                 store_device=bool(skew & 1))


# ---- case 2: tile edges --------------------------------------------------------------
def tile_rows(T, skew):
    """Segments placed against the tile boundaries of the output (tiles are cut
    on addresses: boundary k lies at output offset k T - skew), with gaps."""
    rows = []
    src = [3, 5, 9]

    def put(dst, nbytes, source):
        assert not rows or dst >= rows[-1][0] + rows[-1][1]
        which = {0: 0, 1: 1, -2: 2, -1: None}[source]
        s = 0
        if which is not None:
            s = src[which]
            src[which] += nbytes + 1
        rows.append((dst, nbytes, source, s))
        return dst + nbytes

    b = lambda k: k * T - skew  # noqa: E731
    end = put(b(1), T, 0)                  # exactly one tile, on its boundaries
    end = put(end + 3, T - 1, 1)           # a 3-byte gap, then T - 1
    end = put(end, T + 1, -2)              # back to back, T + 1
    end = put(b(5) - 7, 40, 0)             # the head straddles boundary 5
    end = put(end + 1, b(6) + 1 - (end + 1), 1)  # ends 1 byte into tile 6
    end = put(b(6) + 2, 3 * T + 5, -2)     # several tiles
    end = put(end, 5, -1)                  # zeros over a dirty output, inside one granule
    end = put(end + 9, 2 * T + 11, -1)     # zeros over tiles
    end = put(end, 1, 0)
    return rows, end + 37                  # (an untouched tail behind the last segment)


@pytest.mark.parametrize("store_device", (False, True))
@pytest.mark.parametrize("skew", (0, 3, 15))
@pytest.mark.parametrize("unaligned", (False, True))
def test_tile_edges(dctx, blobs, skew, store_device, unaligned):
    L = _lib()
    T = L.DSX_ASSEMBLE_TILE
    assert T == 65536
    rows, out_len = tile_rows(T, skew)
    run_case(dctx, rows, blobs, skew, out_len, flags=L.DSX_ASSEMBLE_UNALIGNED if unaligned else 0,
             store_device=store_device)


# ---- case 3: every refusal -------------------------------------------------------------
def test_refusals(dctx, blobs):
    L = _lib()
    host, dev = blobs
    out = _torch().full((4096,), PAT, dtype=_torch().uint8, device="cuda:0")
    good = [(0, 100, 0, 7), (100, 50, -2, 3), (160, 40, -1, 0), (200, 10, 1, 0)]
    big = len(host[0])

    def call(rows, seeds=None, store=host[2], out_ptr=None, out_len=4096, flags=0):
        return raw_assemble(dctx, seg_array(rows), dev[:2] if seeds is None else seeds, store,
                            out.data_ptr() if out_ptr is None else out_ptr, out_len, flags)

    def still_works():
        out.fill_(PAT)
        _torch().cuda.synchronize()
        rc, msg = call(good)
        assert rc == 0, msg
        want = gather(good, {0: host[0], 1: host[1], -2: host[2]}, 4096)
        assert np.array_equal(out.cpu().numpy(), want)

    cases = [
        ("overlap", dict(rows=[(0, 100, 0, 0), (99, 10, 0, 0)]), "segment 1: dst_off is below"),
        ("descending", dict(rows=[(500, 10, 0, 0), (100, 10, 0, 0)]), "segment 1: dst_off is below"),
        ("dst beyond", dict(rows=[(0, 10, 0, 0), (4090, 7, 0, 0)]), "segment 1: dst_off + bytes is beyond the output"),
        ("dst far beyond", dict(rows=[(1 << 63, 1 << 63, 0, 0)]), "segment 0: dst_off + bytes is beyond the output"),
        ("src beyond seed", dict(rows=[(0, 10, 0, 0), (10, 10, 1, big - 9)]), "segment 1: src_off + bytes is beyond its source"),
        ("src beyond store", dict(rows=[(0, 10, -2, 95)], store=host[2][:100]), "segment 0: src_off + bytes is beyond its source"),
        ("src wraps", dict(rows=[(0, 10, 0, (1 << 64) - 5)]), "segment 0: src_off + bytes is beyond its source"),
        ("no such seed", dict(rows=[(0, 10, 2, 0)]), "segment 0: source names no seed"),
        ("no seeds at all", dict(rows=[(0, 10, 0, 0)], seeds=[]), "segment 0: source names no seed"),
        ("bad constant", dict(rows=[(0, 10, 0, 0), (10, 10, -3, 0)]), "segment 1: source is neither"),
        ("output in seed", dict(rows=[(0, 10, 1, 0)], out_ptr=dev[0].data_ptr() + 4096, out_len=4096),
         "the output overlaps seed 0"),
        ("output in store", dict(rows=[(0, 10, 1, 0)], store=dev[2], flags=L.DSX_STORE_DEVICE,
                                 out_ptr=dev[2].data_ptr() + big - 1, out_len=1), "the output overlaps the store"),
    ]
    for name, kw, text in cases:
        rc, msg = call(**kw)
        assert rc == L.DSX_E_INVAL, name
        assert text in msg, (name, msg)
        still_works()
    for flags in (L.DSX_OUT_DEVICE, L.DSX_IDS_DEVICE, 1 << 9):
        assert call(good, flags=flags)[0] == L.DSX_E_INVAL
    still_works()
    # nothing to do is not an error
    assert call([])[0] == 0 and call([(5, 0, 0, 0)])[0] == 0


# ---- case 4: dsx_seed_plan against dsx_plan_walk ------------------------------------------
def _index(name):
    from desync_amd.index import IndexFromReader
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return IndexFromReader(f)


def sym_id(s):
    """A 32-byte ID per symbol (bytes: itself)."""
    import hashlib
    return s if isinstance(s, bytes) else hashlib.sha256(b"sym%d" % s).digest()


def raw_seed_plan(ctx, ids, sizes, seeds, null_id, limit, start, flags, seed_sets=None, caps=None):
    """dsx_seed_plan through ctypes, the IDs and ends host or device per flags.
    seeds: [(ids, sizes)] of symbols.  -> (rc, segments, store_chunks, totals)"""
    from desync_amd import IDSet
    L = _lib()
    n = len(ids)
    idarr = np.frombuffer(b"".join(sym_id(s) for s in ids), np.uint8).reshape(-1, 32) if n \
        else np.zeros((0, 32), np.uint8)
    ends = ref.ends_of(sizes, start)
    keep = []
    ip, ep = (idarr.ctypes.data, ends.ctypes.data) if n else (None, None)
    if flags & L.DSX_IDS_DEVICE and n:
        keep.append(to_dev(idarr))
        ip = keep[-1].data_ptr()
    if flags & L.DSX_ENDS_DEVICE and n:
        keep.append(to_dev(ends))
        ep = keep[-1].data_ptr()
    own = seed_sets is None
    if own:
        seed_sets = [IDSet(np.frombuffer(b"".join(sym_id(s) for s in sids), np.uint8).reshape(-1, 32)
                           if len(sids) else np.zeros((0, 32), np.uint8), ctx=ctx) for sids, _ in seeds]
    ns = len(seeds)
    sends = [ref.ends_of(ss) for _, ss in seeds]
    h = (ctypes.c_void_p * max(1, ns))(*[s.h for s in seed_sets])
    e = (ctypes.c_void_p * max(1, ns))(*[a.ctypes.data for a in sends])
    cnt = (ctypes.c_uint64 * max(1, ns))(*[len(a) for a in sends])
    nid = (ctypes.c_uint8 * 32).from_buffer_copy(sym_id(null_id)) if null_id is not None else None
    seg_cap, store_cap = caps if caps is not None else (n, n)
    segs = (L.PlanSeg * max(1, seg_cap))()
    store = np.zeros(max(1, store_cap), np.uint32)
    tot = L.PlanTotals()
    rc = L.lib().dsx_seed_plan(ctx.h, ctypes.c_void_p(ip), ctypes.c_void_p(ep), start, n, h, e, cnt, ns, nid,
                               limit, ctypes.cast(segs, ctypes.c_void_p), seg_cap,
                               ctypes.c_void_p(store.ctypes.data), store_cap, ctypes.byref(tot), flags)
    if own:
        for s in seed_sets:
            s.close()
    td = ref.totals_dict(tot)
    return (rc, [ref.seg_tuple(segs[i]) for i in range(min(td["segments"], seg_cap))],
            store[:min(td["store_unique"], store_cap)].tolist(), td)


PLACEMENTS = (0, 32, 4, 36)  # host/device IDs x host/device ends


@pytest.mark.parametrize("flags", PLACEMENTS)
def test_seed_plan_on_the_goldens(dctx, flags):
    from desync_amd.digest import NewNullChunk
    for target, seed in (("blob2.caibx", "blob1.caibx"), ("blob1.caibx", "blob2.caibx")):
        tix, six = _index(target), _index(seed)
        ids, sizes = [bytes(c.ID) for c in tix.Chunks], [c.Size for c in tix.Chunks]
        sd = ([bytes(c.ID) for c in six.Chunks], [c.Size for c in six.Chunks])
        for limit, null_id in ((0, None), (100, NewNullChunk(32768).ID), (3, NewNullChunk(32768).ID), (3, None)):
            want = ref.walk(ids, sizes, [sd], null_id, limit)
            rc, segs, store, tot = raw_seed_plan(dctx, ids, sizes, [sd], null_id, limit, 0, flags)
            assert rc == 0 and (segs, store, tot) == want, (target, limit, null_id is None)


@pytest.mark.parametrize("flags", PLACEMENTS)
def test_seed_plan_on_random_strings(dctx, flags):
    from test_plan_host import random_case
    rng = random.Random(77 + flags)
    for r in range(24):
        ids, sizes, seeds, null_id, start = random_case(rng)
        limit = (0, 1, 2, 3, 5, 100)[r % 6]
        want = ref.walk(ids, sizes, seeds, null_id, limit, start)
        rc, segs, store, tot = raw_seed_plan(dctx, ids, sizes, seeds, null_id, limit, start, flags)
        assert rc == 0 and (segs, store, tot) == want, (ids, sizes, seeds, null_id, limit, start)


def test_seed_plan_edges(dctx):
    from desync_amd import IDSet
    L = _lib()
    seeds = [([1, 2, 3, 2], [4, 4, 4, 4])]
    # n == 0
    rc, segs, store, tot = raw_seed_plan(dctx, [], [], seeds, 0, 0, 0, 0)
    assert rc == 0 and segs == [] and not any(tot.values())
    # capacity, with the required counts
    rc, segs, store, tot = raw_seed_plan(dctx, [9, 1, 2, 8, 9], [5] * 5, seeds, None, 0, 0, 0, caps=(2, 1))
    assert rc == L.DSX_E_CAPACITY and (tot["segments"], tot["store_unique"]) == (4, 2)
    # device_bytes: the seed keeps its classes once a plan has used it, and gives them back
    before = dctx.stats().device_bytes
    ids = np.frombuffer(b"".join(sym_id(s) for s in range(5000)), np.uint8).reshape(-1, 32)
    s = IDSet(ids, ctx=dctx)
    with_set = dctx.stats().device_bytes
    sd = [(list(range(5000)), [3] * 5000)]
    rc, segs, _, _ = raw_seed_plan(dctx, [7, 8, 9], [3, 3, 3], sd, None, 0, 0, 0, seed_sets=[s])
    assert rc == 0 and segs == [(0, 3, 0, 9, 0, 7, 21)]
    after = dctx.stats().device_bytes
    assert after >= with_set + 4 * 5000
    rc, _, _, _ = raw_seed_plan(dctx, [7, 8, 9], [3, 3, 3], sd, None, 0, 0, 0, seed_sets=[s])
    assert rc == 0 and dctx.stats().device_bytes == after  # built once
    # a wrong number of seed ends
    rc, _, _, _ = raw_seed_plan(dctx, [7], [3], [(list(range(4999)), [3] * 4999)], None, 0, 0, 0, seed_sets=[s])
    assert rc == L.DSX_E_INVAL and b"differs" in L.lib().dsx_last_error(dctx.h)
    s.close()
    assert dctx.stats().device_bytes <= before + (after - with_set)  # (the walk's scratch may have grown)
    # a seed of another context
    other = L.Context(0)
    try:
        s2 = IDSet(ids[:10], ctx=other)
        rc, _, _, _ = raw_seed_plan(dctx, [1], [3], [(list(range(10)), [3] * 10)], None, 0, 0, 0, seed_sets=[s2])
        assert rc == L.DSX_E_INVAL and b"not a set of this context" in L.lib().dsx_last_error(dctx.h)
        s2.close()
    finally:
        other.close()
    assert raw_seed_plan(dctx, [1], [3], seeds, None, 0, 0, L.DSX_OUT_DEVICE)[0] == L.DSX_E_INVAL


# ---- case 5: round trips ---------------------------------------------------------------------
def _blob(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def store_of(index, data, without=()):
    """A MemoryStore with the chunks of `index` (bytes `data`) whose IDs are not in `without`."""
    from desync_amd import Chunk, MemoryStore
    st = MemoryStore()
    skip = {bytes(c.ID) for ix in without for c in ix.Chunks}
    for c in index.Chunks:
        if bytes(c.ID) not in skip:
            st.StoreChunk(Chunk(bytes(c.ID), data[c.Start:c.Start + c.Size]))
    return st


@pytest.mark.parametrize("null_seed", (True, False))
@pytest.mark.parametrize("limit", (0, 3))
@pytest.mark.parametrize("target,seed", (("blob2", "blob1"), ("blob1", "blob2")))
def test_assemble_blob_goldens(dctx, target, seed, limit, null_seed):
    import desync_amd
    tix, six = _index(target + ".caibx"), _index(seed + ".caibx")
    tdata, sdata = _blob(target), _blob(seed)
    store = store_of(tix, tdata, without=[six])
    assert len(store.chunks) == 7
    sd = desync_amd.NewIndexSeed(six, to_dev(np.frombuffer(sdata, np.uint8)))
    out, stats = desync_amd.AssembleBlob(tix, store, [sd], null_seed=null_seed, limit=limit, ctx=dctx)
    assert out.cpu().numpy().tobytes() == tdata
    assert stats == {"chunks-from-seeds": 154, "chunks-from-store": 7, "chunks-in-place": 0,
                     "bytes-copied-from-seeds": 2097152 - 80029, "bytes-cloned-from-seeds": 0, "blocksize": 0,
                     "bytes-total": 2097152, "chunks-total": 161, "seeds": 1 + null_seed}
    sd.close()


def test_assemble_blob_forms_and_empty(dctx):
    import desync_amd
    from desync_amd.index import FormatIndex, Index
    tix, six = _index("blob2.caibx"), _index("blob1.caibx")
    tdata, sdata = _blob("blob2"), _blob("blob1")
    store = store_of(tix, tdata, without=[six])
    dev = to_dev(np.frombuffer(sdata, np.uint8))
    for blob in (sdata, (dev.data_ptr(), dev.numel())):  # host bytes; a pointer with a length
        out, _ = desync_amd.AssembleBlob(tix, store, [desync_amd.NewIndexSeed(six, blob)], ctx=dctx)
        assert out.cpu().numpy().tobytes() == tdata
    # the sequencer's plan equals the host walk's
    sq = desync_amd.NewSeedSequencer(tix, desync_amd.NewIndexSeed(six), null_seed=True, limit=3, ctx=dctx)
    plan = sq.Plan()
    sq.Rewind()
    want = ref.walk([bytes(c.ID) for c in tix.Chunks], [c.Size for c in tix.Chunks],
                    [([bytes(c.ID) for c in six.Chunks], [c.Size for c in six.Chunks])],
                    desync_amd.NewNullChunk(32768).ID, 3)
    assert [tuple(g) for g in plan] == want[0] and plan.store_chunks.tolist() == want[1]
    assert plan.totals == want[2] and len(plan) == 60
    # a missing store chunk, and one of the wrong length
    with pytest.raises(KeyError):
        desync_amd.AssembleBlob(tix, desync_amd.MemoryStore(), [desync_amd.NewIndexSeed(six, dev)], ctx=dctx)
    cid = next(iter(store.chunks))
    short = store_of(tix, tdata, without=[six])
    short.chunks[cid] = short.chunks[cid][:-1]
    with pytest.raises(desync_amd.ChunkInvalid):
        desync_amd.AssembleBlob(tix, short, [desync_amd.NewIndexSeed(six, dev)], ctx=dctx)
    # an empty index: an empty tensor (assemble.go:142-146)
    out, stats = desync_amd.AssembleBlob(Index(FormatIndex(0, 2048, 8192, 32768), []), store, ctx=dctx)
    assert out.numel() == 0 and stats["chunks-total"] == 0 and stats["seeds"] == 1


def test_flipped_seed_byte_is_skipped(dctx):
    import desync_amd
    tix, six = _index("blob2.caibx"), _index("blob1.caibx")
    tdata, sdata = _blob("blob2"), bytearray(_blob("blob1"))
    good = desync_amd.NewSeedSequencer(tix, desync_amd.NewIndexSeed(six, bytes(sdata)), ctx=dctx).Plan()
    g = next(g for g in good if g.source == 0)
    sdata[g.src_off + g.bytes // 2] ^= 0x10  # inside a seed chunk the plan uses
    sd = desync_amd.NewIndexSeed(six, bytes(sdata))
    sq = desync_amd.NewSeedSequencer(tix, sd, ctx=dctx)
    plan = sq.Plan()
    assert [tuple(x) for x in plan] == [tuple(x) for x in good]
    with pytest.raises(desync_amd.SeedInvalid):
        plan.Validate()
    assert sd.IsInvalid()
    again = sq.Plan()
    assert not any(g.source >= 0 for g in again)
    again.Validate()
    full = store_of(tix, tdata)
    out, stats = desync_amd.AssembleBlob(tix, full, [sd], ctx=dctx)
    assert out.cpu().numpy().tobytes() == tdata
    assert stats["chunks-from-store"] == again.totals["store_unique"] == 130  # 131 distinct IDs, one the null chunk's
    # and AssembleBlob finds the bad seed by itself
    sd2 = desync_amd.NewIndexSeed(six, bytes(sdata))
    out, _ = desync_amd.AssembleBlob(tix, full, [sd2], ctx=dctx)
    assert sd2.IsInvalid() and out.cpu().numpy().tobytes() == tdata


def test_round_trip_in_hbm(dctx):
    """A 64 MiB dsx_gen_dedup target whose seeds are two other windows of the
    same stream: cut, hashed, planned and assembled in HBM."""
    import desync_amd
    from desync_amd.index import ChunkArray, FormatIndex, Index
    torch = _torch()
    L = _lib()
    mn, av, mx = 16384, 65536, 262144

    def window(offset, length):
        t = torch.empty(length, dtype=torch.uint8, device="cuda:0")
        L.check(L.lib().dsx_gen_dedup(dctx.h, ctypes.c_void_p(t.data_ptr()), offset, length, 11, 0.5), dctx.h)
        ends = desync_amd.cut_device(t.data_ptr(), length, mn, av, mx, ctx=dctx)
        ids = desync_amd.chunk_ids(t.data_ptr(), length, ends, 0, ctx=dctx)
        return t, Index(FormatIndex(0, mn, av, mx), ChunkArray(ends, b"".join(ids)))

    target, tix = window(64 << 20, 64 << 20)
    s1, ix1 = window((8 << 20) + 12345, 40 << 20)
    s2, ix2 = window((100 << 20) - 777, 48 << 20)
    seeds = [desync_amd.NewIndexSeed(ix1, s1), desync_amd.NewIndexSeed(ix2, s2)]
    host = target.cpu().numpy()
    store = store_of(tix, host.tobytes(), without=[ix1, ix2])
    out, stats = desync_amd.AssembleBlob(tix, store, seeds, ctx=dctx)
    assert torch.equal(out, target)
    assert stats["chunks-total"] == len(tix.Chunks) and stats["bytes-total"] == 64 << 20
    assert stats["chunks-from-seeds"] > len(tix.Chunks) // 4  # the windows do share blocks
    assert 0 < stats["chunks-from-store"] == len(store.chunks)
    for s in seeds:
        s.close()
