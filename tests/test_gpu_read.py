"""dsx_read_ranges on the GPU (desync_amd.readseeker: read_ranges, DeviceIndex,
IndexPos, Cat): range r of a read must equal blob[off:off+len], every byte of
the output outside the destination windows must keep its 0xA5, and the totals
must equal the model's (read_ref.py).  The bad inputs are all ones the call is
specified to answer with counts or to refuse: nothing is written then."""
import ctypes
import hashlib
import io

import numpy as np
import pytest

import read_ref

pytestmark = pytest.mark.gpu

BLOB = 2 << 20
NULL_SIZE = 4096
FILL = 0xA5
E_INVAL, E_STATE = -6, -12


def _torch():
    import torch
    return torch


def _sum(data):
    return hashlib.new("sha512_256", data).digest()


def to_dev(arr):
    t = _torch().from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    _torch().cuda.synchronize()  # (torch's stream is not the context's)
    return t


class World:
    """The fixture: a blob, its synthetic cut list and IDs, and what a store of
    its chunks holds (the null chunks left out)."""

    def __init__(self):
        import desync_amd
        rng = np.random.default_rng(20240611)
        sizes = []
        while sum(sizes) < BLOB - 3 * NULL_SIZE - (200 << 10):
            sizes.append(int(rng.integers(60 << 10, (200 << 10) + 1)) if rng.random() < 0.025
                         else int(rng.integers(1, 4001)))
        sizes[5], sizes[6], sizes[40] = 1, 1, 200 << 10
        self.null_at = len(sizes) // 2
        sizes[self.null_at:self.null_at] = [NULL_SIZE] * 3
        # chunks with repeated content: the store has fewer entries than the index has chunks
        self.copies = {20: 10, 21: 11, 90: 80, 250: 240, 251: 249}
        assert 100 < self.null_at < 230 and len(sizes) > 260
        for dst, src in self.copies.items():
            sizes[dst] = sizes[src]
        sizes.append(BLOB - sum(sizes))
        assert 1 <= sizes[-1] <= 200 << 10 and max(sizes) == 200 << 10 and min(sizes) == 1
        self.ends = np.cumsum(sizes, dtype=np.uint64)
        self.n = len(sizes)
        blob = rng.integers(0, 256, BLOB, dtype=np.uint8)
        a = int(self.ends[self.null_at - 1])
        blob[a:a + 3 * NULL_SIZE] = 0
        starts = np.concatenate([[0], self.ends[:-1]]).astype(np.int64)
        for dst, src in self.copies.items():
            blob[starts[dst]:starts[dst] + sizes[dst]] = blob[starts[src]:starts[src] + sizes[src]]
        self.blob, self.sizes, self.starts = blob, sizes, starts
        raw = blob.tobytes()
        self.ids = np.frombuffer(b"".join(_sum(raw[s:s + z]) for s, z in zip(starts.tolist(), sizes)),
                                 dtype=np.uint8).reshape(-1, 32).copy()
        self.null_id = _sum(bytes(NULL_SIZE))
        self.is_null = [bytes(i) == self.null_id for i in self.ids]
        assert [k for k, z in enumerate(self.is_null) if z] == list(range(self.null_at, self.null_at + 3))
        self.stored = {bytes(i): z for i, z, nul in zip(self.ids, sizes, self.is_null) if not nul}
        self.index = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=NULL_SIZE),
                                      desync_amd.index.ChunkArray(self.ends, self.ids))
        self.d_blob = to_dev(blob)

    def store(self, ctx, extra=None):
        """A DeviceStore of the blob's chunks without the null chunks (after `extra`, a
        list of byte strings put first)."""
        import desync_amd
        s = desync_amd.DeviceStore(BLOB + (1 << 20), self.n + 64, ctx=ctx)
        if extra:
            junk = np.frombuffer(b"".join(extra), np.uint8)
            ids = np.frombuffer(b"".join(_sum(e) for e in extra), np.uint8).reshape(-1, 32)
            t = s.put(to_dev(junk), ids, np.cumsum([len(e) for e in extra], dtype=np.uint64))
            assert t["stored"] == len(extra)
        a, b = self.null_at, self.null_at + 3
        t1 = s.put(self.d_blob, self.ids[:a], self.ends[:a], 0)
        t2 = s.put(self.d_blob, self.ids[b:], self.ends[b:], int(self.ends[b - 1]))
        assert t1["stored"] + t2["stored"] == len(self.stored) <= self.n - 3 - len(self.copies)
        return s

    def model(self, ranges, ends=None, stored=None, null_size=NULL_SIZE):
        return read_ref.totals(self.ends if ends is None else ends, self.ids, ranges,
                               self.stored if stored is None else stored, 0, self.null_id, null_size)


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def store(world, dctx):
    s = world.store(dctx)
    yield s
    s.close()


def out_len_of(ranges):
    return max((d + ln for _, ln, d in read_ref.with_dst(ranges)), default=0) + 37


def raw_read(world, store, ranges, ids=None, ends=None, null_size=NULL_SIZE, out_len=None):
    """One dsx_read_ranges call into an output filled with 0xA5 -> (totals, output)."""
    from desync_amd.readseeker import read_ranges_raw
    ranges = read_ref.with_dst(ranges)
    out = _torch().full((out_len_of(ranges) if out_len is None else out_len,), FILL, dtype=_torch().uint8,
                        device="cuda:0")
    _torch().cuda.synchronize()
    tot = read_ranges_raw(store, world.ids if ids is None else ids, world.ends if ends is None else ends,
                          ranges, out, 0, world.null_id, null_size, n=world.n)
    return tot, out.cpu().numpy()


def check_read(world, store, ranges, **kw):
    """A read that must succeed: the bytes, the untouched rest and the totals."""
    ranges = read_ref.with_dst(ranges)
    tot, got = raw_read(world, store, ranges, **kw)
    want = world.model(ranges)
    assert tot == want
    assert tot["missing"] == tot["wrong_size"] == tot["beyond"] == 0
    assert tot["first_bad_range"] == tot["first_bad_chunk"] == read_ref.BAD_NONE
    assert tot["store_bytes"] + tot["null_bytes"] == tot["bytes"]
    assert np.array_equal(got, read_ref.expected(world.blob, ranges, got.size, FILL))
    return tot


def spread(ranges, residues=None, gap=5):
    """(off, len) -> (off, len, dst_off): ascending windows with gaps, the
    window of range k at an address that is residues[k] modulo 16."""
    out, at = [], 3
    for k, (off, ln) in enumerate(ranges):
        at += gap
        if residues is not None:
            at += (residues[k] - at) % 16
        out.append((off, ln, at))
        at += ln
    return out


# ---- the bytes --------------------------------------------------------------------------------
@pytest.mark.parametrize("around", [0, 65536])
def test_alignment(world, store, around):
    """Every pair of off mod 16 and dst_off mod 16 (the output tensor is 16-byte
    aligned); short lengths, and lengths around a tile of the gather."""
    rng = np.random.default_rng(3 + around)
    ranges, residues = [], []
    for a in range(16):
        for d in range(16):
            ln = 1 + (a * 16 + d) % 49 if not around else around - 17 + (a * 16 + d) % 35
            off = int(rng.integers(0, (BLOB - ln - 16) // 16)) * 16 + a
            ranges.append((off, ln))
            residues.append(d)
    assert {(o % 16, r) for (o, _), r in zip(ranges, residues)} == {(a, d) for a in range(16) for d in range(16)}
    rg = spread(ranges, residues)
    assert all(dst % 16 == r for (_, _, dst), r in zip(rg, residues))
    check_read(world, store, rg)


def test_edges(world, store):
    edges = read_ref.edge_ranges(world.ends)
    tot = check_read(world, store, spread(edges))
    assert tot["ranges"] == len(edges)
    check_read(world, store, edges)  # packed


def test_whole_blob(world, store, dctx):
    import desync_amd
    tot = check_read(world, store, [(0, BLOB)])
    assert tot["pieces"] == world.n and tot["null_bytes"] == 3 * NULL_SIZE
    got, tot2 = desync_amd.read_ranges(world.index, store, [(0, BLOB)])
    assert tot2 == tot
    whole, _stats = desync_amd.AssembleBlob(world.index, store, ctx=dctx)
    assert _torch().equal(got, whole) and np.array_equal(got.cpu().numpy(), world.blob)


@pytest.mark.parametrize("nranges", [1, 63, 64, 65, 255, 256, 257, 513, 4096, 65537])
def test_many_small(world, store, nranges):
    """Packed ranges at random offsets.  The counts are the store tests' scan
    edges: a wave, a workgroup of the count (256 ranges), and at 65,537 ranges
    257 workgroups, so the array scan over their sums takes a second pass with a
    carry.  Lengths of 0 to 300 bytes: a range of length 0 takes no table slot."""
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 513, 4096) if nranges == 4096 else rng.integers(0, 301, nranges)
    offs = [int(rng.integers(0, BLOB - ln + 1)) for ln in lens]
    tot = check_read(world, store, list(zip(offs, lens.tolist())))
    assert tot["ranges"] == nranges
    if nranges == 4096:
        assert tot["pieces"] > 4096
    if nranges == 65537:  # (not one slot a range throughout: some ranges cross a chunk end)
        assert tot["pieces"] > 65537 - int((lens == 0).sum())


def test_null_chunks(world, store):
    a = int(world.ends[world.null_at - 1])
    ranges = [(a, NULL_SIZE), (a + 1, 10), (a + NULL_SIZE - 3, 6), (a - 2, 3 * NULL_SIZE + 4),
              (a + 2 * NULL_SIZE, NULL_SIZE), (a + 3 * NULL_SIZE - 1, 2), (a, 3 * NULL_SIZE)]
    tot = check_read(world, store, spread(ranges))
    assert tot["null_bytes"] == NULL_SIZE + 10 + 6 + 3 * NULL_SIZE + NULL_SIZE + 1 + 3 * NULL_SIZE
    # without a null ID the store is asked, and it does not hold them
    from desync_amd.readseeker import read_ranges_raw
    out = _torch().full((64,), FILL, dtype=_torch().uint8, device="cuda:0")
    _torch().cuda.synchronize()
    t = read_ranges_raw(store, world.ids, world.ends, [(a + 5, 20)], out)
    assert (t["missing"], t["null_bytes"], t["first_bad_chunk"]) == (1, 0, world.null_at)
    assert bool((out == FILL).all())


def test_argument_forms(world, store, dctx):
    import desync_amd
    rng = np.random.default_rng(7)
    ranges = spread([(int(rng.integers(0, BLOB - 70000)), int(rng.integers(0, 70000))) for _ in range(40)])
    want = world.model(ranges)
    d_ids, d_ends = to_dev(world.ids), to_dev(world.ends)
    skew = to_dev(np.concatenate([np.zeros(8, np.uint8), world.ids.reshape(-1)]))  # IDs at 8 modulo 16
    outs = []
    for ids, ends in ((world.ids, world.ends), (d_ids, d_ends), (d_ids.data_ptr(), d_ends.data_ptr()),
                      (world.ids, d_ends), (d_ids, world.ends), (skew.data_ptr() + 8, d_ends)):
        tot, got = raw_read(world, store, ranges, ids=ids, ends=ends)
        assert tot == want
        outs.append(got)
    assert all(np.array_equal(o, outs[0]) for o in outs)
    assert np.array_equal(outs[0], read_ref.expected(world.blob, ranges, outs[0].size, FILL))
    di = desync_amd.DeviceIndex(world.index, dctx)
    for index in (di, di, world.index):
        out = _torch().full((outs[0].size,), FILL, dtype=_torch().uint8, device="cuda:0")
        _torch().cuda.synchronize()
        got, tot = store.read_ranges(index, ranges, out=out)
        assert got is out and tot == want and np.array_equal(got.cpu().numpy(), outs[0])
    got, tot = desync_amd.read_ranges(di, store, [(r[0], r[1]) for r in ranges])  # packed, a new tensor
    assert got.numel() == want["bytes"]
    assert got.cpu().numpy().tobytes() == b"".join(world.blob[o:o + n].tobytes() for o, n, _ in ranges)


def test_no_ranges_and_empty_ranges(world, store):
    tot, got = raw_read(world, store, [], out_len=16)
    assert tot == world.model([]) and (got == FILL).all()
    tot, got = raw_read(world, store, [(0, 0, 3), (77, 0, 3), (BLOB, 0, 9)], out_len=16)
    assert tot == world.model([(0, 0, 3), (77, 0, 3), (BLOB, 0, 9)]) and tot["pieces"] == 0
    assert (got == FILL).all()


def test_chunks_of_size_zero(world, store):
    """An index with empty chunks between the others: they are no pieces and are not looked up."""
    at = [0, 7, 7, world.null_at + 1, world.n - 1]
    ends = np.insert(world.ends, at, [0 if k == 0 else world.ends[k - 1] for k in at])
    ids = np.insert(world.ids, at, np.frombuffer(_sum(b"no such chunk"), np.uint8), axis=0)
    ranges = spread(read_ref.edge_ranges(ends)[:40] + [(0, BLOB), (100, 50000)])
    from desync_amd.readseeker import read_ranges_raw
    out = _torch().full((out_len_of(ranges),), FILL, dtype=_torch().uint8, device="cuda:0")
    _torch().cuda.synchronize()
    for e in (ends, to_dev(ends)):
        tot = read_ranges_raw(store, ids, e, ranges, out, 0, world.null_id, NULL_SIZE)
        assert tot == read_ref.totals(ends, ids, ranges, world.stored, 0, world.null_id, NULL_SIZE)
        assert tot["missing"] == 0
        assert np.array_equal(out.cpu().numpy(), read_ref.expected(world.blob, ranges, out.numel(), FILL))


def test_table_grows_in_a_fresh_context(world):
    """Device ends: the table's first size is a guess, and a read of more pieces
    than it holds runs the emit twice.  Also: a store of another context."""
    import desync_amd
    from desync_amd import _lib
    from desync_amd.readseeker import read_ranges_raw
    ctx = _lib.Context(0)
    try:
        rng = np.random.default_rng(11)
        sizes = rng.integers(1, 4, 3000)
        ends = np.cumsum(sizes, dtype=np.uint64)
        total = int(ends[-1])
        blob = rng.integers(0, 256, total, dtype=np.uint8)
        # (IDs need not be hashes of the bytes: the store trusts them)
        ids = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
        s = desync_amd.DeviceStore(1 << 16, 4096, ctx=ctx)
        assert s.put(to_dev(blob), ids, ends)["stored"] == 3000
        before = ctx.stats().device_bytes
        d_ends = to_dev(ends)
        for _ in range(2):
            out = _torch().full((total + 9,), FILL, dtype=_torch().uint8, device="cuda:0")
            _torch().cuda.synchronize()
            tot = read_ranges_raw(s, ids, d_ends, [(0, total, 4)], out)
            assert (tot["pieces"], tot["store_bytes"], tot["missing"]) == (3000, total, 0)
            assert np.array_equal(out.cpu().numpy(), read_ref.expected(blob, [(0, total, 4)], total + 9, FILL))
        assert ctx.stats().device_bytes >= before + 3000 * 24  # the scratch is accounted for
        # the session's store does not belong to this context
        tot = _lib.ReadTotals()
        rg = _lib.Range(0, 1, 0)
        other = desync_amd.DeviceStore(1 << 12, 8, ctx=_lib.default_context(0))
        rc = _lib.lib().dsx_read_ranges(ctx.h, other.h, ids.ctypes.data, ends.ctypes.data, 0, 3000, None, 0,
                                        ctypes.byref(rg), 1, ctypes.c_void_p(out.data_ptr()), 8,
                                        ctypes.byref(tot), 0)
        assert rc == E_STATE and b"another context" in _lib.lib().dsx_last_error(ctx.h)
        other.close()
        s.close()
    finally:
        ctx.close()


# ---- all or nothing -------------------------------------------------------------------------------
def thousand(world, avoid, rng):
    """999 ranges that do not touch chunk `avoid`, packed with gaps."""
    lo, hi = int(world.starts[avoid]), int(world.ends[avoid])
    out = []
    while len(out) < 999:
        ln = int(rng.integers(1, 3000))
        off = int(rng.integers(0, BLOB - ln))
        if off + ln <= lo or off >= hi:
            out.append((off, ln))
    return out


def check_refused_by_counts(world, store, ranges, want, **kw):
    tot, got = raw_read(world, store, ranges, **kw)
    assert tot == want, (tot, want)
    assert tot["missing"] + tot["wrong_size"] + tot["beyond"] > 0
    assert (got == FILL).all()  # no byte of the output is written
    return tot


def test_missing_chunk_is_all_or_nothing(world, dctx):
    import desync_amd
    s = world.store(dctx)
    all_ids = [bytes(i) for i in world.ids]
    victim = next(k for k in range(150, world.n) if all_ids.count(all_ids[k]) == 1 and not world.is_null[k])
    cid = all_ids[victim]
    s.RemoveChunk(cid)
    stored = {k: v for k, v in world.stored.items() if k != cid}
    rng = np.random.default_rng(13)
    ranges = thousand(world, victim, rng)
    ranges.insert(617, (int(world.starts[victim]), 1))
    ranges = spread(ranges, gap=1)
    want = world.model(ranges, stored=stored)
    assert (want["missing"], want["first_bad_range"], want["first_bad_chunk"]) == (1, 617, victim)
    check_refused_by_counts(world, s, ranges, want)
    out = _torch().full((out_len_of(ranges),), FILL, dtype=_torch().uint8, device="cuda:0")
    _torch().cuda.synchronize()
    with pytest.raises(desync_amd.ChunkMissing) as e:
        desync_amd.read_ranges(world.index, s, ranges, out=out)
    assert e.value.ID == cid and bool((out == FILL).all())
    # several ranges over it: the counts are per (range, chunk) pair
    ranges = spread([(0, BLOB), (int(world.starts[victim]) - 1, 2), (5, 5)])
    want = world.model(ranges, stored=stored)
    assert (want["missing"], want["first_bad_range"]) == (2, 0)
    check_refused_by_counts(world, s, ranges, want)
    s.close()


def test_wrong_size_is_all_or_nothing(world, store):
    """An index that lies about a size: chunk j is one byte longer, j + 1 one shorter."""
    import desync_amd
    j = next(k for k in range(300, world.n) if world.sizes[k] >= 3 and world.sizes[k + 1] > 1)
    assert not any(world.is_null[j - 1:j + 3])
    ends = world.ends.copy()
    ends[j] += 1
    ranges = thousand(world, j, np.random.default_rng(17))
    ranges = [r for r in ranges if r[0] + r[1] <= int(world.starts[j + 1]) or r[0] >= int(world.ends[j + 1])]
    ranges.insert(411, (int(world.starts[j]) + 2, 1))
    ranges = spread(ranges, gap=1)
    want = world.model(ranges, ends=ends)
    assert (want["wrong_size"], want["missing"], want["first_bad_range"], want["first_bad_chunk"]) == (1, 0, 411, j)
    check_refused_by_counts(world, store, ranges, want, ends=ends)
    check_refused_by_counts(world, store, ranges, want, ends=to_dev(ends))
    lying = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=NULL_SIZE),
                             desync_amd.index.ChunkArray(ends, world.ids))
    out = _torch().full((out_len_of(ranges),), FILL, dtype=_torch().uint8, device="cuda:0")
    _torch().cuda.synchronize()
    with pytest.raises(ValueError, match="unexpected size for chunk " + bytes(world.ids[j]).hex()):
        desync_amd.read_ranges(lying, store, ranges, out=out)
    assert bool((out == FILL).all())
    want = world.model([(0, BLOB)], ends=ends)
    assert (want["wrong_size"], want["first_bad_chunk"]) == (2, j)
    check_refused_by_counts(world, store, [(0, BLOB)], want, ends=ends)


def test_null_id_with_another_size(world, store):
    import desync_amd
    a = world.null_at
    ranges = spread([(5, 100), (int(world.starts[a + 1]) + 7, 9), (int(world.starts[a]), 3 * NULL_SIZE), (9, 9)])
    want = world.model(ranges, null_size=NULL_SIZE - 1)
    assert (want["wrong_size"], want["null_bytes"], want["first_bad_range"], want["first_bad_chunk"]) == (4, 0, 1, a)
    check_refused_by_counts(world, store, ranges, want, null_size=NULL_SIZE - 1)
    # the index's own lie: the first null chunk takes a byte of the second
    ends = world.ends.copy()
    ends[a] += 1
    want = world.model(ranges, ends=ends)
    assert (want["wrong_size"], want["first_bad_chunk"]) == (3, a)
    check_refused_by_counts(world, store, ranges, want, ends=ends)
    lying = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=NULL_SIZE),
                             desync_amd.index.ChunkArray(ends, world.ids))
    with pytest.raises(ValueError, match="unexpected size for chunk " + world.null_id.hex()):
        desync_amd.read_ranges(lying, store, ranges)


def test_beyond_the_blob(world, store):
    import desync_amd
    for bad in ((BLOB - 1, 2), (BLOB, 1), (BLOB + 1, 0), (2 ** 64 - 1, 2)):
        ranges = spread([(0, 100), (5000, 100), bad, (7, 7)])
        want = world.model(ranges)
        assert (want["beyond"], want["first_bad_range"], want["first_bad_chunk"]) == (1, 2, read_ref.BAD_NONE)
        check_refused_by_counts(world, store, ranges, want)
        check_refused_by_counts(world, store, ranges, want, ends=to_dev(world.ends))
    with pytest.raises(ValueError, match="range 2 .* is beyond the blob"):
        desync_amd.read_ranges(world.index, store, [(0, 100), (5000, 100), (BLOB - 1, 2)])


def test_device_ends_that_descend(world, store):
    """Device ends are trusted to ascend.  A list that does not gives counts, not a
    fault, and nothing is written: the chunk whose end lies below its start is a
    wrong_size (DESIGN.md 4.10 has why no kernel leaves its buffers)."""
    j = 123
    ends = world.ends.copy()
    ends[j] = ends[j - 1] - 5
    ranges = spread([(0, BLOB), (int(world.starts[j]) - 100, 300), (17, 4000), (BLOB - 9, 9)])
    tot, got = raw_read(world, store, ranges, ends=to_dev(ends))
    assert tot["ranges"] == 4 and tot["wrong_size"] >= 1 and tot["first_bad_range"] == 0
    assert tot["first_bad_chunk"] <= j
    assert (got == FILL).all()
    # on the host the same list is refused
    from desync_amd._lib import DsxError
    with pytest.raises(DsxError, match="non-decreasing"):
        raw_read(world, store, ranges, ends=ends)


def test_after_compaction(world, dctx):
    """Nothing is cached across calls: after Prune has moved every chunk the same reads are right."""
    rng = np.random.default_rng(19)
    junk = [rng.integers(0, 256, int(z), dtype=np.uint8).tobytes() for z in (70000, 1, 12345)]
    s = world.store(dctx, extra=junk)
    ranges = spread(read_ref.edge_ranges(world.ends)[:30] + [(0, BLOB)] + thousand(world, 0, rng)[:200])
    first = check_read(world, s, ranges)
    t = s.Prune(world.index)
    assert t["removed"] == 3 and t["moved"] == len(world.stored)
    assert check_read(world, s, ranges) == first
    s.close()


# ---- refusals ------------------------------------------------------------------------------------
def test_refusals(world, store, dctx):
    from desync_amd import _lib
    L = _lib.lib()
    out = _torch().full((4096,), FILL, dtype=_torch().uint8, device="cuda:0")
    _torch().cuda.synchronize()
    arena, _used = store.arena()

    def call(ranges, flags=0, ends=None, optr=None, olen=4096, ids=world.ids, totals=True, st=store.h):
        rg = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 3)
        ends = world.ends if ends is None else ends
        tot = _lib.ReadTotals()
        rc = L.dsx_read_ranges(dctx.h, st, ids.ctypes.data if ids is not None else None, ends.ctypes.data, 0,
                               world.n, world.null_id, NULL_SIZE, rg.ctypes.data, len(rg),
                               ctypes.c_void_p(out.data_ptr() if optr is None else optr), olen,
                               ctypes.byref(tot) if totals else None, flags)
        return rc, (L.dsx_last_error(dctx.h) or b"").decode()

    assert call([(0, 10, 0)])[0] == 0
    out.fill_(FILL)
    _torch().cuda.synchronize()
    rc, msg = call([(0, 10, 0)], flags=1)
    assert rc == E_INVAL and "flag" in msg
    assert call([(0, 10, 0)], flags=_lib.DSX_STORE_DEVICE)[0] == E_INVAL
    assert call([(0, 10, 0)], totals=False)[0] == E_INVAL
    assert call([(0, 10, 0)], st=None)[0] == E_INVAL
    assert call([(0, 10, 0)], ids=None)[0] == E_INVAL
    rc, msg = call([(0, 10, 0), (0, 4000, 97)])
    assert rc == E_INVAL and "range 1" in msg and "beyond the output" in msg
    rc, msg = call([(0, 10, 0), (0, 2 ** 64 - 1, 5)])
    assert rc == E_INVAL and "range 1" in msg
    rc, msg = call([(0, 10, 50), (0, 10, 70), (0, 10, 60)])
    assert rc == E_INVAL and "range 2" in msg and "below" in msg
    rc, msg = call([(0, 10, 50), (0, 10, 59)])
    assert rc == E_INVAL and "range 1" in msg and "overlaps" in msg
    assert call([(0, 10, 50), (0, 0, 55), (0, 10, 60)])[0] == E_INVAL  # an empty window inside another
    rc, msg = call([(0, 10, 0)], optr=arena + 100, olen=64)
    assert rc == E_INVAL and "arena" in msg
    down = world.ends.copy()
    down[50] = down[49] - 1
    rc, msg = call([(0, 10, 0)], ends=down)
    assert rc == E_INVAL and "non-decreasing" in msg
    _torch().cuda.synchronize()
    assert bool((out == FILL).all())
    # windows that touch are fine, as are repeated and overlapping sources
    assert call([(0, 10, 0), (5, 10, 10), (5, 10, 20), (0, 0, 30)])[0] == 0
    want = np.concatenate([world.blob[0:10], world.blob[5:15], world.blob[5:15]])
    assert np.array_equal(out[:30].cpu().numpy(), want) and bool((out[30:] == FILL).all())


# ---- the front ends ----------------------------------------------------------------------------------
def test_index_pos_valid_case_on_the_device(dctx):
    """readseeker_test.go's valid case: head, the null chunk (not stored), tail."""
    import desync_amd
    size_max = 256 << 10
    head, tail = b"hello, world", b"goodbye, world"
    null = desync_amd.NewNullChunk(size_max)
    s = desync_amd.DeviceStore(1 << 12, 8, ctx=dctx)
    for data in (head, tail):
        s.StoreChunk(desync_amd.Chunk(_sum(data), data))
    chunks, at = [], 0
    for cid, size in ((_sum(head), len(head)), (null.ID, size_max), (_sum(tail), len(tail))):
        chunks.append(desync_amd.IndexChunk(cid, at, size))
        at += size
    idx = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=size_max), chunks)
    want = head + bytes(size_max) + tail
    r = desync_amd.NewIndexReadSeeker(idx, s)
    assert r.read() == want
    assert r.Seek(len(head) + size_max, io.SEEK_SET) == len(head) + size_max
    assert r.read() == tail and r.Read(4) == b""
    r.Seek(7)
    assert r.Read(10) == want[7:17] and r.tell() == 17
    dev = r.read_device(5)
    assert dev.is_cuda and bytes(dev.cpu().numpy()) == want[17:22] and r.tell() == 22
    assert r.ReadAt(len(want) - 3, 10) == tail[-3:] and r.tell() == 22
    # the size mismatch of the reference's other two cases: an error, no hang
    lying = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=size_max),
                             [desync_amd.IndexChunk(_sum(head), 0, 1000), desync_amd.IndexChunk(_sum(tail), 1000, len(tail))])
    r = desync_amd.NewIndexReadSeeker(lying, s)
    r.Seek(200)
    with pytest.raises(ValueError, match="unexpected size for chunk " + _sum(head).hex()):
        r.Read(16)
    assert r.tell() == 200
    s.RemoveChunk(_sum(tail))
    r = desync_amd.NewIndexReadSeeker(idx, s)
    assert r.Read(20) == want[:20]
    with pytest.raises(desync_amd.ChunkMissing):
        r.read()
    s.close()


def test_cat_and_buffered_reader(world, store):
    import desync_amd
    raw = world.blob.tobytes()
    assert desync_amd.Cat(world.index, store, offset=12345, length=300000) == raw[12345:312345]
    assert desync_amd.Cat(world.index, store, offset=BLOB - 77) == raw[-77:]
    sink = io.BytesIO()
    assert desync_amd.Cat(world.index, store, 0, 0, out=sink) == BLOB and sink.getvalue() == raw
    with pytest.raises(EOFError):
        desync_amd.Cat(world.index, store, offset=BLOB - 5, length=6)
    assert io.BufferedReader(desync_amd.NewIndexReadSeeker(world.index, store)).read() == raw
    buffered = io.BufferedReader(desync_amd.NewIndexReadSeeker(world.index, store), buffer_size=65536)
    buffered.seek(int(world.ends[world.null_at]) - 10)
    assert buffered.read(100000) == raw[int(world.ends[world.null_at]) - 10:][:100000]
