"""dsx_chunk_ids_known on the GPU (desync_amd.chunk_ids_known,
DeviceStore.chunk_ids, the known= keywords): whichever path produced an ID,
ids[] must equal hashlib's and known_off[] what dsx_store_locate answers, and
the totals must say which chunks were compared and which hashed (known_ref.py
is the model)."""
import ctypes

import numpy as np
import pytest

import known_ref

pytestmark = pytest.mark.gpu

BLOB = 2 << 20
TILE = 65536
TRIES = 4
E_INVAL, E_STATE = -6, -12
EDGE_SIZES = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]
TILE_SIZES = [TILE - 1, TILE, TILE + 1, 2 * TILE + 17]


def _torch():
    import torch
    return torch


def to_dev(arr):
    t = _torch().from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    _torch().cuda.synchronize()  # (torch's stream is not the context's)
    return t


def ends_of(chunks):
    return np.cumsum([len(c) for c in chunks], dtype=np.uint64)


def new_store(ctx, chunks, arena=None):
    """A DeviceStore filled with `chunks` (byte strings) in that order, and its model."""
    import desync_amd
    raw = b"".join(chunks)
    s = desync_amd.DeviceStore(arena or len(raw) + 4096, len(chunks) + 64, ctx=ctx)
    m = known_ref.StoreModel()
    if chunks:
        ends = ends_of(chunks)
        ids = np.frombuffer(b"".join(known_ref.digest(c) for c in chunks), np.uint8).reshape(-1, 32)
        t = s.put(to_dev(np.frombuffer(raw, np.uint8)), ids, ends)
        m.put(raw, ends)
        assert t["stored"] == len(m.off) and s.counts()["bytes"] == m.used
    return s, m


class World:
    """The fixture: version A as a list of chunks -- mostly 1-4,000 bytes, a few
    of 60-200 KiB, every size around the fingerprint windows and the compare
    tile -- and a store that holds them in another order behind a junk entry of
    odd length, so that a chunk's blob and arena addresses differ by every
    residue modulo 16."""

    def __init__(self, ctx):
        rng = np.random.default_rng(20240923)
        sizes = []
        while sum(sizes) < BLOB - sum(EDGE_SIZES) - sum(TILE_SIZES) - (200 << 10):
            sizes.append(int(rng.integers(60 << 10, (200 << 10) + 1)) if rng.random() < 0.006
                         else int(rng.integers(1, 4001)))
        sizes.append(200 << 10)
        for k, z in enumerate(EDGE_SIZES + TILE_SIZES):  # spread over the list
            sizes.insert(7 + 23 * k, z)
        assert len(sizes) > 23 * 21 and sum(sizes) <= BLOB + (200 << 10)
        self.chunks = [rng.integers(0, 256, z, dtype=np.uint8).tobytes() for z in sizes]
        self.sizes, self.n = sizes, len(sizes)
        self.raw = b"".join(self.chunks)
        self.ends = ends_of(self.chunks)
        self.starts = np.concatenate([[0], self.ends[:-1]]).astype(np.int64)
        self.d_blob = to_dev(np.frombuffer(self.raw, np.uint8))
        order = rng.permutation(self.n)
        junk = rng.integers(0, 256, 13, dtype=np.uint8).tobytes()
        self.store, self.model = new_store(ctx, [junk] + [self.chunks[k] for k in order], BLOB + (1 << 20))
        want_ids, want_off, rec = self.model.answer(self.raw, self.ends)
        assert rec == self.n
        skew = {int((o - s) % 16) for o, s, z in zip(want_off, self.starts, sizes) if z >= 64}
        assert skew == set(range(16))

    def pick(self, lo, hi, taken):
        """The first chunk with lo <= size < hi that no edit has taken."""
        k = next(k for k, z in enumerate(self.sizes) if lo <= z < hi and k not in taken)
        taken.add(k)
        return k


@pytest.fixture(scope="module")
def world(dctx):
    w = World(dctx)
    yield w
    w.store.close()


def check_exact(store, model, d_blob, raw, ends, start=0, **kw):
    """One call; ids and known_off must be the model's and dsx_store_locate's."""
    ids, off, tot = store.chunk_ids(d_blob, ends, start, **kw)
    want_ids, want_off, rec = model.answer(raw, ends, start)
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(off, want_off)
    assert np.array_equal(off, store.locate(ids)[0] if len(ids) else off)
    assert tot["chunks"] == len(ends) == tot["recognised"] + tot["hashed"]
    sizes = np.diff(np.concatenate([[start], ends]).astype(np.int64))
    assert tot["recognised_bytes"] + tot["hashed_bytes"] == int(sizes.sum())
    assert tot["pairs"] >= tot["recognised"] + tot["fp_false"]
    return tot, rec


def test_all_known(world):
    tot, rec = check_exact(world.store, world.model, world.d_blob, world.raw, world.ends)
    assert rec == world.n
    assert tot["hashed"] == 0 and tot["hashed_bytes"] == 0 and tot["untried"] == 0
    assert tot["recognised"] == world.n and tot["recognised_bytes"] == len(world.raw)
    assert tot["compared_bytes"] >= len(world.raw) and tot["pairs"] >= world.n


def test_none_known(world, dctx):
    store, model = new_store(dctx, [], 4096)
    try:
        tot, rec = check_exact(store, model, world.d_blob, world.raw, world.ends)
        assert rec == 0
        assert tot["hashed"] == world.n and tot["hashed_bytes"] == len(world.raw)
        assert tot["compared_bytes"] == 0 and tot["pairs"] == 0 and tot["fp_false"] == 0
    finally:
        store.close()


def test_edited(world):
    """Version B: 7 bytes in front (every chunk moves and is still recognised),
    flips inside the fingerprint windows (no candidate) and outside them (the
    fingerprint passes, the compare must see the flip)."""
    taken, inside, outside = set(), [], []
    c = world.pick(300, 4001, taken); inside.append((c, 0))
    c = world.pick(300, 4001, taken); inside.append((c, world.sizes[c] - 1))
    c = world.pick(300, 4001, taken); inside.append((c, world.sizes[c] // 2))
    c = world.pick(300, 4001, taken); outside.append((c, 40))
    c = world.pick(300, 4001, taken); outside.append((c, 32))                   # the first vector ...
    c = world.pick(300, 4001, taken); outside.append((c, world.sizes[c] - 33))  # ... and the last outside the windows
    c = world.pick(300, 4001, taken); outside.append((c, world.sizes[c] // 2 - 17))
    c = world.pick(300, 4001, taken); outside.append((c, world.sizes[c] // 2 + 16))
    c = world.sizes.index(2 * TILE + 17); taken.add(c); outside.append((c, TILE + 100))
    # the first and the last byte of a compare tile: the pairs' bytes are the chunks with
    # a candidate end to end (the chunks flipped inside a window have none)
    none = {k for k, _ in inside}
    beg = np.concatenate([[0], np.cumsum([0 if k in none else z for k, z in enumerate(world.sizes)])])
    for edge in (0, TILE - 1):
        for t in range(2, int(beg[-1]) // TILE):
            k = int(np.searchsorted(beg, t * TILE + edge, side="right")) - 1
            pos = t * TILE + edge - int(beg[k])
            if k not in taken and not known_ref.in_windows(world.sizes[k], pos):
                break
        else:
            raise AssertionError("no tile edge outside the windows of an unedited chunk")
        taken.add(k)
        outside.append((k, pos))
    b = bytearray(world.raw)
    for k, pos in inside + outside:
        assert known_ref.in_windows(world.sizes[k], pos) == ((k, pos) in inside)
        b[int(world.starts[k]) + pos] ^= 0x5A
    raw = bytes(7) + bytes(b)
    ends = world.ends + np.uint64(7)
    tot, rec = check_exact(world.store, world.model, to_dev(np.frombuffer(raw, np.uint8)), raw, ends, 7)
    assert rec == world.n - len(inside) - len(outside)
    assert tot["hashed"] == len(inside) + len(outside)  # exactly the edited chunks
    assert tot["fp_false"] >= len(outside)
    assert tot["untried"] == 0
    # (no chance candidates: the tile edges above were where the test put them)
    assert tot["pairs"] == world.n - len(inside) and tot["fp_false"] == len(outside)


@pytest.mark.parametrize("size", [4096, 2 * TILE + 17])
def test_collisions(dctx, size):
    """TRIES + 2 entries equal at all three windows that differ at byte 40, and
    a blob with each of them plus a variant the store lacks."""
    rng = np.random.default_rng(size)
    base = bytearray(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
    assert not known_ref.in_windows(size, 40)

    def variant(k):
        v = bytearray(base)
        v[40] = k
        return bytes(v)

    planted = [variant(k) for k in range(TRIES + 2)]
    others = [rng.integers(0, 256, z, dtype=np.uint8).tobytes() for z in (size, 777, size, 5)]
    store, model = new_store(dctx, planted + others[:2])
    try:
        chunks = [others[2]] + planted + [variant(200), others[3], others[0]]
        unknown = 3
        raw, ends = b"".join(chunks), ends_of(chunks)
        tot, rec = check_exact(store, model, to_dev(np.frombuffer(raw, np.uint8)), raw, ends)
        assert rec == len(chunks) - unknown
        assert unknown <= tot["hashed"] <= unknown + len(planted)
        assert tot["fp_false"] >= 1
        assert tot["untried"] >= 1  # the variant the store lacks met more than TRIES candidates
    finally:
        store.close()


@pytest.mark.parametrize("dev_ends", [False, True])
@pytest.mark.parametrize("dev_out", [False, True])
def test_flags_and_start(world, dev_ends, dev_out):
    """The four flag combinations over chunks [k, k + m): start > 0."""
    k, m = 31, 203
    start, ends = int(world.ends[k - 1]), world.ends[k:k + m]
    arg = to_dev(ends).view(_torch().int64) if dev_ends else ends
    ids, off, tot = world.store.chunk_ids(world.d_blob, arg, start, device_out=dev_out)
    if dev_out:
        _torch().cuda.synchronize()
        ids, off = ids.cpu().numpy(), off.cpu().numpy().view(np.uint64)
    want_ids, want_off, rec = world.model.answer(world.raw, ends, start)
    assert np.array_equal(ids, want_ids) and np.array_equal(off, want_off)
    assert tot["recognised"] == rec == m and tot["hashed"] == 0


def test_mixed_through_device_outputs(world, dctx):
    """Hashed and recognised chunks side by side with every output on the
    device, and known_off left out."""
    from desync_amd import _lib
    store, model = new_store(dctx, world.chunks[100:300])
    try:
        n = 400
        ends = world.ends[:n]
        d_ids = _torch().zeros((n, 32), dtype=_torch().uint8, device="cuda:0")
        _torch().cuda.synchronize()
        tot = _lib.KnownTotals()
        rc = _lib.lib().dsx_chunk_ids_known(dctx.h, store.h, ctypes.c_void_p(world.d_blob.data_ptr()),
                                            len(world.raw), 0, ends.ctypes.data, n, 0,
                                            ctypes.c_void_p(d_ids.data_ptr()), None, ctypes.byref(tot),
                                            _lib.DSX_OUT_DEVICE)
        assert rc == 0
        want_ids, _, rec = model.answer(world.raw, ends)
        assert np.array_equal(d_ids.cpu().numpy(), want_ids)
        assert tot.recognised == rec >= 200 and tot.hashed == n - rec > 100
    finally:
        store.close()


def test_no_chunks(world):
    ids, off, tot = world.store.chunk_ids(world.d_blob, np.empty(0, np.uint64))
    assert ids.shape == (0, 32) and off.size == 0
    assert all(v == 0 for v in tot.values())


def test_refusals(world, dctx):
    from desync_amd import _lib
    L = _lib.lib()
    blob = ctypes.c_void_p(world.d_blob.data_ptr())
    length = len(world.raw)
    ids = np.zeros((4, 32), np.uint8)
    good = np.array([10, 20, 20, 30], np.uint64)

    def call(store=world.store.h, ends=good, n=4, start=0, out=ids.ctypes.data, flags=0, algo=0,
             ln=length, ctx=dctx):
        tot = _lib.KnownTotals()
        rc = L.dsx_chunk_ids_known(ctx.h, store, blob, ln, start, ends.ctypes.data, n, algo, out, None,
                                   ctypes.byref(tot), flags)
        return rc, (L.dsx_last_error(ctx.h) or b"").decode()

    assert call()[0] == 0
    rc, why = call(store=None)
    assert rc == E_INVAL and "missing" in why
    rc, why = call(out=None)
    assert rc == E_INVAL and "missing" in why
    for bad in ([10, 9, 20, 30], [10, 20, 30, length + 1]):
        rc, why = call(ends=np.array(bad, np.uint64))
        assert rc == E_INVAL and "chunk ends" in why
    rc, why = call(start=11)
    assert rc == E_INVAL and "chunk ends" in why
    rc, why = call(n=0xFFFFFFF1)
    assert rc == E_INVAL and "0xFFFFFFF0" in why
    for flags in (_lib.DSX_NO_SYNC, _lib.DSX_IDS_DEVICE, 1 << 20):
        rc, why = call(flags=flags)
        assert rc == E_INVAL and "flag" in why
    rc, why = call(algo=7)
    assert rc == E_INVAL and "digest" in why
    other = _lib.Context(0)
    try:
        rc, why = call(ctx=other)
        assert rc == E_STATE and "another context" in why
    finally:
        other.close()
    # nothing above reached the device: the store still answers
    assert call()[0] == 0


PATTERN = 8 << 20


def cdc_versions():
    """The 8 MiB pattern LE64(i * 0x9E3779B97F4A7C15), and the version after a
    4 KiB overwrite at 3 MiB and a 3-byte insertion at 5 MiB."""
    a = (np.arange(PATTERN // 8, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.uint8)
    b = a.copy()
    b[3 << 20:(3 << 20) + 4096] = np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8)
    b = np.concatenate([b[:5 << 20], np.array([1, 2, 3], np.uint8), b[5 << 20:]])
    return a, b


@pytest.mark.parametrize("params,digest", [
    pytest.param((16 << 10, 64 << 10, 256 << 10), "sha512-256", id="params0"),
    pytest.param((2 << 10, 8 << 10, 32 << 10), "sha512-256", id="params1"),
    pytest.param((2 << 10, 8 << 10, 32 << 10), "sha256", id="params1-sha256")])
def test_cdc_end_to_end(dctx, params, digest):
    """Under either package-global digest (set_digest): the keywords pass it
    on to the call."""
    import desync_amd
    before = desync_amd.digest.Digest.Algorithm()
    desync_amd.set_digest(digest)
    try:
        assert desync_amd.digest.Digest.Algorithm() == digest
        _cdc_end_to_end(dctx, params, digest)
    finally:
        desync_amd.set_digest(before)


def _cdc_end_to_end(dctx, params, digest):
    import desync_amd
    from desync_amd.index import encode_to_bytes
    from desync_amd.make import chunk_ids, cut_device
    a, b = cdc_versions()
    d_a, d_b = to_dev(a), to_dev(b)
    plain = desync_amd.DeviceStore(3 * PATTERN, 2 * PATTERN // params[0] + 64, ctx=dctx)
    known = desync_amd.DeviceStore(3 * PATTERN, 2 * PATTERN // params[0] + 64, ctx=dctx)
    try:
        # version A: cut, hashed and put
        ia = desync_amd.ChopBlobs((d_a, [a.size]), plain, *params)
        ib = desync_amd.ChopBlobs((d_a, [a.size]), known, *params, known=True)  # (an empty store: all hashed)
        assert [encode_to_bytes(i) for i in ia] == [encode_to_bytes(i) for i in ib]
        assert plain.counts() == known.counts()
        model = known_ref.StoreModel(digest)
        ends_a = cut_device(d_a.data_ptr(), a.size, *params, ctx=dctx)
        model.put(a.tobytes(), ends_a)
        assert len(model.off) == known.counts()["chunks"]
        # version B against the store of A
        ends_b = cut_device(d_b.data_ptr(), b.size, *params, ctx=dctx)
        ids, off, tot = known.chunk_ids(d_b, ends_b)
        want = np.frombuffer(b"".join(chunk_ids(d_b.data_ptr(), b.size, ends_b, ctx=dctx)),
                             np.uint8).reshape(-1, 32)
        assert np.array_equal(ids, want)
        want_ids, want_off, rec = model.answer(b.tobytes(), ends_b)
        assert np.array_equal(ids, want_ids) and np.array_equal(off, want_off)
        print("chunks", len(ends_b), "hashed", tot["hashed"], "model", len(ends_b) - rec, tot)
        assert tot["hashed"] == len(ends_b) - rec  # the chunks A does not hold, by the model
        assert 0 < tot["hashed"] < len(ends_b) // 10  # (an overwrite and an insertion: a few chunks)
        # the keywords return what the plain calls return
        xa = desync_amd.IndexFromBlobs((d_b, [b.size]), *params, ctx=dctx)
        xb = desync_amd.IndexFromBlobs((d_b, [b.size]), *params, known=known)
        assert [encode_to_bytes(i) for i in xa] == [encode_to_bytes(i) for i in xb]
        ia = desync_amd.ChopBlobs((d_b, [b.size]), plain, *params)
        ib = desync_amd.ChopBlobs((d_b, [b.size]), known, *params, known=True)
        assert [encode_to_bytes(i) for i in ia] == [encode_to_bytes(i) for i in ib]
        assert [encode_to_bytes(i) for i in ib] == [encode_to_bytes(i) for i in xa]
        assert plain.counts() == known.counts()
        assert np.array_equal(plain.entries()[0], known.entries()[0])
        assert desync_amd.ChopBlob(xa[0], d_b, known, known=True) == desync_amd.ChopBlob(xa[0], d_b, plain)
    finally:
        plain.close()
        known.close()
