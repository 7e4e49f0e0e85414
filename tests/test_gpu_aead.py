"""The AEAD store converter on the GPU (dsx_aead_seal / dsx_aead_open,
desync_amd.encrypt, DeviceStore.Seal / PutSealed / WriteLocal / ReadLocal): every
byte against the CPU reference (aead_ref.py, pinned by test_aead_host.py), with
fixed nonces; the 130-bit arithmetic through dsx_selftest_poly1305; tampering;
the refusals; and the round trips through a second store and through a
LocalStore directory."""
import ctypes
import os

import numpy as np
import pytest

import aead_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEST_KEY = bytes.fromhex("6368616e676520746869732070617373776f726420746f206120736563726574")
OTHER_KEY = bytes.fromhex("746f74616c6c7920646966666572656e74206b65792075736564206865726521")


def _torch():
    import torch
    return torch


def _L():
    from desync_amd import _lib
    return _lib


def to_dev(data, residue=0, room=0):
    """The bytes in HBM at an address that is `residue` modulo 16, with `room`
    bytes of 0xAA behind them: -> (pointer, tensor to keep alive)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    t = _torch().full((a.size + room + 32,), 0xAA, dtype=_torch().uint8, device="cuda:0")
    off = (residue - t.data_ptr()) % 16
    if a.size:
        t[off:off + a.size] = _torch().from_numpy(a.copy())
    _torch().cuda.synchronize()  # (torch's stream is not the context's)
    return t.data_ptr() + off, t


def from_dev(ctx, ptr, n):
    out = np.empty(n, dtype=np.uint8)
    if n:
        assert _L().lib().dsx_copy(ctx.h, out.ctypes.data, ctypes.c_void_p(ptr), n) == 0
    return out.tobytes()


def last_error(ctx):
    m = _L().lib().dsx_last_error(ctx.h)
    return m.decode() if m else ""


def raw_seal(ctx, key, src, src_len, ends, start, nonces, out, out_cap, flags=0, n=None, algo=0):
    ends_arr = None
    if not isinstance(ends, int):
        ends_arr = np.ascontiguousarray(ends, dtype=np.uint64)
        n = ends_arr.size if n is None else n
    eptr = ends if isinstance(ends, int) else ends_arr.ctypes.data
    rec_ends = np.zeros(max(1, min(n, 1 << 20)), dtype=np.uint64)
    rc = _L().lib().dsx_aead_seal(ctx.h, algo, key, ctypes.c_void_p(src), src_len, ctypes.c_void_p(eptr),
                                  start, n, nonces, ctypes.c_void_p(out), out_cap, rec_ends.ctypes.data, flags)
    return rc, rec_ends[:n] if n <= rec_ends.size else rec_ends


def raw_open(ctx, key, rec, rec_len, rec_ends, start, out, out_cap, cap=None, flags=0, algo=0):
    rec_ends = np.ascontiguousarray(rec_ends, dtype=np.uint64)
    n = rec_ends.size
    out_ends = np.zeros(max(1, n), dtype=np.uint64)
    cap = n if cap is None else cap
    bad = np.full(max(1, cap), 0xFFFFFFFF, dtype=np.uint32)
    n_bad = ctypes.c_uint64(12345)
    rc = _L().lib().dsx_aead_open(ctx.h, algo, key, ctypes.c_void_p(rec), rec_len, rec_ends.ctypes.data, start,
                                  n, ctypes.c_void_p(out), out_cap, out_ends.ctypes.data, bad.ctypes.data, cap,
                                  ctypes.byref(n_bad), flags)
    return rc, out_ends[:n], bad[:min(cap, n_bad.value)].tolist(), n_bad.value


def seal_and_open_against_the_reference(ctx, sizes, seed, start, residues):
    """Seals chunks of `sizes` lying from byte `start` of a blob, compares the
    records with aead_ref byte for byte, opens them again."""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    total = int(np.sum(sizes))
    blob = rng.integers(0, 256, start + total + 7, dtype=np.uint8).tobytes()
    ends = (start + np.cumsum(sizes)).astype(np.uint64)
    key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    nonces = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    want, want_ends = aead_ref.seal_many(key, nonces, blob, ends, start)
    src, _k1 = to_dev(blob, residues[0])
    out, _k2 = to_dev(b"", residues[1], room=len(want) + 16)
    rc, rec_ends = raw_seal(ctx, key, src, len(blob), ends, start, nonces, out, len(want))
    assert rc == 0, last_error(ctx)
    assert np.array_equal(rec_ends, want_ends)
    got = from_dev(ctx, out, len(want) + 16)
    assert got[len(want):] == b"\xaa" * 16  # nothing behind the last record
    if got[:len(want)] != want:
        g, w = np.frombuffer(got[:len(want)], np.uint8), np.frombuffer(want, np.uint8)
        first = int(np.flatnonzero(g != w)[0])
        rec = int(np.searchsorted(want_ends, first, side="right"))
        raise AssertionError(f"first differing byte {first}: record {rec} of size {sizes[rec]}, "
                             f"at {first - (int(want_ends[rec - 1]) if rec else 0)} in it")
    plain, _k3 = to_dev(b"", residues[2], room=total + 16)
    rc, out_ends, bad, n_bad = raw_open(ctx, key, out, len(want), rec_ends, 0, plain, total)
    assert rc == 0, last_error(ctx)
    assert n_bad == 0 and bad == []
    assert np.array_equal(out_ends, np.cumsum(sizes).astype(np.uint64))
    back = from_dev(ctx, plain, total + 16)
    assert back[:total] == blob[start:start + total] and back[total:] == b"\xaa" * 16
    return key, out, rec_ends, _k2


def test_sizes_in_one_call_at_odd_offsets(dctx):
    """Every size around the cipher block, the MAC block and the tile, and one
    chunk of many tiles, at an odd start in a misaligned blob, into a
    differently misaligned output."""
    T = _L().DSX_AEAD_TILE
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 2 * T + 5, (1 << 20) + 3]
    seal_and_open_against_the_reference(dctx, sizes, 1, start=3, residues=(5, 9, 2))
    st = dctx.stats()
    assert st.device_bytes >= len(sizes) * 160  # the scratch is the context's


def test_tiny_chunks(dctx):
    """5,000 chunks of 1 to 200 bytes: many records per tile, and more than one
    workgroup in the per-record kernels."""
    rng = np.random.default_rng(2)
    sizes = rng.integers(1, 201, 5000).tolist()
    seal_and_open_against_the_reference(dctx, sizes, 3, start=1, residues=(1, 8, 15))


def test_chunks_meeting_tile_edges(dctx):
    """Chunks that end exactly on a tile edge, begin on one, and zero-length
    chunks on it: the (chunk, tile) slots stay distinct."""
    T = _L().DSX_AEAD_TILE
    sizes = [T - 64, 64, 0, 0, T, 10, T - 10, 0, 63, T - 63 + 64, 1]
    seal_and_open_against_the_reference(dctx, sizes, 4, start=0, residues=(0, 0, 0))


def _selftest(ctx, otk, msg):
    ptr, _keep = to_dev(msg, 3)
    tag = (ctypes.c_uint8 * 16)()
    rc = _L().lib().dsx_selftest_poly1305(ctx.h, otk, ctypes.c_void_p(ptr), len(msg), tag)
    assert rc == 0, last_error(ctx)
    return bytes(tag)


def test_selftest_poly1305_edges(dctx):
    """The 130-bit arithmetic where the AEAD cannot steer it: chosen r and s."""
    T = _L().DSX_AEAD_TILE
    one = (1).to_bytes(16, "little")
    rmax = bytes.fromhex("ffffff0ffcffff0ffcffff0ffcffff0f")  # every bit the clamp keeps
    cases = []
    # r = 1, s = 0: each all-0xFF block adds 2^129 - 1, sums around 2^130 - 5
    for blocks in range(1, 7):
        cases.append((one + bytes(16), b"\xff" * (16 * blocks)))
    for extra in (0, 16, 48, 64, 80):
        cases.append((one + bytes(16), b"\xff" * (T + extra)))
    # the largest clamped r, all-0xFF messages; and with an unclamped r the clamp itself
    for n in (16, 64, 320, 16 * 1024 + 16, T - 16, T + 48, 2 * T + 16 * 7):
        cases.append((rmax + bytes(16), b"\xff" * n))
        cases.append((b"\xff" * 32, b"\xff" * n))
    # s all 0xFF: the carry out of 2^128 is dropped
    for n in (0, 16, 64, T + 16):
        cases.append((one + b"\xff" * 16, b"\xff" * n))
        cases.append((rmax + b"\xff" * 16, b"\xff" * n))
    # a final partial block of every length, short and behind a tile edge
    rng = np.random.default_rng(7)
    otk = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    long = rng.integers(0, 256, T + 64 * 3 + 32, dtype=np.uint8).tobytes()
    for j in range(1, 16):
        cases.append((otk, long[:j]))
        cases.append((otk, long[:48 + j]))
        cases.append((otk, long[:T + 64 * 3 + 16 + j]))
        cases.append((rmax + b"\xff" * 16, b"\xff" * (T + j)))
    for otk, msg in cases:
        want = aead_ref.poly1305(otk, msg)
        got = _selftest(dctx, otk, msg)
        assert got == want, (otk.hex(), len(msg))
    # the published one (RFC 8439 2.5.2), as the reference reproduces it
    otk = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    msg = b"Cryptographic Forum Research Group"
    assert _selftest(dctx, otk, msg) == aead_ref.poly1305(otk, msg)


def test_tamper(dctx):
    rng = np.random.default_rng(11)
    sizes = rng.integers(1, 3000, 64).tolist()
    sizes[7] = 0  # (an empty chunk is a sound record of 40 bytes)
    blob = rng.integers(0, 256, sum(sizes), dtype=np.uint8).tobytes()
    nonces = rng.integers(0, 256, 24 * 64, dtype=np.uint8).tobytes()
    recs, rec_ends = aead_ref.seal_many(TEST_KEY, nonces, blob, np.cumsum(sizes), 0)
    bounds = [0] + [int(e) for e in rec_ends]
    records = [bytearray(recs[bounds[i]:bounds[i + 1]]) for i in range(64)]
    plains = [blob[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(64)]
    records[3][5] ^= 0x10        # the nonce
    records[10][24] ^= 0x01      # the first ciphertext byte
    records[20][-17] ^= 0x80     # the last ciphertext byte
    records[30][-1] ^= 0x04      # the tag
    flipped = {3, 10, 20, 30}
    # records too short to hold a nonce and a tag, in between and at the end
    junk = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    items = []  # (record bytes, plaintext or None when bad)
    for i in range(64):
        items.append((bytes(records[i]), None if i in flipped else plains[i]))
        if i == 4:
            items.append((b"", None))
        if i == 16:
            items.append((junk[:23], None))
        if i == 40:
            items.append((junk[:24], None))
    items.append((junk[:39], None))
    data = b"".join(r for r, _ in items)
    ends = np.cumsum([len(r) for r, _ in items]).astype(np.uint64)
    want_bad = [i for i, (_, p) in enumerate(items) if p is None]
    want_plain = b"".join(p if p is not None else bytes(max(0, len(r) - 40)) for r, p in items)
    assert len(want_bad) == 8
    rec, _k1 = to_dev(data, 7)
    out, _k2 = to_dev(b"", 1, room=len(want_plain) + 16)
    rc, out_ends, bad, n_bad = raw_open(dctx, TEST_KEY, rec, len(data), ends, 0, out, len(want_plain))
    assert rc == 0, last_error(dctx)
    assert n_bad == 8 and bad == want_bad
    assert np.array_equal(out_ends, np.cumsum([max(0, len(r) - 40) for r, _ in items]).astype(np.uint64))
    got = from_dev(dctx, out, len(want_plain) + 16)
    assert got[:len(want_plain)] == want_plain  # bad records zero-filled, every other one intact
    assert got[len(want_plain):] == b"\xaa" * 16
    # cap smaller than the count: the first ones, and the full count
    rc, _, bad, n_bad = raw_open(dctx, TEST_KEY, rec, len(data), ends, 0, out, len(want_plain), cap=3)
    assert rc == 0 and n_bad == 8 and bad == want_bad[:3]
    # a wrong key fails every record and releases nothing
    rc, _, bad, n_bad = raw_open(dctx, OTHER_KEY, rec, len(data), ends, 0, out, len(want_plain))
    assert rc == 0 and n_bad == len(items) and bad == list(range(len(items)))
    assert from_dev(dctx, out, len(want_plain)) == bytes(len(want_plain))


def test_refusals(dctx):
    L = _L()
    E = L.DSX_E_INVAL
    blob = bytes(range(200))
    src, _k1 = to_dev(blob)
    out, _k2 = to_dev(b"", room=1024)
    ends = [50, 120, 200]
    nonces = bytes(72)

    def seal(**kw):
        a = dict(key=TEST_KEY, src=src, src_len=200, ends=ends, start=0, nonces=nonces, out=out, out_cap=1024)
        a.update(kw)
        rc, _ = raw_seal(dctx, **a)
        return rc

    assert seal() == 0
    good = from_dev(dctx, out, 320)
    assert seal(algo=1) == E and "algorithm" in last_error(dctx)
    assert seal(flags=L.DSX_OUT_DEVICE) == E and "flag" in last_error(dctx)
    assert seal(flags=1 << 20) == E
    assert seal(ends=[50, 40, 200]) == E and "chunk 1" in last_error(dctx)
    assert seal(start=60) == E and "chunk 0" in last_error(dctx)
    assert seal(ends=[50, 120, 201]) == E and "beyond the buffer" in last_error(dctx)
    assert seal(n=0xFFFFFFF1) == E and "0xFFFFFFF0" in last_error(dctx)
    assert seal(src_len=1 << 40, ends=[1 << 38]) == E and "2^38 - 64" in last_error(dctx)
    assert seal(out_cap=319) == L.DSX_E_CAPACITY and "320" in last_error(dctx)
    assert seal(out=src + 100, out_cap=1024) == E and "overlaps" in last_error(dctx)
    assert seal(key=None) == E
    assert seal(out=0) == E
    assert from_dev(dctx, out, 320) == good  # no refused call wrote anything
    rec_ends = [90, 200, 320]

    def open_(**kw):
        a = dict(key=TEST_KEY, rec=out, rec_len=320, rec_ends=rec_ends, start=0, out=src, out_cap=200)
        a.update(kw)
        return raw_open(dctx, **a)[0]

    assert open_() == 0 and from_dev(dctx, src, 200) == blob
    assert open_(algo=7) == E
    assert open_(flags=L.DSX_ENDS_DEVICE) == E and "flag" in last_error(dctx)
    assert open_(rec_ends=[90, 80, 320]) == E and "record 1" in last_error(dctx)
    assert open_(rec_ends=[90, 200, 321]) == E
    assert open_(out_cap=199) == L.DSX_E_CAPACITY and "200" in last_error(dctx)
    assert open_(out=out + 300, out_cap=200) == E and "overlaps" in last_error(dctx)
    assert open_(key=None) == E
    # n == 0: nothing to do
    assert seal(ends=[]) == 0
    assert raw_open(dctx, TEST_KEY, out, 320, [], 0, src, 200)[3] == 0


def _golden_store(ctx, name="blob1"):
    import desync_amd
    from desync_amd.index import IndexFromReader
    with open(os.path.join(GOLDEN, name), "rb") as f:
        blob = f.read()
    with open(os.path.join(GOLDEN, name + ".caibx"), "rb") as f:
        ix = IndexFromReader(f)
    store = desync_amd.DeviceStore(4 << 20, 1024, ctx=ctx)
    ptr, keep = to_dev(blob, 4)
    store.put_index((ptr, len(blob)), ix)
    return store


def test_device_ends_seal_equals_the_host_ends_call(dctx):
    import desync_amd
    from desync_amd.encrypt import aead_seal
    with _golden_store(dctx) as store:
        conv = desync_amd.NewXChaCha20Poly1305(TEST_KEY, ctx=dctx)
        ids, ends = store.entries()
        n = len(ends)
        assert n == 131
        nonces = np.random.default_rng(5).integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
        buf, rec_ends = store.Seal(conv, nonces=nonces)          # DSX_ENDS_DEVICE
        base, used = store.arena()
        buf2, rec_ends2 = aead_seal(TEST_KEY, base, used, ends, 0, nonces=nonces, ctx=dctx)  # host ends
        arena = from_dev(dctx, base, used)
        want, want_ends = aead_ref.seal_many(TEST_KEY, nonces, arena, ends, 0)
        assert np.array_equal(rec_ends, want_ends) and np.array_equal(rec_ends2, want_ends)
        assert from_dev(dctx, buf.data_ptr(), len(want)) == want
        assert from_dev(dctx, buf2.data_ptr(), len(want)) == want
        # a part of the entries: the start is the end of the entry before
        part, part_ends = store.Seal(conv, first=17, n=30, nonces=nonces[:24 * 30])
        w2, w2_ends = aead_ref.seal_many(TEST_KEY, nonces[:24 * 30], arena, ends[17:47], int(ends[16]))
        assert np.array_equal(part_ends, w2_ends) and from_dev(dctx, part.data_ptr(), len(w2)) == w2


def test_seal_put_sealed_round_trip(dctx):
    import desync_amd
    with _golden_store(dctx) as a, desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as b:
        conv = desync_amd.NewXChaCha20Poly1305(TEST_KEY, ctx=dctx)
        ids, ends = a.entries()
        buf, rec_ends = a.Seal(conv)
        tot = b.PutSealed(buf, rec_ends, ids, conv)
        assert tot["stored"] == len(ends) and tot["stored_bytes"] == int(ends[-1])
        ids_b, ends_b = b.entries()
        assert np.array_equal(ids, ids_b) and np.array_equal(ends, ends_b)
        (pa, ua), (pb, ub) = a.arena(), b.arena()
        assert ua == ub and from_dev(dctx, pa, ua) == from_dev(dctx, pb, ub)
        assert b.Verify() == []
        # a tampered record: named, and nothing is put
        with desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as c:
            bad = buf.clone()
            bad[int(rec_ends[4]) + 30] ^= 1   # in record 5
            bad[int(rec_ends[99]) - 1] ^= 1   # the tag of record 99
            _torch().cuda.synchronize()
            with pytest.raises(desync_amd.AuthenticationError, match="message authentication failed") as e:
                c.PutSealed(bad, rec_ends, ids, conv)
            assert e.value.entries == [5, 99] and "5, 99" in str(e.value)
            assert len(c) == 0
            # sound records under wrong IDs: ChunkInvalid before the put
            wrong = ids.copy()
            wrong[3, 0] ^= 1
            with pytest.raises(desync_amd.ChunkInvalid):
                c.PutSealed(buf, rec_ends, wrong, conv)
            assert len(c) == 0
            assert c.PutSealed(buf, rec_ends, wrong, conv, verify=False)["stored"] == len(ends)


def _synthetic_store(ctx, chunks=300):
    import desync_amd
    rng = np.random.default_rng(21)
    sizes = rng.integers(200, 2000, chunks)
    sizes[5] = 0
    blob = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8).tobytes()
    ends = np.cumsum(sizes).astype(np.uint64)
    ptr, keep = to_dev(blob, 6)
    ids = desync_amd.chunk_ids(ptr, len(blob), ends, 0, ctx=ctx)
    store = desync_amd.DeviceStore(1 << 20, 1024, ctx=ctx)
    store.put((ptr, len(blob)), ids, ends)
    return store


@pytest.mark.parametrize("sealed", [False, True], ids=["plain", "sealed"])
def test_write_local_read_local_round_trip(dctx, tmp_path, sealed):
    import desync_amd
    conv = [desync_amd.NewXChaCha20Poly1305(TEST_KEY, ctx=dctx)] if sealed else []
    ext = conv[0].storageExtension() if sealed else ""
    with _synthetic_store(dctx) as a, desync_amd.DeviceStore(1 << 20, 1024, ctx=dctx) as b:
        ids, ends = a.entries()
        base = str(tmp_path / "store")
        os.mkdir(base)
        assert a.WriteLocal(base, conv) == len(ends) == 300
        # LocalStore's layout: <base>/<hex[0:4]>/<hex><extension>, nothing else left behind
        names = sorted(os.path.relpath(os.path.join(r, f), base) for r, _, fs in os.walk(base) for f in fs)
        assert names == sorted(f"{i.tobytes().hex()[:4]}/{i.tobytes().hex()}{ext}" for i in ids)
        pa, ua = a.arena()
        arena = from_dev(dctx, pa, ua)
        size0 = int(ends[0])
        with open(os.path.join(base, names[0]), "rb") as f:
            first = f.read()
        which = [i for i in range(300) if names[0].endswith(ids[i].tobytes().hex() + ext)][0]
        lo = int(ends[which - 1]) if which else 0
        plain = arena[lo:int(ends[which])]
        assert (aead_ref.open(TEST_KEY, first) if sealed else first) == plain and size0 > 0
        # files of other settings are skipped
        other = os.path.join(base, names[1]) + ".cacnk"
        with open(other, "wb") as f:
            f.write(b"not ours")
        tot = b.ReadLocal(base, conv)
        assert tot["stored"] == 300 and b.Verify() == []
        ids_b, ends_b = b.entries()
        order = np.lexsort(ids.T[::-1])  # ReadLocal walks the directory: by name
        assert np.array_equal(ids_b, ids[order])
        for e in (0, 150, 299):  # the bytes, through the IDs
            assert b.GetChunk(ids[e].tobytes()) == a.GetChunk(ids[e].tobytes())
        assert b.counts()["bytes"] == ua
        if sealed:
            with desync_amd.DeviceStore(1 << 20, 1024, ctx=dctx) as c:
                wrong = [desync_amd.NewXChaCha20Poly1305(OTHER_KEY, ctx=dctx)]
                assert c.ReadLocal(base, wrong)["total"] == 0  # another key: another extension, no file matches
                # the same files under the other key's names: they do not authenticate
                for name in names:
                    p = os.path.join(base, name)
                    os.rename(p, p[:-len(ext)] + wrong[0].storageExtension())
                with pytest.raises(desync_amd.AuthenticationError, match="message authentication failed"):
                    c.ReadLocal(base, wrong)
                assert len(c) == 0 and c.counts()["bytes"] == 0
        with desync_amd.DeviceStore(1 << 20, 1024, ctx=dctx) as c:
            with pytest.raises(ValueError, match="zstd is not available"):
                c.WriteLocal(base, [desync_amd.Compressor()])


def test_random_nonces(dctx):
    import desync_amd
    with _golden_store(dctx) as a, desync_amd.DeviceStore(4 << 20, 1024, ctx=dctx) as b:
        conv = desync_amd.NewXChaCha20Poly1305(TEST_KEY, ctx=dctx)
        ids, ends = a.entries()
        buf1, re1 = a.Seal(conv)
        buf2, re2 = a.Seal(conv)
        assert np.array_equal(re1, re2)
        r1 = from_dev(dctx, buf1.data_ptr(), int(re1[-1]))
        r2 = from_dev(dctx, buf2.data_ptr(), int(re2[-1]))
        starts = [0] + [int(e) for e in re1[:-1]]
        n1 = [r1[s:s + 24] for s in starts]
        n2 = [r2[s:s + 24] for s in starts]
        assert len(set(n1)) == len(n1) and len(set(n2)) == len(n2) and not set(n1) & set(n2)
        assert all(r1[s:e] != r2[s:e] for s, e in zip(starts, re1.tolist()))
        # both open: to the same store content
        assert b.PutSealed(buf1, re1, ids, conv)["stored"] == len(ends)
        assert b.PutSealed(buf2, re2, ids, conv)["present"] == len(ends)
        pa, ua = a.arena()
        i = 60
        assert aead_ref.open(TEST_KEY, r2[starts[i]:int(re2[i])]) == from_dev(dctx, pa, ua)[int(ends[i - 1]):int(ends[i])]


def test_single_chunk_converter(dctx):
    """TestEncryptDecrypt (encrypt_test.go:24-70) for the converter that is built."""
    import desync_amd
    plain = bytes([1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20])
    enc = desync_amd.NewXChaCha20Poly1305(TEST_KEY, ctx=dctx)
    dec = desync_amd.NewXChaCha20Poly1305(TEST_KEY, ctx=dctx)
    stored = enc.toStorage(plain)
    assert len(stored) == len(plain) + 40 and plain not in stored
    assert dec.fromStorage(stored) == plain
    assert aead_ref.open(TEST_KEY, stored) == plain
    assert enc.toStorage(plain) != stored  # a fresh nonce every time
    fixed = enc.toStorage(plain, nonce=bytes(range(24)))
    assert fixed == aead_ref.seal(TEST_KEY, bytes(range(24)), plain)
    assert dec.fromStorage(enc.toStorage(b"")) == b""
    other = desync_amd.NewXChaCha20Poly1305(OTHER_KEY, ctx=dctx)
    with pytest.raises(ValueError, match="chacha20poly1305: message authentication failed"):
        other.fromStorage(stored)
    with pytest.raises(ValueError, match="chacha20poly1305: message authentication failed"):
        dec.fromStorage(stored[:39])
    with pytest.raises(ValueError, match="no nonce prefix found in chunk, not encrypted or wrong algorithm"):
        dec.fromStorage(stored[:23])
    conv = desync_amd.Converters([enc])
    assert conv.fromStorage(conv.toStorage(plain)) == plain
