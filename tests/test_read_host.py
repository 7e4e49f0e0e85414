"""dsx_read_plan, dsx_read_ranges' bindings and IndexPos: what can be checked
without a GPU.  dsx_read_plan runs dsx_read_geom.h, the arithmetic of the count
and emit kernels, on the host; the model is read_ref.py (bisect)."""
import ctypes
import io
import os
import re
import shutil

import numpy as np
import pytest

import read_ref
from desync_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan(ends, ranges, start=0, cap=None):
    """-> (rc, npieces, [(range, chunk, chunk_off, dst_off, bytes)])"""
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    rg = np.ascontiguousarray(read_ref.with_dst(ranges), dtype=np.uint64).reshape(-1, 3)
    n = ctypes.c_uint64(12345)
    if cap is None:
        rc = _lib.lib().dsx_read_plan(ends.ctypes.data, start, ends.size, rg.ctypes.data, len(rg), None, 0,
                                      ctypes.byref(n))
        assert rc in (0, _lib.DSX_E_CAPACITY), rc
        cap = n.value
    out = (_lib.ReadPiece * max(1, cap))()
    rc = _lib.lib().dsx_read_plan(ends.ctypes.data, start, ends.size, rg.ctypes.data, len(rg), out, cap,
                                  ctypes.byref(n))
    got = [(p.range, p.chunk, p.chunk_off, p.dst_off, p.bytes) for p in out[:min(cap, n.value)]]
    return rc, n.value, got


def cut_list(rng, n, start=0, max_size=300 << 10):
    return (start + np.cumsum(rng.integers(1, max_size + 1, n, dtype=np.uint64))).astype(np.uint64)


@pytest.mark.parametrize("n,start,seed", [(1, 0, 1), (2, 0, 2), (7, 0, 3), (257, 0, 4), (4000, 0, 5),
                                          (1, 1000, 6), (300, 123457, 7)])
def test_plan_equals_the_model(n, start, seed):
    rng = np.random.default_rng(seed)
    ends = cut_list(rng, n, start)
    total = int(ends[-1])
    offs = rng.integers(start, total, 300)
    lens = [int(rng.integers(0, min(total - o, 1 << int(rng.integers(1, 22))) + 1)) for o in offs]
    ranges = read_ref.edge_ranges(ends, start) + list(zip(offs.tolist(), lens))
    rc, count, got = plan(ends, ranges, start)
    want = read_ref.pieces(ends, ranges, start)
    assert rc == 0 and count == len(want)
    assert got == want
    assert all(p[4] > 0 for p in got)
    # every byte of every range is covered exactly once, in order
    rg = read_ref.with_dst(ranges)
    at = {}
    for r, _, _, dst, nbytes in got:
        assert dst == at.get(r, rg[r][2])
        at[r] = dst + nbytes
    for r, (_, ln, dst) in enumerate(rg):
        assert at.get(r, dst) == dst + ln


def test_plan_with_chunks_of_size_zero():
    ends = [10, 10, 20, 20, 20, 35, 35]
    ranges = [(0, 35), (10, 10), (9, 2), (20, 0), (19, 16), (34, 1)]
    rc, count, got = plan(ends, ranges)
    assert rc == 0 and got == read_ref.pieces(ends, ranges)
    assert [p[1] for p in got if p[0] == 0] == [0, 2, 5]


def test_plan_by_hand():
    rc, count, got = plan([10, 30], [(5, 10, 100), (0, 30, 200)])
    assert rc == 0 and got == [(0, 0, 5, 100, 5), (0, 1, 0, 105, 5), (1, 0, 0, 200, 10), (1, 1, 0, 210, 20)]


def test_plan_capacity():
    ends = cut_list(np.random.default_rng(9), 50)
    ranges = [(0, int(ends[-1])), (int(ends[3]), int(ends[9] - ends[3]))]
    want = read_ref.pieces(ends, ranges)
    assert len(want) == 56
    for cap in (0, 1, 55):
        rc, count, got = plan(ends, ranges, cap=cap)
        assert rc == _lib.DSX_E_CAPACITY and count == 56 and got == want[:cap]
    rc, count, got = plan(ends, ranges, cap=56)
    assert rc == 0 and count == 56 and got == want


def test_plan_refusals():
    L = _lib.lib()
    n = ctypes.c_uint64()
    ends = np.array([10, 20], dtype=np.uint64)
    rg = np.array([[0, 5, 0]], dtype=np.uint64)
    out = (_lib.ReadPiece * 4)()
    ok = (ends.ctypes.data, 0, 2, rg.ctypes.data, 1, out, 4)
    assert L.dsx_read_plan(*ok, ctypes.byref(n)) == 0 and n.value == 1
    assert L.dsx_read_plan(*ok, None) == _lib.DSX_E_INVAL
    assert L.dsx_read_plan(None, 0, 2, rg.ctypes.data, 1, out, 4, ctypes.byref(n)) == _lib.DSX_E_INVAL
    assert L.dsx_read_plan(ends.ctypes.data, 0, 2, None, 1, out, 4, ctypes.byref(n)) == _lib.DSX_E_INVAL
    assert L.dsx_read_plan(ends.ctypes.data, 0, 2, rg.ctypes.data, 1, None, 4, ctypes.byref(n)) == _lib.DSX_E_INVAL
    down = np.array([20, 10], dtype=np.uint64)
    assert L.dsx_read_plan(down.ctypes.data, 0, 2, rg.ctypes.data, 1, out, 4, ctypes.byref(n)) == _lib.DSX_E_INVAL
    assert L.dsx_read_plan(ends.ctypes.data, 11, 2, rg.ctypes.data, 1, out, 4, ctypes.byref(n)) == _lib.DSX_E_INVAL
    for off, ln in ((0, 21), (20, 1), (21, 0), (2 ** 64 - 1, 2)):  # beyond the blob
        bad = np.array([[off, ln, 0]], dtype=np.uint64)
        assert L.dsx_read_plan(ends.ctypes.data, 0, 2, bad.ctypes.data, 1, out, 4, ctypes.byref(n)) == \
            _lib.DSX_E_INVAL, (off, ln)
    below = np.array([[4, 2, 0]], dtype=np.uint64)  # below start
    assert L.dsx_read_plan(ends.ctypes.data, 5, 2, below.ctypes.data, 1, out, 4, ctypes.byref(n)) == _lib.DSX_E_INVAL
    # no chunks: only the empty range at start
    empty = np.array([[7, 0, 0]], dtype=np.uint64)
    assert L.dsx_read_plan(None, 7, 0, empty.ctypes.data, 1, out, 4, ctypes.byref(n)) == 0 and n.value == 0
    one = np.array([[7, 1, 0]], dtype=np.uint64)
    assert L.dsx_read_plan(None, 7, 0, one.ctypes.data, 1, out, 4, ctypes.byref(n)) == _lib.DSX_E_INVAL


# ---- arguments and bindings ---------------------------------------------------------------
def test_null_context_is_invalid_before_hip_is_touched():
    L = _lib.lib()
    ids = (ctypes.c_uint8 * 32)()
    ends = (ctypes.c_uint64 * 1)(8)
    rg = _lib.Range(0, 8, 0)
    tot = _lib.ReadTotals()
    fake, out = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)  # never dereferenced: the context is NULL
    for flags in (0, _lib.DSX_IDS_DEVICE | _lib.DSX_ENDS_DEVICE, 1 << 20):
        assert L.dsx_read_ranges(None, fake, ids, ends, 0, 1, None, 0, ctypes.byref(rg), 1, out, 8,
                                 ctypes.byref(tot), flags) == _lib.DSX_E_INVAL
    assert L.dsx_read_ranges(None, None, None, None, 0, 0, None, 0, None, 0, None, 0, None, 0) == _lib.DSX_E_INVAL


def test_entry_points_are_bound_exported_and_declared():
    hdr = open(os.path.join(REPO, "include", "dsx.h")).read()
    for name in ("dsx_read_ranges", "dsx_read_plan"):
        assert name in _lib.EXPORTS
        f = getattr(_lib.lib(), name)
        assert f.argtypes is not None and f.restype is ctypes.c_int
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert len(_lib.lib().dsx_read_ranges.argtypes) == 14 and len(_lib.lib().dsx_read_plan.argtypes) == 8


def test_struct_layouts():
    assert ctypes.sizeof(_lib.Range) == 24
    assert ctypes.sizeof(_lib.ReadTotals) == 72
    assert [n for n, _ in _lib.ReadTotals._fields_] == list(read_ref.TOTALS)
    assert ctypes.sizeof(_lib.ReadPiece) == 32 and _lib.ReadPiece.range.offset == 24


def test_abi_version_stays():
    assert _lib.lib().dsx_abi_version() == 5


def test_python_layer_has_the_names():
    import desync_amd
    for name in ("NewIndexReadSeeker", "IndexPos", "Cat", "read_ranges", "DeviceIndex"):
        assert callable(getattr(desync_amd, name)) and name in desync_amd.__all__, name
        assert name in desync_amd.__doc__, name
    assert callable(desync_amd.DeviceStore.read_ranges)
    for name in ("Seek", "Read", "ReadAt", "read_device", "read", "seek", "tell", "readable", "seekable"):
        assert callable(getattr(desync_amd.IndexPos, name)), name


def test_ranges_array_packs_pairs_back_to_back():
    from desync_amd.readseeker import ranges_array
    assert ranges_array([(5, 3), (0, 4), (9, 0), (1, 2)]).tolist() == [[5, 3, 0], [0, 4, 3], [9, 0, 7], [1, 2, 7]]
    assert ranges_array([(5, 3, 100)]).tolist() == [[5, 3, 100]]
    assert ranges_array([]).shape == (0, 3)
    with pytest.raises(ValueError):
        ranges_array([(1, 2, 3, 4)])


# ---- IndexPos over a store in host memory --------------------------------------------------
CHUNK_MAX = 256 << 10  # ChunkSizeMaxDefault


def _index(chunks, size_max=CHUNK_MAX):
    """chunks: [(id, size)]"""
    import desync_amd
    out, at = [], 0
    for cid, size in chunks:
        out.append(desync_amd.IndexChunk(cid, at, size))
        at += size
    return desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=size_max), out)


def _cid(data):
    from desync_amd.digest import Digest
    return Digest.Sum(data)


@pytest.fixture(scope="module")
def valid():
    """readseeker_test.go's valid case: head, the null chunk (not stored), tail."""
    import desync_amd
    head, tail = b"hello, world", b"goodbye, world"
    null = desync_amd.NewNullChunk(CHUNK_MAX)
    store = read_ref.HostStore({_cid(head): head, _cid(tail): tail})
    idx = _index([(_cid(head), len(head)), (null.ID, CHUNK_MAX), (_cid(tail), len(tail))])
    return idx, store, head + bytes(CHUNK_MAX) + tail, head, tail


def test_seeker_size_mismatch_is_an_error():
    """TestIndexReadSeekerSizeMismatchPanic: the index claims 1000 bytes, 4 are stored."""
    import desync_amd
    data = b"data"
    r = desync_amd.NewIndexReadSeeker(_index([(_cid(data), 1000)]), read_ref.HostStore({_cid(data): data}))
    assert r.Seek(200, io.SEEK_SET) == 200
    with pytest.raises(ValueError, match="unexpected size for chunk " + _cid(data).hex()):
        r.Read(16)
    assert r.tell() == 200


def test_seeker_size_mismatch_does_not_loop():
    """TestIndexReadSeekerSizeMismatchNoLoop: a short chunk that is not the last."""
    import desync_amd
    short, tail = b"data", b"trailing"
    store = read_ref.HostStore({_cid(short): short, _cid(tail): tail})
    r = desync_amd.NewIndexReadSeeker(_index([(_cid(short), 1000), (_cid(tail), len(tail))]), store)
    with pytest.raises(ValueError, match="unexpected size for chunk"):
        r.Read(64)
    assert store.calls == 1 and r.tell() == 0


def test_seeker_valid(valid):
    """TestIndexReadSeekerValid: a full read, then a seek to the last chunk."""
    import desync_amd
    idx, store, want, head, tail = valid
    r = desync_amd.NewIndexReadSeeker(idx, store)
    assert r.Length == len(want)
    assert r.read() == want and r.tell() == len(want)
    assert r.Seek(len(head) + CHUNK_MAX, io.SEEK_SET) == len(head) + CHUNK_MAX
    assert r.read() == tail
    assert r.Read(16) == b""  # io.EOF


def test_seeker_empty_index():
    """TestIndexReadSeekerEmptyIndex."""
    import desync_amd
    r = desync_amd.NewIndexReadSeeker(_index([]), read_ref.HostStore({}))
    assert r.read() == b""
    assert r.Seek(0, io.SEEK_SET) == 0
    assert r.Seek(0, io.SEEK_END) == 0
    assert r.Read(16) == b""
    with pytest.raises(EOFError):  # (io.EOF from Seek past the end of an empty index)
        r.Seek(3, io.SEEK_SET)
    assert r.Read(16) == b""


def test_seek_messages_and_whence(valid):
    import desync_amd
    idx, store, want, head, tail = valid
    r = desync_amd.NewIndexReadSeeker(idx, store)
    total = len(want)
    assert r.Seek(5) == 5 and r.Seek(5, io.SEEK_SET) == 5
    assert r.Seek(3, io.SEEK_CUR) == 8 and r.Seek(-8, io.SEEK_CUR) == 0
    assert r.Seek(-4, io.SEEK_END) == total - 4 and r.Read(100) == want[-4:]
    assert r.Seek(0, io.SEEK_END) == total and r.Seek(total, io.SEEK_SET) == total  # exactly Length is fine
    assert r.Seek(7, io.SEEK_SET) == 7
    for args, msg in (((0, 3), "invalid whence"),
                      ((-1, io.SEEK_SET), "unable to seek before start of file"),
                      ((-8, io.SEEK_CUR), "unable to seek before start of file"),
                      ((-total - 1, io.SEEK_END), "unable to seek before start of file"),
                      ((total + 1, io.SEEK_SET),
                       f"seek found chunk ending at position {total}, desired position is {total + 1}"),
                      ((5, io.SEEK_END),
                       f"seek found chunk ending at position {total}, desired position is {total + 5}")):
        with pytest.raises(ValueError) as e:
            r.Seek(*args)
        assert str(e.value) == msg
        assert r.tell() == 7  # unchanged on an error


def test_read_short_at_the_end_and_eof(valid):
    import desync_amd
    idx, store, want, head, tail = valid
    r = desync_amd.NewIndexReadSeeker(idx, store)
    assert r.Read(5) == want[:5] and r.tell() == 5
    assert r.Read(0) == b"" and r.tell() == 5
    assert r.Read(20) == want[5:25]  # across the head into the null chunk
    r.Seek(-6, io.SEEK_END)
    assert r.Read(100) == want[-6:] and r.tell() == len(want)  # a short read
    assert r.Read(100) == b"" and r.Read(1) == b""             # io.EOF
    assert r.ReadAt(3, 9) == want[3:12] and r.tell() == len(want)
    assert r.ReadAt(len(want) - 2, 50) == want[-2:] and r.ReadAt(len(want), 5) == b""
    r.Seek(len(head) - 2)
    assert bytes(r.read_device(6)) == want[len(head) - 2:len(head) + 4] and r.tell() == len(head) + 4


def test_seeker_is_a_file_object(valid):
    import desync_amd
    idx, store, want, head, tail = valid
    r = desync_amd.NewIndexReadSeeker(idx, store)
    assert r.readable() and r.seekable() and not r.writable()
    assert io.BufferedReader(r).read() == want
    r = desync_amd.NewIndexReadSeeker(idx, store)
    buffered = io.BufferedReader(r, buffer_size=4096)
    assert buffered.read(7) == want[:7]
    buffered.seek(len(head) + CHUNK_MAX - 3)
    assert buffered.read(8) == want[len(head) + CHUNK_MAX - 3:][:8]
    sink = io.BytesIO()
    shutil.copyfileobj(desync_amd.NewIndexReadSeeker(idx, store), sink, 1000)
    assert sink.getvalue() == want


def test_seeker_missing_chunk(valid):
    import desync_amd
    idx, store, want, head, tail = valid
    r = desync_amd.NewIndexReadSeeker(idx, read_ref.HostStore({_cid(head): head}))
    assert r.Read(len(head) + 10) == want[:len(head) + 10]  # the null chunk needs no store
    r.Seek(-3, io.SEEK_END)
    with pytest.raises(desync_amd.ChunkMissing) as e:
        r.Read(3)
    assert e.value.ID == _cid(tail) and r.tell() == len(want) - 3


def test_cat(valid):
    import desync_amd
    idx, store, want, head, tail = valid
    assert desync_amd.Cat(idx, store) == want
    assert desync_amd.Cat(idx, store, offset=5) == want[5:]
    assert desync_amd.Cat(idx, store, offset=5, length=30) == want[5:35]
    assert desync_amd.Cat(idx, store, offset=len(want)) == b""
    sink = io.BytesIO()
    assert desync_amd.Cat(idx, store, len(head) + CHUNK_MAX - 1, 4, out=sink) == 4
    assert sink.getvalue() == b"\0" + tail[:3]
    with pytest.raises(EOFError):  # io.CopyN: fewer bytes than asked for
        desync_amd.Cat(idx, store, offset=len(want) - 3, length=4)
    with pytest.raises(ValueError, match="seek found chunk ending at position"):
        desync_amd.Cat(idx, store, offset=len(want) + 1)
