"""dsx_store_copy and desync_amd.copy (Copy, Cache, DeviceStore.CopyFrom / Grow):
what can be checked without a GPU -- the export, the struct layout, the NULL
refusal that comes before any device work, Copy and Cache over two
MemoryStores, and the model (store_copy_ref.py) the GPU tests compare with."""
import ctypes

import numpy as np
import pytest

import store_copy_ref
import store_ref
from desync_amd import _lib


def test_entry_point_is_bound_and_exported():
    assert "dsx_store_copy" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "dsx_store_copy")
    assert _lib.DSX_COPY_ALL == 1024


def test_struct_layout():
    assert ctypes.sizeof(_lib.StoreCopyTotals) == 64
    assert [n for n, _ in _lib.StoreCopyTotals._fields_] == \
        ["total", "copied", "copied_bytes", "present", "repeats", "missing", "first_missing", "reserved"]


def test_abi_version_stays():
    assert _lib.lib().dsx_abi_version() == 5


def test_null_context_is_invalid():
    L = _lib.lib()
    ids = (ctypes.c_uint8 * 32)()
    tot = _lib.StoreCopyTotals()
    fake, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)  # never dereferenced: the context is NULL
    for flags in (0, _lib.DSX_IDS_DEVICE):
        assert L.dsx_store_copy(None, fake, other, ids, 1, ctypes.byref(tot), flags) == _lib.DSX_E_INVAL
    assert L.dsx_store_copy(None, fake, other, None, 0, ctypes.byref(tot), _lib.DSX_COPY_ALL) == _lib.DSX_E_INVAL
    assert L.dsx_store_copy(None, None, None, None, 0, None, 0) == _lib.DSX_E_INVAL


def test_python_layer_has_the_names():
    import desync_amd
    for name in ("CopyFrom", "Grow"):
        assert callable(getattr(desync_amd.DeviceStore, name)), name
    for name in ("Copy", "Cache", "NewCache"):
        assert callable(getattr(desync_amd, name)) and name in desync_amd.__all__, name


# ---- Copy and Cache over two MemoryStores -------------------------------------------------
def _cid(k):
    return bytes([k]) * 32


def _mem(*ks):
    import desync_amd
    m = desync_amd.MemoryStore()
    for k in ks:
        m.StoreChunk(desync_amd.Chunk(_cid(k), b"data-%d" % k))
    return m


class Bar:
    def __init__(self):
        self.calls = []

    def SetTotal(self, n):
        self.calls.append(("SetTotal", n))

    def Start(self):
        self.calls.append("Start")

    def Increment(self):
        self.calls.append("Increment")

    def Finish(self):
        self.calls.append("Finish")


class Counting:
    """A store that counts the calls it passes on."""

    def __init__(self, inner):
        self.inner, self.gets, self.stores = inner, [], []

    def HasChunk(self, cid):
        return self.inner.HasChunk(cid)

    def GetChunk(self, cid):
        self.gets.append(cid)
        return self.inner.GetChunk(cid)

    def StoreChunk(self, chunk):
        self.stores.append(chunk.ID())
        self.inner.StoreChunk(chunk)


@pytest.mark.parametrize("workers", [1, 4])
def test_copy_skips_what_is_present(workers):
    import desync_amd
    src, dst = Counting(_mem(1, 2, 3, 4)), Counting(_mem(2, 9))
    desync_amd.Copy([_cid(k) for k in (1, 2, 3, 1, 2)], src, dst, n=workers)
    assert sorted(dst.inner.chunks) == [_cid(k) for k in (1, 2, 3, 9)]
    assert dst.inner.chunks[_cid(3)] == b"data-3" and dst.inner.chunks[_cid(2)] == b"data-2"
    assert _cid(2) not in src.gets and _cid(2) not in dst.stores
    if workers == 1:
        assert src.gets == [_cid(1), _cid(3)] and dst.stores == [_cid(1), _cid(3)]
    # an (n, 32) array is taken too
    desync_amd.Copy(np.frombuffer(_cid(4), np.uint8).reshape(1, 32), src, dst)
    assert dst.inner.chunks[_cid(4)] == b"data-4"


def test_copy_raises_chunk_missing_for_the_first_id_the_source_lacks():
    import desync_amd
    src, dst = _mem(1, 2), _mem()
    with pytest.raises(desync_amd.ChunkMissing) as e:
        desync_amd.Copy([_cid(1), _cid(7), _cid(2), _cid(8)], src, dst)
    assert e.value.ID == _cid(7)
    assert list(dst.chunks) == [_cid(1)]  # (the reference's loop: what came before stays)


def test_copy_id_in_dst_but_not_in_src_is_no_error():
    import desync_amd
    src, dst = _mem(1), _mem(5)
    desync_amd.Copy([_cid(5), _cid(1)], src, dst)
    assert sorted(dst.chunks) == [_cid(1), _cid(5)]


def test_copy_progress_bar_sequence():
    import desync_amd
    bar = Bar()
    desync_amd.Copy([_cid(1), _cid(2), _cid(1)], _mem(1, 2), _mem(2), pb=bar)
    assert bar.calls == [("SetTotal", 3), "Start", "Increment", "Increment", "Increment", "Finish"]
    bar = Bar()
    with pytest.raises(desync_amd.ChunkMissing):
        desync_amd.Copy([_cid(3), _cid(1)], _mem(1), _mem(), pb=bar)
    assert bar.calls == [("SetTotal", 2), "Start", "Increment", "Finish"]


def test_cache_get_stores_in_local_and_has_looks_in_both():
    import desync_amd
    s, l = Counting(_mem(1, 2)), Counting(_mem(3))  # noqa: E741
    cache = desync_amd.NewCache(s, l)
    assert isinstance(cache, desync_amd.Cache)
    assert cache.HasChunk(_cid(3)) and cache.HasChunk(_cid(1)) and not cache.HasChunk(_cid(4))
    assert cache.GetChunk(_cid(3)) == b"data-3" and s.gets == []  # local first
    assert cache.GetChunk(_cid(1)) == b"data-1"
    assert s.gets == [_cid(1)] and l.stores == [_cid(1)] and l.inner.chunks[_cid(1)] == b"data-1"
    assert cache.GetChunk(_cid(1)) == b"data-1" and s.gets == [_cid(1)]  # now from the local store
    with pytest.raises(desync_amd.ChunkMissing) as e:
        cache.GetChunk(_cid(4))
    assert e.value.ID == _cid(4)
    cache.StoreChunk(desync_amd.Chunk(_cid(6), b"six"))
    assert l.inner.chunks[_cid(6)] == b"six" and _cid(6) not in s.inner.chunks
    cache.Close()  # (stores without Close are left alone)


# ---- the model ----------------------------------------------------------------------------
def _row(k):
    return np.full(32, k, dtype=np.uint8)


def _store(arena_bytes, max_chunks, *chunks):
    m = store_ref.Store(arena_bytes, max_chunks)
    for k, data in chunks:
        m.put(data, _row(k).reshape(1, 32), [len(data)])
    return m


def test_model_rules_by_hand():
    src = _store(100, 10, (1, b"one"), (2, b""), (3, b"three"), (4, b"four"))
    dst = _store(13, 4, (3, b"three"), (9, b"nine"))  # an exact fit in both
    ask = np.stack([_row(k) for k in (4, 3, 4, 9, 2, 2)])  # 9 is in dst only: present
    t = store_copy_ref.copy(dst, src, ask)
    assert t == {"total": 6, "copied": 2, "copied_bytes": 4, "present": 2, "repeats": 2, "missing": 0,
                 "first_missing": store_copy_ref.U64_MAX}
    assert t["total"] == t["copied"] + t["present"] + t["repeats"] + t["missing"]
    assert dst.ids == [_row(k).tobytes() for k in (3, 9, 4, 2)]  # first-occurrence order
    assert bytes(dst.arena) == b"threeninefour" and dst.ends == [5, 9, 13, 13]


def test_model_rules_all_or_nothing():
    src = _store(100, 10, (1, b"one"), (2, b"two"))
    dst = _store(8, 3, (3, b"three"))
    before = (list(dst.ids), list(dst.ends), bytes(dst.arena))
    # missing: 7 and 8 are in neither store; nothing is copied although 1 could be
    t = store_copy_ref.copy(dst, src, np.stack([_row(k) for k in (1, 7, 8, 7, 3)]))
    assert (t["missing"], t["first_missing"], t["copied"], t["present"], t["repeats"]) == (2, 1, 1, 1, 1)
    assert (dst.ids, dst.ends, bytes(dst.arena)) == before
    # one byte too many, then one chunk too many
    t = store_copy_ref.copy(dst, src, np.stack([_row(1), _row(2)]))
    assert t["copied_bytes"] == 6 and not store_copy_ref.fits(dst.counts(), t)
    assert (dst.ids, dst.ends, bytes(dst.arena)) == before
    dst.arena_bytes, dst.max_chunks = 100, 2
    t = store_copy_ref.copy(dst, src, None)
    assert t["copied"] == 2 and not store_copy_ref.fits(dst.counts(), t)
    assert (dst.ids, dst.ends, bytes(dst.arena)) == before
    # the exact fit; DSX_COPY_ALL takes src's entries in entry order
    dst.arena_bytes, dst.max_chunks = 11, 3
    t = store_copy_ref.copy(dst, src, None)
    assert t["total"] == 2 and t["copied"] == 2 and bytes(dst.arena) == b"threeonetwo"
    empty = store_ref.Store(6, 2)
    store_copy_ref.copy(empty, src, None)
    assert (empty.ids, empty.ends, empty.arena) == (src.ids, src.ends, src.arena)
