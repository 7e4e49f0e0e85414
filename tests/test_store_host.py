"""The chunk store in HBM (dsx_store_*, desync_amd.store): what can be checked
without a GPU -- the exports, the struct layouts, the argument checks that come
before any device work, and the dict-and-bytearray model (store_ref.py) the
GPU tests compare with, against the goldens' counts."""
import ctypes
import json
import os

import numpy as np

import store_ref
from desync_amd import _lib
from desync_amd.index import IndexFromReader

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ("dsx_store_create", "dsx_store_destroy", "dsx_store_count", "dsx_store_put",
       "dsx_store_locate", "dsx_store_arena", "dsx_store_entries", "dsx_store_resolve",
       "dsx_store_verify")


def test_new_entry_points_are_bound_and_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name


def test_abi_version_stays():
    assert _lib.lib().dsx_abi_version() == 5


def test_struct_layouts():
    assert ctypes.sizeof(_lib.StoreCounts) == 32
    assert ctypes.sizeof(_lib.StorePutTotals) == 40
    assert [n for n, _ in _lib.StoreCounts._fields_] == ["chunks", "bytes", "max_chunks", "arena_bytes"]
    assert [n for n, _ in _lib.StorePutTotals._fields_] == \
        ["total", "stored", "stored_bytes", "present", "repeats"]


def test_null_context_or_store_is_invalid():
    """Every entry point refuses a NULL context or store before touching HIP
    (without a GPU a HIP call would fail with another code)."""
    L = _lib.lib()
    E = _lib.DSX_E_INVAL
    ids = (ctypes.c_uint8 * 32)()
    ends = (ctypes.c_uint64 * 1)(5)
    h = ctypes.c_void_p()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the other handle is NULL
    tot = _lib.StorePutTotals()
    cnt = _lib.StoreCounts()
    n = ctypes.c_uint64()
    bad = ctypes.c_uint32()
    p = ctypes.c_void_p()
    assert L.dsx_store_create(None, 1024, 4, ctypes.byref(h)) == E and not h.value
    assert L.dsx_store_destroy(None, fake) == E
    assert L.dsx_store_destroy(None, None) == E
    assert L.dsx_store_count(None, ctypes.byref(cnt)) == E
    assert L.dsx_store_put(None, fake, None, 0, ids, ends, 0, 1, ctypes.byref(tot), 0) == E
    assert L.dsx_store_locate(None, fake, ids, 1, None, None, ctypes.byref(n), 0) == E
    assert L.dsx_store_arena(None, ctypes.byref(p), ctypes.byref(n)) == E
    assert L.dsx_store_entries(None, fake, 0, 0, None, None, 0) == E
    assert L.dsx_store_resolve(None, fake, ids, 1, None, 0, ctypes.byref(n), ctypes.byref(n),
                               ctypes.byref(bad), 0) == E
    assert L.dsx_store_verify(None, fake, 0, None, 0, ctypes.byref(n)) == E


def test_package_exports_the_python_layer():
    import desync_amd
    for name in ("DeviceStore", "ChopBlob", "ChunkMissing"):
        assert name in desync_amd.__all__ and hasattr(desync_amd, name), name
    assert issubclass(desync_amd.ChunkMissing, KeyError)
    cid = bytes(range(32))
    e = desync_amd.ChunkMissing(cid)
    assert str(e) == f"chunk {cid.hex()} missing from store" and e.ID == cid


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _index(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        ix = IndexFromReader(f)
    ids = np.frombuffer(b"".join(bytes(c.ID) for c in ix.Chunks), np.uint8).reshape(-1, 32)
    ends = np.cumsum([c.Size for c in ix.Chunks]).astype(np.uint64)
    return ids, ends


def test_model_gives_the_goldens_counts():
    """store_ref on blob1 then blob2: the counts of info_blob1_blob2.json."""
    with open(os.path.join(GOLDEN, "info_blob1_blob2.json")) as f:
        cases = {(c["index"], tuple(c["seeds"])): c["expect"] for c in json.load(f)["cases"]}
    m = store_ref.Store(4 << 20, 1024)
    t1 = m.put(_golden("blob1"), *_index("blob1.caibx"))
    assert t1 == {"total": 161, "stored": 131, "stored_bytes": 1114112, "present": 0, "repeats": 30}
    e = cases[("blob1.caibx", ())]
    assert (t1["total"], t1["stored"], t1["stored_bytes"]) == \
        (e["total"], e["unique"], e["dedup-size-not-in-seed"])
    t2 = m.put(_golden("blob2"), *_index("blob2.caibx"))
    assert t2 == {"total": 161, "stored": 7, "stored_bytes": 80029, "present": 124, "repeats": 30}
    e = cases[("blob2.caibx", ("blob1.caibx",))]
    assert (t2["present"], t2["stored"], t2["stored_bytes"]) == \
        (e["in-seed"], e["not-in-seed-nor-cache"], e["dedup-size-not-in-seed"])
    assert m.counts() == {"chunks": 138, "bytes": 1114112 + 80029, "max_chunks": 1024,
                          "arena_bytes": 4 << 20}


def test_model_is_all_or_nothing():
    blob = bytes(range(200))
    ids = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)
    ends = np.array([50, 50, 120, 200], dtype=np.uint64)
    m = store_ref.Store(200, 4)
    assert m.put(blob, ids, ends)["stored"] == 4 and bytes(m.arena) == blob
    for arena, chunks in ((199, 4), (200, 3)):
        m = store_ref.Store(arena, chunks)
        try:
            m.put(blob, ids, ends)
        except store_ref.Capacity as e:
            assert e.totals["stored"] == 4 and e.totals["stored_bytes"] == 200
        else:
            raise AssertionError("the put fitted")
        assert m.counts()["chunks"] == 0 and not m.arena
    offs, sizes, miss = m.locate(ids)
    assert miss == 4 and all(o == store_ref.OFF_NONE for o in offs) and not any(sizes)
