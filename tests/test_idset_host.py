"""Chunk-ID sets (dsx_idset_*, dsx_dedup, desync_amd.info): what can be
checked without a GPU -- the exports, the argument checks that come before any
device work, and the fixture against a plain dict count over the goldens."""
import ctypes
import json
import os

import pytest

from desync_amd import _lib
from desync_amd.index import IndexFromReader

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ("dsx_idset_create", "dsx_idset_destroy", "dsx_idset_count", "dsx_dedup")


def dict_info(index, seeds=(), cache=None):
    """cmd/desync/info.go:95-185 with Python sets."""
    seed_ids = {bytes(c.ID) for s in seeds for c in s.Chunks}
    seen = set()
    r = {"total": 0, "unique": 0, "in-store": 0, "in-seed": 0, "in-cache": 0,
         "not-in-seed-nor-cache": 0, "size": index.Length(), "dedup-size-not-in-seed": 0,
         "dedup-size-not-in-seed-nor-cache": 0, "dedup-size-not-in-seed-nor-cache-compressed": 0,
         "chunk-size-min": index.Index.ChunkSizeMin, "chunk-size-avg": index.Index.ChunkSizeAvg,
         "chunk-size-max": index.Index.ChunkSizeMax}
    for c in index.Chunks:
        r["total"] += 1
        cid = bytes(c.ID)
        if cid in seen:
            continue
        seen.add(cid)
        in_seed = cid in seed_ids
        in_cache = cache is not None and cache.HasChunk(cid)
        r["in-seed"] += in_seed
        r["in-cache"] += in_cache
        if not in_seed:
            r["dedup-size-not-in-seed"] += c.Size
        if not in_seed and not in_cache:
            r["not-in-seed-nor-cache"] += 1
            r["dedup-size-not-in-seed-nor-cache"] += c.Size
    r["unique"] = len(seen)
    return r


def load_index(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return IndexFromReader(f)


def fixture():
    with open(os.path.join(GOLDEN, "info_blob1_blob2.json")) as f:
        return json.load(f)["cases"]


def test_new_entry_points_are_bound_and_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert (_lib.DSX_IDS_DEVICE, _lib.DSX_SIZES) == (32, 64)
    # the new flags collide with no flag they can be combined with
    others = (_lib.DSX_OUT_DEVICE, _lib.DSX_ENDS_DEVICE)
    assert all(f & (_lib.DSX_IDS_DEVICE | _lib.DSX_SIZES) == 0 for f in others)


def test_package_exports_the_python_layer():
    import desync_amd
    for name in ("IDSet", "dedup", "Info"):
        assert name in desync_amd.__all__ and hasattr(desync_amd, name), name


def test_null_context_is_invalid():
    L = _lib.lib()
    ids = (ctypes.c_uint8 * 32)()
    ends = (ctypes.c_uint64 * 1)(5)
    h = ctypes.c_void_p()
    tot = _lib.DedupTotals()
    assert L.dsx_idset_create(None, ids, 1, 0, ctypes.byref(h)) == _lib.DSX_E_INVAL
    assert not h.value
    assert L.dsx_dedup(None, ids, ends, 0, 1, None, None, None, ctypes.byref(tot), 0) \
        == _lib.DSX_E_INVAL
    assert L.dsx_idset_destroy(None, None) == _lib.DSX_E_INVAL
    assert L.dsx_idset_count(None, None, None) == _lib.DSX_E_INVAL


def test_totals_struct_layout():
    assert ctypes.sizeof(_lib.DedupTotals) == 5 * 8
    assert [n for n, _ in _lib.DedupTotals._fields_] == \
        ["total", "unique", "in_seed", "size", "size_not_in_seed"]


@pytest.mark.parametrize("k", range(4))
def test_fixture_equals_a_dict_count_over_the_goldens(k):
    case = fixture()[k]
    got = dict_info(load_index(case["index"]), [load_index(s) for s in case["seeds"]])
    for key, want in case["expect"].items():
        assert got[key] == want, (case["index"], case["seeds"], key)


def test_fixture_holds_the_reference_figures():
    cases = fixture()
    assert [(c["index"], c["seeds"]) for c in cases] == [
        ("blob1.caibx", []), ("blob2.caibx", []), ("blob1.caibx", ["blob2.caibx"]),
        ("blob2.caibx", ["blob1.caibx"])]
    for c in cases:
        e = c["expect"]
        assert (e["total"], e["unique"], e["size"]) == (161, 131, 2097152)
        assert (e["chunk-size-min"], e["chunk-size-avg"], e["chunk-size-max"]) == (2048, 8192, 32768)
        if c["seeds"]:
            assert (e["in-seed"], e["dedup-size-not-in-seed"], e["not-in-seed-nor-cache"]) == \
                (124, 80029, 7)
        else:
            assert (e["in-seed"], e["dedup-size-not-in-seed"]) == (0, 1114112)


def test_host_id_forms_agree():
    """An (n,32) array, a list of 32-byte IDs and an Index give the same rows."""
    import numpy as np
    from desync_amd import info
    ix = load_index("blob1.caibx")
    a = info._host_ids(ix)
    b = info._host_ids([c.ID for c in ix.Chunks])
    c = info._host_ids(np.array(a))
    assert a.shape == (161, 32) and np.array_equal(a, b) and np.array_equal(a, c)
    with pytest.raises(ValueError):
        info._host_ids([b"short"])
