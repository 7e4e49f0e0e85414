"""dsx_store_prune (desync_amd.store: Prune, RemoveChunk, Verify(repair)): what
can be checked without a GPU -- the export, the struct layout, the NULL
refusals that come before any device work, and the model (store_prune_ref.py)
the GPU tests compare with, on the goldens."""
import ctypes
import os

import numpy as np

import store_prune_ref
from desync_amd import _lib
from desync_amd.index import IndexFromReader

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_entry_point_is_bound_and_exported():
    assert "dsx_store_prune" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "dsx_store_prune")
    assert _lib.DSX_PRUNE_REMOVE == 512


def test_struct_layout():
    assert ctypes.sizeof(_lib.StorePruneTotals) == 64
    assert [n for n, _ in _lib.StorePruneTotals._fields_] == \
        ["entries", "kept", "kept_bytes", "removed", "removed_bytes", "moved", "moved_bytes", "unmatched"]


def test_abi_version_stays():
    assert _lib.lib().dsx_abi_version() == 5


def test_null_context_or_store_is_invalid():
    L = _lib.lib()
    ids = (ctypes.c_uint8 * 32)()
    tot = _lib.StorePruneTotals()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the other handle is NULL
    for flags in (0, _lib.DSX_PRUNE_REMOVE):
        assert L.dsx_store_prune(None, fake, ids, 1, 0, ctypes.byref(tot), flags) == _lib.DSX_E_INVAL
        assert L.dsx_store_prune(fake, None, ids, 1, 0, ctypes.byref(tot), flags) == _lib.DSX_E_INVAL
        assert L.dsx_store_prune(None, None, None, 0, 0, None, flags) == _lib.DSX_E_INVAL


def test_python_layer_has_the_methods():
    import desync_amd
    for name in ("Prune", "RemoveChunk", "Verify"):
        assert callable(getattr(desync_amd.DeviceStore, name)), name


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _index(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        ix = IndexFromReader(f)
    ids = np.frombuffer(b"".join(bytes(c.ID) for c in ix.Chunks), np.uint8).reshape(-1, 32)
    ends = np.cumsum([c.Size for c in ix.Chunks]).astype(np.uint64)
    return ids, ends


def _both():
    m = store_prune_ref.Store(4 << 20, 1024)
    for name in ("blob1", "blob2"):
        m.put(_golden(name), *_index(name + ".caibx"))
    assert m.counts()["chunks"] == 138
    return m


def _holds_every_chunk_of(m, name):
    blob = _golden(name)
    ids, ends = _index(name + ".caibx")
    lo = 0
    for cid, hi in zip(ids, ends.tolist()):
        assert m.get(cid.tobytes()) == blob[lo:hi]
        lo = hi


def test_model_pruned_to_blob2():
    m = _both()
    used = len(m.arena)
    wanted = {r.tobytes() for r in _index("blob2.caibx")[0]}
    first_gone = next(e for e, cid in enumerate(m.ids) if cid not in wanted)
    t = m.prune(_index("blob2.caibx")[0])
    assert (t["entries"], t["kept"], t["removed"], t["unmatched"]) == (138, 131, 7, 0)
    assert t["kept_bytes"] + t["removed_bytes"] == used and t["kept_bytes"] == len(m.arena)
    # every survivor behind the first chunk dropped moves (no golden chunk is empty)
    assert t["moved"] == 131 - first_gone
    assert t["moved_bytes"] == len(m.arena) - (m.ends[first_gone - 1] if first_gone else 0)
    assert m.counts()["chunks"] == 131 and m.ends[-1] == len(m.arena)
    _holds_every_chunk_of(m, "blob2")


def test_model_pruned_to_blob1():
    m = _both()
    t = m.prune(_index("blob1.caibx")[0])
    assert (t["kept"], t["removed"], t["removed_bytes"]) == (131, 7, 80029)
    assert (t["moved"], t["moved_bytes"]) == (0, 0)  # the seven removed entries are the last
    assert len(m.arena) == 1114112
    _holds_every_chunk_of(m, "blob1")


def test_model_pruned_to_both_moves_nothing():
    m = _both()
    before = (list(m.ids), list(m.ends), bytes(m.arena), dict(m.pos))
    both = np.concatenate([_index("blob1.caibx")[0], _index("blob2.caibx")[0]])
    t = m.prune(both)
    assert t == {"entries": 138, "kept": 138, "kept_bytes": len(m.arena), "removed": 0, "removed_bytes": 0,
                 "moved": 0, "moved_bytes": 0, "unmatched": 0}
    assert (m.ids, m.ends, bytes(m.arena), m.pos) == before


def test_model_remove_mode_and_unmatched():
    m = _both()
    ids1, ids2 = _index("blob1.caibx")[0], _index("blob2.caibx")[0]
    keep = _both()
    tk = keep.prune(ids2)
    only1 = np.stack([r for r in ids1 if r.tobytes() not in {x.tobytes() for x in ids2}])
    absent = np.arange(64, dtype=np.uint8).reshape(2, 32)
    tr = m.prune(np.concatenate([only1, only1[:3], absent, absent[:1]]), remove=True)
    assert tr["unmatched"] == 2 and tk["unmatched"] == 0
    assert {k: v for k, v in tr.items() if k != "unmatched"} == {k: v for k, v in tk.items() if k != "unmatched"}
    assert (m.ids, m.ends, m.arena, m.pos) == (keep.ids, keep.ends, keep.arena, keep.pos)
    assert m.prune(np.empty((0, 32), np.uint8), remove=True)["removed"] == 0
    assert m.prune(np.empty((0, 32), np.uint8))["removed"] == 131 and not m.arena and not m.pos
