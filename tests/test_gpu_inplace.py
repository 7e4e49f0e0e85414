"""dsx_assemble_inplace, dsx_chunk_keep and AssembleBlob(out=, have=) on the GPU:
version updates inside one buffer (insertions, a deletion, swapped halves,
scattered replacement from a DeviceStore, a zero run, a second seed, growth
and shrinkage) in every direction and at three address skews, every refusal
with the buffer compared byte for byte, and the resumed extract.  Cuts come
from the oracle, IDs from hashlib; the totals are compared with those the
numpy executor of inplace_ref.py derives from the schedule."""
import ctypes
import hashlib

import numpy as np
import pytest

import inplace_ref as ref
from oracle import oracle as o

pytestmark = pytest.mark.gpu

PAT = 0xA5
CANARY = 64
TILE = 65536
SIZES = (2048, 8192, 32768)
RNG = np.random.default_rng(20261020)


def _torch():
    import torch
    return torch


def _L():
    from desync_amd import _lib
    return _lib


def rand(n):
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


_INDEX = {}


def index_of(data, sizes=SIZES, algo="sha512_256"):
    """The Index of `data`: the oracle's cuts, hashlib's IDs (cached)."""
    from desync_amd.index import ChunkArray, FormatIndex, Index
    key = (hashlib.sha256(data).digest(), sizes, algo)
    if key not in _INDEX:
        ends = o.chunk_stream(np.frombuffer(data, np.uint8), *sizes) if data else np.zeros(0, np.uint64)
        ids, at = [], 0
        for e in ends.tolist():
            ids.append(hashlib.new(algo, data[at:e]).digest())
            at = e
        _INDEX[key] = (ends, b"".join(ids))
    ends, ids = _INDEX[key]
    return Index(FormatIndex(0, *sizes), ChunkArray(ends.copy(), ids))


def memory_store(index, data, without=()):
    from desync_amd import Chunk, MemoryStore
    st = MemoryStore()
    skip = {bytes(c.ID) for ix in without for c in ix.Chunks}
    for c in index.Chunks:
        if bytes(c.ID) not in skip:
            st.StoreChunk(Chunk(bytes(c.ID), data[c.Start:c.Start + c.Size]))
    return st


def to_dev(data):
    t = _torch().from_numpy(np.frombuffer(data, np.uint8).copy()).to("cuda:0")
    _torch().cuda.synchronize()
    return t


class Buffer:
    """`cap` bytes `skew` bytes behind a 16-byte boundary, between two canaries,
    holding `old` and PAT behind it."""

    def __init__(self, old, cap, skew):
        torch = _torch()
        self.raw = torch.full((CANARY + 48 + cap + CANARY,), PAT, dtype=torch.uint8, device="cuda:0")
        base = self.raw.data_ptr()
        self.off = CANARY + ((-(base + CANARY)) % 16) + skew
        self.view = self.raw[self.off:self.off + cap]
        assert self.view.data_ptr() % 16 == skew % 16
        self.view[:len(old)] = torch.from_numpy(np.frombuffer(old, np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        self.before = self.raw.cpu().numpy().copy()

    def host(self):
        _torch().cuda.synchronize()
        return self.raw.cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.host(), self.before)

    def check(self, new):
        """The buffer holds `new`; nothing behind it or around it changed."""
        got, want = self.host(), self.before.copy()
        want[self.off:self.off + len(new)] = np.frombuffer(new, np.uint8)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, ("first wrong byte at buffer offset", int(bad[0]) - self.off)


@pytest.fixture(scope="module")
def v1():
    """1.5 MiB: random bytes with a run of zeros (chunks of the full 32 KiB)."""
    a, b = rand(700_000), rand(1_572_864 - 700_000 - 150_000)
    return a + bytes(150_000) + b


def scattered(v1):
    v2 = bytearray(v1)
    for at in (5, 300_001, 555_555, 1_200_000, 1_500_000):
        v2[at:at + 3000] = rand(3000)
    return bytes(v2)


# name -> (v1 -> v2, what serves the store chunks, window)
CASES = {
    "insert-1": (lambda v: rand(1) + v, "memory", 65536),
    "insert-4097": (lambda v: rand(4097) + v, "memory", 131072),
    "insert-200000": (lambda v: rand(200_000) + v, "memory", 65536),
    "delete": (lambda v: v[70_001:], "memory", 131072),
    "swap": (lambda v: v[len(v) // 2:] + v[:len(v) // 2], "memory", 65536),
    "scattered": (scattered, "device", 131072),
    "zero-run": (lambda v: v[:300_000] + bytes(300_000) + v[300_000:900_000], "memory", 65536),
    "second-seed": (None, "memory", 131072),
    "grow": (lambda v: v + rand(500_000), "memory", 65536),
    "shrink": (lambda v: v[:700_001], "memory", 131072),
}
_SEED_BLOB = rand(600_000)


def make_v2(name, v1):
    if name == "second-seed":
        return v1[:600_000] + _SEED_BLOB[100_000:500_000] + v1[600_000:]
    return CASES[name][0](v1)


def run_update(dctx, old, new, kind, window, sizes=SIZES, extra_seed=None, skews=(0, 1, 19)):
    """old -> new inside one buffer, in the three direction modes at each skew."""
    import desync_amd
    from desync_amd import extract
    L = _L()
    i1, i2 = index_of(old, sizes), index_of(new, sizes)
    seeds, without = [], [i1]
    if extra_seed is not None:
        six = index_of(extra_seed, sizes)
        seeds, without = [desync_amd.NewIndexSeed(six, to_dev(extra_seed))], [i1, six]
    if kind == "device":
        store = desync_amd.DeviceStore(4 << 20, 4096, ctx=dctx)
        store.put_index(to_dev(new), i2)
        full = store
    else:
        store = memory_store(i2, new, without=without)  # only what neither the buffer nor a seed holds
        full = memory_store(i2, new, without=without[1:])
    # the yardstick: the out-of-place assembly of the same target
    ref_out, ref_stats = desync_amd.AssembleBlob(i2, full, seeds, ctx=dctx)
    assert ref_out.cpu().numpy().tobytes() == new
    cap = max(len(old), len(new)) + 4099
    n = len(i2.Chunks)
    for skew in skews:
        for flags in (0, L.DSX_INPLACE_ASCENDING, L.DSX_INPLACE_DESCENDING):
            buf = Buffer(old, cap, skew)
            trace = {}
            out, stats = extract.assemble_blob_inplace(i2, store, seeds, True, 0, dctx, True, buf.view, i1,
                                                       window, len(old), flags=flags, trace=trace)
            buf.check(new)
            assert out.data_ptr() == buf.view.data_ptr() and out.numel() == len(new)
            assert _torch().equal(out, ref_out)
            tot = stats["inplace"]
            print(f"inplace {len(old)}->{len(new)} window={window} skew={skew} flags={flags}: {tot} "
                  f"in-place={stats['chunks-in-place']} store={stats['chunks-from-store']} "
                  f"seeds={stats['chunks-from-seeds']} of {n}")
            assert stats["chunks-in-place"] + stats["chunks-from-store"] + stats["chunks-from-seeds"] == n
            assert stats["chunks-in-place"] == tot["kept_chunks"]
            if flags:
                assert tot["direction"] == flags
            ends = np.asarray([c.Start + c.Size for c in i2.Chunks], dtype=np.uint64)
            rc, la, sg, want = ref.schedule(trace["segs"], ends, trace["keep"], len(old), len(new), skew % 16,
                                            TILE, window, len(old), flags)
            assert rc == 0
            assert {k: tot[k] for k in ref.TOTAL_KEYS} == want
            if skew == skews[0]:  # (the executor costs a second at these sizes: once per direction)
                ref.same_totals(tot, ref.execute(la, sg, trace["segs"], ends, trace["keep"], len(old),
                                                 len(new), skew % 16, window, tot["stash_peak"]))
    for s in seeds:
        s.close()
    if kind == "device":
        store.close()
    return stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_version_update(dctx, v1, name):
    v2 = make_v2(name, v1)
    stats = run_update(dctx, v1, v2, CASES[name][1], CASES[name][2],
                       extra_seed=_SEED_BLOB if name == "second-seed" else None)
    if name == "scattered":
        assert stats["chunks-in-place"] > stats["chunks-total"] * 3 // 4
        assert 0 < stats["chunks-from-store"] <= 5 * 4
    if name == "zero-run":
        assert stats["chunks-from-store"] <= 6  # the zeros come from the null seed
    if name.startswith("insert"):
        assert stats["chunks-from-seeds"] > stats["chunks-total"] // 2  # moved inside the buffer


def test_chunks_larger_than_a_window(dctx):
    """16 / 64 / 256 KiB chunks, 64 KiB windows: a chunk spans several."""
    sizes = (16384, 65536, 262144)
    old = rand(1_000_000) + bytes(600_000) + rand(1_400_000)
    new = rand(4097) + old[:2_000_000] + old[2_300_000:]
    run_update(dctx, old, new, "memory", 65536, sizes=sizes, skews=(19,))


def test_identity(dctx, v1):
    import desync_amd
    i1 = index_of(v1)
    buf = Buffer(v1, len(v1) + 100, 3)
    out, stats = desync_amd.AssembleBlob(i1, desync_amd.MemoryStore(), ctx=dctx, out=buf.view, have=i1)
    assert buf.unchanged()
    assert stats["chunks-in-place"] == len(i1.Chunks) and stats["chunks-from-store"] == 0
    assert stats["inplace"]["launches"] == 0 and stats["inplace"]["written_bytes"] == 0


# ---- refusals: the buffer stays byte for byte what it was --------------------------------
def raw_inplace(ctx, rows, ends, buf_ptr, buf_cap, have_len, new_len, seeds=(), store=None, window=65536,
                stash=0, flags=0, keep=None):
    L = _L()
    segs = ref.make_segs(rows)
    ends = np.asarray(ends, dtype=np.uint64)
    ns = len(seeds)
    ptrs = (ctypes.c_void_p * max(1, ns))(*[p for p, _ in seeds])
    lens = (ctypes.c_uint64 * max(1, ns))(*[n for _, n in seeds])
    sp, sl = (store.ctypes.data, store.size) if store is not None else (None, 0)
    tot = L.InplaceTotals()
    rc = L.lib().dsx_assemble_inplace(
        ctx.h, ctypes.c_void_p(segs.ctypes.data if len(segs) else None), len(segs),
        ctypes.c_void_p(ends.ctypes.data), ends.size, None if keep is None else keep.ctypes.data, ptrs,
        lens, ns, ctypes.c_void_p(sp), sl, ctypes.c_void_p(buf_ptr), buf_cap, have_len, new_len, window,
        stash, flags, ctypes.byref(tot))
    msg = L.lib().dsx_last_error(ctx.h)
    return rc, (msg.decode() if msg else ""), tot


def test_refusals_leave_the_buffer_alone(dctx, v1):
    import desync_amd
    L = _L()
    half = 512 * 1024
    old = v1[:2 * half]
    buf = Buffer(old, 2 * half + 5000, 1)
    ptr, cap = buf.view.data_ptr(), buf.view.numel()
    ends = [half, 2 * half]
    swap = [[0, half, half, 0, 1, ref.SELF], [half, half, 0, 1, 1, ref.SELF]]
    # the stash: swapped halves need one half
    rc, msg, tot = raw_inplace(dctx, swap, ends, ptr, cap, 2 * half, 2 * half, stash=half - 1)
    assert rc == L.DSX_E_CAPACITY and tot.stash_peak == half and "DSX_" not in msg and buf.unchanged()
    # an external seed inside the buffer
    good = [[0, half, 0, 0, 1, 0], [half, half, 0, 1, 1, ref.SELF]]
    other = to_dev(old)
    rc, msg, _ = raw_inplace(dctx, good, ends, ptr, cap, 2 * half, 2 * half, seeds=[(ptr + cap - 10, half)])
    assert rc == L.DSX_E_INVAL and "overlaps seed 0" in msg and buf.unchanged()
    # lengths beyond the capacity
    rc, msg, _ = raw_inplace(dctx, good, ends, ptr, 2 * half - 1, half, 2 * half, seeds=[(other.data_ptr(), half)])
    assert rc == L.DSX_E_INVAL and "new_len" in msg and buf.unchanged()
    rc, msg, _ = raw_inplace(dctx, good, ends, ptr, cap, cap + 1, 2 * half, seeds=[(other.data_ptr(), half)])
    assert rc == L.DSX_E_INVAL and "have_len" in msg and buf.unchanged()
    # bad segments, each named
    for rows, what in (
            ([[0, half, 0, 0, 1, 1], good[1]], "segment 0: source names no seed"),
            ([[0, half, 1, 0, 1, 0], good[1]], "segment 0: src_off + bytes is beyond its source"),
            ([good[0], [half, half, half + 1, 1, 1, ref.SELF]], "segment 1: src_off + bytes is beyond the old"),
            ([good[0], [half - 1, half, 0, 1, 1, ref.SELF]], "segment 1: dst_off is below"),
            ([good[0], [half, half + 1, 0, 1, 1, ref.SELF]], "segment 1: "),
            ([good[0], [half, half, 0, 1, 1, -7]], "segment 1: source is neither")):
        rc, msg, _ = raw_inplace(dctx, rows, ends, ptr, cap, 2 * half, 2 * half, seeds=[(other.data_ptr(), half)])
        assert rc == L.DSX_E_INVAL and what in msg and buf.unchanged(), (rows, msg)
    rc, msg, _ = raw_inplace(dctx, good, ends, ptr, cap, 2 * half, 2 * half, seeds=[(other.data_ptr(), half)],
                             window=65536 + 16)
    assert rc == L.DSX_E_INVAL and "window" in msg and buf.unchanged()
    rc, _, _ = raw_inplace(dctx, good, ends, ptr, cap, 2 * half, 2 * half, seeds=[(other.data_ptr(), half)], flags=1)
    assert rc == L.DSX_E_INVAL and buf.unchanged()
    # through AssembleBlob: StorageError carries the needed stash
    new = old[half:] + old[:half]
    i1, i2 = index_of(old), index_of(new)
    with pytest.raises(desync_amd.StorageError) as e:
        desync_amd.AssembleBlob(i2, memory_store(i2, new, without=[i1]), ctx=dctx, out=buf.view, have=i1,
                                window=65536, stash=4096)
    assert e.value.needed > 4096 and e.value.code == L.DSX_E_CAPACITY and buf.unchanged()
    # ... and with that stash the call goes through
    out, stats = desync_amd.AssembleBlob(i2, memory_store(i2, new, without=[i1]), ctx=dctx, out=buf.view,
                                         have=i1, window=65536, stash=e.value.needed)
    buf.check(new)
    assert stats["inplace"]["stash_peak"] == e.value.needed


def test_public_assemble_still_refuses(dctx, v1):
    """dsx_assemble knows no SELF source and no output that overlaps a seed."""
    L = _L()
    buf = Buffer(v1[:100_000], 100_000, 0)
    ptr = buf.view.data_ptr()
    seed = to_dev(v1[:50_000])
    ptrs = (ctypes.c_void_p * 1)(seed.data_ptr())
    lens = (ctypes.c_uint64 * 1)(50_000)
    segs = ref.make_segs([[0, 1000, 5000, 0, 1, ref.SELF]])
    rc = L.lib().dsx_assemble(dctx.h, ctypes.c_void_p(segs.ctypes.data), 1, ptrs, lens, 1, None, 0,
                              ctypes.c_void_p(ptr), 100_000, 0)
    assert rc == L.DSX_E_INVAL and b"segment 0: source is neither" in L.lib().dsx_last_error(dctx.h)
    segs = ref.make_segs([[0, 1000, 5000, 0, 1, 0]])
    ptrs = (ctypes.c_void_p * 1)(ptr + 50_000)
    rc = L.lib().dsx_assemble(dctx.h, ctypes.c_void_p(segs.ctypes.data), 1, ptrs, lens, 1, None, 0,
                              ctypes.c_void_p(ptr), 100_000, 0)
    assert rc == L.DSX_E_INVAL and b"the output overlaps seed 0" in L.lib().dsx_last_error(dctx.h)
    assert buf.unchanged()


# ---- the resumed extract: dsx_chunk_keep ----------------------------------------------------
def test_chunk_keep_and_resume(dctx, v1):
    import desync_amd
    from desync_amd import extract
    v2 = scattered(v1)
    masks = {}
    for algo, code in (("sha512_256", "sha512-256"), ("sha256", "sha256")):
        ix = index_of(v2, algo=algo)
        ends = np.asarray([c.Start + c.Size for c in ix.Chunks], dtype=np.uint64)
        ids = np.frombuffer(b"".join(bytes(c.ID) for c in ix.Chunks), np.uint8).reshape(-1, 32)
        n = len(ends)
        pick = np.random.default_rng(5).random(n) < 0.5
        content = bytearray(rand(len(v2)))  # noise, and v2's chunks at a random half of the positions
        at = 0
        for i, e in enumerate(ends.tolist()):
            if pick[i]:
                content[at:e] = v2[at:e]
            at = e
        k = int(np.flatnonzero(pick)[-1])  # the last chunk that is there is cut by have_len
        have_len = int(ends[k]) - 5
        want = pick & (ends <= have_len)
        assert pick[k] and not want[k] and want.sum() > 10
        buf = Buffer(bytes(content), len(v2) + 777, 19)
        got = extract.chunk_keep(buf.view.data_ptr(), have_len, ends, ids, ctx=dctx, algo=code)
        assert np.array_equal(got.astype(bool), want), np.flatnonzero(got.astype(bool) != want)
        assert buf.unchanged()
        masks[algo] = (want, buf, have_len, ix, ends)
    # AssembleBlob completes the buffer (the package's digest is SHA-512/256)
    want, buf, have_len, ix, ends = masks["sha512_256"]
    sizes = np.diff(ends, prepend=np.uint64(0))
    out, stats = desync_amd.AssembleBlob(ix, memory_store(ix, v2), ctx=dctx, out=buf.view, have=have_len,
                                         window=131072)
    buf.check(v2)
    assert stats["chunks-in-place"] == int(want.sum())
    assert stats["inplace"]["written_bytes"] == int(sizes[~want].sum())
    assert stats["seeds"] == 1  # the null seed alone: no self seed


def test_old_index_that_lies_is_skipped(dctx, v1):
    """have=Index whose index claims, at one place, a chunk of the target that
    is not there: Plan.Validate marks the self seed invalid, the call goes on
    as for unknown content and the result is still the target."""
    import desync_amd
    from desync_amd.index import ChunkArray, FormatIndex, Index
    v2 = rand(4097) + v1
    i1, i2 = index_of(v1), index_of(v2)
    old_ids = {bytes(c.ID) for c in i1.Chunks}
    fresh = next(c for c in i2.Chunks if bytes(c.ID) not in old_ids)
    ends = np.asarray([c.Start + c.Size for c in i1.Chunks], dtype=np.uint64)
    ids = bytearray(b"".join(bytes(c.ID) for c in i1.Chunks))
    ids[32 * 7:32 * 8] = bytes(fresh.ID)
    liar = Index(FormatIndex(0, *SIZES), ChunkArray(ends, bytes(ids)))
    buf = Buffer(v1, len(v2) + 10, 1)
    out, stats = desync_amd.AssembleBlob(i2, memory_store(i2, v2), ctx=dctx, out=buf.view, have=liar)
    buf.check(v2)
    honest = Buffer(v1, len(v2) + 10, 1)
    _, hstats = desync_amd.AssembleBlob(i2, memory_store(i2, v2), ctx=dctx, out=honest.view, have=i1)
    honest.check(v2)
    # the fallback shows: no self seed, everything that moved comes from the store instead
    assert stats["seeds"] == 1 and hstats["seeds"] == 2
    assert stats["chunks-from-store"] > hstats["chunks-from-store"]
    assert hstats["chunks-from-seeds"] > stats["chunks-from-seeds"]
