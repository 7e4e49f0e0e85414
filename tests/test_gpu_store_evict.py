"""dsx_store_track, dsx_store_touch, dsx_store_stamps and dsx_store_evict on the
GPU against store_evict_ref's model: after every call the evicted IDs, the
totals, the entries, the ends, the stamps, the clock and every used arena byte
must equal the model's.  The stores are small and shaped so that every path of
the selection runs: several workgroups of 256 entries with a partial last one,
a boundary class that spans workgroups, empty entries at the boundary, needs
bound by chunks and by bytes, stamps of 1 to 8 bytes, pins in host and device
memory.  Every refusal is one the library gives before any device work."""
import ctypes
import hashlib

import numpy as np
import pytest

import store_evict_ref as ref
import store_ref

pytestmark = pytest.mark.gpu

WINDOW = 65536  # the compaction's smallest scratch: an eviction here moves many windows


def _L():
    from desync_amd import _lib
    return _lib


def _torch():
    import torch
    return torch


def _dev(arr):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()  # (torch's stream is not the context's)
    return t


def chunks(seed, n, hi, zeros=(), lo=0):
    """n chunks of lo..hi bytes (those in `zeros` empty) with random IDs -> (blob, ids, ends)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, n)
    sizes[list(zeros)] = 0
    ends = np.cumsum(sizes).astype(np.uint64)
    blob = rng.integers(0, 256, int(ends[-1]) + 1, dtype=np.uint8)
    return blob, rng.integers(0, 256, (n, 32), dtype=np.uint8), ends


class Pair:
    """A DeviceStore and the model, given the same calls."""

    def __init__(self, dctx, arena, max_chunks, track=True):
        import desync_amd
        self.gpu = desync_amd.DeviceStore(arena, max_chunks, ctx=dctx, track=track)
        self.model = ref.Store(arena, max_chunks, track=track)

    def close(self):
        self.gpu.close()

    def put(self, blob, ids, ends):
        want = self.model.put(blob.tobytes(), ids, ends)
        assert self.gpu.put(_dev(blob), ids, ends) == want

    def track(self):
        self.model.track()
        self.gpu.Track()

    def touch(self, ids, stamp=None, device=False):
        want = self.model.touch(ids, stamp)
        assert self.gpu.Touch(_dev(ids) if device else ids, stamp) == want

    def evict(self, need_bytes=0, need_chunks=0, pin=None, window=WINDOW, dry=False, device=False):
        """Both evict; the totals and the victims must agree -> the totals, or
        None when both refuse for capacity (with equal totals)."""
        L = _L()
        mpin = np.empty((0, 32), np.uint8) if pin is None else pin
        gpin = _dev(pin) if device and pin is not None else pin
        try:
            want = self.model.evict(need_bytes, need_chunks, mpin, dry)
        except store_ref.Capacity as e:
            with pytest.raises(L.DsxError) as exc:
                self.gpu.Evict(need_bytes, need_chunks, gpin, window, dry)
            assert exc.value.code == L.DSX_E_CAPACITY and exc.value.totals == e.totals
            return None
        got = self.gpu.Evict(need_bytes, need_chunks, gpin, window, dry)
        got["ids"] = got["ids"].tobytes()
        assert got == want
        return want

    def need_for(self, k, pin=()):
        """The byte need whose shortest prefix is the first k of the use order."""
        pinned = {r.tobytes() for r in np.asarray(pin, np.uint8).reshape(-1, 32)}
        order = self.model.order(pinned)
        assert k >= 1 and self.model.size(order[k - 1]) > 0, "the k-th victim must bring bytes"
        return self.model.arena_bytes - len(self.model.arena) + sum(self.model.size(e) for e in order[:k])

    def same(self):
        assert gpu_state(self.gpu) == model_state(self.model)


def gpu_state(s, whole=False):
    from desync_amd.encrypt import _download
    ids, ends = s.entries()
    ptr, used = s.arena()
    c = s.counts()
    out = {"counts": c, "ids": ids.tobytes(), "ends": [int(e) for e in ends],
           "arena": _download(s.ctx, ptr, c["arena_bytes"] if whole else used).tobytes()}
    if s.tracked:
        stamps, clock = s.stamps()
        out.update(stamps=[int(t) for t in stamps], clock=clock)
    return out


def model_state(m):
    out = {"counts": m.counts(), "ids": b"".join(m.ids), "ends": [int(e) for e in m.ends], "arena": bytes(m.arena)}
    if m.tracked:
        out.update(stamps=[int(t) for t in m.stamps], clock=int(m.clock))
    return out


@pytest.fixture
def pair(dctx):
    made = []

    def make(arena, max_chunks, track=True):
        made.append(Pair(dctx, arena, max_chunks, track))
        return made[-1]
    yield make
    for p in made:
        p.close()


# ---- 1. order ------------------------------------------------------------------------------
def test_order(dctx, pair):
    """1,500 entries of 0-4 KiB from five puts (six workgroups, the last
    partial), seeded touches, then an eviction whose byte need ends in the
    middle of a stamp class; a twin store pruned of the model's victims has the
    same arena, IDs and ends."""
    import desync_amd
    p = pair(4 << 20, 1600)
    twin = desync_amd.DeviceStore(4 << 20, 1600, ctx=dctx)
    blob, ids, ends = chunks(1, 1500, 4096)
    for k in range(5):
        lo, hi = 300 * k, 300 * (k + 1)
        base = int(ends[lo - 1]) if lo else 0
        part = blob[base:int(ends[hi - 1]) + 1]
        p.put(part, ids[lo:hi], ends[lo:hi] - np.uint64(base))
        twin.put(_dev(part), ids[lo:hi], ends[lo:hi] - np.uint64(base))
    rng = np.random.default_rng(2)
    for _ in range(3):
        p.touch(ids[rng.random(1500) < 0.3])
    p.same()
    order = p.model.order(set())
    k = next(k for k in range(400, 1200) if p.model.stamps[order[k - 1]] == p.model.stamps[order[k]]
             == p.model.stamps[order[k - 40]] == p.model.stamps[order[k + 40]] and p.model.size(order[k - 1]))
    tot = p.evict(need_bytes=p.need_for(k))
    assert tot["evicted"] == k and tot["moved_bytes"] > 4 * WINDOW
    assert tot["cutoff"] in p.model.stamps  # the class is cut: some of it went, some of it stays
    p.same()
    twin._prune(np.frombuffer(tot["ids"], np.uint8).reshape(-1, 32), remove=True, window=WINDOW)
    a, b = gpu_state(twin), gpu_state(p.gpu)
    assert (a["ids"], a["ends"], a["arena"]) == (b["ids"], b["ends"], b["arena"])
    twin.close()


# ---- 2. ties ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", ["bytes", "chunks"])
def test_ties(pair, bound):
    """700 entries of one put, all with one stamp: the lowest entry numbers go
    first, the class spans three workgroups, and entries 515-525 are empty.
    bytes: the need is met by entry 514, so the empty ones behind it stay;
    chunks: the prefix ends among the empty ones."""
    p = pair(2 << 20, 700)
    blob, ids, ends = chunks(3, 700, 2048, zeros=range(515, 526), lo=1)
    p.put(blob, ids, ends)
    assert set(p.model.stamps) == {1}
    if bound == "bytes":
        tot = p.evict(need_bytes=p.need_for(515))
        assert tot["evicted"] == 515
    else:
        tot = p.evict(need_chunks=520)
        assert tot["evicted"] == 520
    assert tot["ids"] == ids[:tot["evicted"]].tobytes() and tot["cutoff"] == 1
    p.same()


# ---- 3. two needs ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chunks", "bytes", "both"])
def test_two_needs(pair, case):
    """Bound by need_chunks, by need_bytes, and by both at different prefixes."""
    p = pair(1 << 20, 640)
    blob, ids, ends = chunks(4, 600, 1500, lo=1)
    p.put(blob[:int(ends[299]) + 1], ids[:300], ends[:300])
    p.put(blob[int(ends[299]):], ids[300:], ends[300:] - ends[299])
    p.touch(ids[::3])
    m = p.model
    order = m.order(set())
    room_b, room_c = m.arena_bytes - len(m.arena), m.max_chunks - len(m.ids)
    k_chunks, k_bytes = 333, 120
    need_c = room_c + k_chunks if case != "bytes" else 0
    need_b = p.need_for(k_bytes) if case != "chunks" else 0
    if case == "both":  # the bytes are met first, the chunks later: the longer prefix is the answer
        assert sum(m.size(e) for e in order[:k_chunks]) + room_b > need_b
    tot = p.evict(need_bytes=need_b, need_chunks=need_c)
    assert tot["evicted"] == (k_bytes if case == "bytes" else k_chunks)
    p.same()
    if case == "both":  # and the other way round: few chunks, many bytes
        order = m.order(set())
        need_b = p.need_for(150)
        tot = p.evict(need_bytes=need_b, need_chunks=m.max_chunks - len(m.ids) + 10)
        assert tot["evicted"] == 150
        p.same()


# ---- 4. wide stamps ----------------------------------------------------------------------------
WIDE = {
    1: (1,),
    2: (0x100, 0x7F, 0xFF, 2),
    5: (0x100000007, 0x100000003, 0xFFFF0000, 0xFFFE0000, 0x1000000, 5),
    8: (0xFFFFFFFFFFFFFFF0, 0x8000000000000000, 0x7FFFFF0000000000, 0x7FFFFE0000000000, 0x10000000000, 0x100),
}


@pytest.mark.parametrize("passes", sorted(WIDE))
def test_wide_stamps(pair, passes):
    """Caller-given stamps of 1, 2, 5 and 8 bytes: the descent runs that many
    passes, and the cutoff is a class whose stamp differs from its neighbours'
    in a middle byte.  The store is tracked after its put: the entries start
    at stamp 0."""
    p = pair(1 << 20, 320, track=False)
    blob, ids, ends = chunks(5 + passes, 300, 1000)
    p.put(blob, ids, ends)
    p.track()
    p.same()
    stamps = WIDE[passes]
    rng = np.random.default_rng(passes)
    group = rng.integers(0, len(stamps) + 1, 300)  # the last group keeps stamp 0
    for g, t in enumerate(stamps):
        p.touch(ids[group == g], stamp=t, device=bool(g % 2))
    assert p.model.clock == max(stamps) and p.gpu.stamps()[1] == max(stamps)
    order = p.model.order(set())
    target = sorted(stamps)[len(stamps) // 2]  # a class in the middle of the order
    inside = [k for k in range(1, 300) if p.model.stamps[order[k - 1]] == target == p.model.stamps[order[k]]
              and p.model.size(order[k - 1])]
    tot = p.evict(need_bytes=p.need_for(inside[len(inside) // 2]))
    assert tot["cutoff"] == target
    p.same()
    tot = p.evict(need_chunks=p.model.max_chunks - 5)  # down to five entries: the cutoff moves up
    assert tot["kept"] == 5
    p.same()


# ---- 5. pins ---------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_pins(pair, device):
    """The oldest entries are pinned and survive; a pinned ID the store lacks is
    ignored; a need the unpinned entries cannot meet is DSX_E_CAPACITY and
    leaves every buffer as it was."""
    p = pair(1 << 20, 600)
    blob, ids, ends = chunks(6, 520, 1500, lo=1)
    p.put(blob, ids, ends)
    p.touch(ids[260:])
    absent = np.random.default_rng(7).integers(0, 256, (2, 32), dtype=np.uint8)
    pin = np.concatenate([ids[:40], absent, ids[10:20], ids[400:410]])
    before = gpu_state(p.gpu, whole=True)
    assert p.evict(need_bytes=(1 << 20) - 1000, pin=pin, device=device) is None  # the pins hold more than that
    assert gpu_state(p.gpu, whole=True) == before
    tot = p.evict(need_bytes=p.need_for(300, pin), pin=pin, device=device)
    assert tot["pinned"] == 50 and tot["evicted"] == 300
    assert tot["ids"] == np.concatenate([ids[40:260], ids[260:340]]).tobytes()
    assert p.gpu.entries()[0][:40].tobytes() == ids[:40].tobytes()
    p.same()


# ---- 6. nothing to do, dry -------------------------------------------------------------------
def test_nothing_and_dry(pair):
    """Room that is there already: no buffer changes.  DSX_EVICT_DRY reports the
    victims of the real call that follows and moves nothing."""
    p = pair(1 << 20, 400)
    blob, ids, ends = chunks(8, 300, 1200)
    p.put(blob, ids, ends)
    p.touch(ids[::2])
    before = gpu_state(p.gpu, whole=True)
    room = (1 << 20) - int(ends[-1])
    tot = p.evict(need_bytes=room, need_chunks=100, pin=ids[:5])
    assert tot["evicted"] == 0 and tot["pinned"] == 5 and tot["evictable"] == 295 and tot["ids"] == b""
    assert gpu_state(p.gpu, whole=True) == before
    dry = p.evict(need_bytes=room + 90000, need_chunks=130, dry=True)
    assert dry["evicted"] > 0 and dry["moved_bytes"] > 0
    assert gpu_state(p.gpu, whole=True) == before
    real = p.evict(need_bytes=room + 90000, need_chunks=130)
    assert real == dry
    p.same()


# ---- 7. after ----------------------------------------------------------------------------------
def test_after(pair):
    """locate, read_ranges and Verify answer for the compacted store; a later put
    reuses the room and takes the next clock value."""
    from desync_amd.readseeker import read_ranges_raw
    torch = _torch()
    p = pair(256 << 10, 300)
    blob, _, ends = chunks(9, 200, 1000)
    raw, lo, sums = blob.tobytes(), 0, []
    for e in ends.tolist():
        sums.append(hashlib.new("sha512_256", raw[lo:e]).digest())
        lo = e
    ids = np.frombuffer(b"".join(sums), np.uint8).reshape(-1, 32)
    p.put(blob, ids, ends)
    p.touch(ids[50:120])
    tot = p.evict(need_chunks=300 - 200 + 90)
    assert tot["evicted"] == 90
    p.same()
    offs, sizes, miss = p.gpu.locate(ids)
    want = p.model.locate(ids)
    assert ([int(o) for o in offs], [int(z) for z in sizes], miss) == want and miss == 90
    assert p.gpu.verify_entries() == []
    kept = np.array([i for i in range(200) if sums[i] in p.model.pos])
    kends = np.cumsum([len(p.model.get(sums[i])) for i in kept], dtype=np.uint64)
    total = int(kends[-1])
    out = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rt = read_ranges_raw(p.gpu, ids[kept], kends, [(0, total)], out, 0, bytes(32), 0, n=len(kept))
    assert rt["missing"] == 0 and rt["wrong_size"] == 0
    assert out.cpu().numpy().tobytes() == b"".join(p.model.get(sums[i]) for i in kept)
    clock = p.model.clock
    blob2, ids2, ends2 = chunks(10, 80, 1000)
    ids2[5] = ids[60]  # a chunk the store holds: present, and stamped too
    p.put(blob2, ids2, ends2)
    assert p.model.clock == clock + 1
    p.same()


# ---- 8. refusals -------------------------------------------------------------------------------
def test_refusals(dctx):
    """Before any device work: an untracked store (DSX_E_STATE with a text), a
    store of another context, unknown flag bits, n_pin beyond the limit.  And an
    untracked store is charged nothing for stamps."""
    import desync_amd
    L = _L()
    lib = L.lib()
    before = dctx.stats().device_bytes
    plain = desync_amd.DeviceStore(1 << 16, 1000, ctx=dctx)
    mid = dctx.stats().device_bytes
    tracked = desync_amd.DeviceStore(1 << 16, 1000, ctx=dctx, track=True)
    after = dctx.stats().device_bytes
    assert (after - mid) - (mid - before) == 1000 * 8
    tot, miss, clock = L.StoreEvictTotals(), ctypes.c_uint64(), ctypes.c_uint64()
    one = np.zeros((1, 32), np.uint8)
    assert lib.dsx_store_touch(dctx.h, plain.h, one.ctypes.data, 1, 0, ctypes.byref(miss), 0) == L.DSX_E_STATE
    assert b"track" in lib.dsx_last_error(dctx.h)
    assert lib.dsx_store_evict(dctx.h, plain.h, 1, 0, None, 0, None, 0, 0, ctypes.byref(tot), 0) == L.DSX_E_STATE
    assert b"track" in lib.dsx_last_error(dctx.h)
    assert lib.dsx_store_stamps(dctx.h, plain.h, 0, 0, None, ctypes.byref(clock), 0) == L.DSX_E_STATE
    with pytest.raises(L.DsxError):
        plain.Touch(one)
    other = L.Context(0)
    try:
        foreign = desync_amd.DeviceStore(1 << 16, 100, ctx=other, track=True)
        for rc in (lib.dsx_store_track(dctx.h, foreign.h),
                   lib.dsx_store_touch(dctx.h, foreign.h, one.ctypes.data, 1, 0, None, 0),
                   lib.dsx_store_stamps(dctx.h, foreign.h, 0, 0, None, None, 0),
                   lib.dsx_store_evict(dctx.h, foreign.h, 1, 0, None, 0, None, 0, 0, ctypes.byref(tot), 0)):
            assert rc == L.DSX_E_INVAL
        foreign.close()
    finally:
        other.close()
    h = tracked.h
    assert lib.dsx_store_evict(dctx.h, h, 1, 0, None, 0, None, 0, 0, ctypes.byref(tot), 1) == L.DSX_E_INVAL
    assert lib.dsx_store_evict(dctx.h, h, 1, 0, None, 0, None, 0, 0, ctypes.byref(tot), L.DSX_PRUNE_REMOVE) == L.DSX_E_INVAL
    assert lib.dsx_store_evict(dctx.h, h, 1, 0, one.ctypes.data, 0xFFFFFFF1, None, 0, 0, ctypes.byref(tot), 0) == L.DSX_E_INVAL
    assert lib.dsx_store_evict(dctx.h, h, 1, 0, None, 3, None, 0, 0, ctypes.byref(tot), 0) == L.DSX_E_INVAL
    assert lib.dsx_store_touch(dctx.h, h, one.ctypes.data, 1, 0, None, L.DSX_EVICT_DRY) == L.DSX_E_INVAL
    assert lib.dsx_store_touch(dctx.h, h, None, 0, 0, ctypes.byref(miss), 0) == 0  # n == 0: the clock stays
    assert tracked.stamps()[1] == 0
    assert lib.dsx_store_track(dctx.h, h) == 0 and dctx.stats().device_bytes == after  # idempotent
    with pytest.raises(L.DsxError) as exc:  # an empty store has nothing to evict
        tracked.Evict(need_bytes=(1 << 16) + 1)
    assert exc.value.code == L.DSX_E_CAPACITY and exc.value.totals["evictable"] == 0
    plain.close()
    tracked.close()


# ---- 9. life -------------------------------------------------------------------------------------
class GpuLife:
    def __init__(self, dctx):
        import desync_amd
        self.ctx = dctx
        self.stores = {"A": desync_amd.DeviceStore(ref.ARENA, ref.CHUNKS, ctx=dctx, track=True),
                       "B": desync_amd.DeviceStore(ref.ARENA // 2, ref.CHUNKS // 2, ctx=dctx, track=True)}
        self.flip = 0

    def close(self):
        for s in self.stores.values():
            s.close()

    def state(self, name):
        return gpu_state(self.stores[name])

    def _ids(self, ids):
        self.flip += 1
        return _dev(ids) if self.flip % 2 and len(ids) else ids  # device memory every other time

    def apply(self, op):
        L = _L()
        kind, s = op["op"], self.stores[op["store"]]
        try:
            if kind == "put":
                blob, ids, ends = ref.pool().gather(op["picks"])
                return {"refused": None, "totals": s.put(_dev(blob), self._ids(ids), ends)}
            if kind == "copy":
                src = self.stores[op["src"]]
                tot = s.CopyFrom(src) if op["ids"] is None else s.CopyFrom(src, self._ids(op["ids"]))
                return {"refused": "missing" if tot["missing"] else None, "totals": tot}
            if kind == "evict":
                tot = s.Evict(op["need_bytes"], op["need_chunks"], self._ids(op["pin"]), WINDOW, op["dry"])
                tot["ids"] = tot["ids"].tobytes()
                return {"refused": None, "totals": tot}
        except L.DsxError as e:
            assert e.code == L.DSX_E_CAPACITY, e
            return {"refused": "capacity", "totals": e.totals}
        if kind == "touch":
            return {"missing": s.Touch(self._ids(op["ids"]), op["stamp"])}
        if kind == "prune":
            return {"totals": s._prune(op["ids"], remove=op["remove"], window=WINDOW)}
        if kind == "grow":
            return {"totals": s.Grow(op["arena_bytes"], op["max_chunks"])}
        raise ValueError(kind)


@pytest.mark.parametrize("seed", ref.LIFE_SEEDS)
def test_life(dctx, seed):
    """Sixty mixed calls -- put, copy, a copy of every entry into an emptied
    store, touch, evict, prune, remove and Grow -- with every buffer of both
    stores compared with the model after every call.  test_store_evict_host.py
    shows that these scripts tell the planted-mistake models from the true one."""
    backend = GpuLife(dctx)
    try:
        ref.drive(seed, backend)
    finally:
        backend.close()


# ---- 10. Python: a store that evicts by itself ---------------------------------------------------
def test_python_bounded(dctx):
    """A DeviceStore(evict=True) of 1 MiB takes puts of 256 KiB without end and
    holds the most recent ones; a chunk present and named by the put that forces
    the eviction survives it; a put larger than the arena is refused and leaves
    the store unchanged; a Cache with such a local store serves more distinct
    chunks than the local store holds."""
    import desync_amd
    L = _L()
    s = desync_amd.DeviceStore(1 << 20, 4096, ctx=dctx, evict=True)
    assert s.tracked
    puts = [chunks(100 + k, 128, 4096) for k in range(9)]
    keep = puts[0][1][3].copy()  # a chunk of the first put, named again by every later one
    size3 = int(puts[0][2][3] - puts[0][2][2])
    for k, (blob, ids, ends) in enumerate(puts):
        if k:  # the same bytes under the same ID, appended to the put
            data = puts[0][0][int(puts[0][2][2]):int(puts[0][2][3])]
            blob = np.concatenate([blob[:int(ends[-1])], data, np.zeros(1, np.uint8)])
            ids = np.concatenate([ids, keep[None]])
            ends = np.concatenate([ends, [ends[-1] + np.uint64(size3)]]).astype(np.uint64)
        tot = s.put(_dev(blob), ids, ends)
        assert tot["stored"] == 128 and tot["present"] == (1 if k else 0)
        assert s.HasChunk(keep.tobytes())
    c = s.counts()
    assert c["bytes"] <= 1 << 20
    held = {r.tobytes() for r in s.entries()[0]}
    assert all(r.tobytes() in held for r in puts[-1][1]) and all(r.tobytes() in held for r in puts[-2][1])
    assert not any(r.tobytes() in held for r in puts[0][1][:3])  # the oldest went
    assert s.GetChunk(keep.tobytes()) == puts[0][0][int(puts[0][2][2]):int(puts[0][2][3])].tobytes()
    before = gpu_state(s)
    big = chunks(300, 300, 8192)
    assert int(big[2][-1]) > 1 << 20
    with pytest.raises(L.DsxError) as exc:
        s.put(_dev(big[0]), big[1], big[2])
    assert exc.value.code == L.DSX_E_CAPACITY and exc.value.totals["stored"] == 300
    assert gpu_state(s) == before
    s.close()
    # a bounded cache in front of a big store
    big_store = desync_amd.DeviceStore(2 << 20, 1024, ctx=dctx)
    blob, ids, ends = chunks(400, 400, 4096)
    big_store.put(_dev(blob), ids, ends)
    small = desync_amd.DeviceStore(64 << 10, 64, ctx=dctx, evict=True)
    cache = desync_amd.Cache(big_store, small)
    raw = blob.tobytes()
    for i in range(0, 400, 2):
        lo = int(ends[i - 1]) if i else 0
        assert cache.GetChunk(ids[i].tobytes()) == raw[lo:int(ends[i])]
    assert 0 < len(small) <= 64 and small.counts()["bytes"] <= 64 << 10
    assert small.HasChunk(ids[398].tobytes()) and not small.HasChunk(ids[0].tobytes())
    small.close()
    big_store.close()


# ---- 11. touch on use, the clock's end, a copy of everything that evicts -----------------------
def _hashed(seed, n, hi):
    blob, _, ends = chunks(seed, n, hi, lo=1)
    raw, lo, sums = blob.tobytes(), 0, []
    for e in ends.tolist():
        sums.append(hashlib.new("sha512_256", raw[lo:e]).digest())
        lo = e
    return blob, np.frombuffer(b"".join(sums), np.uint8).reshape(-1, 32).copy(), ends


def test_touch_on_use(dctx):
    """GetChunk stamps the chunk it returns; AssembleBlob stamps the store chunks
    of its plan, out of place and in place, each with one new clock value;
    read_ranges and locate stamp nothing."""
    import desync_amd
    torch = _torch()
    s = desync_amd.DeviceStore(1 << 20, 200, ctx=dctx, track=True)
    blob, ids, ends = _hashed(21, 100, 3000)
    s.put(_dev(blob), ids, ends)
    want = [1] * 100
    assert ([int(t) for t in s.stamps()[0]], s.stamps()[1]) == (want, 1)
    s.locate(ids[:10])
    assert [int(t) for t in s.stamps()[0]] == want
    raw = blob.tobytes()
    assert s.GetChunk(ids[7].tobytes()) == raw[int(ends[6]):int(ends[7])]
    want[7] = 2
    assert ([int(t) for t in s.stamps()[0]], s.stamps()[1]) == (want, 2)
    pick = [40, 41, 42, 90, 3]
    sizes = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
    index = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=4096),
                             desync_amd.index.ChunkArray(np.cumsum(sizes[pick]).astype(np.uint64), ids[pick]))
    data = b"".join(raw[int(ends[i]) - int(sizes[i]):int(ends[i])] for i in pick)
    out, _ = desync_amd.AssembleBlob(index, s, ctx=dctx, null_seed=False)
    assert out.cpu().numpy().tobytes() == data
    for i in pick:
        want[i] = 3
    assert ([int(t) for t in s.stamps()[0]], s.stamps()[1]) == (want, 3)
    buf = torch.zeros(len(data) + 100, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    out, _ = desync_amd.AssembleBlob(index, s, ctx=dctx, null_seed=False, out=buf)
    assert out.cpu().numpy().tobytes() == data
    for i in pick:
        want[i] = 4
    assert ([int(t) for t in s.stamps()[0]], s.stamps()[1]) == (want, 4)
    s.read_ranges(index, [(0, 100)])
    assert ([int(t) for t in s.stamps()[0]], s.stamps()[1]) == (want, 4)
    s.close()


def test_clock_saturates(pair):
    """A caller's stamp of UINT64_MAX ends the clock's range: later uses are
    stamped UINT64_MAX too, never 0, and ties go by entry number."""
    p = pair(1 << 20, 300)
    blob, ids, ends = chunks(22, 200, 1000, lo=1)
    p.put(blob[:int(ends[99]) + 1], ids[:100], ends[:100])
    p.touch(ids[:50], stamp=ref.U64_MAX)
    p.touch(ids[50:60])                                            # DSX_STAMP_NOW at the end of the range
    p.put(blob[int(ends[99]):], ids[100:], ends[100:] - ends[99])  # and a put's stamp
    stamps, clock = p.gpu.stamps()
    assert clock == ref.U64_MAX and int(stamps[55]) == ref.U64_MAX == int(stamps[150]) and int(stamps[70]) == 1
    p.same()
    tot = p.evict(need_chunks=300 - 200 + 60)  # the 40 of stamp 1, then the first 20 at the end of the range
    assert tot["ids"] == np.concatenate([ids[:20], ids[60:100]]).tobytes() and tot["cutoff"] == ref.U64_MAX
    p.same()


def test_copy_all_evicts(dctx):
    """CopyFrom of every entry into a full DeviceStore(evict=True): the room is
    made with the source's IDs as the pin list, so what both stores hold stays."""
    import desync_amd
    src = desync_amd.DeviceStore(1 << 20, 200, ctx=dctx)
    dst = desync_amd.DeviceStore(96 << 10, 200, ctx=dctx, evict=True)
    blob, ids, ends = chunks(23, 120, 1000, lo=1)
    dst.put(_dev(blob), ids, ends)                      # ~60 KB: the oldest
    blob2, ids2, ends2 = chunks(24, 100, 1000, lo=1)
    ids2[:10] = ids[:10]                                # ten IDs both hold (the put trusts them)
    src.put(_dev(blob2), ids2, ends2)
    tot = dst.CopyFrom(src)
    assert tot["copied"] == 90 and tot["present"] == 10
    held = {r.tobytes() for r in dst.entries()[0]}
    assert all(r.tobytes() in held for r in ids2) and dst.counts()["bytes"] <= 96 << 10
    assert len(held) < 210  # something went
    src.close()
    dst.close()
