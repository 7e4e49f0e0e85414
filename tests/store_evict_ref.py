"""store_prune_ref's model with use tracking and eviction (dsx_store_track,
dsx_store_touch, dsx_store_evict): stamps, a clock, the stamping rules of put,
copy and prune, and evict as its literal definition -- sort the unpinned
entries by (stamp, entry number), take the shortest prefix that makes the room.
Then seeded scripts of mixed calls over two such stores, the driver that runs
one against a backend, and planted-mistake models the scripts must tell from
the true one."""
import copy as _copy

import numpy as np

import store_copy_ref
import store_prune_ref
import store_ref

EVICT_TOTALS = ("entries", "evicted", "evicted_bytes", "kept", "kept_bytes", "moved", "moved_bytes",
                "pinned", "evictable", "evictable_bytes", "cutoff")


def _rows(ids):
    return [r.tobytes() for r in np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)]


U64_MAX = 0xFFFFFFFFFFFFFFFF


def _next(clock):
    """++clock, saturating: it never wraps to the oldest stamp."""
    return min(clock + 1, U64_MAX)


class Untracked(Exception):
    pass


class Store(store_prune_ref.Store):
    def __init__(self, arena_bytes, max_chunks, track=False):
        super().__init__(arena_bytes, max_chunks)
        self.tracked, self.stamps, self.clock = False, [], 0
        if track:
            self.track()

    def track(self):
        if not self.tracked:
            self.tracked, self.stamps, self.clock = True, [0] * len(self.ids), 0

    def size(self, e):
        return self.ends[e] - (self.ends[e - 1] if e else 0)

    def _stamp(self, cids, t):
        self.stamps += [0] * (len(self.ids) - len(self.stamps))
        for cid in cids:
            e = self.pos.get(cid)
            if e is not None:
                self.stamps[e] = t

    def put(self, blob, ids, ends, start=0):
        tot = super().put(blob, ids, ends, start)  # (a refusal raises: nothing is stamped)
        if self.tracked and len(ends):
            self.clock = _next(self.clock)
            self._stamp(_rows(ids), self.clock)
        return tot

    def prune(self, ids, remove=False):
        by_id = dict(zip(self.ids, self.stamps)) if self.tracked else {}
        tot = super().prune(ids, remove)
        if self.tracked:
            self.stamps = self.carried(by_id)
        return tot

    def carried(self, by_id):
        """The survivors' stamps after a prune."""
        return [by_id[cid] for cid in self.ids]

    def touch(self, ids, stamp=None):
        """-> n_missing; stamp None: DSX_STAMP_NOW."""
        if not self.tracked:
            raise Untracked()
        cids = _rows(ids)
        if not cids:
            return 0
        t = _next(self.clock) if stamp is None else int(stamp)
        self._stamp(cids, t)
        self.clock = max(self.clock, t)
        return sum(1 for cid in cids if cid not in self.pos)

    def order(self, pinned):
        """The unpinned entries, least recently used first."""
        return sorted((e for e, cid in enumerate(self.ids) if cid not in pinned),
                      key=lambda e: (self.stamps[e], e))

    def evict(self, need_bytes=0, need_chunks=0, pin=(), dry=False):
        """-> the totals with "ids", the victims' IDs in entry order; raises
        store_ref.Capacity (with the totals) and changes nothing if not even
        every unpinned entry makes the room."""
        if not self.tracked:
            raise Untracked()
        pinned = set(_rows(pin)) if len(pin) else set()
        order = self.order(pinned)
        tot = dict.fromkeys(EVICT_TOTALS, 0)
        tot.update(entries=len(self.ids), kept=len(self.ids), kept_bytes=len(self.arena),
                   pinned=len(self.ids) - len(order), evictable=len(order),
                   evictable_bytes=sum(self.size(e) for e in order))
        room_b, room_c, k = self.arena_bytes - len(self.arena), self.max_chunks - len(self.ids), 0
        while room_b < need_bytes or room_c < need_chunks:
            if k == len(order):
                raise store_ref.Capacity(tot)
            room_b, room_c, k = room_b + self.size(order[k]), room_c + 1, k + 1
        victims = sorted(order[:k])
        tot["ids"] = b"".join(self.ids[e] for e in victims)
        if not victims:
            return tot
        tot["cutoff"] = max(self.stamps[e] for e in victims)
        target = _copy.deepcopy(self) if dry else self
        p = target.prune(np.frombuffer(tot["ids"], np.uint8).reshape(-1, 32), remove=True)
        tot.update(evicted=p["removed"], evicted_bytes=p["removed_bytes"], kept=p["kept"],
                   kept_bytes=p["kept_bytes"], moved=p["moved"], moved_bytes=p["moved_bytes"])
        return tot


def copy(dst, src, ids=None):
    """store_copy_ref.copy with the stamping rules -> the totals."""
    n = len(src.ids) if ids is None else len(ids)
    before, was_empty = dst.counts(), not dst.ids
    tot = store_copy_ref.copy(dst, src, ids)
    if tot["missing"] or not store_copy_ref.fits(before, tot) or n == 0:
        return tot
    new = dst.ids[len(dst.ids) - tot["copied"]:]
    named = list(src.ids) if ids is None else _rows(ids)
    if new and ids is None and was_empty and dst.tracked and src.tracked:
        dst.stamps, dst.clock = list(src.stamps), src.clock  # carried over
        return tot
    if dst.tracked:
        dst.clock = _next(dst.clock)
        dst._stamp(named, dst.clock)
    if new and src.tracked:
        src.clock = _next(src.clock)
        src._stamp(new, src.clock)
    return tot


# ---- planted mistakes ------------------------------------------------------------------------
class TiesDescending(Store):
    """Among equal stamps the entry appended later goes first."""

    def order(self, pinned):
        return sorted((e for e, cid in enumerate(self.ids) if cid not in pinned),
                      key=lambda e: (self.stamps[e], -e))


class PruneDropsStamps(Store):
    """A prune leaves the stamps where they were: survivor k gets old entry k's."""

    def carried(self, by_id):
        return list(by_id.values())[:len(self.ids)]


class PutSkipsPresent(Store):
    """A put stamps only what it appended."""

    def put(self, blob, ids, ends, start=0):
        n = len(self.ids)
        tot = store_prune_ref.Store.put(self, blob, ids, ends, start)
        if self.tracked and len(ends):
            self.clock = _next(self.clock)
            self._stamp(self.ids[n:], self.clock)
        return tot


MUTANTS = (TiesDescending, PruneDropsStamps, PutSkipsPresent)


# ---- seeded scripts of mixed calls --------------------------------------------------------------
NPOOL = 400
ARENA, CHUNKS = 96 << 10, 260   # store A; B is half of it
LIFE_SEEDS = (11, 12, 13)
LIFE_OPS = 60


class Pool:
    """NPOOL chunks of 0-1,023 bytes (every seventh empty) with random IDs over one blob."""

    def __init__(self):
        rng = np.random.default_rng(4242)
        sizes = rng.integers(0, 1024, NPOOL).astype(np.int64)
        sizes[::7] = 0
        self.sizes = sizes
        self.ends = np.cumsum(sizes)
        self.starts = self.ends - sizes
        self.blob = rng.integers(0, 256, int(self.ends[-1]), dtype=np.uint8)
        self.ids = rng.integers(0, 256, (NPOOL, 32), dtype=np.uint8)
        self.absent = rng.integers(0, 256, (8, 32), dtype=np.uint8)

    def gather(self, picks):
        """-> (blob, ids, ends) of the chunks `picks` laid back to back from 0."""
        picks = np.asarray(picks, dtype=np.int64)
        parts = [self.blob[self.starts[i]:self.ends[i]] for i in picks]
        blob = np.concatenate(parts + [np.zeros(1, np.uint8)])
        return blob, self.ids[picks], np.cumsum(self.sizes[picks]).astype(np.uint64)


_pool = None


def pool():
    global _pool
    if _pool is None:
        _pool = Pool()
    return _pool


class Life:
    """Two tracked stores, one op at a time -> a result of plain values."""

    def __init__(self, store_cls=Store):
        self.cls = store_cls
        self.stores = {"A": store_cls(ARENA, CHUNKS, track=True), "B": store_cls(ARENA // 2, CHUNKS // 2, track=True)}

    def state(self, name):
        s = self.stores[name]
        return {"counts": s.counts(), "ids": b"".join(s.ids), "ends": [int(e) for e in s.ends],
                "arena": bytes(s.arena), "stamps": [int(t) for t in s.stamps], "clock": int(s.clock)}

    def apply(self, op):
        kind, s = op["op"], self.stores[op["store"]]
        if kind == "put":
            blob, ids, ends = pool().gather(op["picks"])
            try:
                return {"refused": None, "totals": s.put(blob.tobytes(), ids, ends)}
            except store_ref.Capacity as e:
                return {"refused": "capacity", "totals": e.totals}
        if kind == "copy":
            before = s.counts()
            tot = copy(s, self.stores[op["src"]], op["ids"])
            refused = "missing" if tot["missing"] else None if store_copy_ref.fits(before, tot) else "capacity"
            return {"refused": refused, "totals": tot}
        if kind == "touch":
            return {"missing": s.touch(op["ids"], op["stamp"])}
        if kind == "evict":
            try:
                tot = s.evict(op["need_bytes"], op["need_chunks"], op["pin"], op["dry"])
            except store_ref.Capacity as e:
                return {"refused": "capacity", "totals": e.totals}
            return {"refused": None, "totals": tot}
        if kind == "prune":
            return {"totals": s.prune(op["ids"], remove=op["remove"])}
        if kind == "grow":
            new = self.cls(op["arena_bytes"], op["max_chunks"], track=True)
            tot = copy(new, s, None)
            self.stores[op["store"]] = new
            return {"totals": tot}
        raise ValueError(kind)


def _held(s):
    return np.frombuffer(b"".join(s.ids), np.uint8).reshape(-1, 32).copy()


def _some(rng, s, frac):
    held = _held(s)
    return held[rng.random(len(held)) < frac]


def script(seed):
    """LIFE_OPS ops, generated on the true model: put, copy, copy of every entry
    into an emptied store, touch, evict, prune, remove and Grow."""
    rng = np.random.default_rng(seed)
    life, ops, p = Life(), [], pool()

    def do(op):
        ops.append(op)
        life.apply(op)

    do({"op": "put", "store": "A", "picks": np.arange(0, 120)})
    do({"op": "put", "store": "A", "picks": np.arange(100, 150)})             # 20 present: stamped too
    do({"op": "touch", "store": "A", "ids": _held(life.stores["A"])[5:60:3], "stamp": None})
    do({"op": "prune", "store": "A", "ids": _held(life.stores["A"])[0:40:2], "remove": True})
    do({"op": "evict", "store": "A", "need_bytes": ARENA - 20000, "need_chunks": 0,
        "pin": np.empty((0, 32), np.uint8), "dry": False})
    do({"op": "copy", "store": "B", "src": "A", "ids": None})                 # every entry into an empty store
    do({"op": "put", "store": "B", "picks": np.arange(200, 240)})
    while len(ops) < LIFE_OPS:
        name = "A" if rng.random() < 0.6 else "B"
        s, other = life.stores[name], "B" if name == "A" else "A"
        r = rng.random()
        if r < 0.25:
            n = int(rng.choice([1, 9, 40, 90]))
            lo = int(rng.integers(0, NPOOL - n + 1))
            do({"op": "put", "store": name, "picks": np.arange(lo, lo + n)})
        elif r < 0.45:
            ids = np.concatenate([_some(rng, s, rng.uniform(0.05, 0.5)), p.absent[:2]])
            stamp = None if rng.random() < 0.7 else s.clock + int(rng.choice([0, 1, 300, 70000]))
            do({"op": "touch", "store": name, "ids": ids, "stamp": stamp or None})
        elif r < 0.70:
            c = s.counts()
            need_b = int(rng.integers(0, c["arena_bytes"] + 1)) if rng.random() < 0.7 else 0
            need_c = int(rng.integers(0, c["max_chunks"] + 1)) if rng.random() < 0.5 else 0
            pin = np.concatenate([_some(rng, s, rng.choice([0.0, 0.1, 0.6])), p.absent[2:3]])
            do({"op": "evict", "store": name, "need_bytes": need_b, "need_chunks": need_c, "pin": pin,
                "dry": bool(rng.random() < 0.2)})
        elif r < 0.80:
            remove = bool(rng.random() < 0.5)
            do({"op": "prune", "store": name, "ids": _some(rng, s, 0.3 if remove else 0.7), "remove": remove})
        elif r < 0.92:
            if rng.random() < 0.3:
                do({"op": "prune", "store": name, "ids": np.empty((0, 32), np.uint8), "remove": False})
                do({"op": "copy", "store": name, "src": other, "ids": None})
            else:
                ids = np.concatenate([_some(rng, life.stores[other], rng.uniform(0.1, 0.5)),
                                      p.absent[3:4] if rng.random() < 0.2 else p.absent[:0]])
                do({"op": "copy", "store": name, "src": other, "ids": ids})
        else:
            c = s.counts()
            do({"op": "grow", "store": name, "arena_bytes": max(c["bytes"], c["arena_bytes"] + int(rng.integers(-8192, 8192))),
                "max_chunks": max(c["chunks"], c["max_chunks"] + int(rng.integers(-20, 20)))})
    return ops


class Mismatch(AssertionError):
    pass


def drive(seed, backend):
    """Runs script(seed) on the true model and on `backend` (apply(op), state(name))
    side by side: every result and, after every call, every buffer of both
    stores must be equal."""
    life = Life()
    for pos, op in enumerate(script(seed)):
        want, got = life.apply(op), backend.apply(op)
        if want != got:
            raise Mismatch(f"seed {seed}, op {pos} {op['op']} on {op['store']}: want {want!r:.300}, got {got!r:.300}")
        for name in ("A", "B"):
            a, b = life.state(name), backend.state(name)
            if a != b:
                key = next(k for k in a if a[k] != b[k])
                raise Mismatch(f"seed {seed}, store {name} after op {pos} {op['op']} on {op['store']}: {key} differs")
