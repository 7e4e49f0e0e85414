"""The life of the chunk store in HBM as seeded sequences of mixed calls: a
chunk pool, a model of named stores (store_prune_ref.Store, store_copy_ref.copy
and read_ref composed), a deterministic script generator, and the driver that
runs one script against the model and a backend side by side and stops at the
first difference.  test_store_life_host.py runs the scripts on the model alone;
test_gpu_store_life.py gives the driver a backend of desync_amd.DeviceStore.

An op is a dict with "op" and its arguments; a result is a dict of plain
Python values (ints, bytes, lists, dicts), so that two results compare with ==.
"""
import functools
import hashlib

import numpy as np

import known_ref
import read_ref
import store_copy_ref
import store_prune_ref
import store_ref

WINDOW = 65536
NULL_SIZE = 4096
FILL = 0xA5
PAD = 0xEE
BIG = 70000  # longer than one 64 KiB gather tile

# name -> (arena bytes, max chunks, context): A and B share a context, C has its own
PROFILES = {
    "narrow": dict(npool=900, pool_seed=9001, ops=120,
                   stores={"A": (320 << 10, 700, 0), "B": (128 << 10, 300, 0), "C": (192 << 10, 400, 1)}),
    "wide": dict(npool=140000, pool_seed=9002, ops=8,
                 stores={"A": (2 << 20, 140000, 0), "B": (1 << 20, 100000, 0)}),
}
NARROW_SEEDS = (1, 2, 3, 4)
SCRIPTS = [("narrow", s) for s in NARROW_SEEDS] + [("wide", 0)]

MUTATING = ("put", "prune", "copy", "grow", "grow_refused", "remove_chunk", "put_sealed")
QUERIES = ("locate", "entries", "get", "read", "assemble", "verify", "known")
FOREIGN = ("idset", "dedup", "chunk_ids", "chunk_keep")


def _sum(data):
    return hashlib.new("sha512_256", data).digest()


NULL_ID = _sum(bytes(NULL_SIZE))


# ---- the chunk pool ---------------------------------------------------------------------
class Pool:
    """`npool` chunks over one random blob.  Narrow: sizes i % 50 (empty ones
    among them), every 97th 4,097 bytes, three of 70,000; the IDs are the
    chunks' SHA-512/256 sums, except a few liars whose ID is the sum of other
    bytes (a put trusts its IDs; Verify finds them, and a known op recognises
    their bytes under their ID: no other chunk has a liar's bytes).  Wide:
    sizes i % 16 and random IDs."""

    def __init__(self, profile):
        p = PROFILES[profile]
        n = p["npool"]
        rng = np.random.default_rng(p["pool_seed"])
        self.wide = profile == "wide"
        if self.wide:
            sizes = np.arange(n, dtype=np.uint64) % 16
        else:
            sizes = np.arange(n, dtype=np.uint64) % 50
            sizes[96::97] = 4097
            sizes[[150, 420, 777]] = BIG
        self.sizes = sizes
        self.ends = np.cumsum(sizes).astype(np.uint64)
        self.starts = (self.ends - sizes).astype(np.uint64)
        self.blob = rng.integers(0, 256, int(self.ends[-1]), dtype=np.uint8)
        self.liars = set()
        if self.wide:
            self.ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            assert len({r.tobytes() for r in self.ids}) == n
        else:
            raw = self.blob.tobytes()
            sums = []
            for i in range(n):
                data = raw[int(self.starts[i]):int(self.ends[i])]
                if i % 211 == 5:
                    sums.append(_sum(data + b"!"))
                    self.liars.add(sums[-1])
                else:
                    sums.append(_sum(data))
            self.ids = np.frombuffer(b"".join(sums), dtype=np.uint8).reshape(-1, 32).copy()
            # a known op recognises a liar's bytes under the liar's ID: no other chunk may
            # have those bytes under its own
            by_bytes = {}
            for i in range(n):
                by_bytes.setdefault(raw[int(self.starts[i]):int(self.ends[i])], set()).add(sums[i])
            assert all(len(ids) == 1 for ids in by_bytes.values()), "equal bytes under two IDs"
        self.absent = rng.integers(0, 256, (64, 32), dtype=np.uint8)  # IDs of no chunk

    def gather(self, picks, pad=0):
        """The chunks `picks` (pool numbers, repeats allowed) laid back to back
        behind `pad` bytes -> (blob, ids, ends, start)."""
        picks = np.asarray(picks, dtype=np.int64)
        sizes = self.sizes[picks].astype(np.int64)
        ends = pad + np.cumsum(sizes)
        total = int(ends[-1]) if len(picks) else pad
        blob = np.full(total + 3, PAD, dtype=np.uint8)
        if total > pad:
            src = np.repeat(self.starts[picks].astype(np.int64) - (ends - sizes), sizes) + np.arange(pad, total)
            blob[pad:total] = self.blob[src]
        return blob, self.ids[picks], ends.astype(np.uint64), pad

    def data(self, i):
        return self.blob[int(self.starts[i]):int(self.ends[i])].tobytes()


@functools.lru_cache(maxsize=None)
def pool_of(profile):
    return Pool(profile)


# ---- the model ----------------------------------------------------------------------------
class Life:
    """Named stores and one op at a time -> what the GPU call must return."""

    def __init__(self, profile, store_cls=store_prune_ref.Store, copy_fn=store_copy_ref.copy):
        self.profile, self.pool = profile, pool_of(profile)
        self.store_cls, self.copy_fn = store_cls, copy_fn
        self.stores = {k: store_cls(a, m) for k, (a, m, _) in PROFILES[profile]["stores"].items()}
        self.last_change = dict.fromkeys(self.stores)   # the kind of the last call that changed the entries
        self.last_refused = dict.fromkeys(self.stores, False)  # the last mutating call was refused

    def apply(self, op):
        return getattr(self, "_" + op["op"])(op)

    def state(self, name):
        """What the driver compares after every mutating op."""
        s = self.stores[name]
        offs, sizes, miss = s.locate(np.frombuffer(b"".join(s.ids), np.uint8).reshape(-1, 32))
        return {"counts": s.counts(), "ids": b"".join(s.ids), "ends": [int(e) for e in s.ends],
                "arena": bytes(s.arena), "locate": ([int(o) for o in offs], [int(z) for z in sizes], miss)}

    def _done(self, name, kind, changed, refused):
        if changed:
            self.last_change[name] = kind
        self.last_refused[name] = bool(refused)

    # ---- mutating ops ----
    def _put(self, op):
        blob, ids, ends, start = self.pool.gather(op["picks"], op["pad"])
        return self._put_bytes(op["store"], blob, ids, ends, start)

    def _put_bytes(self, name, blob, ids, ends, start):
        try:
            tot = self.stores[name].put(blob.tobytes(), ids, ends, start)
        except store_ref.Capacity as e:
            self._done(name, "put", False, True)
            return {"refused": "capacity", "totals": e.totals}
        self._done(name, "put", tot["stored"] > 0, False)
        return {"refused": None, "totals": tot}

    def _prune(self, op):
        tot = self.stores[op["store"]].prune(op["ids"], remove=op["remove"])
        self._done(op["store"], "prune", tot["removed"] > 0, False)
        return {"refused": None, "totals": tot}

    def _remove_chunk(self, op):
        tot = self.stores[op["store"]].prune(np.frombuffer(op["id"], np.uint8).reshape(1, 32), remove=True)
        self._done(op["store"], "prune", tot["removed"] > 0, not tot["removed"])
        return {"refused": None if tot["removed"] else "missing"}

    def _copy(self, op):
        dst, src = self.stores[op["store"]], self.stores[op["src"]]
        before = dst.counts()
        tot = self.copy_fn(dst, src, op["ids"])
        refused = "missing" if tot["missing"] else None if store_copy_ref.fits(before, tot) else "capacity"
        self._done(op["store"], "copy", not refused and tot["copied"] > 0, refused)
        return {"refused": refused, "totals": tot}

    def _grow(self, op):
        old = self.stores[op["store"]]
        new = self.store_cls(op["arena_bytes"], op["max_chunks"])
        tot = self.copy_fn(new, old, None)
        refused = None if store_copy_ref.fits(new.counts() | {"chunks": 0, "bytes": 0}, tot) else "capacity"
        if not refused:
            self.stores[op["store"]] = new
        self.last_refused[op["store"]] = bool(refused)
        return {"refused": refused, "totals": tot}

    _grow_refused = _grow

    def _put_sealed(self, op):
        src = self.stores[op["src"]]
        ids = src.ids[op["first"]:op["first"] + op["n"]]
        if any(cid in self.pool.liars for cid in ids):
            self.last_refused[op["store"]] = True
            return {"refused": "invalid", "totals": None}
        parts = [src.get(cid) for cid in ids]
        blob = np.frombuffer(b"".join(parts) + b"\0", np.uint8)
        ends = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        return self._put_bytes(op["store"], blob, np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32), ends, 0)

    # ---- queries ----
    def _locate(self, op):
        offs, sizes, miss = self.stores[op["store"]].locate(op["ids"])
        return {"offs": [int(o) for o in offs], "sizes": [int(z) for z in sizes], "missing": miss}

    def _entries(self, op):
        s = self.stores[op["store"]]
        return {"ids": b"".join(s.ids), "ends": [int(e) for e in s.ends]}

    def _get(self, op):
        s = self.stores[op["store"]]
        return {"data": s.get(op["id"]) if op["id"] in s.pos else None}

    def _stored(self, name):
        s = self.stores[name]
        return {cid: s.ends[e] - (s.ends[e - 1] if e else 0) for e, cid in enumerate(s.ids)}

    def index_of(self, op):
        """The index a read or an assemble names -> (ids (n, 32), ends, blob):
        op["chunks"] is a list of (32-byte ID, size, bytes or None for zeros)."""
        ids = np.frombuffer(b"".join(c[0] for c in op["chunks"]), np.uint8).reshape(-1, 32)
        ends = np.cumsum([c[1] for c in op["chunks"]], dtype=np.uint64)
        blob = np.frombuffer(b"".join(bytes(c[1]) if c[2] is None else c[2] for c in op["chunks"]), np.uint8)
        return ids, ends, blob

    def _read(self, op):
        ids, ends, blob = self.index_of(op)
        rg = read_ref.with_dst(op["ranges"])
        tot = read_ref.totals(ends, ids, rg, self._stored(op["store"]), 0, NULL_ID, NULL_SIZE)
        out_len = sum(ln for _, ln, _ in rg) + 37
        if tot["missing"] or tot["wrong_size"] or tot["beyond"]:
            out = np.full(out_len, FILL, dtype=np.uint8)  # all or nothing
        else:
            out = read_ref.expected(blob, rg, out_len, FILL)
        return {"totals": {k: int(v) for k, v in tot.items()}, "out": out.tobytes()}

    def _assemble(self, op):
        stored = self._stored(op["store"])
        for cid, size, _ in op["chunks"]:
            if cid == NULL_ID and size == NULL_SIZE:
                continue
            if cid not in stored:
                return {"error": ("missing", cid), "out": None}
            if stored[cid] != size:
                return {"error": ("size", cid), "out": None}
        for cid, _, _ in op["chunks"]:  # the read-back check: a chunk that does not hash to its ID
            if cid in self.pool.liars:
                return {"error": ("invalid", cid), "out": None}
        return {"error": None, "out": self.index_of(op)[2].tobytes()}

    def _verify(self, op):
        s = self.stores[op["store"]]
        return {"bad": [e for e, cid in enumerate(s.ids) if cid in self.pool.liars]}

    def _known(self, op):
        """dsx_chunk_ids_known: a chunk whose bytes an entry holds gets that
        entry's ID (a liar's too), the others their hash; then the offsets by
        ID (known_ref.StoreModel over the entries as they lie now)."""
        s = self.stores[op["store"]]
        blob, _, ends, start = self.pool.gather(op["picks"], op["pad"])
        model = known_ref.StoreModel("sha512_256")
        model.put(bytes(s.arena), s.ends, 0, ids=s.ids)
        ids, off, rec = model.answer(blob.tobytes(), ends, start)
        return {"ids": ids.tobytes(), "known_off": [int(o) for o in off], "recognised": int(rec),
                "hashed": len(ends) - int(rec)}

    # ---- foreign calls on a context the stores use ----
    def _idset(self, op):
        ids = self.pool.ids[op["picks"]]
        return {"n": len(ids), "unique": len({r.tobytes() for r in ids})}

    def _dedup(self, op):
        ids, sizes = self.pool.ids[op["picks"]], self.pool.sizes[op["picks"]]
        seed_first = {}
        for j, r in enumerate(self.pool.ids[op["seed_picks"]]):
            seed_first.setdefault(r.tobytes(), j)
        first, seedp, own = [], [], {}
        tot = {"total": len(ids), "unique": 0, "in_seed": 0, "size": int(sizes.sum()), "size_not_in_seed": 0}
        for i, r in enumerate(ids):
            r = r.tobytes()
            first.append(own.setdefault(r, i))
            seedp.append(seed_first.get(r, 0xFFFFFFFF))
            if first[i] == i:
                tot["unique"] += 1
                if r in seed_first:
                    tot["in_seed"] += 1
                else:
                    tot["size_not_in_seed"] += int(sizes[i])
        return {"first": first, "seed": seedp, "totals": tot}

    def _chunk_ids(self, op):
        blob, _, ends, start = self.pool.gather(op["picks"], op["pad"])
        raw, out, lo = blob.tobytes(), [], start
        for e in ends.tolist():
            out.append(_sum(raw[lo:e]))
            lo = e
        return {"ids": b"".join(out)}

    def _chunk_keep(self, op):
        blob, ids, ends = chunk_keep_args(self.pool, op)
        raw, keep, lo = blob.tobytes(), [], 0
        for i, e in enumerate(ends.tolist()):
            keep.append(int(e <= op["have_len"] and _sum(raw[lo:e]) == ids[i].tobytes()))
            lo = e
        return {"keep": keep}


def chunk_keep_args(pool, op):
    """-> (blob, ids, ends) of a chunk_keep op: the picks back to back from 0,
    a few IDs replaced by IDs of no chunk."""
    blob, ids, ends, _ = pool.gather(op["picks"], 0)
    ids = ids.copy()
    ids[op["wrong"]] = pool.absent[:len(op["wrong"])]
    return blob, ids, ends


# ---- the script generator ------------------------------------------------------------------
def _rows(ids):
    return np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32).copy()


def _held(store):
    return _rows(store.ids)


def _put_op(name, picks, pad, ids_dev=False, ends_dev=False):
    return {"op": "put", "store": name, "picks": np.asarray(picks, dtype=np.int64), "pad": int(pad),
            "ids_dev": bool(ids_dev), "ends_dev": bool(ends_dev)}


def _prune_op(name, ids, remove=False, window=0, ids_dev=False):
    return {"op": "prune", "store": name, "ids": np.ascontiguousarray(ids, np.uint8).reshape(-1, 32),
            "remove": bool(remove), "window": int(window), "ids_dev": bool(ids_dev)}


def _copy_op(dst, src, ids=None, ids_dev=False):
    ids = None if ids is None else np.ascontiguousarray(ids, np.uint8).reshape(-1, 32)
    return {"op": "copy", "store": dst, "src": src, "ids": ids, "ids_dev": bool(ids_dev)}


def _known_op(name, picks, pad):
    assert pad % 2 == 1
    return {"op": "known", "store": name, "picks": np.asarray(picks, dtype=np.int64), "pad": int(pad)}


def _with_dups(rng, picks, k):
    """k more picks, each a copy of one already there, at random places."""
    picks = list(picks)
    for _ in range(k):
        picks.insert(int(rng.integers(0, len(picks) + 1)), picks[int(rng.integers(0, len(picks)))])
    return picks


def _index_chunks(rng, life, name, lie=None, count=40):
    """An index of up to `count` stored chunks in a shuffled order with null
    chunks between them; lie: "missing" or "size" puts one such chunk in."""
    s, pool = life.stores[name], life.pool
    chunks = []
    order = rng.permutation(len(s.ids)).tolist()
    wrong = order.pop() if lie == "size" and order else None  # (its true size is not in the index as well)
    for e in order[:count]:
        cid = s.ids[e]
        chunks.append((cid, len(s.get(cid)), s.get(cid)))
    for _ in range(2):
        chunks.insert(int(rng.integers(0, len(chunks) + 1)), (NULL_ID, NULL_SIZE, None))
    if lie == "missing":
        cid = pool.absent[int(rng.integers(0, 64))].tobytes()
        chunks.insert(int(rng.integers(0, len(chunks) + 1)), (cid, 33, None))
    elif wrong is not None:
        cid = s.ids[wrong]
        chunks.insert(int(rng.integers(0, len(chunks) + 1)), (cid, len(s.get(cid)) + 1, None))
    return chunks


def _query_op(rng, life, name, kind, lie=None):
    s, pool = life.stores[name], life.pool
    if kind == "locate":
        held = _held(s)
        some = held[rng.integers(0, len(held), 40)] if len(held) else held
        ask = np.concatenate([some, pool.absent[rng.integers(0, 64, 5)], some[:7]])
        return {"op": "locate", "store": name, "ids": ask[rng.permutation(len(ask))]}
    if kind == "get":
        cid = s.ids[int(rng.integers(0, len(s.ids)))] if s.ids and rng.random() < 0.8 \
            else pool.absent[int(rng.integers(0, 64))].tobytes()
        return {"op": "get", "store": name, "id": cid}
    if kind == "read":
        chunks = _index_chunks(rng, life, name, lie, count=70000 if pool.wide else 40)
        ends = np.cumsum([c[1] for c in chunks])
        total = int(ends[-1])
        ranges = read_ref.edge_ranges(ends)
        for _ in range(8):
            off = int(rng.integers(0, total))
            ranges.append((off, int(rng.integers(0, total - off + 1))))
        return {"op": "read", "store": name, "chunks": chunks, "ranges": ranges}
    if kind == "assemble":
        return {"op": "assemble", "store": name, "chunks": _index_chunks(rng, life, name, lie)}
    if kind == "known":  # chunks the store holds and chunks it lacks, repeats among them
        n = int(rng.choice([1, 17, 64, 300, 700]))
        return _known_op(name, rng.integers(0, len(pool.ids), n), 2 * int(rng.integers(0, 8)) + 1)
    return {"op": kind, "store": name}  # entries, verify


def _foreign_op(rng, pool, kind, ctx):
    n = int(rng.choice([1, 17, 64, 300, 700]))
    picks = rng.integers(0, len(pool.ids), n)
    if kind == "idset":
        return {"op": "idset", "ctx": ctx, "picks": picks}
    if kind == "dedup":
        return {"op": "dedup", "ctx": ctx, "picks": picks, "seed_picks": rng.integers(0, len(pool.ids), max(1, n // 2))}
    if kind == "chunk_ids":
        return {"op": "chunk_ids", "ctx": ctx, "picks": picks, "pad": int(rng.integers(1, 16))}
    blob_len = int(pool.sizes[picks].sum())
    return {"op": "chunk_keep", "ctx": ctx, "picks": picks, "have_len": int(rng.integers(0, blob_len + 1)),
            "wrong": rng.integers(0, n, min(n, 3)).tolist()}


def _subset(rng, store, frac, extra=None):
    held = _held(store)
    keep = held[rng.random(len(held)) < frac]
    keep = np.concatenate([keep, keep[:3]] + ([extra] if extra is not None else []))
    return keep[rng.permutation(len(keep))]


def _not_held(pool, *stores):
    """Three pool IDs that none of the stores holds, and two IDs of no chunk."""
    out = [r for r in pool.ids[::37] if not any(r.tobytes() in s.pos for s in stores)][:3]
    return np.concatenate([np.array(out, dtype=np.uint8).reshape(-1, 32), pool.absent[:2]])


def _prologue(rng, life, do):
    """Forces what chance does not give (see conditions())."""
    pool, A, B, C = life.pool, "A", "B", "C"
    do(_put_op(A, _with_dups(rng, range(0, 40), 3), 7))                       # A < 64
    do(_foreign_op(rng, pool, "idset", 0))
    do(_put_op(A, _with_dups(rng, range(40, 120), 2), 1, ids_dev=True))       # up through 64
    do(_put_op(B, range(100, 160), 13, ends_dev=True))
    do(_put_op(B, [1, 420, 2, 777], 5, ids_dev=True))                         # refused: too many bytes
    do(_put_op(A, range(120, 300), 5, ids_dev=True, ends_dev=True))           # up through 256
    do(_foreign_op(rng, pool, "dedup", 0))
    do(_put_op(A, _with_dups(rng, range(300, 640), 5), 3))                    # up through 512
    do(_put_op(A, range(640, 900), 9))                                        # refused: too many chunks
    do(_put_op(A, range(760, 790), 2))                                        # accepted after a refusal
    do(_prune_op(A, pool.ids[6:7], remove=True, window=WINDOW, ids_dev=True))  # moves > 2 windows
    do(_query_op(rng, life, A, "read"))
    do(_copy_op(B, A, np.concatenate([_held(life.stores[A])[200:260], pool.absent[7:9]])))  # refused: missing
    do(_copy_op(B, A))                                                        # refused: capacity
    do(_prune_op(B, _held(life.stores[B])[::2], window=WINDOW))
    do(_copy_op(B, A, _held(life.stores[A])[300:350][::-1], ids_dev=True))    # a copy after a prune
    do(_known_op(B, range(80, 380), 3))                                       # known right after a copy
    do(_prune_op(B, _held(life.stores[B])[10:20], remove=True))               # a prune after a copy
    do(_known_op(B, list(range(0, 900, 7)) + list(range(300, 350)), 5))       # ... after a compaction in place
    do(_query_op(rng, life, B, "assemble"))
    do(_prune_op(B, np.empty((0, 32), np.uint8)))                             # B pruned to nothing ...
    do(_foreign_op(rng, pool, "chunk_ids", 0))
    do(_put_op(B, _with_dups(rng, range(200, 260), 2), 4, ids_dev=True))      # ... and refilled
    do({"op": "grow", "store": A, "arena_bytes": 400 << 10, "max_chunks": 800})
    # known right after a Grow, liars among the picks; then B straight after A on the
    # context's one KnownScratch, with fewer chunks against a smaller store
    do(_known_op(A, list(range(0, 900, 2)) + [5, 216, 427, 638, 849], 7))
    do(_known_op(B, range(90, 330), 1))
    do({"op": "grow_refused", "store": A, "arena_bytes": 400 << 10,
        "max_chunks": life.stores[A].counts()["chunks"] - 1})
    do({"op": "put_sealed", "store": B, "src": A, "first": 10, "n": 40, "nonce_seed": 1})
    do(_query_op(rng, life, B, "entries"))
    do(_query_op(rng, life, A, "locate"))
    do(_query_op(rng, life, A, "get"))
    do(_query_op(rng, life, A, "verify"))
    do({"op": "remove_chunk", "store": A, "id": life.stores[A].ids[77]})
    do({"op": "remove_chunk", "store": A, "id": pool.absent[9].tobytes()})            # ChunkMissing
    do(_query_op(rng, life, A, "read", "missing"))
    do(_query_op(rng, life, A, "assemble", "size"))
    do(_prune_op(A, _subset(rng, life.stores[A], 0.6, _not_held(pool, life.stores[A]))))   # down through 512
    do(_put_op(A, range(860, 880), 6, ends_dev=True))                         # a put after a prune
    do(_prune_op(A, _subset(rng, life.stores[A], 0.35), window=WINDOW))       # down through 256
    do(_put_op(C, range(0, 200), 11))
    do(_put_op(C, range(180, 500), 4, ends_dev=True))                         # refused: too many chunks
    do(_prune_op(C, _held(life.stores[C])[1::3], remove=True, ids_dev=True))
    do(_put_op(C, range(150, 330), 8, ids_dev=True))
    do(_query_op(rng, life, C, "read", "size"))
    do(_query_op(rng, life, C, "assemble", "missing"))
    do(_prune_op(A, _held(life.stores[A])[:30]))                              # down through 64
    do(_foreign_op(rng, pool, "chunk_keep", 1))
    do(_put_op(A, range(400, 500), 3))                                        # a put after a prune


def _random_op(rng, life, after_prune):
    pool = life.pool
    names = list(life.stores)
    r = rng.random()
    if after_prune and rng.random() < 0.7:  # the next put goes into a table a prune has rebuilt
        r, name = 0.0, after_prune.pop()
    else:
        name = names[int(rng.integers(0, len(names)))]
    s = life.stores[name]
    if r < 0.32:
        room = s.max_chunks - len(s.ids)
        n = int(rng.choice([3, 20, 90, 250, 400]))
        if rng.random() < 0.6:
            n = max(1, min(n, room))  # fits by count (the bytes may still refuse it)
        lo = int(rng.integers(0, len(pool.ids) - n + 1))
        picks = _with_dups(rng, range(lo, lo + n), int(rng.integers(0, 4)))
        return _put_op(name, picks, int(rng.integers(1, 32)), rng.random() < 0.5, rng.random() < 0.5)
    if r < 0.52:
        remove = rng.random() < 0.4
        frac = rng.uniform(0.05, 0.5) if remove else rng.uniform(0.2, 0.9)
        extra = _not_held(pool, s) if rng.random() < 0.5 else None
        return _prune_op(name, _subset(rng, s, frac, extra), remove, WINDOW if rng.random() < 0.5 else 0,
                         rng.random() < 0.5)
    if r < 0.62:
        dst, src = ("A", "B") if rng.random() < 0.5 else ("B", "A")
        if rng.random() < 0.3:
            return _copy_op(dst, src)
        extra = _not_held(pool, life.stores[dst], life.stores[src])[1:4:2] if rng.random() < 0.25 else None
        return _copy_op(dst, src, _subset(rng, life.stores[src], rng.uniform(0.05, 0.6), extra), rng.random() < 0.5)
    if r < 0.66:
        cid = s.ids[int(rng.integers(0, len(s.ids)))] if s.ids and rng.random() < 0.8 else pool.absent[3].tobytes()
        return {"op": "remove_chunk", "store": name, "id": cid}
    base_arena, base_chunks, _ = PROFILES[life.profile]["stores"][name]
    c = s.counts()
    if r < 0.69:
        return {"op": "grow", "store": name,
                "arena_bytes": max(c["bytes"], base_arena + int(rng.integers(-(32 << 10), 64 << 10))),
                "max_chunks": max(c["chunks"], base_chunks + int(rng.integers(-50, 100)))}
    if r < 0.71 and c["bytes"]:
        return {"op": "grow_refused", "store": name, "arena_bytes": c["bytes"] - 1, "max_chunks": c["max_chunks"]}
    src = "A" if name != "A" else "B"
    have = len(life.stores[src].ids)
    if r < 0.74 and have:
        n = min(have, int(rng.integers(1, 60)))
        return {"op": "put_sealed", "store": name, "src": src, "first": int(rng.integers(0, have - n + 1)),
                "n": n, "nonce_seed": int(rng.integers(0, 1 << 30))}
    if r < 0.87:
        kind = QUERIES[int(rng.integers(0, len(QUERIES)))]
        lie = [None, None, "missing", "size"][int(rng.integers(0, 4))] if kind in ("read", "assemble") else None
        return _query_op(rng, life, name, kind, lie)
    return _foreign_op(rng, pool, FOREIGN[int(rng.integers(0, len(FOREIGN)))], int(rng.integers(0, 2)))


def _wide_script(life, do):
    pool = life.pool
    do(_put_op("A", np.arange(100000), 5, ids_dev=True, ends_dev=True))
    do(_prune_op("A", pool.ids[0:100000:3], remove=True, window=WINDOW, ids_dev=True))
    kept = np.flatnonzero(np.arange(100000) % 3 != 0)
    do(_put_op("A", np.concatenate([kept[-30000:], np.arange(100000, 140000)]), 3, ends_dev=True))  # 30,000 present
    do(_copy_op("B", "A"))                                        # refused: capacity
    held = _held(life.stores["A"])
    do(_prune_op("A", held[np.linspace(0, len(held) - 1, 90000).astype(np.int64)], ids_dev=True))
    do(_copy_op("B", "A"))
    ask = np.concatenate([_held(life.stores["B"])[5000:80000], pool.absent[:1], pool.absent[1:2]])
    do(_copy_op("A", "B", ask, ids_dev=True))                     # refused: missing
    do(_query_op(np.random.default_rng(0), life, "B", "read"))


@functools.lru_cache(maxsize=None)
def _build(profile, seed):
    """-> (the ops of the script, the steps of walk()): the generator and the
    walk share one pass over one model."""
    life = Life(profile)
    ops, steps, after_prune, known = [], [], [], {}

    def step(pos, op, extra=False):
        want = life.apply(op)
        states = {}
        if op["op"] in MUTATING:
            for name in touched(op):
                if (want.get("refused") or name != op["store"]) and name in known:
                    s = life.stores[name]
                    assert (known[name]["counts"], known[name]["ids"], known[name]["arena"]) == \
                        (s.counts(), b"".join(s.ids), bytes(s.arena)), "the model changed a store it must not change"
                else:
                    known[name] = life.state(name)
                states[name] = known[name]
        steps.append((pos, op, want, states, extra))
        return want

    def do(op):
        pos = len(ops)
        ops.append(op)
        res = step(pos, op)
        if op["op"] == "prune" and res["totals"]["removed"]:
            after_prune.append(op["store"])
        if pos % 10 == 9:
            for q in periodic(life, seed, pos):
                step(pos, q, extra=True)
        return res

    if profile == "wide":
        _wide_script(life, do)
    else:
        rng = np.random.default_rng(seed)
        _prologue(rng, life, do)
        while len(ops) < PROFILES[profile]["ops"]:
            do(_random_op(rng, life, after_prune))
    return tuple(ops), tuple(steps)


def script(profile, seed):
    """The deterministic list of ops of (profile, seed)."""
    return _build(profile, seed)[0]


def periodic(life, seed, pos):
    """The queries that run on every store after every tenth op."""
    rng = np.random.default_rng([seed, pos])
    # wide: no known.  Its pool has random IDs over chunks of 0-15 bytes, so equal bytes lie
    # under many IDs: they fill fingerprint buckets beyond DSX_KNOWN_TRIES, and which path
    # answers such a chunk, and with which of the IDs, is not determined
    kinds = ("locate", "entries", "get", "read") if life.pool.wide else QUERIES
    return [_query_op(rng, life, name, kind) for name in life.stores for kind in kinds]


# ---- the driver ------------------------------------------------------------------------------
def describe(op):
    parts = [op["op"]]
    for k, v in op.items():
        if k == "op":
            continue
        if isinstance(v, np.ndarray):
            v = f"<{len(v)}>"
        elif isinstance(v, (list, tuple)) and len(v) > 4:
            v = f"<{len(v)}>"
        elif isinstance(v, bytes):
            v = v.hex()[:8]
        parts.append(f"{k}={v}")
    return " ".join(parts)


class Mismatch(AssertionError):
    def __init__(self, profile, seed, pos, ops, what):
        self.profile, self.seed, self.pos, self.what = profile, seed, pos, what
        last = "; ".join(f"[{i}] {describe(ops[i])}" for i in range(max(0, pos - 4), pos + 1))
        super().__init__(f"{profile} seed {seed}, op {pos}: {what}\nlast five ops: {last}")


def _first_difference(want, got):
    if isinstance(want, dict) and isinstance(got, dict):
        for k in want:
            if k not in got or want[k] != got[k]:
                return f"{k}: " + _first_difference(want[k], got.get(k))
    w, g = repr(want), repr(got)
    return f"want {w[:200]}{'...' if len(w) > 200 else ''}, got {g[:200]}{'...' if len(g) > 200 else ''}"


def touched(op):
    """The stores whose state is compared after a mutating op."""
    return [op["store"]] + ([op["src"]] if "src" in op else [])


def walk(profile, seed):
    """The script on the model: a tuple of steps (pos, op, the result the call
    must give, {store: the state it must leave}, extra), the periodic queries
    after every tenth op included (extra: the op is one of them, not one of
    the script's).  The states are of the stores a mutating op
    touches; one the op must not change (any store after a refusal, the source
    of a copy) keeps the state of its last comparison, which is asserted."""
    return _build(profile, seed)[1]


def drive(profile, seed, backend, log=None, extras=True):
    """Runs script(profile, seed) on `backend` (apply(op) -> result, state(name)
    -> state) beside the model's walk and raises Mismatch at the first op whose
    result, or whose stores afterwards, differ.  A refused op must leave the
    stores as they were: the state compared is then the one from before it.
    `log` collects the backend's results and states; extras=False runs the
    script's own ops alone, without the periodic queries."""
    ops = script(profile, seed)
    for pos, op, want, states, extra in walk(profile, seed):
        if extra and not extras:
            continue
        try:
            got = backend.apply(op)
        except Exception as e:
            raise Mismatch(profile, seed, pos, ops, f"{describe(op)} raised {e!r}, want {repr(want)[:200]}") from e
        if log is not None:
            log.append((pos, describe(op), got, extra))
        if want != got:
            raise Mismatch(profile, seed, pos, ops, f"{describe(op)}: " + _first_difference(want, got))
        for name, model in states.items():
            real = backend.state(name)
            if log is not None:
                log.append((pos, name, real, extra))
            if model != real:
                raise Mismatch(profile, seed, pos, ops,
                               f"store {name} after {describe(op)}: " + _first_difference(model, real))


class ModelBackend:
    """A Life as the driver's backend: the host test's stand-in for the GPU."""

    def __init__(self, life):
        self.life = life

    def apply(self, op):
        return self.life.apply(op)

    def state(self, name):
        return self.life.state(name)


# ---- the conditions a script must meet ---------------------------------------------------------
def conditions(profile, seed):
    """Walks the script on the model and counts what the GPU test relies on."""
    life = Life(profile)
    c = dict.fromkeys(("put_after_prune", "prune_moves", "emptied", "put_after_emptied", "prune_3_windows",
                       "put_refused", "copy_refused_missing", "copy_refused_capacity", "put_after_refusal",
                       "copy_after_prune", "grow", "grow_refused", "put_sealed", "prune_after_copy",
                       "put_over_65536", "prune_over_65536", "copy_over_65536"), 0)
    up, down, emptied = set(), set(), set()
    kinds = []
    for op in script(profile, seed):
        kind, name = op["op"], op.get("store")
        if kind not in MUTATING:
            life.apply(op)
            kinds.append(kind)
            continue
        was, refused_before = life.last_change[name], life.last_refused[name]
        n_before = len(life.stores[name].ids)
        res = life.apply(op)
        kinds.append(kind)
        tot, ok = res.get("totals") or {}, not res.get("refused")
        n_after = len(life.stores[name].ids)
        if name == "A":
            up |= {t for t in (64, 256, 512) if n_before < t < n_after}
            down |= {t for t in (64, 256, 512) if n_before > t > n_after}
        if kind == "put":
            stored = ok and tot["stored"] > 0
            c["put_after_prune"] += stored and was == "prune"
            c["put_refused"] += res["refused"] == "capacity"
            c["put_after_refusal"] += stored and refused_before
            c["put_after_emptied"] += stored and name in emptied
            c["put_over_65536"] += stored and tot["stored"] > 65536
            if stored:
                emptied.discard(name)
        elif kind == "prune":
            c["prune_moves"] += tot["moved_bytes"] > 0
            c["prune_3_windows"] += op["window"] == WINDOW and tot["moved_bytes"] > 2 * WINDOW
            c["prune_after_copy"] += tot["removed"] > 0 and was == "copy"
            c["prune_over_65536"] += tot["removed"] > 0 and tot["kept"] > 65536
            if n_before and not n_after:
                c["emptied"] += 1
                emptied.add(name)
        elif kind == "copy":
            c["copy_refused_missing"] += res["refused"] == "missing"
            c["copy_refused_capacity"] += res["refused"] == "capacity"
            c["copy_after_prune"] += ok and tot["copied"] > 0 and was == "prune"
            c["copy_over_65536"] += ok and tot["copied"] > 65536
        elif kind == "grow":
            c["grow"] += ok
        elif kind == "grow_refused":
            c["grow_refused"] += res["refused"] == "capacity"
        elif kind == "put_sealed":
            c["put_sealed"] += ok and tot["stored"] > 0
    c = {k: int(v) for k, v in c.items()}
    c.update(ops=len(kinds), up=sorted(up), down=sorted(down), kinds=kinds)
    return c


def known_conditions(profile, seed):
    """What the known ops of a script meet, counted over the script's own ops
    on the model's walk: a known op on a store whose last change was a prune
    with remove that removed, a copy that copied, a Grow; one on B as the
    step straight after one on A (one context, one KnownScratch) with another
    chunk count; and what the answers hold."""
    pool = pool_of(profile)
    c = dict.fromkeys(("known", "after_prune_remove", "after_copy", "after_grow", "b_after_a", "liar_ids",
                       "recognised", "hashed", "both_in_one", "big_recognised", "big_hashed",
                       "empty_recognised"), 0)
    last = {}
    prev = None
    for pos, op, want, _states, extra in walk(profile, seed):
        kind, name = op["op"], op.get("store")
        if kind in MUTATING:
            tot = want.get("totals") or {}
            if want.get("refused"):
                pass
            elif kind == "prune" and tot["removed"]:
                last[name] = "prune_remove" if op["remove"] else "prune"
            elif kind == "remove_chunk":
                last[name] = "prune_remove"
            elif kind == "copy" and tot["copied"]:
                last[name] = "copy"
            elif kind == "grow":
                last[name] = "grow"
            elif kind in ("put", "put_sealed") and tot["stored"]:
                last[name] = "put"
        if kind == "known" and not extra:
            ids = [want["ids"][k:k + 32] for k in range(0, len(want["ids"]), 32)]
            sizes = pool.sizes[op["picks"]]
            rec = np.array(want["known_off"]) != known_ref.OFF_NONE
            assert int(rec.sum()) == want["recognised"]  # (narrow: the store holds an ID only with its bytes)
            c["known"] += 1
            for what in ("prune_remove", "copy", "grow"):
                c["after_" + what] += last.get(name) == what
            c["b_after_a"] += (name == "B" and prev is not None and prev["op"] == "known"
                               and prev["store"] == "A" and len(prev["picks"]) != len(op["picks"]))
            c["liar_ids"] += sum(i in pool.liars for i in ids)
            c["recognised"] += want["recognised"]
            c["hashed"] += want["hashed"]
            c["both_in_one"] += want["recognised"] > 0 and want["hashed"] > 0
            c["big_recognised"] += int((rec & (sizes == BIG)).sum())
            c["big_hashed"] += int((~rec & (sizes == BIG)).sum())
            c["empty_recognised"] += int((rec & (sizes == 0)).sum())
        prev = op
    return {k: int(v) for k, v in c.items()}
