"""A context's chain state through seeded scripts of mixed calls.

Every cut list comes from one chain state per context (dsx_ctx::state and the
staging list dsx_ctx::out) that every chain call shares: dsx_cut_device
(synchronous and queued), dsx_cut_device_many, dsx_cut_host, dsx_index_host,
the stream's batches and the shards.  include/dsx.h ("One chain state per
context", beside dsx_ctx_create) says which call may run inside which
protocol; csrc/dsx_chain_owner.h is the rule in code.  This module has the
inputs, the scripts, a model that predicts every call's answer, and the driver
that compares a backend with the model:

    script(seed)        60 ops; chain ops are drawn inside live protocols on purpose
    conditions(seed)    what a script holds (tests/test_ctx_life_host.py asserts it)
    Model               the contract: code, exact list, IDs, untouched outputs, the
                        protocol dsx_last_error names
    ModelBackend        the model as a backend (and the base of the broken fakes)
    drive(backend, ops) runs a script; Mismatch at the first op that differs

No GPU import here: tests/test_gpu_ctx_life.py has the backend over libdsx.so.
"""
import functools
import hashlib

import numpy as np

import cut_cap_ref as cc
from oracle import oracle as o
from oracle import seam

KiB, MiB = 1024, 1 << 20
OK, E_INVAL, E_CAPACITY, E_STATE = 0, -6, -7, -12
SHA512_256, SHA256 = 0, 1  # DSX_DIGEST_*

# the parameter sets; "D" (cut_cap_ref.DFLT) is the one at which the dense tile
# is dense and the zero-run composition was built
PSETS = {"A": (2 * KiB, 8 * KiB, 32 * KiB), "B": (4096, 16384, 65536), "D": cc.DFLT}

BATCH = 8 * MiB            # the product library's stream batch (dsx_stream_begin)
STREAM_LEN = 20 * MiB + 5  # three batches: the second and third on a carried chain
STREAM_PSET = "B"
SHARD_LEN, SHARD_SPLIT, SHARD_PSET = 3 * MiB, 1_500_001, "B"
QUEUE_DEPTH = 8            # kQueueDepth

SEEDS = (1, 2, 3, 4, 5, 6, 7)
NOPS = 60

CHAIN_KINDS = ("cut", "cut_queued", "many", "cut_host", "index_host", "shard_local")
SYNC_KINDS = ("cut", "many", "cut_host", "index_host", "shard_local")
NEUTRAL_KINDS = ("chunk_ids", "idset_dedup", "store_put_read", "known", "aead")
FAILING_KINDS = ("cut_short", "queued_short", "many_refused")
RESOLVES = ("shard_resolve", "shard_collect")


def _sum(data, algo=SHA512_256):
    return (hashlib.new("sha512_256", data) if algo == SHA512_256 else hashlib.sha256(data)).digest()


# ------------------------------------------------------------------ the pool
class Pool:
    """The blobs, built once, with the oracle's list per parameter set."""

    def __init__(self):
        self.blobs = {
            "u256k": o.synth_uniform(91, 0, 256 * KiB),
            "u1m": o.synth_uniform(92, 0, 1 * MiB + 12345),
            "u3m": o.synth_uniform(93, 0, 3 * MiB + 1),
            "zero": cc.zero_runs().data,
            "dense": cc.dense_small().data,
            "tiny": o.synth_uniform(94, 0, 1000),
            "empty": np.empty(0, np.uint8),
        }
        self.psets = {name: ("A", "B") for name in self.blobs}
        self.psets["zero"] = ("A", "B", "D")
        self.psets["dense"] = ("D",)  # (dense at this discriminator only)
        self._want = {}
        self._ids = {}
        self.stream = o.synth_uniform(95, 0, STREAM_LEN)
        self.stream_want = o.chunk_stream(self.stream, *PSETS[STREAM_PSET])
        self.shard = o.synth_uniform(96, 0, SHARD_LEN)
        whole = o.chunk_stream(self.shard, *PSETS[SHARD_PSET])
        self.shard_geo = ((0, SHARD_SPLIT), (SHARD_SPLIT, SHARD_LEN - SHARD_SPLIT))
        self.shard_want = [whole[(whole > np.uint64(s)) & (whole <= np.uint64(s + n))]
                           for s, n in self.shard_geo]

    def want(self, blob, pset):
        key = (blob, pset)
        if key not in self._want:
            assert pset in self.psets[blob], key
            d = self.blobs[blob]
            if blob == "zero" and pset == "D":
                w = cc.zero_runs().want
            elif blob == "dense":
                w = cc.dense_small().want
            else:
                w = o.chunk_stream(d, *PSETS[pset]) if d.size else np.empty(0, np.uint64)
            self._want[key] = w
        return self._want[key]

    def ids(self, blob, pset, algo=SHA512_256):
        key = (blob, pset, algo)
        if key not in self._ids:
            raw, s, out = self.blobs[blob].tobytes(), 0, []
            for e in self.want(blob, pset).tolist():
                out.append(_sum(raw[s:e], algo))
                s = e
            self._ids[key] = out
        return self._ids[key]

    def many(self, op):
        """dsx_cut_device_many's arguments and answer for a many op ->
        (data, blob_ends, ends, first, groups, singles)."""
        parts = [self.blobs[b] for b in op["blobs"]]
        data = np.concatenate(parts) if parts else np.empty(0, np.uint8)
        be = np.cumsum([p.size for p in parts]).astype(np.uint64)
        if op.get("bad"):
            be = be.copy()
            be[0], be[1] = be[1], be[0]  # (decreasing)
            return data, be, None, None, 0, 0
        ends, first, b0 = [], [0], 0
        for b, p in zip(op["blobs"], parts):
            e = self.want(b, op["pset"]) + np.uint64(b0)
            ends.append(e)
            first.append(first[-1] + e.size)
            b0 += p.size
        groups, singles = many_items(be, op["big_blob"] or many_default_big(op["pset"]),
                                     op["group_bytes"] or (8 << 30))
        return (data, be, np.concatenate(ends) if ends else np.empty(0, np.uint64),
                np.array(first, np.uint64), groups, singles)

    def shard_converges(self):
        """oracle/seam.py on the CPU: both ranks resolve in one round to the
        true chain's cuts of their shard (the scripts never need a resync)."""
        p = PSETS[SHARD_PSET]
        total = SHARD_LEN
        recs, spec = [], []
        for s, n in self.shard_geo:
            rec, cuts, _ = seam.shard_local(self.shard, s, n, total, *p)
            recs.append(rec)
            spec.append(cuts)
        for r in (0, 1):
            res = seam.resolve(recs, r, p[0], p[2])
            if res[0] != "ok":
                return False
            got = seam.rank_cuts(res[1], res[2], spec[r])
            # (a rank's list ends at its shard's end: the cuts past it are the next rank's)
            s, n = self.shard_geo[r]
            got = got[got <= np.uint64(s + n)]
            if not np.array_equal(got, self.shard_want[r]):
                return False
        return True


@functools.lru_cache(maxsize=None)
def pool():
    return Pool()


def many_default_big(pset):
    """many_default_big_blob (dsx_engine.cpp): min(kManyMaxBatched, 4088 * d);
    far above every blob of the pool."""
    return 4088 * int(o.params(*PSETS[pset]).d)


def many_items(blob_ends, big_blob, group_bytes):
    """many_plan (csrc/dsx_many_plan.h) restated -> (groups, singles): the scan
    launches of the batched walk and the blobs on the one-blob path."""
    groups = singles = 0
    is_open, start, b0 = False, 0, 0
    for b1 in (int(x) for x in blob_ends):
        n = b1 - b0
        if n == 0:
            continue
        single = n >= big_blob or n > group_bytes
        if not single and is_open and b1 - start <= group_bytes:
            pass
        else:
            start = b0
            if single:
                singles += 1
            else:
                groups += 1
            is_open = not single
        b0 = b1
    return groups, singles


def op_len(op):
    """Bytes a chain op chunks."""
    P = pool()
    if op["op"] == "many":
        return sum(P.blobs[b].size for b in op["blobs"])
    if op["op"] == "shard_local":
        return P.shard_geo[op["rank"]][1]
    return P.blobs[op["blob"]].size


def op_upper(op):
    """The documented bound of a chain op's cut count."""
    mn = PSETS[op["pset"]][0] if "pset" in op else PSETS[SHARD_PSET][0]
    if op["op"] == "many":
        return op_len(op) // mn + len(op["blobs"])
    return op_len(op) // mn + 2


# ----------------------------------------------------------------- the model
class Expect(dict):
    """A call's predicted answer: rc; n (the count, None: not asserted); list
    (the exact cut list, None: none returned); ids; first / groups / singles
    (many); untouched (a sentinel-filled output must be as it was); err (what
    dsx_last_error must contain); value (a neutral op's result); popq (a
    stream_pop_all: the chunks so far must continue the oracle's list)."""

    def __getattr__(self, k):
        return self.get(k)


class Model:
    """The contract of include/dsx.h, "One chain state per context"."""

    def __init__(self):
        self.P = pool()
        self.stream = None  # {"pushed", "popped", "eof"}
        self.shard = None   # {"rank", "stale", "pending"}: since the last dsx_shard_local
        self.round_open = False  # a shard_local whose resolve or collect is still to come
        self.queue = []     # the queued ops, oldest first
        self.last_list = np.empty(0, np.uint64)  # (what the last chain call left: the fakes)

    # -- state
    def stream_unfinished(self):
        s = self.stream
        return s is not None and not (s["eof"] and s["popped"] == self.P.stream_want.size)

    def batches_issued(self):
        s = self.stream
        if s is None:
            return 0
        if s["eof"]:
            return -(-s["pushed"] // BATCH)
        return max(0, (s["pushed"] - 1) // BATCH)  # (one byte is held back)

    def shard_valid(self):
        return self.shard is not None and not self.shard["stale"]

    def allows_plain_cut(self):
        """The driver's periodic cut: only where it changes no later answer."""
        return not self.stream_unfinished() and not self.round_open

    def _refuse_in_stream(self):
        return Expect(rc=E_STATE, err="stream", untouched=True)

    def _chain(self):
        """A chain call other than dsx_shard_local runs: a waiting shard is stale."""
        if self.shard is not None:
            self.shard["stale"] = True

    # -- one op: predict() is pure, commit() moves the state
    def predict(self, op):
        k = op["op"]
        P = self.P
        if k in ("cut", "cut_host", "index_host"):
            if self.stream_unfinished():
                return self._refuse_in_stream()
            w = P.want(op["blob"], op["pset"])
            if op.get("short"):
                assert w.size >= 2
                # (a failed call leaves a host output as it was; a device
                # output nothing at or past cap)
                return Expect(rc=E_CAPACITY, n=w.size, untouched=op.get("out") != "device")
            e = Expect(rc=OK, n=w.size, list=w)
            if k == "index_host":
                e["ids"] = P.ids(op["blob"], op["pset"], op["algo"])
            return e
        if k == "cut_queued":
            if self.stream_unfinished():
                return self._refuse_in_stream()
            assert P.blobs[op["blob"]].size, "an empty blob is not queued"
            if len(self.queue) >= QUEUE_DEPTH:
                return Expect(rc=E_STATE, err="queued", untouched=True)
            return Expect(rc=OK)
        if k == "result":
            if not self.queue:
                return Expect(rc=E_STATE)
            q = self.queue[0]
            w = P.want(q["blob"], q["pset"])
            if q["blob"] == "dense" and self.stream_unfinished():
                return self._refuse_in_stream()  # (the redo is a chain call; the scripts never get here)
            if q.get("short"):
                return Expect(rc=E_CAPACITY, n=w.size)
            return Expect(rc=OK, n=w.size, list=w)
        if k == "many":
            if op.get("bad"):  # refused on its arguments, before the owner is asked
                return Expect(rc=E_INVAL, err="blob ends decrease", untouched=True)
            if self.stream_unfinished():
                return self._refuse_in_stream()
            _, _, ends, first, groups, singles = P.many(op)
            return Expect(rc=OK, n=ends.size, list=ends, first=first, groups=groups, singles=singles)
        if k == "shard_local":
            if self.stream_unfinished():
                return Expect(rc=E_STATE, err="stream")
            return Expect(rc=OK)
        if k in ("shard_resolve", "shard_resolve_async"):
            if self.shard is None or self.shard["stale"]:
                return Expect(rc=E_STATE, err="shard", untouched=True)
            if k == "shard_resolve_async":
                return Expect(rc=OK)
            w = P.shard_want[self.shard["rank"]]
            return Expect(rc=OK, n=w.size, list=w)
        if k == "shard_collect":
            if self.shard is None or not self.shard["pending"] or self.shard["stale"]:
                return Expect(rc=E_STATE, err="shard")
            w = P.shard_want[self.shard["rank"]]
            return Expect(rc=OK, n=w.size, list=w)
        if k == "stream_begin":
            if self.stream_unfinished():
                return Expect(rc=E_STATE, err="stream")  # (no output to leave alone)
            if self.queue:
                return Expect(rc=E_STATE, err="queued")
            return Expect(rc=OK)
        if k == "stream_push":
            assert self.stream is not None and not self.stream["eof"]
            return Expect(rc=OK)
        if k == "stream_pop_all":
            s = self.stream
            assert s is not None
            return Expect(rc=OK, popq=(s["popped"], s["pushed"], s["eof"]))
        if k == "stream_end":
            return Expect(rc=OK)
        if k in NEUTRAL_KINDS:
            return Expect(rc=OK, value=neutral_value(op))
        raise ValueError(k)

    def commit(self, op, exp, got=None):
        k = op["op"]
        if k in RESOLVES or (k == "shard_resolve_async" and exp.rc != OK):
            self.round_open = False
        if exp.rc == E_STATE or exp.rc == E_INVAL:
            if k == "result" and self.queue:
                self.queue.pop(0)  # (a refused redo loses its call)
            if k == "shard_collect" and self.shard is not None:
                self.shard["pending"] = False
            return
        if k in ("cut", "cut_host", "index_host", "many"):
            self._chain()
            self.last_list = exp.list if exp.list is not None else self.last_list
        elif k == "cut_queued":
            self._chain()
            self.queue.append(op)
            self.last_list = self.P.want(op["blob"], op["pset"])
        elif k == "result":
            q = self.queue.pop(0)
            if q["blob"] == "dense":
                self._chain()  # dsx_result's synchronous redo
                self.last_list = self.P.want(q["blob"], q["pset"])
        elif k == "shard_local":
            self.shard = {"rank": op["rank"], "stale": False, "pending": False}
            self.round_open = True
            self.last_list = self.P.shard_want[op["rank"]]
        elif k == "shard_resolve_async":
            self.shard["pending"] = True
        elif k == "shard_collect":  # (like a resolved shard, it stays valid until a chain call)
            self.shard["pending"] = False
        elif k == "stream_begin":
            self._chain()
            self.stream = {"pushed": 0, "popped": 0, "eof": False}
        elif k == "stream_push":
            self.stream["pushed"] += op["n"]
            self.stream["eof"] = bool(op.get("eof"))
        elif k == "stream_pop_all":
            self.stream["popped"] += len(got["list"])
        elif k == "stream_end":
            self.stream = None


def neutral_value(op):
    """What a neutral op must return, from hashlib and numpy alone."""
    P = pool()
    k, blob, pset = op["op"], op["blob"], op["pset"]
    want, raw = P.want(blob, pset), P.blobs[blob].tobytes()
    if k == "chunk_ids":
        return tuple(P.ids(blob, pset, op["algo"]))
    ids = P.ids(blob, pset)
    if k == "idset_dedup":
        # the list: every ID, then the first half again; the seed: every other ID
        lst = ids + ids[:max(1, len(ids) // 2)]
        seed = ids[::2]
        first, where = [], {}
        for i, x in enumerate(lst):
            where.setdefault(x, i)
            first.append(where[x])
        spos = {}
        for i, x in enumerate(seed):
            spos.setdefault(x, i)
        return tuple(first), tuple(spos.get(x, 0xFFFFFFFF) for x in lst)
    if k == "store_put_read":
        return hashlib.sha256(b"".join(raw[a:a + n] for a, n in read_ranges_of(op))).hexdigest()
    if k == "known":
        return tuple(ids), len(ids)  # the IDs, and every chunk found in the store
    if k == "aead":
        return hashlib.sha256(raw).hexdigest(), int(want.size)
    raise ValueError(k)


def read_ranges_of(op):
    """store_put_read's byte ranges: the head, a stretch across the middle
    chunk ends, the last byte."""
    n = pool().blobs[op["blob"]].size
    return [(0, min(n, 100)), (n // 3, min(n - n // 3, 70001)), (n - 1, 1)]


def dedup_list(op):
    """idset_dedup's arguments -> (ids, sizes, seed ids)."""
    P = pool()
    ids = P.ids(op["blob"], op["pset"])
    w = P.want(op["blob"], op["pset"])
    sizes = np.diff(np.concatenate([[np.uint64(0)], w]).astype(np.int64)).astype(np.uint64)
    k = max(1, len(ids) // 2)
    return ids + ids[:k], np.concatenate([sizes, sizes[:k]]), ids[::2]


# --------------------------------------------------------------- the scripts
def _cut(blob, pset, out="host", short=False):
    return {"op": "cut", "blob": blob, "pset": pset, "out": out, "short": short}


class _Gen:
    """Builds one script; its own Model knows which protocol is live."""

    SAFE = ("u256k", "u1m", "tiny")  # no longer than a shard, cut with the shard's min

    def __init__(self, seed):
        self.rng = np.random.default_rng(7000 + seed)
        self.pad_rng = np.random.default_rng(9000 + seed)  # (its own: the pads move no segment)
        self.m = Model()
        self.ops = []

    @property
    def shard_live(self):
        return self.m.round_open

    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def emit(self, op):
        exp = self.m.predict(op)
        got = realize(self.m, op, exp)
        self.m.commit(op, exp, got)
        self.ops.append(op)
        return exp

    # -- arguments
    def blob(self, queued=False):
        """(blob, pset) of a cut: inside a shard round only what an unguarded
        library could run in bounds."""
        if self.shard_live:
            return self.pick(self.SAFE), SHARD_PSET
        names = ["u256k", "u1m", "u3m", "zero", "tiny", "dense"] + ([] if queued else ["empty"])
        b = self.pick(names)
        return b, self.pick(pool().psets[b])

    def many_op(self, variant=None, out=None):
        v = int(self.rng.integers(4)) if variant is None else variant
        blobs, group, big = {
            0: (("u256k", "tiny", "empty", "u256k"), 0, 0),                 # one scan
            1: (("u256k", "tiny", "empty", "u256k"), 300 * KiB, 0),         # two scans
            2: (("u256k", "tiny", "u256k", "u256k"), 300 * KiB, 0),         # three scans
            3: (("tiny", "u1m", "tiny"), 0, 512 * KiB),                     # group, one-blob path, group
        }[v]
        pset = SHARD_PSET if self.shard_live else self.pick(("A", "B"))
        return {"op": "many", "blobs": blobs, "pset": pset, "out": out or self.pick(("host", "device")),
                "group_bytes": group, "big_blob": big, "bad": False}

    def chain_op(self, kind):
        if kind == "cut":
            b, p = self.blob()
            return _cut(b, p, self.pick(("host", "device")))
        if kind == "cut_queued":
            b, p = self.blob(queued=True)
            return {"op": "cut_queued", "blob": b, "pset": p, "short": False}
        if kind == "many":
            return self.many_op()
        if kind == "cut_host":
            b, p = self.blob()
            return {"op": "cut_host", "blob": b, "pset": p}
        if kind == "index_host":
            b, p = self.blob()
            return {"op": "index_host", "blob": b, "pset": p, "algo": self.pick((SHA512_256, SHA256))}
        if kind == "shard_local":
            return {"op": "shard_local", "rank": int(self.rng.integers(2)),
                    "nosync": bool(self.rng.integers(2))}
        raise ValueError(kind)

    def neutral_op(self, kind):
        op = {"op": kind, "blob": self.pick(("u256k", "u1m")), "pset": self.pick(("A", "B"))}
        if kind == "chunk_ids":
            op["algo"] = self.pick((SHA512_256, SHA256))
        return op

    # -- segments
    def resolve(self, asynchronous=None):
        """The round's resolve, synchronous or resolve_async + collect."""
        if asynchronous is None:
            asynchronous = bool(self.rng.integers(2))
        if not asynchronous:
            return self.emit({"op": "shard_resolve", "out": self.pick(("host", "device"))})
        exp = self.emit({"op": "shard_resolve_async"})
        if exp.rc == OK:
            exp = self.emit({"op": "shard_collect"})
        return exp

    def drain(self):
        while self.m.queue:
            self.emit({"op": "result"})

    def seg_path(self, kinds):
        """The chain kinds one after the other, each adjacent to the next, from
        a quiet context; then the round's resolve, if one is open, and the
        queued calls' results."""
        for k in kinds:
            self.emit(self.chain_op(k))
        if self.shard_live:
            self.resolve()
        self.drain()

    def seg_intrusion(self, kind, between_async=False):
        """local -> the intruder -> resolve; after a refusal the recovery:
        local again, resolve OK."""
        self.emit(self.chain_op("shard_local"))
        if between_async:
            self.emit({"op": "shard_resolve_async"})
        self.emit(self.chain_op(kind) if kind in CHAIN_KINDS else self.neutral_op(kind))
        if between_async:
            exp = self.emit({"op": "shard_collect"})
        else:
            exp = self.resolve()
        self.drain()
        if exp.rc == E_STATE:
            self.emit(self.chain_op("shard_local"))
            exp = self.resolve(asynchronous=False)
            assert exp.rc == OK

    def seg_stream(self, refused, neutral, begin_again, chain_when_finished):
        self.emit({"op": "stream_begin"})
        self.emit({"op": "stream_push", "n": BATCH + 1, "eof": False})
        if self.rng.integers(2):
            self.emit({"op": "stream_pop_all"})
        self.emit({"op": "stream_push", "n": BATCH, "eof": False})  # (batch 2: on the carried chain)
        mid = [self.chain_op(k) for k in refused] + [self.neutral_op(neutral)]
        if begin_again:
            mid.append({"op": "stream_begin"})
        for i in self.rng.permutation(len(mid)):
            self.emit(mid[int(i)])
        self.emit({"op": "stream_pop_all"})
        self.emit({"op": "stream_push", "n": STREAM_LEN - 2 * BATCH - 1, "eof": True})
        self.emit({"op": "stream_pop_all"})
        if chain_when_finished:  # every chunk popped: the stream no longer owns the chain
            self.emit(self.chain_op(chain_when_finished))
            if self.shard_live:
                self.resolve(asynchronous=False)
        self.emit({"op": "stream_end"})

    def seg_queue(self, depth, sync_kind, dense_at, begin_refused):
        """`depth` queued calls, a synchronous chain call with two pending and
        more queued behind it, results oldest first."""
        for i in range(depth):
            if i == 2:
                self.emit(self.chain_op(sync_kind))
                if self.shard_live:
                    self.resolve(asynchronous=False)  # (queued calls pending, nothing between)
                if begin_refused:
                    self.emit({"op": "stream_begin"})
            if i == dense_at:
                self.emit({"op": "cut_queued", "blob": "dense", "pset": "D", "short": False})
            else:
                self.emit(self.chain_op("cut_queued"))
        self.drain()

    def seg_failing(self, which):
        big = self.pick(("u1m", "u3m", "zero"))
        if which == "cut_short":
            self.emit(_cut(big, self.pick(("A", "B")), self.pick(("host", "device")), short=True))
        elif which == "queued_short":
            self.emit({"op": "cut_queued", "blob": big, "pset": self.pick(("A", "B")), "short": True})
            self.emit({"op": "result"})
        else:
            op = self.many_op()
            op["bad"] = True
            self.emit(op)
        self.emit(self.chain_op(self.pick(("cut", "cut_host", "many", "index_host"))))

    def pad(self):
        """A neutral call or a plain cut between two segments."""
        rng, self.rng = self.rng, self.pad_rng
        try:
            k = self.pick(NEUTRAL_KINDS + ("cut", "cut"))
            self.emit(self.chain_op("cut") if k == "cut" else self.neutral_op(k))
        finally:
            self.rng = rng


def _tour():
    """A closed walk over the chain kinds that takes every ordered pair (a, b),
    a == b included, exactly once (Hierholzer): 37 kinds, 36 adjacencies."""
    n = len(CHAIN_KINDS)
    unused = {a: list(range(n)) for a in range(n)}
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if unused[a]:
            stack.append(unused[a].pop())
        else:
            out.append(stack.pop())
    return [CHAIN_KINDS[a] for a in reversed(out)]


def _build(seed, pads):
    """The seed's segments in their seeded order, pads[k] pads before segment k
    (pads[-1]: after the last) -> the _Gen."""
    i = SEEDS.index(seed)
    g = _Gen(seed)
    ns = len(SEEDS)
    tour = _tour()
    lo, hi = i * (len(tour) - 1) // ns, (i + 1) * (len(tour) - 1) // ns
    segs = [lambda: g.seg_path(tour[lo:hi + 1])]  # this seed's share of the ordered pairs
    # every chain kind a second time between local and resolve; every neutral kind once
    segs.append(lambda: g.seg_intrusion(CHAIN_KINDS[i % 6], between_async=i % 2 == 1))
    segs.append(lambda: g.seg_intrusion(CHAIN_KINDS[(i + 2) % 6], between_async=i % 2 == 0))
    segs.append(lambda: g.seg_intrusion(NEUTRAL_KINDS[i % 5]))
    segs.append(lambda: g.seg_stream((CHAIN_KINDS[i % 6], CHAIN_KINDS[(i + 3) % 6]), NEUTRAL_KINDS[(i + 2) % 5],
                                     begin_again=i % 3 == 0,
                                     chain_when_finished=("cut", None, "shard_local")[i % 3]))
    segs.append(lambda: g.seg_queue((4, 5, 4, 8, 4, 6, 4)[i], SYNC_KINDS[i % 5],
                                    dense_at=1 if i in (0, 2, 4, 5) else -1, begin_refused=i in (1, 3, 6)))
    for which in FAILING_KINDS:
        segs.append(lambda which=which: g.seg_failing(which))
    order = [int(k) for k in g.rng.permutation(len(segs))]
    pads = list(pads) + [0] * (len(segs) + 1 - len(pads))
    for n, k in enumerate(order):
        for _ in range(pads[n]):
            g.pad()
        segs[k]()
    for _ in range(pads[len(segs)]):
        g.pad()
    assert g.m.stream is None and not g.m.queue and not g.m.round_open
    g.nsegs = len(segs)
    return g


@functools.lru_cache(maxsize=None)
def script(seed):
    """The 60 ops of a seed (a tuple of dicts: do not change them): the
    segments that hold the conditions, and pads in the gaps up to 60."""
    bare = _build(seed, ())
    spare = NOPS - len(bare.ops)
    assert spare >= 0, (seed, len(bare.ops))
    gaps = np.random.default_rng(8000 + seed).integers(bare.nsegs + 1, size=spare)
    g = _build(seed, np.bincount(gaps, minlength=bare.nsegs + 1).tolist())
    assert len(g.ops) == NOPS, (seed, len(g.ops))
    return tuple(g.ops)


def describe(op):
    return " ".join(f"{k}={v}" for k, v in op.items())


# ---------------------------------------------------------------- conditions
def conditions(seed):
    """Counts what script(seed) holds, by walking it with a Model of its own."""
    ops, m = script(seed), Model()
    c = {"pairs": set(), "intruder_chain": {}, "intruder_neutral": {}, "refused_in_carried_stream": {},
         "neutral_in_stream": {}, "sync_with_two_queued": {}, "dense_queued_with_later": 0,
         "failing_then_chain": 0, "failing": 0, "begin_refused_for_queue": 0, "stale_refusals": 0,
         "stream_refusals": 0, "max_queue": 0, "bounds_ok": True, "nops": len(ops), "scans": set(),
         "direct_resolves": 0, "recoveries": 0}
    ran_prev = None        # the chain kind the previous op ran, or None
    since_local = None     # the ops since the live shard's local
    shard_len = None
    refused_round = False
    for pos, op in enumerate(ops):
        k = op["op"]
        exp = m.predict(op)
        ran = k in CHAIN_KINDS and exp.rc in (OK, E_CAPACITY)
        if ran and ran_prev:
            c["pairs"].add((ran_prev, k))
        # inside a shard round: the unguarded library's bounds
        if since_local is not None and k in CHAIN_KINDS and k != "shard_local" and exp.rc != E_INVAL:
            mn = PSETS[SHARD_PSET][0]
            if not (PSETS[op["pset"]][0] == mn and op_len(op) <= shard_len
                    and op_upper(op) <= shard_len // mn + 4):
                c["bounds_ok"] = False
        if since_local is not None and k != "shard_local" and (k in CHAIN_KINDS or k in NEUTRAL_KINDS):
            since_local.append(k)
        round_ends = k in RESOLVES or (k == "shard_resolve_async" and exp.rc != OK)
        if round_ends and since_local is not None:
            for x in since_local:
                if x in CHAIN_KINDS:
                    c["intruder_chain"][x] = c["intruder_chain"].get(x, 0) + 1
                elif x in NEUTRAL_KINDS:
                    c["intruder_neutral"][x] = c["intruder_neutral"].get(x, 0) + 1
            if exp.rc == OK and not since_local:
                c["direct_resolves"] += 1
                c["recoveries"] += refused_round
            refused_round = exp.rc == E_STATE
            since_local = None
        if k in ("shard_resolve", "shard_resolve_async", "shard_collect") and exp.rc == E_STATE and exp.err == "shard":
            c["stale_refusals"] += 1
        if m.stream_unfinished():
            if exp.rc == E_STATE and exp.err == "stream":
                c["stream_refusals"] += 1
                if k in CHAIN_KINDS and m.batches_issued() >= 2:
                    c["refused_in_carried_stream"][k] = c["refused_in_carried_stream"].get(k, 0) + 1
            if k in NEUTRAL_KINDS:
                c["neutral_in_stream"][k] = c["neutral_in_stream"].get(k, 0) + 1
        if k == "stream_begin" and exp.rc == E_STATE and exp.err == "queued":
            c["begin_refused_for_queue"] += 1
        if ran and k in SYNC_KINDS and len(m.queue) >= 2:
            c["sync_with_two_queued"][k] = c["sync_with_two_queued"].get(k, 0) + 1
        if k == "many" and exp.rc == OK:
            c["scans"].add((exp.groups, exp.singles))
        failing = exp.rc in (E_CAPACITY, E_INVAL)
        if failing:
            c["failing"] += 1
            nxt = ops[pos + 1] if pos + 1 < len(ops) else None
            c["failing_then_chain"] += nxt is not None and nxt["op"] in CHAIN_KINDS
        got = realize(m, op, exp)
        m.commit(op, exp, got)
        if k == "shard_local" and exp.rc == OK:  # (inside a round: the intruder that replaces the shard)
            since_local, shard_len = (["shard_local"] if since_local is not None else []), op_len(op)
        c["max_queue"] = max(c["max_queue"], len(m.queue))
        ran_prev = k if ran else None
    # the dense tile queued with later calls behind it
    q = []
    for op in ops:
        if op["op"] == "cut_queued":
            q.append(op)
        elif op["op"] == "result" and q:
            first = q.pop(0)
            c["dense_queued_with_later"] += first["blob"] == "dense" and len(q) >= 1
    return c


# ------------------------------------------------------------------ the driver
class Mismatch(AssertionError):
    def __init__(self, pos, op, what, extra=False):
        self.pos, self.op, self.what, self.extra = pos, op, what, extra
        super().__init__(f"op {pos}{' (the periodic cut after it)' if extra else ''}: {describe(op)}: {what}")


def realize(model, op, exp):
    """The answer of a library that keeps the contract, as a backend returns
    it: {"rc", "n", "list", "ids", "first", "groups", "singles", "untouched",
    "err", "value"}."""
    got = {"rc": exp.rc, "n": exp.n, "list": exp.list, "ids": exp.ids, "first": exp.first,
           "groups": exp.groups, "singles": exp.singles, "untouched": True if exp.untouched else None,
           "err": f"{exp.err}: refused" if exp.err else "", "value": exp.value}
    if exp.popq is not None:
        base, pushed, eof = exp.popq
        w = model.P.stream_want
        # confirmed: the bytes up to the chunk's start + max are scanned
        mx = PSETS[STREAM_PSET][2]
        hi = w.size if eof else int(np.searchsorted(w, np.uint64(max(0, pushed - 1 - mx)), side="right"))
        got["list"] = w[base:max(base, hi)]
    return got


def compare(model, exp, got):
    """None, or what differs."""
    if got["rc"] != exp.rc:
        return f"returned {got['rc']}, the contract says {exp.rc} (last error: {got.get('err')!r})"
    if exp.n is not None and got["n"] != exp.n:
        return f"count {got['n']}, the oracle's {exp.n}"
    if exp.popq is not None:
        base, pushed, eof = exp.popq
        w, g = model.P.stream_want, np.asarray(got["list"], dtype=np.uint64)
        if g.size and int(g[-1]) > pushed:
            return f"a chunk ends at {int(g[-1])}, {pushed} bytes pushed"
        if not np.array_equal(g, w[base:base + g.size]):
            return f"the stream's chunks from #{base} on differ from the oracle's"
        if eof and base + g.size != w.size:
            return f"{base + g.size} chunks at the end of the stream, the oracle has {w.size}"
    elif exp.list is not None:
        if got["list"] is None or not np.array_equal(np.asarray(got["list"], dtype=np.uint64), exp.list):
            return "the cut list differs from the oracle's"
    if exp.ids is not None and list(got["ids"]) != list(exp.ids):
        return "the chunk IDs differ from hashlib's"
    if exp.first is not None and not np.array_equal(got["first"], exp.first):
        return "blob_first differs"
    if exp.groups is not None and (got["groups"], got["singles"]) != (exp.groups, exp.singles):
        return f"{got['groups']} groups and {got['singles']} one-blob runs, the plan says {exp.groups} and {exp.singles}"
    if exp.untouched and got["untouched"] is not True:
        return "a refused call wrote its output"
    if exp.err and exp.err not in (got.get("err") or "").lower():
        return f"dsx_last_error {got.get('err')!r} does not name the {exp.err!r} protocol"
    if exp.value is not None and got["value"] != exp.value:
        return "a neutral call's result differs"
    return None


PERIODIC = _cut("u256k", SHARD_PSET, "host")


def drive(backend, ops, log=None, extras=True):
    """Runs `ops` on the backend and compares every answer with the model's;
    after every tenth op a plain cut where the model allows one.  Mismatch at
    the first difference; returns the number of ops compared."""
    m = Model()
    done = 0
    for pos, op in enumerate(ops):
        steps = [(op, False)]
        if extras and (pos + 1) % 10 == 0:
            steps.append((PERIODIC, True))
        for step, extra in steps:
            if extra and not m.allows_plain_cut():
                continue
            exp = m.predict(step)
            got = backend.apply(step)
            if log is not None:
                log.append((pos, step, exp.rc, got["rc"]))
            what = compare(m, exp, got)
            if what:
                raise Mismatch(pos, step, what, extra)
            m.commit(step, exp, got)
            done += 1
    return done


class ModelBackend:
    """The model as a backend: what a library that keeps the contract returns."""

    def __init__(self):
        self.m = Model()

    def apply(self, op):
        exp = self.m.predict(op)
        got = realize(self.m, op, exp)
        self.m.commit(op, exp, got)
        return got
