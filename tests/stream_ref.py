"""The streaming chunker ABI (dsx_stream_*, include/dsx.h) as seeded scripts of
pushes, pops and restarts: the ops, a model that says what every call may
return, a pure-Python stream on the oracle (ModelBackend), the script
generators S1-S8 and the driver that runs one script on a backend and stops at
the first op the model does not allow.  test_stream_host.py runs the scripts
on the ModelBackend; test_gpu_stream_life.py gives the driver a backend over
libdsx.so's raw C ABI.  No GPU and no torch here.

Exact expectations rest on DSX_STREAM_SYNC: commit(n, SYNC) scans everything
held as a non-final batch and collects it, so a script places batch seams at
any byte, and what the library has confirmed afterwards is the chain rule with
is_last = false over the bytes fed since the chain origin (oracle/seam.py's
spec_chain): `confirmable(fed)`.  The model asserts
  * always: the chunks popped since the chain origin are a prefix of
    confirmable(fed) (a pop that returns 0 early is legal);
  * after a SYNC commit: popping until 0 yields exactly confirmable(fed);
  * after EOF: popping until dsx_stream_done() yields exactly
    o.chunk_stream(data[origin:fed]) shifted by origin.

An op is a dict with "op" and its arguments (byte ranges of the script's data
are explicit); a result is a dict of plain values, so two runs compare with ==.
"""
import functools
import hashlib
import itertools

import numpy as np

from oracle import oracle as o
from oracle import seam as oseam

OK, E_INVAL, E_STATE = 0, -6, -12
F_EOF, F_SYNC = 1, 2
SHA512_256, SHA256 = 0, 1
BATCH, BATCH_IDS = 8 << 20, 128 << 20  # bytes per product batch (with chunk IDs)
SMALL, MID, DEFAULT = (64, 256, 1024), (4096, 16384, 65536), (16384, 65536, 262144)
CAPS = (1, 2, 7, 128)


def odd_sizes(prm):
    """The push sizes S1 cycles through."""
    return (0, 1, 47, 48, 49, prm[0] - 1, prm[2], prm[2] + 1)


def digest(algo, data):
    return hashlib.new("sha512_256", data).digest() if algo == SHA512_256 else hashlib.sha256(data).digest()


def joined(seed, pieces, piece, mx, tail=0):
    """`pieces` runs of o.synth_uniform (seeds seed, seed + 1, ...; `piece`
    bytes each, `tail` more on the last) joined with zero runs of 5*max + 17
    bytes, so that forced start + max cuts occur."""
    gen = o.synth_uniform_c if piece >= (1 << 20) else o.synth_uniform
    zero = np.zeros(5 * mx + 17, np.uint8)
    parts = []
    for i in range(pieces):
        if i:
            parts.append(zero)
        parts.append(gen(seed + i, 0, piece + (tail if i == pieces - 1 else 0)))
    return np.concatenate(parts)


# ---- the chain rule over a byte range ----------------------------------------------------
def confirmable_of(arr, prm):
    """The cuts a non-final scan of `arr` (a chain that starts at arr[0])
    confirms, relative to its start."""
    if len(arr) == 0:
        return []
    cands = o.candidates(arr, *prm).tolist()
    return oseam.spec_chain(cands, 0, prm[0], prm[2], len(arr), len(arr), False)


def final_of(arr, prm):
    return o.chunk_stream(arr, *prm).tolist() if len(arr) else []


# ---- the model ---------------------------------------------------------------------------
class Model:
    """What every call of a script may return, from the script's data alone."""

    def __init__(self, datasets):
        self.datasets = datasets
        self.active = False
        self.eof = False
        self.c = dict.fromkeys(COUNTERS, 0)
        self.sizes, self.skip_commits, self.caps = set(), set(), set()
        self.sync_points = []  # (data key, params, origin, fed) of every SYNC commit
        self.unpopped = False  # the last call was an unpop that gave chunks back
        self._cands, self._whole = {}, {}

    # -- the reference lists --
    def confirmable(self, H):
        if H <= self.origin:
            return []
        k = (self.key, self.prm, self.origin)
        if k not in self._cands:
            self._cands[k] = o.candidates(self.data[self.origin:], *self.prm)
        c = self._cands[k]
        rel = H - self.origin
        c = c[:np.searchsorted(c, rel, "right")].tolist()
        return [self.origin + x for x in oseam.spec_chain(c, 0, self.prm[0], self.prm[2], rel, rel, False)]

    def whole(self, origin):
        """The cuts of the stream from `origin` continued behind the data by
        2*max zeros (a cut at or before a position does not depend on the
        bytes behind it, so these are the cuts of any continuation)."""
        k = (self.key, self.prm, origin)
        if k not in self._whole:
            ext = np.concatenate([self.data[origin:], np.zeros(2 * self.prm[2], np.uint8)])
            self._whole[k] = [origin + x for x in final_of(ext, self.prm)]
        return self._whole[k]

    def allowed(self):
        k = (self.origin, self.fed, self.eof)
        if self._allowed_key != k:
            if self.eof:
                self._allowed = [self.origin + x for x in final_of(self.data[self.origin:self.fed], self.prm)]
            else:
                self._allowed = self.confirmable(self.fed)
            self._allowed_key = k
        return self._allowed

    def _restart(self, at):
        self.origin = self.cur = at
        self.taken, self.must, self.issued, self.group = [], 0, False, None
        self.seams, self.drained, self._allowed_key = [], False, None

    def _id_of(self, lo, hi):
        return digest(self.ids, self.data[lo:hi].tobytes())

    # -- one op --
    def apply(self, op, res):
        """None, or what is wrong with `res`."""
        if not self.active and op["op"] not in ("begin", "end", "dense_mark", "dense_check"):
            return None if res["rc"] == E_STATE else f"rc {res['rc']} on a context without a stream, want {E_STATE}"
        return getattr(self, "_" + op["op"])(op, res)

    def _begin(self, op, res):
        if self.active:
            finished = self.eof and len(self.taken) == len(self.allowed())
            if finished and not self.drained:
                raise AssertionError("bad script: begin where dsx_stream_done() is not determined")
            if not finished:
                self.c["refused_begin"] += 1
                return None if res["rc"] == E_STATE else f"begin on an unfinished stream: rc {res['rc']}"
            self.c["begin_after_done"] += 1
        if res["rc"] != OK:
            return f"begin: rc {res['rc']}"
        if not self.active and self.c["begin"] and tuple(op["params"]) != self.prm:
            self.c["begin_other_params"] += 1  # (after an end, on the buffers the stream before sized)
        self.c["begin"] += 1
        self.active, self.eof = True, False
        self.prm, self.key, self.data = tuple(op["params"]), op["data"], self.datasets[op["data"]]
        self.fed = self.src = self.skip = 0
        self.ids, self.batch, self.skip_n = -1, BATCH, 0
        self._restart(0)
        return None

    def _end(self, op, res):
        self.active, self.group = False, None
        return None if res["rc"] == OK else f"end: rc {res['rc']}"

    def _feed(self, op, res, n, flags):
        if self.eof:
            self.c["refused_after_eof_" + op["op"]] += 1
            return None if res["rc"] == E_STATE else f"{op['op']} after EOF: rc {res['rc']}, want {E_STATE}"
        if res["rc"] != OK:
            return f"{op['op']}: rc {res['rc']}"
        assert op["lo"] == self.src, "bad script: the bytes fed are not the next ones"
        self.sizes.add(n)
        self.c["want_gt_n"] += op.get("want", n) > n
        if self.skip and n:
            d = min(self.skip, n)
            self.skip, n, self.skip_n = self.skip - d, n - d, self.skip_n + 1
            self.src += d
            if not self.skip:
                self.skip_commits.add(self.skip_n)
        self.src += n
        sched = self.seams[-1] if self.seams else self.origin
        self.fed += n
        if res["hend"] != self.fed:
            return f"{op['op']}: the window ends at {res['hend']}, want {self.fed}"
        if self.fed - self.origin > self.batch:
            self.issued = True
        if flags & F_EOF:
            self.eof = True
            all_scanned = self.fed == sched and self.fed > self.origin
            self.c["eof_after_sync_all" + ("_ids" if self.ids >= 0 else "")] += all_scanned
            self.c["eof_one_byte"] += self.fed - sched == 1
            self.c["empty_stream"] += self.fed == 0
            self.c["shorter_than_min"] += 0 < self.fed - self.origin < self.prm[0]
            if self.fed > sched:
                self.seams.append(self.fed)
                self.issued = True
            self.must = len(self.allowed())
        elif flags & F_SYNC:
            self.sync_points.append((self.key, self.prm, self.origin, self.fed))
            if self.fed > sched:
                self.c["single_byte_batch"] += self.fed - sched == 1
                self.seams.append(self.fed)
                self.issued = True
                conf, w = self.confirmable(self.fed), set(self.whole(self.origin))
                if conf and conf[-1] == self.fed:
                    forced = self.fed - (conf[-2] if len(conf) > 1 else self.origin) == self.prm[2]
                    self.c["sync_on_max_cut" if forced else "sync_on_hash_cut"] += 1
                self.c["sync_before_cut"] += self.fed + 1 in w
                self.c["sync_after_cut"] += self.fed - 1 in w
            self.must = len(self.confirmable(self.fed))
        return None

    def _push(self, op, res):
        return self._feed(op, res, op["n"], F_EOF if op["eof"] else 0)

    def _fill(self, op, res):
        return self._feed(op, res, op["n"], op["flags"])

    def _buffer_only(self, op, res):
        want = E_STATE if self.eof else OK
        self.c["refused_after_eof_buffer"] += self.eof
        return None if res["rc"] == want else f"buffer: rc {res['rc']}, want {want}"

    def _commit_only(self, op, res):
        want = E_STATE if self.eof else OK
        self.c["refused_after_eof_commit"] += self.eof
        return None if res["rc"] == want else f"commit: rc {res['rc']}, want {want}"

    def _chunk(self, start, end, ok, cid, where):
        """One popped chunk [start, end) against the lists."""
        al = self.allowed()
        k = len(self.taken)
        if k >= len(al):
            return f"{where}: chunk [{start}, {end}) before its cut is confirmed ({k} confirmable at fed {self.fed})"
        if (start, end) != (self.cur, al[k]):
            return f"{where}: chunk [{start}, {end}), want [{self.cur}, {al[k]})"
        if not ok:
            return f"{where}: the bytes of chunk [{start}, {end}) differ from the data"
        if self.ids >= 0:
            if cid is None:
                return f"{where}: chunk [{start}, {end}) has no ID"
            if cid != self._id_of(start, end):
                return f"{where}: wrong ID for chunk [{start}, {end})"
        elif cid is not None:
            return f"{where}: an ID without dsx_stream_ids"
        inside = sum(start < s < end for s in self.seams)
        self.c["chunk_3_batches" + ("_ids" if self.ids >= 0 else "")] += inside >= 2
        self.taken.append(end)
        self.cur = end
        return None

    def _empty(self, res, where):
        if len(self.taken) < self.must:
            return f"{where}: returned 0 with {self.must - len(self.taken)} confirmed chunks unpopped"
        if res["start"] != self.cur:
            return f"{where}: start {res['start']}, want {self.cur}"
        if self.eof and len(self.taken) == len(self.allowed()):
            self.drained = True
        return None

    def _done_is(self, res, where):
        finished = self.eof and len(self.taken) == len(self.allowed())
        if not finished and res["done"] != 0:
            return f"{where}: dsx_stream_done() is {res['done']} before the last pop"
        if finished and self.drained and res["done"] != 1:
            return f"{where}: dsx_stream_done() is {res['done']} after the last pop"
        return None

    def _pop(self, op, res, where="pop"):
        self.group = None
        if res["rc"] == 1:
            bad = self._chunk(res["start"], res["start"] + res["size"], res["ok"], res["id"], where)
            self.c["pop_after_unpop"] += bad is None and self.unpopped
        elif res["rc"] == 0:
            bad = self._empty(res, where)
        else:
            bad = f"{where}: rc {res['rc']}"
        self.unpopped = False
        return bad or self._done_is(res, where)

    def _pop_many(self, op, res, where="pop_many"):
        self.group = None
        self.caps.add(op["cap"])
        if op["with_ids"] and self.ids < 0:
            self.c["refused_pop_many_ids"] += 1
            return None if res["rc"] == E_STATE and not res["ends"] else \
                f"{where} asks for IDs without dsx_stream_ids: rc {res['rc']}, want {E_STATE}"
        if res["rc"] == 0:
            return self._empty(res, where) or self._done_is(res, where)
        if res["rc"] != 1:
            return f"{where}: rc {res['rc']} ({len(res['ends'])} chunks)"
        n, queued = len(res["ends"]), self.must - len(self.taken)
        if not 1 <= n <= op["cap"]:
            return f"{where}: {n} chunks for cap {op['cap']}"
        if not self.eof and n < min(op["cap"], queued):
            return f"{where}: {n} chunks, {queued} are queued"
        if not res["ok"]:
            return f"{where}: the bytes from dsx_stream_chunk_data() differ from the data"
        start, lo = res["start"], res["start"]
        for i, e in enumerate(res["ends"]):
            cid = res["ids"][i] if res["ids"] is not None else (self._id_of(lo, e) if self.ids >= 0 else None)
            bad = self._chunk(lo, e, True, cid, f"{where} chunk {i}")
            if bad:
                return bad
            lo = e
        self.c["pop_after_unpop"] += self.unpopped
        self.unpopped = False
        self.c["pop_many_ids" if op["with_ids"] else "pop_many_no_ids" if self.ids >= 0 else "pop_many_plain"] += 1
        wpos, wlen, wok = res["window"]
        if wpos > start or wpos + wlen != self.fed or not wok:
            return f"{where}: the window [{wpos}, {wpos + wlen}) {'holds' if wok else 'differs from'} the data, " \
                   f"want [{start}, {self.fed}) covered"
        self.group = (start, list(res["ends"]))
        return self._done_is(res, where)

    def _drain(self, op, res):
        for i, step in enumerate(res["steps"]):
            where = f"drain step {i}"
            bad = self._pop_many(op, step, where) if op["cap"] else self._pop(op, step, where)
            if bad:
                return bad
        self.group = None
        return None

    def _unpop(self, op, res):
        if res["pos"] is None:
            assert self.group is None, "the driver lost a live group"
            return None
        assert self.group is not None, "the driver kept a dead group"
        start, ends = self.group
        pos = start if op["k"] == 0 else ends[min(op["k"], len(ends)) - 1]
        if res["pos"] != pos:
            return f"unpop: the driver asked for {res['pos']}, the model for {pos}"
        if res["rc"] != OK:
            return f"unpop({pos}): rc {res['rc']}"
        self.c["unpop_mid"] += start < pos < ends[-1]
        self.c["unpop_start"] += pos == start
        self.unpopped = pos < ends[-1]
        self.taken = [t for t in self.taken if t <= pos]
        self.cur, self.group = pos, None
        return None

    def _advance(self, op, res):
        if res["rc"] != OK:
            return f"advance: rc {res['rc']}"
        n, held = op["n"], self.fed - self.cur
        tag = "_ids" if self.ids >= 0 else ""
        kind = ("adv_eof_inside" if n <= held else "adv_eof_past") if self.eof else \
            "adv_zero" if n == 0 else "adv_inside" if n < held else "adv_exact" if n == held else \
            "adv_past_1" if n == held + 1 else "adv_past_3max" if n >= held + 3 * self.prm[2] else "adv_past"
        self.c[kind + tag] += 1
        self.c["adv_before_first" + tag] += self.fed == 0
        self.c["adv_after_unpop" + tag] += self.unpopped
        self.c["adv_on_pending_skip"] += self.skip > 0
        target = self.cur + n
        if target > self.fed:  # (bytes still owed to an earlier Advance stay owed)
            self.skip += target - self.fed
            self.fed = target
            self.skip_n = 0
        self._restart(target)
        self.unpopped = False
        if self.eof:
            self.skip = 0
            self.issued = self.fed > target
            self.must = len(self.allowed())
        if res["hend"] != self.fed:
            return f"advance: the window ends at {res['hend']}, want {self.fed}"
        return None

    def _flush(self, op, res):
        if res["rc"] != OK:
            return f"flush: rc {res['rc']}"
        if (res["start"], res["size"]) != (self.cur, self.fed - self.cur):
            return f"flush: chunk [{res['start']}, +{res['size']}), want [{self.cur}, +{self.fed - self.cur})"
        if not res["ok"]:
            return "flush: the bytes of the chunk differ from the data"
        if res["id"] is not None:
            return "flush: the chunk has an ID (it is hashed by nobody)"
        self.c["flush"] += 1
        self.eof = False
        self._restart(self.fed)
        self.unpopped = False
        return None

    def _ids(self, op, res):
        if self.issued:
            self.c["refused_ids"] += 1
            return None if res["rc"] == E_STATE else f"ids mid-chain: rc {res['rc']}, want {E_STATE}"
        if res["rc"] != OK:
            return f"ids({op['algo']}): rc {res['rc']}"
        self.c["ids_on" if op["algo"] >= 0 else "ids_off"] += 1
        self.c["ids_toggle_at_restart"] += self.origin > 0 and (op["algo"] >= 0) != (self.ids >= 0)
        self.ids = op["algo"]
        if op["algo"] >= 0:
            self.batch = BATCH_IDS
        self.group = None
        return None

    def _done(self, op, res):
        return self._done_is(res, "done")

    def _dense_mark(self, op, res):
        self.dense0 = res["count"]
        return None

    def _dense_check(self, op, res):
        if res["count"] is not None and not res["count"] > self.dense0:
            return f"dense_fallbacks stayed at {res['count']}: no dense redo inside the stream"
        return None


COUNTERS = (
    "begin", "begin_after_done", "begin_other_params", "refused_begin", "refused_ids", "refused_pop_many_ids",
    "refused_after_eof_push", "refused_after_eof_fill", "refused_after_eof_buffer", "refused_after_eof_commit",
    "want_gt_n", "sync_on_hash_cut", "sync_on_max_cut", "sync_before_cut", "sync_after_cut", "single_byte_batch",
    "chunk_3_batches", "chunk_3_batches_ids", "eof_after_sync_all", "eof_after_sync_all_ids", "eof_one_byte",
    "empty_stream", "shorter_than_min", "pop_after_unpop", "unpop_mid", "unpop_start", "pop_many_ids",
    "pop_many_no_ids", "pop_many_plain", "flush", "ids_on", "ids_off", "ids_toggle_at_restart", "adv_on_pending_skip",
) + tuple(k + t for t in ("", "_ids") for k in (
    "adv_zero", "adv_inside", "adv_exact", "adv_past_1", "adv_past_3max", "adv_past", "adv_eof_inside",
    "adv_eof_past", "adv_before_first", "adv_after_unpop"))


# ---- a pure-Python stream on the oracle ------------------------------------------------------
class ModelBackend:
    """dsx_stream_* restated on the oracle, over the bytes it is given (not
    the script's data): every held byte is scanned at a SYNC or EOF commit and
    never earlier, which the model allows."""
    fake_base = 0x1000

    def __init__(self):
        self.active = False
        self.h = np.empty(1 << 16, np.uint8)

    # -- internals --
    def _restart(self, at):
        self.cuts, self.idq, self.has_id, self.pin = [], [], False, at
        self.grp, self.grp_ids = [], []
        self.origin = self.sched = self.carry = at
        self.done_ = self.final_pending = False

    def _held(self, lo, hi):
        return self.h[lo - self.hbase:hi - self.hbase]

    def _queue(self, cuts):
        for e in cuts:
            if e > self.carry:
                self.cuts.append(e)
                if self.ids_ >= 0:
                    self.idq.append(digest(self.ids_, self._held(self.carry, e).tobytes()))
                self.carry = e

    def _scan(self, last):
        arr = self._held(self.origin, self.hend)
        cuts = final_of(arr, self.prm) if last else self.confirmed(arr)
        self._queue([self.origin + x for x in cuts])
        self.sched = self.hend
        if last:
            self.done_ = True

    def confirmed(self, arr):
        return confirmable_of(arr, self.prm)

    def _pump(self, sync):
        if self.eof:
            if self.hend > self.sched:
                self._scan(True)
            elif not self.done_:
                self.final_pending = True
        elif sync and self.hend > self.sched:
            self._scan(False)

    # -- the ABI --
    def begin(self, mn, av, mx):
        if self.active and not (self.done_ and not self.cuts):
            return E_STATE
        self.active, self.eof, self.ids_, self.prm = True, False, -1, (mn, av, mx)
        self.hbase = self.hend = self.cur = self.skip = 0
        self.want = 0
        self._restart(0)
        return OK

    def end(self):
        self.active = False
        return OK

    def buffer(self, want):
        if not self.active or self.eof:
            return E_STATE
        need = self.hend - self.hbase + want
        if need > len(self.h):  # (a grow: a new base pointer)
            n = np.empty(max(2 * len(self.h), need), np.uint8)
            n[:self.hend - self.hbase] = self.h[:self.hend - self.hbase]
            self.h, self.fake_base = n, self.fake_base + 0x1000
        self.want = want
        return OK

    def dropped(self, n):
        """The bytes of a commit of n that an Advance beyond the held bytes drops."""
        d = min(self.skip, n)
        self.skip -= d
        return d

    def commit_bytes(self, data, flags):
        if not self.active or self.eof:
            return E_STATE
        n = len(data)
        if n > self.want:
            return E_INVAL
        d = self.dropped(n) if self.skip and n else 0
        at = self.hend - self.hbase
        self.h[at:at + n - d] = data[d:]
        self.hend += n - d
        self.eof = bool(flags & F_EOF)
        self._pump(bool(flags & F_SYNC))
        return OK

    def commit(self, n, flags):
        return self.commit_bytes(np.empty(0, np.uint8), flags) if n == 0 else E_INVAL

    def push(self, data, eof):
        return self.buffer(len(data)) or self.commit_bytes(data, F_EOF if eof else 0)

    def pop(self):
        if not self.active:
            return E_STATE, 0, 0, None, None
        if not self.cuts and self.final_pending:
            self._queue([self.hend])
            self.final_pending, self.done_ = False, True
        if not self.cuts:
            return 0, self.cur, 0, None, None
        e = self.cuts.pop(0)
        self.has_id = False
        if self.idq and len(self.idq) > len(self.cuts):  # aligned from the back
            self.last_id, self.has_id = self.idq.pop(0), True
        start, self.pin, self.cur = self.cur, self.cur, e
        return 1, start, e - start, self._held(start, e), self.last_id if self.has_id else None

    def pop_many(self, cap, with_ids):
        if with_ids and self.ids_ < 0:
            return E_STATE, 0, [], None, None
        rc, first, _, _, _ = self.pop()
        if rc <= 0:
            return rc, first, [], None, None
        ends, idl, self.grp, self.grp_ids = [], [], [], []
        while True:
            ends.append(self.cur)
            self.grp.append(self.cur)
            if self.has_id:
                self.grp_ids.append(self.last_id)
            if with_ids and not self.has_id:
                self.pin, self.grp_ids = first, []
                self.unpop(ends[-2] if len(ends) > 1 else first)
                ends.pop()
                return (1 if ends else E_STATE), first, ends, idl, self._held(first, ends[-1] if ends else first)
            idl.append(self.last_id if self.has_id else None)
            if len(ends) >= cap or not self.cuts:
                break
            if self.pop()[0] <= 0:
                break
        self.pin = first
        return 1, first, ends, (idl if with_ids else None), self._held(first, ends[-1])

    def unpop(self, pos):
        if pos == self.cur:
            return OK
        if pos < self.pin or pos > self.cur:
            return E_INVAL
        with_ids = len(self.grp_ids) == len(self.grp)
        for i in reversed(range(len(self.grp))):
            if self.grp[i] <= pos:
                break
            self.cuts.insert(0, self.grp[i])
            if with_ids:
                self.requeue_id(self.grp_ids[i])
        self.cur, self.grp, self.grp_ids = pos, [], []
        return OK

    def requeue_id(self, cid):
        self.idq.insert(0, cid)

    def window(self):
        return self.fake_base, self.hbase, self.h[:self.hend - self.hbase]

    def advance(self, n):
        target = self.cur + n
        if target > self.hend:
            self.skip += target - self.hend
            self.hbase = self.hend = target
        self.cur = target
        self._restart(target)
        if self.eof:
            self.skip = 0
            self._pump(False)
        return OK

    def flush(self):
        start, size = self.cur, self.hend - self.cur
        chunk = self._held(start, self.hend)
        self.cur = self.hend
        cid = self.flush_id()
        self._restart(self.hend)
        self.eof = False
        return OK, start, size, chunk, cid

    def flush_id(self):
        return None

    def ids(self, algo):
        if self.sched != self.origin or self.cuts:
            return E_STATE
        self.ids_ = algo
        return OK

    def done(self):
        return int(self.active and self.done_ and not self.cuts)

    def dense_fallbacks(self):
        return None


# ---- the driver -------------------------------------------------------------------------------
def new_state(datasets):
    return {"datasets": datasets, "data": None, "group": None, "room": {"grow": 0, "move": 0, "neither": 0}}


def _same(got, data, lo, hi):
    return 0 <= lo <= hi <= len(data) and len(got) == hi - lo and bool(np.array_equal(np.asarray(got), data[lo:hi]))


def _pop_res(be, data):
    rc, start, size, chunk, cid = be.pop()
    return {"rc": rc, "start": start, "size": size, "ok": rc != 1 or _same(chunk, data, start, start + size),
            "id": cid, "done": be.done()}


def _pop_many_res(be, data, st, cap, with_ids):
    rc, start, ends, ids, chunk = be.pop_many(cap, with_ids)
    res = {"rc": rc, "start": start, "ends": list(ends), "ids": None if ids is None else list(ids), "ok": True,
           "window": None, "done": be.done()}
    if rc == 1 and ends:
        res["ok"] = _same(chunk, data, start, ends[-1])
        _, wpos, win = be.window()
        inside = wpos <= start <= wpos + len(win)
        res["window"] = (wpos, len(win), inside and _same(win[start - wpos:], data, start, wpos + len(win)))
        st["group"] = (start, list(ends))
    return res


def execute(op, be, st):
    """One op on a backend -> its result (with the bytes the calls expose
    already compared with the script's data)."""
    k, data = op["op"], st["data"]
    if k not in ("push", "fill", "buffer_only", "commit_only", "done", "dense_mark", "dense_check", "pop_many",
                 "unpop"):
        group, st["group"] = st["group"], None  # a group lives across feeding calls and queries only
    if k == "begin":
        rc = be.begin(*op["params"])
        if rc == OK:
            st["data"] = st["datasets"][op["data"]]
        return {"rc": rc}
    if k == "end":
        return {"rc": be.end()}
    if k in ("push", "fill"):
        base0, pos0, _ = be.window()
        piece = data[op["lo"]:op["lo"] + op["n"]]
        assert len(piece) == op["n"], "bad script: it feeds more than its data"
        if k == "push":
            rc = be.push(piece, op["eof"])
        else:
            rc = be.buffer(op["want"]) or be.commit_bytes(piece, op["flags"])
        base, pos, win = be.window()
        if rc == OK:
            st["room"]["grow" if base != base0 else "move" if pos > pos0 else "neither"] += 1
        return {"rc": rc, "hend": pos + len(win)}
    if k == "buffer_only":
        return {"rc": be.buffer(op["want"])}
    if k == "commit_only":
        return {"rc": be.commit(0, op["flags"])}
    if k == "pop":
        return _pop_res(be, data)
    if k == "pop_many":
        st["group"] = None
        return _pop_many_res(be, data, st, op["cap"], op["with_ids"])
    if k == "drain":
        steps = []
        while len(steps) < 1 << 20:
            steps.append(_pop_many_res(be, data, st, op["cap"], op["with_ids"]) if op["cap"] else _pop_res(be, data))
            if steps[-1]["rc"] != 1:
                break
        st["group"] = None
        return {"rc": steps[-1]["rc"], "steps": steps}
    if k == "unpop":
        group, st["group"] = st["group"], None
        if group is None:
            return {"rc": OK, "pos": None}
        pos = group[0] if op["k"] == 0 else group[1][min(op["k"], len(group[1])) - 1]
        return {"rc": be.unpop(pos), "pos": pos}
    if k == "advance":
        rc = be.advance(op["n"])
        _, pos, win = be.window()
        return {"rc": rc, "hend": pos + len(win)}
    if k == "flush":
        rc, start, size, chunk, cid = be.flush()
        return {"rc": rc, "start": start, "size": size, "ok": rc != OK or _same(chunk, data, start, start + size),
                "id": cid}
    if k == "ids":
        return {"rc": be.ids(op["algo"])}
    if k == "done":
        return {"rc": OK, "done": be.done()}
    if k in ("dense_mark", "dense_check"):
        return {"rc": OK, "count": be.dense_fallbacks()}
    raise AssertionError(f"unknown op {k}")


def describe(op):
    return " ".join([op["op"]] + [f"{k}={v}" for k, v in op.items() if k != "op"])


class Mismatch(AssertionError):
    def __init__(self, name, pos, ops, what):
        self.name, self.pos, self.what = name, pos, what
        last = "; ".join(f"[{i}] {describe(ops[i])}" for i in range(max(0, pos - 4), pos + 1))
        super().__init__(f"{name}, op {pos}: {what}\nlast five ops: {last}")


def record(backend, sc):
    """The script's results on a backend, unjudged."""
    st = new_state(sc["data"])
    return [execute(op, backend, st) for op in sc["ops"]]


def drive(backend, sc, log=None):
    """Runs script `sc` on `backend` and raises Mismatch at the first op whose
    result the model does not allow.  -> the model (its counters, and which of
    the host buffer's three outcomes the feeding calls showed)."""
    model, st = Model(sc["data"]), new_state(sc["data"])
    for pos, op in enumerate(sc["ops"]):
        try:
            res = execute(op, backend, st)
        except Exception as e:
            raise Mismatch(sc["name"], pos, sc["ops"], f"{describe(op)} raised {e!r}") from e
        if log is not None:
            log.append(res)
        what = model.apply(op, res)
        if what:
            raise Mismatch(sc["name"], pos, sc["ops"], what)
    model.room = st["room"]
    return model


# ---- the script generators ----------------------------------------------------------------------
class Builder:
    """Writes a script while it runs it on the model and the ModelBackend, so
    that a generator can ask where the stream stands."""

    def __init__(self, name, datasets):
        self.name, self.datasets, self.ops = name, datasets, []
        self.m, self.be, self.st = Model(datasets), ModelBackend(), new_state(datasets)

    def do(self, **op):
        self.ops.append(op)
        res = execute(op, self.be, self.st)
        what = self.m.apply(op, res)
        assert not what, (self.name, len(self.ops) - 1, describe(op), what)
        return res

    def script(self):
        return {"name": self.name, "ops": tuple(self.ops), "data": self.datasets}

    @property
    def left(self):
        return len(self.m.data) - self.m.src

    def begin(self, prm, key):
        return self.do(op="begin", params=tuple(prm), data=key)

    def push(self, n, eof=0):
        return self.do(op="push", lo=self.m.src, n=min(int(n), self.left), eof=int(eof))

    def fill(self, n, want=None, flags=0):
        n = min(int(n), self.left)
        return self.do(op="fill", lo=self.m.src, n=n, want=n if want is None else int(want), flags=flags)

    def sync(self, n):
        return self.fill(n, flags=F_SYNC)

    def eof(self, n):
        return self.fill(n, flags=F_EOF)

    def pop(self):
        return self.do(op="pop")

    def pop_many(self, cap, with_ids=False):
        return self.do(op="pop_many", cap=int(cap), with_ids=bool(with_ids))

    def drain(self, cap=0, with_ids=False):
        return self.do(op="drain", cap=int(cap), with_ids=bool(with_ids))

    def unpop(self, k):
        return self.do(op="unpop", k=int(k))

    def advance(self, n):
        return self.do(op="advance", n=int(n))

    def flush(self):
        return self.do(op="flush")

    def ids(self, algo):
        return self.do(op="ids", algo=int(algo))

    def end(self):
        return self.do(op="end")

    def done(self):
        return self.do(op="done")

    def feed_to(self, pos, sizes):
        """Pushes of `sizes` until the next bytes reach stream position `pos`
        exactly; the last commit is a SYNC."""
        need = pos - self.m.fed + self.m.skip
        assert 0 < need <= self.left, (pos, need, self.left)
        if need > 4 * self.m.prm[2]:  # (the way there in one piece)
            self.push(need - 3 * self.m.prm[2])
            need = 3 * self.m.prm[2]
        while True:
            n = next(sizes)
            if n >= need:
                return self.sync(need)
            self.push(n)
            need -= n


def s1():
    """Seams, no IDs: a SYNC at c - 1, c and c + 1 of three hash cuts and two
    start + max cuts, with one restart per case; pushes of the odd sizes."""
    prm = SMALL
    b = Builder("S1", {"d": joined(101, 22, 44 << 10, prm[2])})
    b.begin(prm, "d")
    sizes, restarts = itertools.cycle(odd_sizes(prm)), itertools.cycle(("flush", "exact", "past"))
    for forced, nth in ((False, 2), (False, 5), (False, 9), (True, 0), (True, 1)):
        for delta in (-1, 0, 1):
            o0 = b.m.origin
            assert o0 == b.m.fed
            w = b.m.whole(o0)
            kind = [c for p, c in zip([o0] + w, w) if (c - p == prm[2]) == forced]
            b.feed_to(kind[nth] + delta, sizes)
            b.drain()
            how = next(restarts)
            if how == "flush":
                b.flush()
            else:
                b.advance(b.m.fed - b.m.cur + (3 if how == "past" else 0))
    b.eof(500)
    b.drain()
    b.end()
    return b.script()


def _adv_amount(rng, b, kind):
    held, mx = b.m.fed - b.m.cur, b.m.prm[2]
    return {"zero": 0, "inside": int(rng.integers(0, held + 1)), "exact": held,
            "past": held + int(rng.integers(1, 300)),
            "far": held + 3 * mx + int(rng.integers(0, 50))}[kind]


def s2(seed, prm, total):
    """A seeded mix of about 150 ops drawn from all of them."""
    rng = np.random.default_rng([2, seed])
    mx = prm[2]
    pieces = 4
    b = Builder(f"S2-{seed}", {"d": joined(200 + 10 * seed, pieces, (total - 3 * (5 * mx + 17)) // pieces, mx)})
    b.begin(prm, "d")
    algo = (-1, SHA512_256, SHA256)[seed % 3]
    if algo >= 0:
        b.ids(algo)
    step = total // 50

    def size():
        return int(rng.choice(odd_sizes(prm))) if rng.random() < 0.3 else int(rng.integers(1, 2 * step))

    while len(b.ops) < 150:
        r = rng.random()
        if b.m.eof and r < 0.3 or b.left == 0:
            if not b.m.eof:
                b.eof(0)
            b.drain(int(rng.choice(CAPS)), b.m.ids >= 0)
            b.end()
            b.begin(prm, "d")
            if algo >= 0:
                b.ids(algo)
        elif r < 0.26:
            b.push(size())
        elif r < 0.42:
            b.sync(size())
        elif r < 0.47:
            n = size()
            b.fill(n, n + int(rng.integers(1, 3 * mx)))
        elif r < 0.57:
            b.pop()
        elif r < 0.70:
            b.pop_many(int(rng.choice(CAPS)), b.m.ids >= 0 and rng.random() < 0.5)
        elif r < 0.77:
            b.unpop(int(rng.integers(0, 4)))
        elif r < 0.81:
            b.drain(int(rng.choice((0,) + CAPS)), b.m.ids >= 0 and rng.random() < 0.5)
        elif r < 0.87:
            b.advance(_adv_amount(rng, b, str(rng.choice(("zero", "inside", "exact", "past", "far")))))
        elif r < 0.90:
            b.flush()
        elif r < 0.94:
            b.ids(algo if b.m.ids < 0 and algo >= 0 else -1)
        elif r < 0.96:
            if b.m.ids < 0:
                b.pop_many(int(rng.choice(CAPS)), True)
            else:
                b.begin(prm, "d") if not (b.m.eof and len(b.m.taken) == len(b.m.allowed())) else b.done()
        elif r < 0.98:
            b.do(op="buffer_only", want=int(rng.integers(0, 4 * mx)))
        else:
            b.done()
    if not b.m.eof:
        b.eof(min(b.left, step))
    b.drain()
    b.end()
    return b.script()


def s3(algo):
    """IDs across seams: a zero run fed 20 KiB per SYNC (a chunk over four
    batches), batches of one byte, pop_many with and without IDs, IDs switched
    off and on at a flush and at an advance, refused mid-chain."""
    prm, other = MID, SHA256 if algo == SHA512_256 else SHA512_256
    rng = np.random.default_rng([3, algo])
    piece = (3 << 20) // 3 - (5 * prm[2] + 17)
    b = Builder(f"S3-{algo}", {"d": joined(300 + algo, 3, piece, prm[2])})
    b.begin(prm, "d")
    b.ids(algo)
    with_ids = itertools.cycle((True, False))

    def pops():
        if rng.random() < 0.5:
            b.pop_many(int(rng.choice(CAPS)), next(with_ids))  # (refused while the IDs are off)
            if rng.random() < 0.5:
                b.unpop(int(rng.integers(0, 3)))
        b.drain(int(rng.choice((0, 7, 128))), next(with_ids) and b.m.ids >= 0)

    def stretch(upto, zero_from):
        while b.m.src < upto:
            if b.m.src >= zero_from:
                b.sync(min(20 << 10, upto - b.m.src))
                if rng.random() < 0.4:
                    pops()
                continue
            n = int(rng.choice((1, 1, 47, 4095, 20000, 70000, 150000, 200000)))
            n = min(n, zero_from - b.m.src, upto - b.m.src)
            b.sync(n) if rng.random() < 0.8 else b.push(n)
            if rng.random() < 0.6:
                pops()

    run = 5 * prm[2] + 17
    stretch(piece + run, piece)                    # the first zero run in 20 KiB batches
    b.sync(1)
    b.ids(-1)                                      # mid-chain: refused
    pops()
    b.flush()
    b.ids(-1)                                      # IDs off at a flush ...
    stretch(piece + run + 300000, 1 << 40)
    b.ids(algo)                                    # (refused: mid-chain)
    b.drain()
    b.advance(b.m.fed - b.m.cur)
    b.ids(other)                                   # ... and the other digest at an advance
    stretch(2 * (piece + run), 2 * piece + run)    # the second zero run
    b.sync(100000)
    b.pop_many(7, True)
    b.unpop(3)                                     # to the middle of the group: the same chunks and IDs again
    b.pop()
    b.pop_many(2, False)
    b.unpop(1)
    b.pop_many(128, True)
    pops()
    b.flush()
    b.ids(algo)
    stretch(len(b.m.data) - 5000, 1 << 40)
    b.sync(4999)
    b.eof(1)
    b.drain(128, True)
    b.end()
    return b.script()


def s4():
    """Advance: by 0, inside a held chunk, exactly to fed, 1 and 3*max bytes
    beyond it with the skipped bytes over 1, 2 and 5 commits, before the first
    byte, after EOF, with chunks popped ahead and unpopped; IDs off and on."""
    prm = SMALL
    mn, _, mx = prm
    b = Builder("S4", {"d": joined(401, 6, 40 << 10, mx)})
    for algo in (-1, SHA512_256):
        b.begin(prm, "d")
        if algo >= 0:
            b.ids(algo)
        wid = algo >= 0
        b.advance(37)                              # before the first byte
        b.sync(4000)
        b.pop()
        b.pop()
        b.advance(0)                               # the held bytes start a chain of their own
        b.sync(1000)
        b.drain()
        b.sync(3000)
        b.pop()
        b.advance(max(1, (b.m.allowed()[len(b.m.taken)] - b.m.cur) // 3))  # inside the next chunk
        b.sync(500)
        b.drain(7, wid)
        b.sync(2000)
        b.pop()
        b.advance(b.m.fed - b.m.cur)               # exactly to fed
        b.sync(2000)
        b.drain()
        b.advance(b.m.fed - b.m.cur + 1)           # 1 byte beyond: one commit
        b.sync(1500)
        b.drain(2, wid)
        b.advance(b.m.fed - b.m.cur + 1)
        b.push(0)                                  # ... an empty commit first
        b.sync(1500)
        b.drain()
        for commits in ((3 * mx + 500,), (2 * mx, mx + 700), (mx, 1, mx - 1, mx // 2, mx // 2 + 900)):
            b.advance(b.m.fed - b.m.cur + 3 * mx)  # 3*max beyond: the skipped bytes over 1, 2, 5 commits
            for i, n in enumerate(commits):
                if i == len(commits) - 1:
                    b.sync(n)
                elif i == 2:
                    b.fill(n, n + 777)
                else:
                    b.push(n)
            b.drain()
        b.advance(b.m.fed - b.m.cur + 10)          # an Advance on top of bytes still owed
        b.advance(0)
        b.advance(5)
        b.sync(3000)
        b.drain()
        b.sync(6000)
        b.pop_many(7, wid)
        b.unpop(3)                                 # to the middle of the group; the same chunks and IDs again
        b.pop()
        b.pop_many(7, wid)
        b.unpop(2)                                 # chunks popped ahead go back first
        b.advance(50)
        b.sync(100)
        b.drain(128, wid)
        b.sync(5000)
        b.pop_many(128, False)
        b.unpop(0)
        b.advance(b.m.fed - b.m.cur - 1)
        b.eof(3000)
        b.pop()
        b.advance((b.m.fed - b.m.cur) // 2)        # after EOF, inside the held bytes
        b.drain(7, wid)
        b.done()
        b.end()
        b.begin(prm, "d")
        if algo >= 0:
            b.ids(algo)
        b.sync(2000)
        b.eof(1000)
        b.pop()
        b.advance(b.m.fed - b.m.cur + 5)           # after EOF, beyond them: the stream is over
        b.drain()
        b.done()
        b.end()
    return b.script()


def s5():
    """The end of a stream: EOF right after a SYNC of all bytes (IDs off and
    on, the queue popped in between or not), EOF with one byte left, an empty
    stream, one shorter than min, exactly max zeros; done() and the calls
    refused after EOF."""
    prm = SMALL
    b = Builder("S5", {"d": joined(501, 2, 8 << 10, prm[2]), "z": np.zeros(prm[2], np.uint8)})

    def refused():
        b.do(op="buffer_only", want=10)
        b.do(op="commit_only", flags=0)
        b.push(0)
        b.fill(0, 5)

    for algo in (-1, SHA512_256, SHA256):
        for popped in (True, False):
            b.begin(prm, "d")
            if algo >= 0:
                b.ids(algo)
            b.push(3000)
            b.sync(b.left)
            if popped:
                b.drain(7 if algo >= 0 else 0, algo >= 0)
            b.eof(0)
            b.done()
            refused()
            b.drain(128 if not popped else 0, algo >= 0 and not popped)
            b.done()
            b.end()
        b.begin(prm, "d")
        if algo >= 0:
            b.ids(algo)
        b.sync(b.left - 1)
        b.eof(1)                                   # one byte left
        b.drain(0, False)
        b.done()
        b.end()
        b.begin(prm, "d")                          # an empty stream
        if algo >= 0:
            b.ids(algo)
        b.eof(0)
        b.done()
        b.pop()
        b.done()
        refused()
        b.begin(prm, "d")                          # (it ended on its own: no end)
        if algo >= 0:
            b.ids(algo)
        b.push(prm[0] - 5, eof=1)                  # shorter than min
        b.drain(2, algo >= 0)
        b.done()
        b.begin(prm, "z")
        if algo >= 0:
            b.ids(algo)
        b.eof(prm[2])                              # exactly max zeros
        b.drain()
        b.done()
        b.begin(prm, "z")
        if algo >= 0:
            b.ids(algo)
        b.sync(prm[2])                             # ... and with the SYNC on the forced cut
        b.eof(0)
        b.drain(1, algo >= 0)
        b.done()
        b.end()
    return b.script()


def s6():
    """Context reuse: a stream at 16K/64K/256K, end, one at 64/256/1024 with
    IDs whose first batch has seventy times the cuts; begin refused while a
    stream is unfinished and accepted after one ended on its own."""
    b = Builder("S6", {"big": joined(601, 2, 1 << 20, DEFAULT[2]), "small": joined(602, 3, 300 << 10, SMALL[2])})
    b.begin(DEFAULT, "big")
    b.push(1 << 20)
    b.sync(1 << 20)
    b.pop_many(128)
    b.begin(SMALL, "small")                        # refused
    b.sync(500000)
    b.pop()
    b.end()                                        # unfinished, dropped
    b.begin(SMALL, "small")
    b.ids(SHA256)
    b.sync(600 << 10)                              # ~2,400 cuts in one batch
    b.drain(128, True)
    b.begin(DEFAULT, "big")                        # refused
    b.sync(b.left - 70)
    b.pop_many(7, True)
    b.unpop(2)
    b.eof(70)
    b.drain(128, True)
    b.done()
    b.begin(SMALL, "small")                        # accepted: the stream ended on its own
    b.sync(100000)                                 # (begin switched the IDs off)
    b.drain(128, False)
    b.eof(10)
    b.drain()
    b.end()
    return b.script()


def s7():
    """Product batches and the host buffer, default params, 44 MiB + 13: run 1
    pushes seeded pieces of 1-3 MiB and pops after each.  The buffer moves its
    held bytes down only when they are at most a quarter of it, and it holds
    everything from the last popped group on: the piece before the one that
    overflows the 32 MiB buffer is a SYNC popped chunk by chunk, so that the
    consumer and the pinned chunk stand within two chunks of the fed position.
    Run 2, on the same context, feeds 40 MiB before its first pop: the buffer
    grows."""
    prm = DEFAULT
    total = (44 << 20) + 13
    run = 5 * prm[2] + 17
    b = Builder("S7", {"p": joined(701, 2, (total - run) // 2, prm[2], tail=(total - run) % 2)})
    assert len(b.datasets["p"]) == total
    rng = np.random.default_rng(7)
    for second in (False, True):
        sizes, left = [], total
        while left:
            sizes.append(min(left, int(rng.integers(1 << 20, (3 << 20) + 1))))
            left -= sizes[-1]
        ends = np.cumsum(sizes).tolist()
        sync_at = next(i for i in range(len(sizes)) if ends[i] + sizes[i + 1] > 4 * BATCH)
        b.begin(prm, "p")
        for i, n in enumerate(sizes):
            last = i == len(sizes) - 1
            if second:
                b.push(n, eof=last)
                if ends[i] >= 40 << 20:
                    b.drain(4096)
            elif i == sync_at:
                b.sync(n)
                b.drain()                          # one by one: the last pop pins one chunk, not the group
            else:
                b.push(n, eof=last)
                b.drain(4096)
        b.done()
        b.end()
    return b.script()


def s8(algo):
    """The dense redo inside a stream: a tile with a candidate every 48 bytes
    behind 1 MiB of uniform data and a SYNC, so the lane overflow is found on
    a batch that continues a chain."""
    from test_gpu_seam_record import dense_tile
    data = np.concatenate([o.synth_uniform(801, 0, 1 << 20), dense_tile(), o.synth_uniform(802, 0, 64 << 10)])
    b = Builder(f"S8-{algo}", {"t": data})
    b.begin(DEFAULT, "t")
    if algo >= 0:
        b.ids(algo)
    b.sync(1 << 20)
    b.drain()
    b.do(op="dense_mark")
    b.sync(len(dense_tile()))
    b.do(op="dense_check")
    b.pop_many(7, algo >= 0)
    b.unpop(3)
    b.drain(128, algo >= 0)
    b.eof(b.left)
    b.drain()
    b.done()
    b.end()
    return b.script()


S2_CASES = ((1, SMALL, 2 << 20), (2, SMALL, 2 << 20), (3, SMALL, 2 << 20), (4, MID, 6 << 20))
SCRIPTS = {"S1": s1, "S4": s4, "S5": s5, "S6": s6, "S7": s7}
SCRIPTS.update({f"S2-{seed}": functools.partial(s2, seed, prm, total) for seed, prm, total in S2_CASES})
SCRIPTS.update({f"S3-{a}": functools.partial(s3, a) for a in (SHA512_256, SHA256)})
SCRIPTS.update({f"S8-{a}": functools.partial(s8, a) for a in (-1, SHA512_256)})
NAMES = sorted(SCRIPTS)


@functools.lru_cache(maxsize=None)
def script(name):
    """The deterministic script `name`: {"name", "ops", "data"}."""
    return SCRIPTS[name]()
