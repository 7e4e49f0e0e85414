"""A context's chain state through seeded scripts of mixed calls, on the GPU.

tests/ctx_life_ref.py has the scripts, the model and the driver
(tests/test_ctx_life_host.py checks them on the CPU); this file has the
backend over libdsx.so's C ABI and one directed test per line of the contract
(include/dsx.h, "One chain state per context"), so that a failure names the
line.  Every list is compared in full with the CPU oracle's, every output the
library writes sits in a sentinel-fenced buffer (cut_cap_ref.FencedOut), and
every script and directed case runs on a context of its own.

The directed tests list the codes they expect.  Should streams and shards get
a chain state of their own one day, only those codes change: the rule stays
"the exact list or the documented refusal, never another list".
"""
import ctypes
import hashlib

import numpy as np
import pytest

import ctx_life_ref as r
from ctx_life_ref import E_CAPACITY, E_INVAL, E_STATE, OK
from cut_cap_ref import SEAM_MAX_CUTS, SENTINEL, FencedOut

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))


# ---------------------------------------------------------------- the inputs
class Inputs:
    """The pool in HBM, uploaded once, and both ranks' seam records from
    helper contexts (the script's context plays one rank, the record of the
    other comes from here)."""

    def __init__(self):
        import torch
        from desync_amd import _lib, shard
        import desync_amd
        self.P = r.pool()
        self.dev = {}
        for name, data in self.P.blobs.items():
            self.dev[name] = torch.from_numpy(np.ascontiguousarray(data)).to("cuda")
        self.shard = torch.from_numpy(self.P.shard).to("cuda")
        self.many = {}
        self.params = {k: desync_amd.Params(*v) for k, v in r.PSETS.items()}
        torch.cuda.synchronize()
        L = _lib.lib()
        self.rec_host, self.rec_dev = [], []
        for rank, (start, length) in enumerate(self.P.shard_geo):
            ctx = _lib.Context(0)
            try:
                rec = _lib.Seam()
                _lib.check(L.dsx_shard_local(ctx.h, ctypes.c_void_p(self.shard.data_ptr() + start),
                                             64 if rank else 0, start, length, r.SHARD_LEN,
                                             ctypes.byref(self.params[r.SHARD_PSET].c),
                                             ctypes.c_void_p(ctypes.addressof(rec)), 0), ctx.h)
            finally:
                ctx.close()
            self.rec_host.append(rec)
            raw = np.frombuffer(ctypes.string_at(ctypes.addressof(rec), shard.SEAM_BYTES), np.uint8).copy()
            self.rec_dev.append(torch.from_numpy(raw).to("cuda"))
        torch.cuda.synchronize()

    def many_dev(self, op):
        import torch
        key = op["blobs"]
        if key not in self.many:
            data = self.P.many(dict(op, bad=False))[0]
            self.many[key] = torch.from_numpy(np.ascontiguousarray(data)).to("cuda")
            torch.cuda.synchronize()
        return self.many[key]


@pytest.fixture(scope="module")
def inputs():
    return Inputs()


# --------------------------------------------------------------- the backend
def _fence(f, rc, n):
    """The fence's verdict -> (the list a successful call wrote, untouched?).
    Whatever the call answered, it wrote nothing in front of its output,
    nothing at or past cap, and nothing past the count it reported."""
    a = f.read()
    g = f.guard
    clean = a == np.uint64(SENTINEL)
    assert clean[:g].all(), "the front guard was written"
    assert clean[g + f.cap:].all(), "an entry at or past cap was written"
    if rc == OK:
        assert n <= f.cap and clean[g + n:].all(), "an entry past the list was written"
        return a[g:g + n].copy(), bool(clean.all())
    return None, bool(clean.all())


class GpuBackend:
    """ctx_life_ref's ops over the raw C ABI (and desync_amd's wrappers for the
    neutral calls, which add nothing of their own) on one context."""

    def __init__(self, ctx, inputs):
        from desync_amd import _lib
        self._lib, self.L, self.ctx, self.inp = _lib, _lib.lib(), ctx, inputs
        self.P = inputs.P
        self.pending = []        # the queued calls' fences, oldest first
        self.rec = None          # this rank's seam record: ("host", Seam) or ("dev", tensor)
        self.rank = None
        self.async_out = None    # dsx_shard_resolve_async's fence, code word and record
        self.pushed = 0
        self.pos = 0             # the end of the last chunk popped

    # -- helpers
    def _err(self):
        d = self.L.dsx_last_error(self.ctx.h)
        return d.decode() if d else ""

    def _got(self, rc, **kw):
        got = {"rc": rc, "n": None, "list": None, "ids": None, "first": None, "groups": None,
               "singles": None, "untouched": None, "err": self._err(), "value": None}
        got.update(kw)
        return got

    def _p(self, pset):
        return ctypes.byref(self.inp.params[pset].c)

    def apply(self, op):
        return getattr(self, "_" + op["op"])(op)

    # -- chain ops
    def _cut(self, op):
        t, w = self.inp.dev[op["blob"]], self.P.want(op["blob"], op["pset"])
        upper = r.op_upper(op)
        f = FencedOut(upper, w.size - 1 if op.get("short") else upper, op["out"])
        n = ctypes.c_uint64(0xDEAD)
        rc = self.L.dsx_cut_device(self.ctx.h, ctypes.c_void_p(t.data_ptr()), t.numel(), self._p(op["pset"]),
                                   f.ptr_or_null, f.cap, ctypes.byref(n),
                                   self._lib.DSX_OUT_DEVICE if op["out"] == "device" else 0)
        lst, clean = _fence(f, rc, n.value)
        return self._got(rc, n=n.value, list=lst, untouched=clean)

    def _cut_queued(self, op):
        t, w = self.inp.dev[op["blob"]], self.P.want(op["blob"], op["pset"])
        upper = r.op_upper(op)
        f = FencedOut(upper, w.size - 1 if op.get("short") else upper, "device")
        n = ctypes.c_uint64(0xDEAD)
        rc = self.L.dsx_cut_device(self.ctx.h, ctypes.c_void_p(t.data_ptr()), t.numel(), self._p(op["pset"]),
                                   f.ptr_or_null, f.cap, ctypes.byref(n),
                                   self._lib.DSX_OUT_DEVICE | self._lib.DSX_NO_SYNC)
        if rc != OK:
            return self._got(rc, untouched=_fence(f, rc, 0)[1])
        self.pending.append(f)
        return self._got(rc)

    def _result(self, op):
        n = ctypes.c_uint64(0xDEAD)
        rc = self.L.dsx_result(self.ctx.h, ctypes.byref(n))
        if not self.pending:
            return self._got(rc)
        f = self.pending.pop(0)
        lst, _ = _fence(f, rc, n.value)
        return self._got(rc, n=n.value, list=lst)

    def _many(self, op):
        _, be, _, _, _, _ = self.P.many(op)
        t = self.inp.many_dev(op)
        nb = len(op["blobs"])
        upper = r.op_upper(op)
        f, first = FencedOut(upper, upper, op["out"]), FencedOut(nb + 1, nb + 1, "host")
        n, totals = ctypes.c_uint64(0xDEAD), self._lib.ManyTotals()
        opts = self._lib.ManyOpts(op["big_blob"], op["group_bytes"])
        rc = self.L.dsx_cut_device_many(self.ctx.h, ctypes.c_void_p(t.data_ptr()), t.numel(), be.ctypes.data,
                                        nb, self._p(op["pset"]), f.ptr, f.cap, ctypes.byref(n), first.ptr,
                                        ctypes.byref(opts), ctypes.byref(totals),
                                        self._lib.DSX_OUT_DEVICE if op["out"] == "device" else 0)
        lst, clean = _fence(f, rc, n.value)
        fst, clean1 = _fence(first, rc, nb + 1)
        return self._got(rc, n=n.value, list=lst, first=fst, groups=totals.groups, singles=totals.single_blobs,
                         untouched=clean and clean1)

    def _cut_host(self, op):
        data = self.P.blobs[op["blob"]]
        upper = r.op_upper(op)
        f = FencedOut(upper, upper, "host")
        n = ctypes.c_uint64(0xDEAD)
        rc = self.L.dsx_cut_host(self.ctx.h, ctypes.c_void_p(data.ctypes.data), data.size, self._p(op["pset"]),
                                 f.ptr, f.cap, ctypes.byref(n))
        lst, clean = _fence(f, rc, n.value)
        return self._got(rc, n=n.value, list=lst, untouched=clean)

    def _index_host(self, op):
        data = self.P.blobs[op["blob"]]
        upper = r.op_upper(op)
        f = FencedOut(upper, upper, "host")
        ids = np.full((3 * upper, 32), 0xA5, np.uint8)  # (the IDs' fence: a third of it is the output)
        n = ctypes.c_uint64(0xDEAD)
        rc = self.L.dsx_index_host(self.ctx.h, ctypes.c_void_p(data.ctypes.data), data.size, self._p(op["pset"]),
                                   op["algo"], f.ptr, ctypes.c_void_p(ids[upper:].ctypes.data), f.cap,
                                   ctypes.byref(n))
        lst, clean = _fence(f, rc, n.value)
        k = n.value if rc == OK else 0
        assert (ids[:upper] == 0xA5).all() and (ids[upper + k:] == 0xA5).all(), "IDs outside the list"
        return self._got(rc, n=n.value, list=lst, untouched=clean,
                         ids=[bytes(x) for x in ids[upper:upper + k]] if rc == OK else None)

    # -- shards
    def _shard_local(self, op):
        import torch
        from desync_amd import shard
        rank = op["rank"]
        start, length = self.P.shard_geo[rank]
        if op["nosync"]:
            rec = torch.zeros(shard.SEAM_BYTES, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ptr, flags = rec.data_ptr(), self._lib.DSX_SEAM_DEVICE | self._lib.DSX_NO_SYNC
        else:
            rec = self._lib.Seam()
            ptr, flags = ctypes.addressof(rec), 0
        rc = self.L.dsx_shard_local(self.ctx.h, ctypes.c_void_p(self.inp.shard.data_ptr() + start),
                                    64 if rank else 0, start, length, r.SHARD_LEN, self._p(r.SHARD_PSET),
                                    ctypes.c_void_p(ptr), flags)
        if rc == OK:
            self.rec, self.rank = ("dev" if op["nosync"] else "host", rec), rank
        return self._got(rc)

    def _records(self, device):
        """(all ranks' records, this rank's own) in host or device memory."""
        import torch
        from desync_amd import shard
        where, mine = self.rec
        if device:
            if where == "host":
                raw = np.frombuffer(ctypes.string_at(ctypes.addressof(mine), shard.SEAM_BYTES), np.uint8).copy()
                mine = torch.from_numpy(raw).to("cuda")
            else:
                self._lib.check(self.L.dsx_sync(self.ctx.h), self.ctx.h)  # (the record is in flight)
            recs = [mine if k == self.rank else self.inp.rec_dev[k] for k in (0, 1)]
            allrec = torch.cat(recs)
            torch.cuda.synchronize()
            return allrec, mine, allrec.data_ptr(), mine.data_ptr()
        assert where == "host"
        arr = (self._lib.Seam * 2)(*[mine if k == self.rank else self.inp.rec_host[k] for k in (0, 1)])
        return arr, mine, ctypes.addressof(arr), ctypes.addressof(mine)

    def _shard_upper(self):
        return self.P.shard_geo[self.rank][1] // r.PSETS[r.SHARD_PSET][0] + 6 + SEAM_MAX_CUTS

    def _shard_resolve(self, op):
        device = self.rec[0] == "dev"
        keep, mine, all_ptr, my_ptr = self._records(device)
        f = FencedOut(self._shard_upper(), self._shard_upper(), op["out"], True)
        n = ctypes.c_uint64(0xDEAD)
        flags = (self._lib.DSX_SEAM_DEVICE if device else 0) | \
                (self._lib.DSX_OUT_DEVICE if op["out"] == "device" else 0)
        rc = self.L.dsx_shard_resolve(self.ctx.h, ctypes.c_void_p(all_ptr), 2, self.rank,
                                      ctypes.c_void_p(my_ptr), f.ptr, f.cap, ctypes.byref(n), flags)
        lst, clean = _fence(f, rc, n.value)
        return self._got(rc, n=n.value, list=lst, untouched=clean)

    def _shard_resolve_async(self, op):
        import torch
        keep, mine, all_ptr, my_ptr = self._records(True)
        f = FencedOut(self._shard_upper(), self._shard_upper(), "device", True)
        code = torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = self.L.dsx_shard_resolve_async(self.ctx.h, ctypes.c_void_p(all_ptr), 2, self.rank, f.ptr, f.cap,
                                            ctypes.c_void_p(code.data_ptr()))
        if rc != OK:
            return self._got(rc, untouched=_fence(f, rc, 0)[1])
        self.async_out = (f, code, keep, mine, my_ptr)
        return self._got(rc)

    def _shard_collect(self, op):
        f, code, keep, mine, my_ptr = self.async_out
        n = ctypes.c_uint64(0xDEAD)
        rc = self.L.dsx_shard_collect(self.ctx.h, ctypes.c_void_p(my_ptr), None, None, ctypes.byref(n))
        if rc != OK:  # (a stale shard's emit may have written the list it was launched for)
            return self._got(rc, n=n.value)
        lst, _ = _fence(f, rc, n.value)
        assert int(code.cpu()[0]) == 0
        return self._got(rc, n=n.value, list=lst)

    # -- the stream
    def _stream_begin(self, op):
        rc = self.L.dsx_stream_begin(self.ctx.h, self._p(r.STREAM_PSET))
        if rc == OK:
            self.pushed = self.pos = 0
        return self._got(rc)

    def _stream_push(self, op):
        src = self.P.stream[self.pushed:self.pushed + op["n"]]
        rc = self.L.dsx_stream_push(self.ctx.h, ctypes.c_void_p(src.ctypes.data), src.size, int(op["eof"]))
        self.pushed += src.size
        return self._got(rc)

    def _stream_pop_all(self, op):
        ends = []
        while True:
            start, size = ctypes.c_uint64(), ctypes.c_uint64()
            rc = self.L.dsx_stream_pop(self.ctx.h, ctypes.byref(start), ctypes.byref(size))
            if rc <= 0:
                break
            assert start.value == self.pos and size.value > 0, "the popped chunks are not contiguous"
            self.pos = start.value + size.value
            ends.append(self.pos)
        return self._got(rc, list=np.array(ends, dtype=np.uint64))

    def _stream_end(self, op):
        return self._got(self.L.dsx_stream_end(self.ctx.h))

    # -- neutral calls
    def _neutral(self, fn):
        try:
            return self._got(OK, value=fn())
        except self._lib.DsxError as e:
            return self._got(e.code)

    def _ids_array(self, op):
        return np.frombuffer(b"".join(self.P.ids(op["blob"], op["pset"])), np.uint8).reshape(-1, 32)

    def _chunk_ids(self, op):
        import desync_amd
        t = self.inp.dev[op["blob"]]
        return self._neutral(lambda: tuple(desync_amd.chunk_ids(
            t.data_ptr(), t.numel(), self.P.want(op["blob"], op["pset"]), 0, ctx=self.ctx, algo=op["algo"])))

    def _idset_dedup(self, op):
        import desync_amd

        def run():
            ids, sizes, seed = r.dedup_list(op)
            as_rows = lambda x: np.frombuffer(b"".join(x), np.uint8).reshape(-1, 32)  # noqa: E731
            with desync_amd.IDSet(as_rows(seed), ctx=self.ctx) as s:
                first, seedp, _ = desync_amd.dedup(as_rows(ids), sizes, sizes=True, seed=s, ctx=self.ctx)
            return tuple(first.tolist()), tuple(seedp.tolist())
        return self._neutral(run)

    def _filled_store(self, op):
        import desync_amd
        t, w = self.inp.dev[op["blob"]], self.P.want(op["blob"], op["pset"])
        s = desync_amd.DeviceStore(2 * t.numel() + r.MiB, w.size + 16, ctx=self.ctx)
        tot = s.put(t, self._ids_array(op), w)
        assert tot["stored"] == w.size and tot["stored_bytes"] == t.numel(), tot
        return s

    def _store_put_read(self, op):
        import desync_amd
        from desync_amd.index import ChunkArray

        def run():
            w = self.P.want(op["blob"], op["pset"])
            with self._filled_store(op) as s:
                index = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=r.PSETS[op["pset"]][2]),
                                         ChunkArray(w, self._ids_array(op)))
                out, _ = s.read_ranges(index, r.read_ranges_of(op))
                return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
        return self._neutral(run)

    def _known(self, op):
        import desync_amd

        def run():
            with self._filled_store(op) as s:
                ids, offs, _ = desync_amd.chunk_ids_known(s, self.inp.dev[op["blob"]],
                                                          self.P.want(op["blob"], op["pset"]))
            return tuple(bytes(x) for x in ids), int((offs != np.uint64(desync_amd.store.OFF_NONE)).sum())
        return self._neutral(run)

    def _aead(self, op):
        from desync_amd import encrypt

        def run():
            t, w = self.inp.dev[op["blob"]], self.P.want(op["blob"], op["pset"])
            nonces = bytes(range(24)) * int(w.size)
            rec, rec_ends = encrypt.aead_seal(KEY, t.data_ptr(), t.numel(), w, 0, nonces=nonces, ctx=self.ctx)
            plain, ends, bad = encrypt.aead_open(KEY, rec.data_ptr(), int(rec_ends[-1]), rec_ends, 0, ctx=self.ctx)
            ok = not bad and np.array_equal(ends, w)
            return hashlib.sha256(plain.cpu().numpy().tobytes()).hexdigest(), int(w.size) if ok else -1
        return self._neutral(run)


def run(inputs, ops, extras=False):
    """Drives ops on a fresh context -> the codes the library returned."""
    from desync_amd import _lib
    ctx = _lib.Context(0)
    try:
        log = []
        r.drive(GpuBackend(ctx, inputs), ops, log=log, extras=extras)
        return [got for _, _, _, got in log]
    finally:
        ctx.close()


# ---------------------------------------------------------------- the scripts
@pytest.mark.parametrize("seed", r.SEEDS)
def test_script(inputs, seed):
    """60 mixed calls and the periodic cuts: every code, list, ID and refusal
    as the model predicts, from the first op to the last."""
    codes = run(inputs, r.script(seed), extras=True)
    assert len(codes) >= r.NOPS + 2
    assert {OK, E_STATE, E_CAPACITY, E_INVAL} <= set(codes)


# ------------------------------------------------ one test per contract line
def _op(kind, seed=0):
    """A chain or neutral op of `kind` with arguments a shard round allows
    (the shard's min, no longer than a shard)."""
    g = r._Gen(1)
    g.m.round_open = True
    return g.chain_op(kind) if kind in r.CHAIN_KINDS else g.neutral_op(kind)


LOCAL0 = {"op": "shard_local", "rank": 0, "nosync": False}
LOCAL1 = {"op": "shard_local", "rank": 1, "nosync": False}
RESOLVE = {"op": "shard_resolve", "out": "device"}
STREAM_HEAD = [{"op": "stream_begin"}, {"op": "stream_push", "n": r.BATCH + 1, "eof": False},
               {"op": "stream_push", "n": r.BATCH, "eof": False}]  # (batch 2 runs on the carried chain)
STREAM_TAIL = [{"op": "stream_pop_all"},
               {"op": "stream_push", "n": r.STREAM_LEN - 2 * r.BATCH - 1, "eof": True},
               {"op": "stream_pop_all"}, {"op": "stream_end"}]


@pytest.mark.parametrize("kind", [k for k in r.CHAIN_KINDS if k != "shard_local"])
def test_chain_call_between_local_and_resolve_makes_the_shard_stale(inputs, kind):
    """... resolve answers DSX_E_STATE and writes nothing; the round starts
    over with dsx_shard_local and resolves to the exact list."""
    tail = [{"op": "result"}] if kind == "cut_queued" else []
    ops = [LOCAL1, _op(kind), RESOLVE] + tail + [LOCAL1, RESOLVE]
    assert run(inputs, ops) == [OK, OK, E_STATE] + [OK] * len(tail) + [OK, OK]


@pytest.mark.parametrize("kind", [k for k in r.CHAIN_KINDS if k != "shard_local"])
def test_chain_call_before_collect_makes_the_shard_stale(inputs, kind):
    """The same between dsx_shard_resolve_async and dsx_shard_collect, and for
    dsx_shard_resolve_async itself after the intruder."""
    tail = [{"op": "result"}] if kind == "cut_queued" else []
    ops = [dict(LOCAL0, nosync=True), {"op": "shard_resolve_async"}, _op(kind), {"op": "shard_collect"}] + tail
    assert run(inputs, ops) == [OK, OK, OK, E_STATE] + [OK] * len(tail)
    ops = [LOCAL0, _op(kind), {"op": "shard_resolve_async"}] + tail + [LOCAL0, {"op": "shard_resolve_async"},
                                                                       {"op": "shard_collect"}]
    assert run(inputs, ops) == [OK, OK, E_STATE] + [OK] * len(tail) + [OK, OK, OK]


def test_a_second_local_replaces_the_shard(inputs):
    assert run(inputs, [LOCAL0, LOCAL1, RESOLVE]) == [OK, OK, OK]  # (rank 1's list, exact)


@pytest.mark.parametrize("kind", r.NEUTRAL_KINDS)
def test_neutral_call_between_local_and_resolve(inputs, kind):
    assert run(inputs, [LOCAL1, _op(kind), RESOLVE]) == [OK, OK, OK]
    assert run(inputs, [LOCAL0, {"op": "shard_resolve_async"}, _op(kind), {"op": "shard_collect"}]) == [OK] * 4


@pytest.mark.parametrize("nosync", [False, True])
@pytest.mark.parametrize("rank", [0, 1])
def test_direct_path_still_resolves(inputs, rank, nosync):
    """local -> resolve with nothing between, host and device records, the
    synchronous and the asynchronous resolve; a resolved shard resolves again."""
    local = {"op": "shard_local", "rank": rank, "nosync": nosync}
    assert run(inputs, [local, {"op": "shard_resolve", "out": "host"}, RESOLVE]) == [OK, OK, OK]
    assert run(inputs, [local, {"op": "shard_resolve_async"}, {"op": "shard_collect"}]) == [OK, OK, OK]


@pytest.mark.parametrize("kind", r.CHAIN_KINDS)
def test_chain_call_inside_a_stream_is_refused(inputs, kind):
    """... with the stream on a carried batch; nothing is written, and the
    rest of the stream equals the oracle's."""
    ops = STREAM_HEAD + [_op(kind), {"op": "stream_begin"}] + STREAM_TAIL
    assert run(inputs, ops) == [OK, OK, OK, E_STATE, E_STATE, OK, OK, OK, OK]


@pytest.mark.parametrize("kind", r.NEUTRAL_KINDS)
def test_neutral_call_inside_a_stream(inputs, kind):
    ops = STREAM_HEAD + [_op(kind)] + STREAM_TAIL
    assert run(inputs, ops) == [OK] * len(ops)


def test_finished_stream_no_longer_owns_the_chain(inputs):
    """Every chunk popped, the stream not ended yet: chain calls run, and so
    does a new stream."""
    ops = STREAM_HEAD + STREAM_TAIL[:-1] + [r._cut("u1m", "A"), LOCAL0, RESOLVE] + STREAM_HEAD + STREAM_TAIL
    assert run(inputs, ops) == [OK] * len(ops)


def test_stream_begin_waits_for_the_queue(inputs):
    """dsx_stream_begin with uncollected queued calls is refused (dsx_result's
    redo never runs inside a stream); after the results it begins."""
    q = [{"op": "cut_queued", "blob": "dense", "pset": "D", "short": False},
         {"op": "cut_queued", "blob": "u1m", "pset": "A", "short": False}]
    ops = q + [{"op": "stream_begin"}, {"op": "result"}, {"op": "stream_begin"}, {"op": "result"}] + \
        STREAM_HEAD + STREAM_TAIL
    assert run(inputs, ops) == [OK, OK, E_STATE, OK, E_STATE, OK] + [OK] * 7


@pytest.mark.parametrize("kind", r.SYNC_KINDS)
def test_sync_call_with_three_queued(inputs, kind):
    """Any call may run between a queued call and its dsx_result: the results
    come oldest first, each exact (the dense tile's through its redo)."""
    q = [{"op": "cut_queued", "blob": "u3m", "pset": "A", "short": False},
         {"op": "cut_queued", "blob": "dense", "pset": "D", "short": False},
         {"op": "cut_queued", "blob": "zero", "pset": "B", "short": False}]
    g = r._Gen(2)
    tail = [RESOLVE] if kind == "shard_local" else []  # (nothing between: the direct path)
    ops = q + [g.chain_op(kind)] + tail + [{"op": "result"}] * 3 + [r._cut("u256k", "B", "device")]
    assert run(inputs, ops) == [OK] * len(ops)


@pytest.mark.parametrize("which", r.FAILING_KINDS)
def test_next_call_after_a_failing_one(inputs, which):
    """"The context's next call is not affected": cut, exact."""
    g = r._Gen(3)
    bad = dict(g.many_op(variant=2), bad=True)
    ops, want = {
        "cut_short": ([r._cut("zero", "D", "device", short=True), r._cut("zero", "D", "host", short=True)],
                      [E_CAPACITY, E_CAPACITY]),
        "queued_short": ([{"op": "cut_queued", "blob": "u3m", "pset": "B", "short": True}, {"op": "result"}],
                         [OK, E_CAPACITY]),
        "many_refused": ([bad], [E_INVAL]),
    }[which]
    after = [r._cut("u3m", "A", "host"), r._cut("dense", "D", "device")]
    assert run(inputs, ops + after) == want + [OK, OK]
