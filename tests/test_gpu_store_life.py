"""The chunk store in HBM through seeded sequences of mixed calls
(store_life_ref.py has the scripts, the model and the driver): puts, prunes,
copies, Grow, RemoveChunk and PutSealed on three stores in two contexts, with
IDSet, dedup, chunk_ids and chunk_keep between them on the same scratch.  After
every mutating call, accepted or refused, the totals or the refusal, counts(),
every entry and the used arena must equal the model's; the queries (locate,
entries, GetChunk, read_ranges, AssembleBlob, Verify, chunk_ids_known) run where the script has
them and on every store after every tenth op.  Every malformed input is one
the library refuses by contract: capacity, missing IDs, an index that lies to
a read."""
import ctypes

import numpy as np
import pytest

import store_life_ref as life_ref
from store_life_ref import FILL, NULL_ID, NULL_SIZE, PROFILES, drive

pytestmark = pytest.mark.gpu

PATTERN = 0xC3
PATTERN64 = 0xC3C3C3C3C3C3C3C3
KEY = bytes(range(32))


def _torch():
    import torch
    return torch


def _L():
    from desync_amd import _lib
    return _lib


class GpuBackend:
    """desync_amd.DeviceStore (and the raw C ABI where the class hides a
    placement) as the driver's backend."""

    def __init__(self, profile, ctxs):
        import desync_amd
        self.pool = life_ref.pool_of(profile)
        self.ctxs = ctxs
        self.stores = {name: desync_amd.DeviceStore(arena, chunks, ctx=ctxs[c])
                       for name, (arena, chunks, c) in PROFILES[profile]["stores"].items()}
        self.uploads = 0

    def close(self):
        for s in self.stores.values():
            s.close()

    def dev(self, arr, fill=PATTERN):
        """The array's bytes in a tensor filled with a pattern, at an address
        whose residue modulo 16 changes from upload to upload -> (pointer, tensor)."""
        torch = _torch()
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        residue, self.uploads = self.uploads % 16, self.uploads + 1
        t = torch.full((a.size + 32,), fill, dtype=torch.uint8, device="cuda:0")
        off = (residue - t.data_ptr()) % 16
        if a.size:
            t[off:off + a.size] = torch.from_numpy(a.copy())
        torch.cuda.synchronize()  # (torch's stream is not the context's)
        return t.data_ptr() + off, t

    def apply(self, op):
        return getattr(self, "_" + op["op"])(op)

    def state(self, name):
        from desync_amd.encrypt import _download
        s = self.stores[name]
        ids, ends = s.entries()
        ptr, used = s.arena()
        offs, sizes, miss = s.locate(ids) if len(ids) else ([], [], 0)
        return {"counts": s.counts(), "ids": ids.tobytes(), "ends": [int(e) for e in ends],
                "arena": _download(s.ctx, ptr, used).tobytes(),
                "locate": ([int(o) for o in offs], [int(z) for z in sizes], miss)}

    # ---- mutating ops ----
    def _refusable(self, call):
        L = _L()
        try:
            return {"refused": None, "totals": call()}
        except L.DsxError as e:
            assert e.code == L.DSX_E_CAPACITY, e
            return {"refused": "capacity", "totals": e.totals}

    def _put(self, op):
        blob, ids, ends, start = self.pool.gather(op["picks"], op["pad"])
        bptr, _k1 = self.dev(blob)
        iarg, _k2 = self.dev(ids) if op["ids_dev"] else (ids, None)
        earg, _k3 = self.dev(ends) if op["ends_dev"] else (ends, None)
        return self._refusable(lambda: self.stores[op["store"]].put((bptr, blob.size), iarg, earg, start,
                                                                    n=len(ends)))

    def _prune(self, op):
        L = _L()
        s = self.stores[op["store"]]
        n = len(op["ids"])
        flags = L.DSX_PRUNE_REMOVE if op["remove"] else 0
        iptr, _k = (op["ids"].ctypes.data if n else None), None
        if op["ids_dev"] and n:
            iptr, _k = self.dev(op["ids"])
            flags |= L.DSX_IDS_DEVICE
        tot = L.StorePruneTotals()
        with s._lock:
            rc = L.lib().dsx_store_prune(s.ctx.h, s.h, ctypes.c_void_p(iptr), n, op["window"], ctypes.byref(tot),
                                         flags)
        assert rc == 0, (rc, L.lib().dsx_last_error(s.ctx.h))
        return {"refused": None, "totals": {k: getattr(tot, k) for k, _ in L.StorePruneTotals._fields_}}

    def _remove_chunk(self, op):
        import desync_amd
        try:
            self.stores[op["store"]].RemoveChunk(op["id"])
        except desync_amd.ChunkMissing as e:
            assert e.ID == op["id"]
            return {"refused": "missing"}
        return {"refused": None}

    def _copy(self, op):
        dst, src = self.stores[op["store"]], self.stores[op["src"]]
        if op["ids"] is None:
            res = self._refusable(lambda: dst.CopyFrom(src))
        elif op["ids_dev"]:
            iptr, _k = self.dev(op["ids"])
            res = self._refusable(lambda: dst.CopyFrom(src, iptr, n=len(op["ids"])))
        else:
            res = self._refusable(lambda: dst.CopyFrom(src, op["ids"]))
        if res["totals"]["missing"]:
            res["refused"] = "missing"
        return res

    def _grow(self, op):
        return self._refusable(lambda: self.stores[op["store"]].Grow(op["arena_bytes"], op["max_chunks"]))

    _grow_refused = _grow

    def _put_sealed(self, op):
        import desync_amd
        dst, src = self.stores[op["store"]], self.stores[op["src"]]
        conv = desync_amd.encrypt.NewXChaCha20Poly1305(KEY)
        nonces = np.random.default_rng(op["nonce_seed"]).bytes(24 * op["n"])
        records, rec_ends = src.Seal(conv, op["first"], op["n"], nonces)
        assert rec_ends.size == op["n"] and int(rec_ends[-1]) <= records.numel()
        ids = src.entries()[0][op["first"]:op["first"] + op["n"]]
        try:
            return self._refusable(lambda: dst.PutSealed(records, rec_ends, ids, conv))
        except desync_amd.ChunkInvalid as e:
            assert e.ID in self.pool.liars
            return {"refused": "invalid", "totals": None}

    # ---- queries: into outputs filled with a pattern ----
    def _locate(self, op):
        L = _L()
        s = self.stores[op["store"]]
        ids = np.ascontiguousarray(op["ids"])
        n = len(ids)
        offs, sizes = np.full(n + 3, PATTERN64, np.uint64), np.full(n + 3, PATTERN64, np.uint64)
        miss = ctypes.c_uint64()
        with s._lock:
            rc = L.lib().dsx_store_locate(s.ctx.h, s.h, ids.ctypes.data, n, offs.ctypes.data, sizes.ctypes.data,
                                          ctypes.byref(miss), 0)
        assert rc == 0 and np.all(offs[n:] == PATTERN64) and np.all(sizes[n:] == PATTERN64)
        return {"offs": offs[:n].tolist(), "sizes": sizes[:n].tolist(), "missing": miss.value}

    def _entries(self, op):
        L = _L()
        s = self.stores[op["store"]]
        n = s.counts()["chunks"]
        ids, ends = np.full((n + 1, 32), PATTERN, np.uint8), np.full(n + 1, PATTERN64, np.uint64)
        with s._lock:
            rc = L.lib().dsx_store_entries(s.ctx.h, s.h, 0, n, ids.ctypes.data, ends.ctypes.data, 0)
        assert rc == 0 and np.all(ids[n] == PATTERN) and ends[n] == PATTERN64
        return {"ids": ids[:n].tobytes(), "ends": ends[:n].tolist()}

    def _get(self, op):
        import desync_amd
        try:
            return {"data": self.stores[op["store"]].GetChunk(op["id"])}
        except desync_amd.ChunkMissing:
            return {"data": None}

    def _index(self, op):
        ids = np.frombuffer(b"".join(c[0] for c in op["chunks"]), np.uint8).reshape(-1, 32)
        return ids, np.cumsum([c[1] for c in op["chunks"]], dtype=np.uint64)

    def _read(self, op):
        from desync_amd.readseeker import read_ranges_raw
        torch = _torch()
        ids, ends = self._index(op)
        out_len = sum(ln for _, ln in op["ranges"]) + 37
        out = torch.full((out_len,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        iarg, earg = ids, ends
        if self.uploads % 2:  # the index in HBM every other time
            (iarg, _k1), (earg, _k2) = self.dev(ids), self.dev(ends)
        tot = read_ranges_raw(self.stores[op["store"]], iarg, earg, op["ranges"], out, 0, NULL_ID, NULL_SIZE,
                              n=len(ends))
        return {"totals": {k: int(v) for k, v in tot.items()}, "out": out.cpu().numpy().tobytes()}

    def _assemble(self, op):
        import desync_amd
        s = self.stores[op["store"]]
        ids, ends = self._index(op)
        index = desync_amd.Index(desync_amd.FormatIndex(ChunkSizeMax=NULL_SIZE),
                                 desync_amd.index.ChunkArray(ends, ids))
        try:
            out, _stats = desync_amd.AssembleBlob(index, s, ctx=s.ctx)
        except desync_amd.ChunkMissing as e:
            return {"error": ("missing", e.ID), "out": None}
        except desync_amd.ChunkInvalid as e:
            return {"error": ("invalid", e.ID), "out": None}
        except ValueError as e:
            text = "unexpected size for chunk "
            assert str(e).startswith(text), e
            return {"error": ("size", bytes.fromhex(str(e)[len(text):])), "out": None}
        return {"error": None, "out": out.cpu().numpy().tobytes()}

    def _verify(self, op):
        return {"bad": self.stores[op["store"]].verify_entries()}

    def _known(self, op):
        blob, _, ends, start = self.pool.gather(op["picks"], op["pad"])
        ptr, _k1 = self.dev(blob)
        earg, _k2 = self.dev(ends) if self.uploads % 2 else (ends, None)  # the ends in HBM every other time
        ids, off, tot = self.stores[op["store"]].chunk_ids((ptr, blob.size), earg, start, n=len(ends),
                                                           algo=_L().DSX_DIGEST_SHA512_256)
        assert tot["chunks"] == len(ends) and tot["untried"] == 0, tot
        return {"ids": ids.tobytes(), "known_off": [int(o) for o in off], "recognised": tot["recognised"],
                "hashed": tot["hashed"]}

    # ---- foreign calls on a context the stores use ----
    def _idset(self, op):
        import desync_amd
        ids = self.pool.ids[op["picks"]]
        arg, _k = self.dev(ids) if self.uploads % 2 else (ids, None)
        with desync_amd.IDSet(arg, ctx=self.ctxs[op["ctx"]], n=len(ids)) as s:
            return {"n": len(s), "unique": s.unique}

    def _dedup(self, op):
        import desync_amd
        ctx = self.ctxs[op["ctx"]]
        with desync_amd.IDSet(self.pool.ids[op["seed_picks"]], ctx=ctx) as seed:
            first, seedp, tot = desync_amd.dedup(self.pool.ids[op["picks"]], self.pool.sizes[op["picks"]],
                                                 sizes=True, seed=seed, ctx=ctx)
        return {"first": first.tolist(), "seed": seedp.tolist(), "totals": tot}

    def _chunk_ids(self, op):
        import desync_amd
        blob, _, ends, start = self.pool.gather(op["picks"], op["pad"])
        ptr, _k = self.dev(blob)
        got = desync_amd.chunk_ids(ptr, blob.size, ends, start, ctx=self.ctxs[op["ctx"]],
                                   algo=_L().DSX_DIGEST_SHA512_256)
        return {"ids": b"".join(bytes(g) for g in got)}

    def _chunk_keep(self, op):
        from desync_amd import extract
        blob, ids, ends = life_ref.chunk_keep_args(self.pool, op)
        ptr, _k = self.dev(blob)
        keep = extract.chunk_keep(ptr, op["have_len"], ends, ids, ctx=self.ctxs[op["ctx"]], algo="sha512-256")
        return {"keep": keep.tolist()}


@pytest.fixture(scope="module")
def second_ctx():
    ctx = _L().Context(0)
    yield ctx
    ctx.close()


def run(profile, seed, ctxs, extras=True):
    backend = GpuBackend(profile, ctxs)
    log = []
    try:
        drive(profile, seed, backend, log=log, extras=extras)
    finally:
        backend.close()
    return log


@pytest.mark.parametrize("seed", life_ref.NARROW_SEEDS)
def test_narrow(dctx, second_ctx, seed):
    """120 ops on A and B (one context) and C (another), with the periodic
    queries on every store.  Then the script's 120 ops again on fresh stores,
    whose tables draw new salts: both runs must return the same totals and
    answers and leave the same entries and arenas."""
    first = [x for x in run("narrow", seed, [dctx, second_ctx]) if not x[3]]
    again = run("narrow", seed, [dctx, second_ctx], extras=False)
    assert len(first) == len(again)
    for a, b in zip(first, again):
        if a != b:
            raise life_ref.Mismatch("narrow", seed, a[0], life_ref.script("narrow", seed),
                                    f"{a[1]}: the second run, on fresh stores with new salts, differs from the first")


def test_wide(dctx):
    """More than 65,536 entries appended or kept by a put, a prune and a copy,
    each right after a call of another kind on the same scratch."""
    run("wide", 0, [dctx])
