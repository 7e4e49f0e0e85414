"""Seed plans and in-HBM assembly: the read side (``desync extract``).

Reference interface:
    NewIndexSeed, FileSeed                       (fileseed.go:14-36)
    NewSeedSequencer, SeedSequencer.Plan/Rewind  (sequencer.go:31-79)
    Plan.Validate, fileSeedSegment.Validate      (sequencer.go:104-176, fileseed.go:183-196)
    AssembleFile, ExtractStats                   (assemble.go:93-309, extractstats.go)

The target and seed IDs are matched on the GPU (dsx_seed_plan: the seeds'
ID tables give 32-bit classes, a host walk over them gives the plan), the
plan's segments are gathered out of the seed blobs and the fetched store chunks
by one kernel (dsx_assemble), and the result is re-hashed where it lies
(dsx_chunk_ids).  Blobs are device memory; nothing is written to files, no
reflinks, no chunk compression (a store is any object with ``GetChunk(id) ->
bytes``).
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from . import _lib, digest
from ._lib import DSX_SRC_NULL, DSX_SRC_STORE, DsxError, lib
from .errors import ChunkInvalid, ChunkMissing
from .index import ChunkArray, Index
from .info import IDSet, _host_ids, _is_device
from .make import chunk_ids

SEG_DTYPE = np.dtype([("dst_off", "<u8"), ("bytes", "<u8"), ("src_off", "<u8"), ("first", "<u4"),
                      ("count", "<u4"), ("source", "<i4"), ("seed_first", "<u4")])
assert SEG_DTYPE.itemsize == ctypes.sizeof(_lib.PlanSeg)

Segment = namedtuple("Segment", "first count dst_off bytes source seed_first src_off")
Segment.__doc__ = """One plan entry (SeedSegmentCandidate, sequencer.go:21-25): target chunks
[first, first + count) = target bytes [dst_off, dst_off + bytes), from seed number ``source``
(>= 0, chunk ``seed_first`` on, byte ``src_off`` of its blob), the null seed (SRC_NULL) or the
packed store buffer at ``src_off`` (SRC_STORE)."""
SRC_NULL, SRC_STORE = DSX_SRC_NULL, DSX_SRC_STORE
SRC_SELF = _lib.DSX_SRC_SELF  # in-place assembly: the output buffer's own old content


class SeedInvalid(Exception):
    """fileSeedSegment.Validate: "seed index for %s doesn't match its data"."""

    def __init__(self, seed, number):
        self.seed, self.number = seed, number
        super().__init__(f"seed index for seed {number} doesn't match its data")


class StorageError(DsxError):
    """An in-place assembly that its stash cannot hold (DSX_E_CAPACITY):
    ``.needed`` is the stash it takes, ``.totals`` the call's totals."""

    def __init__(self, needed, totals):
        super().__init__(_lib.DSX_E_CAPACITY, f"the stash takes {needed} bytes")
        self.needed, self.totals = int(needed), totals


def _check(rc, ctx):
    """check() with the context's detail for argument errors too."""
    if rc < 0:
        d = lib().dsx_last_error(ctx.h) if rc == _lib.DSX_E_INVAL else None
        if d:
            raise DsxError(rc, d.decode())
        _lib.check(rc, ctx.h)
    return rc


def _index_arrays(index):
    """(ids (n, 32) uint8, ends uint64) of an Index."""
    chunks = index.Chunks
    ids = _host_ids(index)
    if isinstance(chunks, ChunkArray) and chunks._list is None:
        if chunks._start:
            raise ValueError("an index to extract starts at 0")
        return ids, chunks._ends
    n = len(chunks)
    ends = np.cumsum(np.fromiter((c.Size for c in chunks), np.uint64, n), dtype=np.uint64)
    return ids, np.ascontiguousarray(ends, dtype=np.uint64)


class IndexSeed:
    """FileSeed (fileseed.go:14-36): a seed index and its blob in HBM.  ``blob``
    is a device tensor, a ``(device pointer, length)`` pair, or host bytes
    (uploaded once); None for a seed that is only planned with."""

    def __init__(self, index: Index, blob=None):
        self.index = index
        self.ids, self.ends = _index_arrays(index)
        self._blob = blob
        self._dev = None
        self._set = None
        self._invalid = False

    def SetInvalid(self, value: bool):
        self._invalid = bool(value)

    def IsInvalid(self) -> bool:
        return self._invalid

    def idset(self, ctx):
        if self._set is None or self._set.ctx is not ctx or self._set.h is None:
            self._set = IDSet(self.ids, ctx=ctx)
        return self._set

    def device_blob(self, ctx):
        """-> (pointer, length) of the seed blob on the context's device."""
        if self._dev is None:
            b = self._blob
            if b is None:
                raise ValueError("the seed has no blob to copy from")
            if isinstance(b, tuple):
                self._dev = (int(b[0]), int(b[1]), None)
            elif _is_device(b):
                if not b.is_contiguous():
                    raise ValueError("a seed blob must be contiguous")
                self._dev = (b.data_ptr(), b.numel() * b.element_size(), b)
            else:
                import torch
                t = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(f"cuda:{ctx.device}") \
                    if len(b) else torch.empty(0, dtype=torch.uint8, device=f"cuda:{ctx.device}")
                torch.cuda.synchronize(t.device)  # (the upload ran on torch's stream, not the context's)
                self._dev = (t.data_ptr(), t.numel(), t)
        return self._dev[0], self._dev[1]

    def close(self):
        if self._set is not None:
            self._set.close()
            self._set = None


def NewIndexSeed(index: Index, blob=None) -> IndexSeed:
    """NewIndexSeed (fileseed.go:24-36)."""
    return IndexSeed(index, blob)


class Plan:
    """A Plan (sequencer.go:27): a sequence of :class:`Segment` in target order.
    ``.segs`` is the same as a structured array (dsx_plan_seg_t), ``source``
    numbering the sequencer's seeds; ``.store_chunks`` the target positions of
    the distinct store chunks in packed-buffer order (the fetch list);
    ``.totals`` dsx_plan_totals_t as a dict."""

    def __init__(self, sequencer, segs, store_chunks, totals):
        self.sequencer = sequencer
        self.segs = segs
        self.store_chunks = store_chunks
        self.totals = totals

    def __len__(self):
        return len(self.segs)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self.segs)))]
        g = self.segs[i]
        return Segment(int(g["first"]), int(g["count"]), int(g["dst_off"]), int(g["bytes"]),
                       int(g["source"]), int(g["seed_first"]), int(g["src_off"]))

    def __iter__(self):
        return (self[i] for i in range(len(self.segs)))

    def Validate(self):
        """Plan.Validate (sequencer.go:104-176): re-hashes, on the resident seed
        blob, every seed chunk the plan uses (fileSeedSegment.Validate,
        fileseed.go:183-196).  On a mismatch, or a segment whose seed bytes
        differ in length from the target's ("wrong size", fileseed.go:165-167),
        the seed is marked invalid and :class:`SeedInvalid` raised; the
        sequencer skips it in its next Plan() (InvalidSeedActionSkip)."""
        sq = self.sequencer
        segs = self.segs
        for k, seed in enumerate(sq.seeds):
            mine = segs[segs["source"] == k]
            if not len(mine):
                continue
            p0 = mine["seed_first"].astype(np.int64)
            p1 = p0 + mine["count"].astype(np.int64)
            starts = np.where(p0 > 0, seed.ends[np.maximum(p0, 1) - 1], 0).astype(np.uint64)
            if np.any(seed.ends[p1 - 1] - starts != mine["bytes"]):
                seed.SetInvalid(True)
                raise SeedInvalid(seed, k)
            # the union of the used chunk ranges, as maximal runs
            order = np.argsort(p0, kind="stable")
            runs = []
            for a, b in zip(p0[order].tolist(), p1[order].tolist()):
                if runs and a <= runs[-1][1]:
                    runs[-1][1] = max(runs[-1][1], b)
                else:
                    runs.append([a, b])
            if len(runs) > 64:  # one launch over the span instead of one per run
                runs = [[runs[0][0], runs[-1][1]]]
                used = np.zeros(len(seed.ends), dtype=bool)
                for a, b in zip(p0.tolist(), p1.tolist()):
                    used[a:b] = True
            else:
                used = None
            ptr, length = seed.device_blob(sq.ctx)
            for a, b in runs:
                start = int(seed.ends[a - 1]) if a else 0
                if int(seed.ends[b - 1]) > length:
                    seed.SetInvalid(True)
                    raise SeedInvalid(seed, k)
                got = np.frombuffer(b"".join(chunk_ids(ptr, length, seed.ends[a:b], start, ctx=sq.ctx)),
                                    dtype=np.uint8).reshape(-1, 32)
                bad = np.any(got != seed.ids[a:b], axis=1)
                if used is not None:
                    bad &= used[a:b]
                if bad.any():
                    seed.SetInvalid(True)
                    raise SeedInvalid(seed, k)


class SeedSequencer:
    """SeedSequencer (sequencer.go:13-79) over an index and :class:`IndexSeed`
    seeds.  ``null_seed``: the null-chunk seed AssembleFile prepends
    (assemble.go:151-158); ``limit``: the chunks one seed match may hold (0: no
    limit; the reference uses 100 when it cannot reflink).  Plan() always plans
    the whole index; Rewind() is kept for the reference's callers."""

    def __init__(self, index: Index, *seeds, null_seed=True, limit=0, ctx=None, device=0):
        self.index = index
        self.seeds = list(seeds)
        self.null_seed = bool(null_seed)
        self.limit = int(limit)
        self.ctx = ctx or _lib.default_context(device)
        self.ids, self.ends = _index_arrays(index)

    def Rewind(self):
        pass

    def Plan(self) -> Plan:
        n = len(self.ends)
        ctx = self.ctx
        active = [k for k, s in enumerate(self.seeds) if not s.IsInvalid()]
        sets = [self.seeds[k].idset(ctx) for k in active]
        ns = len(active)
        h = (ctypes.c_void_p * max(1, ns))(*[s.h for s in sets])
        ends = (ctypes.c_void_p * max(1, ns))(*[self.seeds[k].ends.ctypes.data for k in active])
        counts = (ctypes.c_uint64 * max(1, ns))(*[len(self.seeds[k].ends) for k in active])
        null_id = None
        if self.null_seed:
            null_id = (ctypes.c_uint8 * 32).from_buffer_copy(
                digest.NewNullChunk(self.index.Index.ChunkSizeMax).ID)
        segs = np.zeros(max(1, n), dtype=SEG_DTYPE)
        store = np.zeros(max(1, n), dtype=np.uint32)
        tot = _lib.PlanTotals()
        _check(lib().dsx_seed_plan(
            ctx.h, ctypes.c_void_p(self.ids.ctypes.data), ctypes.c_void_p(self.ends.ctypes.data), 0, n,
            h, ends, counts, ns, null_id, self.limit, ctypes.c_void_p(segs.ctypes.data), n,
            ctypes.c_void_p(store.ctypes.data), n, ctypes.byref(tot), 0), ctx)
        totals = {k: getattr(tot, k) for k, _ in _lib.PlanTotals._fields_}
        segs = segs[:totals["segments"]].copy()
        if active != list(range(ns)):  # number the sources as the sequencer's seeds
            remap = np.array(active + [0], dtype=np.int32)
            src = segs["source"]
            segs["source"] = np.where(src >= 0, remap[np.maximum(src, 0)], src)
        return Plan(self, segs, store[:totals["store_unique"]].copy(), totals)


def NewSeedSequencer(index: Index, *seeds, null_seed=True, limit=0, ctx=None, device=0) -> SeedSequencer:
    """NewSeedSequencer (sequencer.go:32-37)."""
    return SeedSequencer(index, *seeds, null_seed=null_seed, limit=limit, ctx=ctx, device=device)


def _assemble_args(plan, store_bytes, ctx, flags):
    """-> (d_seeds, seed_lens, nseeds, store pointer, store length, flags, the
    segment array, what must stay alive) for dsx_assemble and
    dsx_assemble_inplace."""
    sq = plan.sequencer
    ns = len(sq.seeds)
    used = set(np.unique(plan.segs["source"]).tolist())
    ptrs, lens = [], []
    for k, s in enumerate(sq.seeds):
        p, ln = s.device_blob(ctx) if k in used else (0, 0)
        ptrs.append(p)
        lens.append(ln)
    d_seeds = (ctypes.c_void_p * max(1, ns))(*ptrs)
    d_lens = (ctypes.c_uint64 * max(1, ns))(*lens)
    keep = None
    if isinstance(store_bytes, tuple):
        sptr, slen, flags = int(store_bytes[0]), int(store_bytes[1]), flags | _lib.DSX_STORE_DEVICE
    elif _is_device(store_bytes):
        sptr, slen, flags = store_bytes.data_ptr(), store_bytes.numel() * store_bytes.element_size(), \
            flags | _lib.DSX_STORE_DEVICE
    else:
        keep = np.frombuffer(store_bytes, dtype=np.uint8) if not isinstance(store_bytes, np.ndarray) \
            else np.ascontiguousarray(store_bytes, dtype=np.uint8)
        sptr, slen = (keep.ctypes.data if keep.size else 0), keep.size
    segs = np.ascontiguousarray(plan.segs)
    return d_seeds, d_lens, ns, sptr, slen, flags, segs, keep


def assemble(plan: Plan, out, store_bytes=b"", ctx=None, flags=0):
    """dsx_assemble of a plan into the device tensor ``out``; ``store_bytes``
    is the packed store buffer: host bytes (or a uint8 array), a device
    tensor, or a ``(device pointer, length)`` pair (a DeviceStore's arena)."""
    ctx = ctx or plan.sequencer.ctx
    d_seeds, d_lens, ns, sptr, slen, flags, segs, _alive = _assemble_args(plan, store_bytes, ctx, flags)
    _check(lib().dsx_assemble(ctx.h, ctypes.c_void_p(segs.ctypes.data), len(segs), d_seeds, d_lens, ns,
                              ctypes.c_void_p(sptr), slen, ctypes.c_void_p(out.data_ptr()),
                              out.numel() * out.element_size(), flags), ctx)
    return out


def assemble_inplace(plan: Plan, out, have_len, keep=None, store_bytes=b"", ctx=None, flags=0,
                     window=0, stash=0):
    """dsx_assemble_inplace: the device tensor ``out`` holds ``have_len`` bytes
    of old content and becomes the plan's target.  ``plan.segs`` may name
    ``SRC_SELF`` (the buffer's own old content); ``keep`` is one byte per
    target chunk, set where the chunk already lies at its place.  ``flags``
    may force a direction (DSX_INPLACE_ASCENDING / DSX_INPLACE_DESCENDING).
    Returns dsx_inplace_totals_t as a dict; a stash too small raises
    :class:`StorageError` with ``.needed``, and the buffer is unchanged."""
    sq = plan.sequencer
    ctx = ctx or sq.ctx
    d_seeds, d_lens, ns, sptr, slen, flags, segs, _alive = _assemble_args(plan, store_bytes, ctx, flags)
    ends = np.ascontiguousarray(sq.ends, dtype=np.uint64)
    kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    new_len = int(ends[-1]) if ends.size else 0
    tot = _lib.InplaceTotals()
    rc = lib().dsx_assemble_inplace(
        ctx.h, ctypes.c_void_p(segs.ctypes.data if len(segs) else None), len(segs),
        ctypes.c_void_p(ends.ctypes.data if ends.size else None), ends.size,
        ctypes.c_void_p(kp.ctypes.data) if kp is not None and kp.size else None,
        d_seeds, d_lens, ns, ctypes.c_void_p(sptr), slen, ctypes.c_void_p(out.data_ptr()),
        out.numel() * out.element_size(), int(have_len), new_len, int(window), int(stash), flags,
        ctypes.byref(tot))
    totals = {k: getattr(tot, k) for k, _ in _lib.InplaceTotals._fields_ if k != "reserved"}
    if rc == _lib.DSX_E_CAPACITY:
        raise StorageError(totals["stash_peak"], totals)
    _check(rc, ctx)
    return totals


def chunk_keep(ptr, have_len, ends, ids, ctx=None, algo=None):
    """dsx_chunk_keep: which chunks of a target (``ends``, ``ids`` (n, 32)
    uint8, both host arrays) already lie at their place in the device buffer
    ``ptr[0:have_len]`` of unknown content -> a uint8 mask, one byte per chunk
    (assemble.go:38-48).  A chunk reaching beyond ``have_len`` is not kept."""
    from .make import _digest_code
    ctx = ctx or _lib.default_context()
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint8)
    keep = np.zeros(ends.size, dtype=np.uint8)
    kept = ctypes.c_uint64()
    if ends.size:
        _check(lib().dsx_chunk_keep(ctx.h, ctypes.c_void_p(ptr), int(have_len),
                                    ctypes.c_void_p(ends.ctypes.data), ends.size,
                                    ctypes.c_void_p(ids.ctypes.data), _digest_code(algo),
                                    ctypes.c_void_p(keep.ctypes.data), ctypes.byref(kept), 0), ctx)
        assert int(keep.sum()) == kept.value
    return keep


def AssembleBlob(index: Index, store, seeds=(), null_seed=True, limit=0, ctx=None, device=0,
                 validate=True, out=None, have=None, window=0, stash=0):
    """AssembleFile (assemble.go:93-309) into HBM: returns ``(uint8 device
    tensor, ExtractStats dict)``.

    1. plan (SeedSequencer.Plan); 2. Plan.Validate: a seed whose blob does not
    match its index is skipped and the plan made again (InvalidSeedActionSkip,
    assemble.go:171-190); 3. the plan's ``store_chunks`` are fetched from
    ``store`` (``GetChunk(id) -> bytes``) and each length checked against the
    index; 4. dsx_assemble (with a :class:`DeviceStore` of the same context
    nothing is fetched: 3. is dsx_store_resolve, which points the plan's store
    segments at the store's arena, and 4. reads the arena in place; a chunk the
    store does not hold raises :class:`ChunkMissing`, a stored size that differs
    from the index's ``ValueError("unexpected size for chunk <hex>")``,
    assemble.go:75-77; with a :class:`Cache` of two such stores the plan's store
    chunks are first copied into its local store, one dsx_store_copy, and that
    store is the one read); 5. dsx_chunk_ids of the result against the index's
    IDs, the read-back check of assemble.go:208-229: a mismatch raises
    :class:`ChunkInvalid`.  An empty index gives an empty tensor
    (assemble.go:142-146).

    The stats carry extractstats.go's JSON keys.  Go counts a repeated store
    chunk as from the self seed or from the store depending on goroutine
    timing; here, always: ``chunks-from-store`` is the number of distinct
    chunks fetched, ``chunks-from-seeds`` every other chunk (file seeds, the
    null seed, and repeats of a fetched chunk, which are copied out of the
    packed buffer as the self seed would copy them), and
    ``bytes-copied-from-seeds`` their bytes.  ``seeds`` counts the null seed.
    ``chunks-in-place``, ``bytes-cloned-from-seeds`` and ``blocksize`` are 0.

    In place (``extract -k``, assemble.go:29-49, :89-92): with ``out``, a uint8
    device tensor of at least ``index.Length()`` bytes, the target is built
    inside that buffer (dsx_assemble_inplace) and ``(out[:length], stats)``
    returned; nothing of the target's size is allocated.  ``have`` says what
    the buffer holds.  An :class:`Index`: the old version, ``out[:have.Length()]``.
    It joins the sequencer as the first file seed (ties go to it), its segments
    become moves inside the buffer, and a chunk with the same start, end and ID
    in both indexes that the plan took from it is kept; Plan.Validate re-hashes
    what the plan uses of it like any seed's, and if that fails the seed is
    skipped and the call goes on as for an ``int``.  An ``int``: that many
    bytes of unknown content (a resumed extract); dsx_chunk_keep hashes the
    target's chunks where they would lie and keeps those that match, and there
    is no self seed.  None: nothing usable.  ``window`` and ``stash`` are
    dsx_assemble_inplace's (0: its defaults); a stash too small raises
    :class:`StorageError` with ``.needed`` and leaves the buffer as it was.
    Only chunks that are written are fetched from ``store`` or looked up in a
    DeviceStore.  The read-back check hashes one span, from the first to the
    last chunk not kept.  ``chunks-in-place`` counts the kept chunks,
    ``chunks-from-store`` the distinct chunks fetched, ``chunks-from-seeds``
    the rest, chunks moved inside the buffer included; ``stats["inplace"]``
    holds dsx_inplace_totals_t.  Deviation: Go counts a chunk as in place only
    on the store path (writeChunk); here a kept chunk is kept and counted
    whatever the plan chose for it.
    """
    import torch

    ctx = ctx or _lib.default_context(device)
    seeds = list(seeds)
    if out is not None:
        return assemble_blob_inplace(index, store, seeds, null_seed, limit, ctx, validate, out, have,
                                     window, stash)
    if have is not None:
        raise ValueError("have= describes out=")
    sq = SeedSequencer(index, *seeds, null_seed=null_seed, limit=limit, ctx=ctx)
    n = len(sq.ends)
    stats = {"chunks-from-seeds": 0, "chunks-from-store": 0, "chunks-in-place": 0,
             "bytes-copied-from-seeds": 0, "bytes-cloned-from-seeds": 0, "blocksize": 0,
             "bytes-total": index.Length(), "chunks-total": n, "seeds": len(seeds) + bool(null_seed)}
    dev = f"cuda:{ctx.device}"
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), stats
    while True:
        plan = sq.Plan()
        if not validate:
            break
        try:
            plan.Validate()
            break
        except SeedInvalid:
            sq.Rewind()  # the seed is marked: the next plan does without it
    raw = sq.ids.tobytes()
    length = int(sq.ends[-1])
    out = torch.empty(length, dtype=torch.uint8, device=dev)
    from .copy import Cache, Copy, _on_device
    from .store import DeviceStore
    if isinstance(store, Cache) and _on_device(store.s, store.l) and store.l.ctx is ctx:
        # a cache of two stores in HBM: one dsx_store_copy brings what the plan
        # needs into the local store, which is then read in place
        Copy(sq.ids[plan.store_chunks], store.s, store.l)
        store = store.l
    if isinstance(store, DeviceStore) and store.ctx is ctx:
        # the chunks are in HBM already: point the plan's store segments at the
        # arena (dsx_store_resolve) and gather out of it in place; a tracked store
        # counts them as used first
        if store.tracked and len(plan.store_chunks):
            store.Touch(sq.ids[plan.store_chunks])
        miss, wrong, bad = store.resolve(sq.ids, plan.segs)
        if miss or wrong:
            cid = raw[32 * bad:32 * bad + 32]
            if not store.HasChunk(cid):
                raise ChunkMissing(cid)
            raise ValueError(f"unexpected size for chunk {cid.hex()}")  # assemble.go:75-77
        with store._lock:
            assemble(plan, out, store.arena(), ctx=ctx)
    else:
        sizes = np.diff(sq.ends, prepend=np.uint64(0))
        parts = []
        for i in plan.store_chunks.tolist():
            cid = raw[32 * i:32 * i + 32]
            data = store.GetChunk(cid)
            if len(data) != int(sizes[i]):
                raise ChunkInvalid(cid, digest.Digest.Sum(data))
            parts.append(bytes(data))
        packed = b"".join(parts)
        assemble(plan, out, packed, ctx=ctx)
    got = chunk_ids(out.data_ptr(), length, sq.ends, 0, ctx=ctx)
    got = np.frombuffer(b"".join(got), dtype=np.uint8).reshape(-1, 32)
    bad = np.flatnonzero(np.any(got != sq.ids, axis=1))
    if bad.size:
        i = int(bad[0])
        raise ChunkInvalid(raw[32 * i:32 * i + 32], got[i].tobytes())
    t = plan.totals
    stats["chunks-from-store"] = t["store_unique"]
    stats["chunks-from-seeds"] = n - t["store_unique"]
    stats["bytes-copied-from-seeds"] = t["seed_bytes"] + t["null_bytes"] + t["store_bytes"] - t["store_len"]
    return out, stats


def _same_chunks(ends, ids, old_ends, old_ids):
    """One byte per target chunk: the old index has a chunk with the same
    start, end and ID."""
    n = len(ends)
    keep = np.zeros(n, dtype=np.uint8)
    if not n or not len(old_ends):
        return keep
    starts = np.concatenate([np.zeros(1, dtype=np.uint64), ends[:-1]])
    old_starts = np.concatenate([np.zeros(1, dtype=np.uint64), old_ends[:-1]])
    j = np.minimum(np.searchsorted(old_ends, ends), len(old_ends) - 1)
    same = (old_ends[j] == ends) & (old_starts[j] == starts) & (ends > starts)
    same &= np.all(old_ids[j] == ids, axis=1)
    keep[same] = 1
    return keep


def assemble_blob_inplace(index, store, seeds, null_seed, limit, ctx, validate, out, have, window,
                          stash, flags=0, trace=None):
    """AssembleBlob(out=...): see there.  ``flags`` may force a direction
    (DSX_INPLACE_ASCENDING / DSX_INPLACE_DESCENDING); ``trace`` (a dict)
    receives what went into dsx_assemble_inplace: ``segs``, ``keep``,
    ``have_len``."""
    from .copy import Cache, Copy, _on_device
    from .store import DeviceStore
    if not _is_device(out) or out.element_size() != 1 or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 device tensor")
    cap = out.numel()
    length = index.Length()
    if cap < length:
        raise ValueError(f"out holds {cap} bytes, the index needs {length}")
    own = None
    if isinstance(have, Index):
        if have.Length() > cap:
            raise ValueError("have is longer than out")
        own = IndexSeed(have, (out.data_ptr(), have.Length()))
        have_len = have.Length()
    else:
        have_len = int(have or 0)
        if not 0 <= have_len <= cap:
            raise ValueError("have is longer than out")
    sq = SeedSequencer(index, *(([own] if own else []) + seeds), null_seed=null_seed, limit=limit, ctx=ctx)
    n = len(sq.ends)
    stats = {"chunks-from-seeds": 0, "chunks-from-store": 0, "chunks-in-place": 0,
             "bytes-copied-from-seeds": 0, "bytes-cloned-from-seeds": 0, "blocksize": 0,
             "bytes-total": length, "chunks-total": n, "seeds": len(seeds) + bool(null_seed)}
    if n == 0:
        return out[:0], stats
    while True:
        plan = sq.Plan()
        if not validate:
            break
        try:
            plan.Validate()
            break
        except SeedInvalid:
            sq.Rewind()  # the seed is marked: the next plan does without it
    segs = plan.segs.copy()
    if own is not None and not own.IsInvalid():
        mine = segs["source"] == 0
        keep = _same_chunks(sq.ends, sq.ids, own.ends, own.ids)
        if validate:  # only what Plan.Validate re-hashed is trusted to lie there
            hashed = np.zeros(n, dtype=bool)
            for f, c in zip(segs["first"][mine].tolist(), segs["count"][mine].tolist()):
                hashed[f:f + c] = True
            keep &= hashed
        stats["seeds"] += 1
    else:  # unknown content (or an old index that lied): ask the bytes themselves
        mine = np.zeros(len(segs), dtype=bool)
        keep = chunk_keep(out.data_ptr(), have_len, sq.ends, sq.ids, ctx=ctx)
    if own is not None:  # number the sources without the self seed
        src = segs["source"]
        segs["source"] = np.where(mine, SRC_SELF, np.where(src > 0, src - 1, src))
        own.close()
    # a kept chunk is not written: nothing is fetched for it
    st = (segs["source"] == SRC_STORE) & (keep[segs["first"]] != 0)
    segs["source"][st] = SRC_NULL
    segs["src_off"][st] = 0
    sm = segs["source"] == SRC_STORE
    sizes = np.diff(sq.ends, prepend=np.uint64(0))
    raw = sq.ids.tobytes()
    if trace is not None:
        trace.update(segs=segs, keep=keep, have_len=have_len)
    shim = SeedSequencer(index, *seeds, null_seed=null_seed, limit=limit, ctx=ctx)
    if isinstance(store, Cache) and _on_device(store.s, store.l) and store.l.ctx is ctx:
        Copy(sq.ids[np.unique(segs["first"][sm])], store.s, store.l)
        store = store.l
    if isinstance(store, DeviceStore) and store.ctx is ctx:
        if store.tracked and sm.any():
            store.Touch(sq.ids[np.unique(segs["first"][sm])])
        miss, wrong, bad = store.resolve(sq.ids, segs)
        if miss or wrong:
            cid = raw[32 * bad:32 * bad + 32]
            if not store.HasChunk(cid):
                raise ChunkMissing(cid)
            raise ValueError(f"unexpected size for chunk {cid.hex()}")  # assemble.go:75-77
        offs, at = np.unique(segs["src_off"][sm], return_index=True)  # (one arena offset a distinct chunk)
        fetched, fetched_bytes = int(offs.size), int(sizes[segs["first"][sm][at]].sum())
        with store._lock:
            totals = assemble_inplace(Plan(shim, segs, None, None), out, have_len, keep, store.arena(),
                                      ctx=ctx, flags=flags, window=window, stash=stash)
    else:
        # the packed buffer holds the chunks still needed, in the plan's order
        chunks = plan.store_chunks
        old_offs = np.cumsum(sizes[chunks], dtype=np.uint64) - sizes[chunks]
        sel = np.isin(old_offs, segs["src_off"][sm])
        new_offs = np.cumsum(sizes[chunks][sel], dtype=np.uint64) - sizes[chunks][sel]
        segs["src_off"][sm] = new_offs[np.searchsorted(old_offs[sel], segs["src_off"][sm])]
        parts = []
        for i in chunks[sel].tolist():
            cid = raw[32 * i:32 * i + 32]
            data = store.GetChunk(cid)
            if len(data) != int(sizes[i]):
                raise ChunkInvalid(cid, digest.Digest.Sum(data))
            parts.append(bytes(data))
        fetched, fetched_bytes = int(sel.sum()), int(sizes[chunks][sel].sum())
        totals = assemble_inplace(Plan(shim, segs, None, None), out, have_len, keep, b"".join(parts),
                                  ctx=ctx, flags=flags, window=window, stash=stash)
    if validate:
        named = np.zeros(n, dtype=bool)
        for f, c in zip(segs["first"].tolist(), segs["count"].tolist()):
            named[f:f + c] = True
        todo = np.flatnonzero((keep == 0) | ~named)
        if todo.size:  # one span, from the first to the last chunk not kept
            a, b = int(todo[0]), int(todo[-1]) + 1
            got = chunk_ids(out.data_ptr(), length, sq.ends[a:b], int(sq.ends[a - 1]) if a else 0, ctx=ctx)
            got = np.frombuffer(b"".join(got), dtype=np.uint8).reshape(-1, 32)
            bad = np.flatnonzero(np.any(got != sq.ids[a:b], axis=1))
            if bad.size:
                i = a + int(bad[0])
                raise ChunkInvalid(raw[32 * i:32 * i + 32], got[i - a].tobytes())
    stats["chunks-in-place"] = totals["kept_chunks"]
    stats["chunks-from-store"] = fetched
    stats["chunks-from-seeds"] = n - totals["kept_chunks"] - fetched
    stats["bytes-copied-from-seeds"] = totals["written_bytes"] - fetched_bytes
    stats["inplace"] = totals
    return out[:length], stats
