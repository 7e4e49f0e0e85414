"""Chunk-ID sets on the GPU: dedup, seed lookup and the ``desync info`` report.

Reference interface:
    desync info's counters                       (cmd/desync/info.go:95-185)
    FileSeed.pos, the seed's ID -> positions map (fileseed.go:24-36, :92-95)
    the self seed's map of the chunks written    (selfseed.go)

The IDs are hashed into an open-addressing table in HBM by libdsx's kernels
(dsx_idset_create / dsx_dedup); nothing here loops over chunks
in Python except the ``HasChunk`` questions of a store or cache, which are
asked on the host for first occurrences only, as the reference asks them.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import DSX_ENDS_DEVICE, DSX_IDS_DEVICE, DSX_OUT_DEVICE, DSX_SIZES, check, lib
from .index import ChunkArray, Index

POS_NONE = _lib.DSX_POS_NONE


def _is_device(x):
    return bool(getattr(x, "is_cuda", False)) and hasattr(x, "data_ptr")


def _chunks_of(x):
    return x.Chunks if isinstance(x, Index) else None


def _host_ids(ids):
    """(n, 32) uint8 array of a numpy array, a list of 32-byte IDs or an Index."""
    chunks = _chunks_of(ids)
    if chunks is not None:
        if isinstance(chunks, ChunkArray) and chunks._list is None:
            return chunks._ids
        ids = [c.ID for c in chunks]
    if isinstance(ids, np.ndarray):
        if ids.dtype != np.uint8 or ids.size % 32:
            raise ValueError("IDs must be an (n, 32) uint8 array")
        return np.ascontiguousarray(ids).reshape(-1, 32)
    ids = [bytes(i) for i in ids]
    if any(len(i) != 32 for i in ids):
        raise ValueError("every chunk ID must be 32 bytes")
    return np.frombuffer(b"".join(ids), dtype=np.uint8).reshape(-1, 32)


def _ids_arg(ids, n):
    """-> (pointer, count, DSX_IDS_DEVICE or 0, object to keep alive).  A device
    tensor of n*32 bytes, or an integer device pointer with ``n``, stays in HBM."""
    if isinstance(ids, int):
        if n is None:
            raise ValueError("a device pointer needs n, the number of IDs")
        return ids, int(n), DSX_IDS_DEVICE, None
    if _is_device(ids):
        nbytes = ids.numel() * ids.element_size()
        if nbytes % 32 or not ids.is_contiguous():
            raise ValueError("device IDs must be contiguous, 32 bytes each")
        return ids.data_ptr(), nbytes // 32, DSX_IDS_DEVICE, ids
    arr = _host_ids(ids)
    return arr.ctypes.data, arr.shape[0], 0, arr


class IDSet:
    """A set of chunk IDs resident on the GPU (dsx_idset_t): the seed side of
    :func:`dedup`.  ``ids`` is an ``(n, 32) uint8`` array, a list of 32-byte
    IDs, an :class:`Index`, or device memory (a tensor of n*32 bytes, or an
    integer pointer with ``n``).  Duplicates are allowed; seeds from several
    indexes are concatenated by the caller (info.go:100-114).  The set keeps
    its own device copy.  ``len()`` is the number of IDs it was built from,
    ``.unique`` the number of distinct ones."""

    def __init__(self, ids, ctx=None, device=0, n=None):
        self.ctx = ctx or _lib.default_context(device)
        self.h = None
        ptr, n, flags, keep = _ids_arg(ids, n)
        h = ctypes.c_void_p()
        check(lib().dsx_idset_create(self.ctx.h, ctypes.c_void_p(ptr), n, flags, ctypes.byref(h)),
              self.ctx.h)
        self.h = h
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().dsx_idset_count(self.h, ctypes.byref(a), ctypes.byref(b)))
        self._n, self.unique = a.value, b.value

    def __len__(self):
        return self._n

    def close(self):
        if self.h is not None:
            if self.ctx.h:  # (a closed context has freed its sets)
                lib().dsx_idset_destroy(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dedup(ids, ends, start=0, seed=None, sizes=False, ctx=None, device=0, n=None, out=None):
    """dsx_dedup: which chunks repeat inside the list and which the seed holds.

    ``ids`` as for :class:`IDSet`; ``ends`` the chunk end offsets (the first
    chunk starts at ``start``), or with ``sizes=True`` the chunk sizes: a host
    array, a device tensor of uint64, or an integer device pointer.  ``seed``
    is an :class:`IDSet` of the same context, or None.

    Returns ``(first_pos, seed_pos, totals)``: ``first_pos[i]`` is the lowest
    position with chunk i's ID (``first_pos[i] == i``: a first occurrence),
    ``seed_pos[i]`` the lowest position of that ID in the seed or ``POS_NONE``
    (None without a seed), both ``np.uint32``; ``totals`` a dict with
    info.go's counters ``total``, ``unique``, ``in_seed``, ``size`` and
    ``size_not_in_seed``.  With ``out=(first_ptr, seed_ptr)`` (device pointers
    to n uint32 each, either may be None) the per-chunk results stay in HBM
    and are returned as None.
    """
    ctx = ctx or (seed.ctx if seed is not None else _lib.default_context(device))
    iptr, n, flags, _keep_ids = _ids_arg(ids, n)
    if isinstance(ends, int):
        eptr, _keep_ends = ends, None
        flags |= DSX_ENDS_DEVICE
    elif _is_device(ends):
        if ends.numel() * ends.element_size() != 8 * n or not ends.is_contiguous():
            raise ValueError("device ends must be n contiguous uint64")
        eptr, _keep_ends = ends.data_ptr(), ends
        flags |= DSX_ENDS_DEVICE
    else:
        _keep_ends = np.ascontiguousarray(ends, dtype=np.uint64)
        if _keep_ends.size != n:
            raise ValueError(f"{n} IDs but {_keep_ends.size} chunk ends")
        eptr = _keep_ends.ctypes.data
    if sizes:
        flags |= DSX_SIZES
    first = seedp = None
    if out is not None:
        flags |= DSX_OUT_DEVICE
        fptr, sptr = out
    else:
        first = np.empty(n, dtype=np.uint32)
        fptr = first.ctypes.data
        sptr = None
        if seed is not None:
            seedp = np.empty(n, dtype=np.uint32)
            sptr = seedp.ctypes.data
    tot = _lib.DedupTotals()
    check(lib().dsx_dedup(ctx.h, ctypes.c_void_p(iptr), ctypes.c_void_p(eptr), int(start), n,
                          seed.h if seed is not None else None, ctypes.c_void_p(fptr),
                          ctypes.c_void_p(sptr), ctypes.byref(tot), flags), ctx.h)
    totals = {k: getattr(tot, k) for k, _ in _lib.DedupTotals._fields_}
    return first, seedp, totals


def Info(index, seeds=(), store=None, cache=None, device=0, ctx=None):
    """``desync info`` (cmd/desync/info.go:95-185) of an :class:`Index`: a dict
    with the JSON keys of its report.  ``seeds`` are seed indexes (Index
    objects, ID arrays or lists), merged into one set as info.go:100-114 does.
    ``store`` and ``cache`` are any objects with ``HasChunk(id)``; they are
    asked on the host, for first occurrences only, and fill ``in-store``,
    ``in-cache``, ``not-in-seed-nor-cache`` and
    ``dedup-size-not-in-seed-nor-cache``.

    The chunks' ``Size`` fields are what is summed (DSX_SIZES), so a
    hand-built, non-contiguous chunk list counts as the reference counts it.
    ``dedup-size-not-in-seed-nor-cache-compressed`` is always 0: it needs the
    stored (compressed) chunk sizes, and chunk codecs are out of scope here.
    """
    ctx = ctx or _lib.default_context(device)
    chunks = index.Chunks
    n = len(chunks)
    ids = _host_ids(index)
    if isinstance(chunks, ChunkArray) and chunks._list is None:
        sizes = np.diff(chunks._ends, prepend=np.uint64(chunks._start))
    else:
        sizes = np.fromiter((c.Size for c in chunks), np.uint64, n)
    seeds = list(seeds)
    seed = None
    try:
        if seeds:
            seed = IDSet(np.concatenate([_host_ids(s) for s in seeds]), ctx=ctx)
        first, seedp, tot = dedup(ids, sizes, sizes=True, seed=seed, ctx=ctx)
    finally:
        if seed is not None:
            seed.close()
    res = {
        "total": tot["total"], "unique": tot["unique"], "in-store": 0, "in-seed": tot["in_seed"],
        "in-cache": 0, "not-in-seed-nor-cache": tot["unique"] - tot["in_seed"],
        "size": index.Length(), "dedup-size-not-in-seed": tot["size_not_in_seed"],
        "dedup-size-not-in-seed-nor-cache": tot["size_not_in_seed"],
        "dedup-size-not-in-seed-nor-cache-compressed": 0,
        "chunk-size-min": index.Index.ChunkSizeMin, "chunk-size-avg": index.Index.ChunkSizeAvg,
        "chunk-size-max": index.Index.ChunkSizeMax,
    }
    if (store is not None or cache is not None) and n:
        firsts = np.flatnonzero(first == np.arange(n, dtype=np.uint32))
        in_seed = seedp[firsts] != POS_NONE if seedp is not None else np.zeros(firsts.size, bool)
        raw = ids.tobytes()
        nor_n = nor_size = 0
        for k, i in enumerate(firsts.tolist()):
            cid = raw[32 * i:32 * i + 32]
            if store is not None and store.HasChunk(cid):  # info.go:198-223
                res["in-store"] += 1
            in_cache = cache is not None and bool(cache.HasChunk(cid))
            res["in-cache"] += in_cache
            if not in_seed[k] and not in_cache:
                nor_n += 1
                nor_size += int(sizes[i])
        res["not-in-seed-nor-cache"] = nor_n
        res["dedup-size-not-in-seed-nor-cache"] = nor_size
    return res
