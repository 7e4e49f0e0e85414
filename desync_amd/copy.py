"""Copying chunks between stores, and a cache in front of a store.

Reference interface:
    Copy                      (copy.go:9-58; what ``desync cache`` runs)
    Cache, NewCache           (cache.go:9-63; ``desync extract -c``)

Between two :class:`DeviceStore` s of one context :func:`Copy` is a single
dsx_store_copy: which chunks the destination lacks, where they go and the copy
itself are decided and done by kernels, and no chunk crosses to the host
(DESIGN.md 4.7).  For any other pair of stores it is the reference's loop, one
``HasChunk`` / ``GetChunk`` / ``StoreChunk`` per chunk.
"""
from __future__ import annotations

import threading
from concurrent.futures import ThreadPoolExecutor

from .errors import ChunkMissing
from .info import _host_ids
from .store import DeviceStore
from .stream import Chunk


def _on_device(src, dst):
    """Both are DeviceStores of one context: dsx_store_copy applies."""
    return isinstance(src, DeviceStore) and isinstance(dst, DeviceStore) and src.ctx is dst.ctx


def Copy(ids, src, dst, n=1, pb=None):
    """Copy (copy.go:9-58): copies the chunks ``ids`` names from ``src`` into
    ``dst``, skipping those ``dst`` already holds (it is asked first: an ID it
    holds need not be in ``src``).  ``ids`` is an iterable of 32-byte IDs, an
    ``(n, 32)`` uint8 array or an :class:`Index`; duplicates are allowed.

    With two :class:`DeviceStore` s of one context this is one dsx_store_copy,
    all or nothing: if any ID is in neither store, :class:`ChunkMissing` is
    raised for the first such ID in ``ids`` and nothing has been copied.  For
    any other pair it is the reference's loop with ``n`` worker threads, which
    stops at the first chunk ``src`` lacks (:class:`ChunkMissing`); chunks
    copied before stay, as in the reference.

    ``pb``, if given, is a ProgressBar: ``SetTotal(len(ids))``, ``Start()``, one
    ``Increment()`` per ID, ``Finish()``."""
    ids = _host_ids(ids)
    if pb is not None:
        pb.SetTotal(len(ids))
        pb.Start()
    try:
        if _on_device(src, dst):
            tot = dst.CopyFrom(src, ids) if len(ids) else None
            if pb is not None:
                for _ in range(len(ids)):
                    pb.Increment()
            if tot and tot["missing"]:
                raise ChunkMissing(ids[tot["first_missing"]].tobytes())
            return
        stop = threading.Event()

        def one(cid):
            if stop.is_set():
                return
            try:
                if pb is not None:
                    pb.Increment()
                if dst.HasChunk(cid):
                    return
                try:
                    data = src.GetChunk(cid)
                except ChunkMissing:
                    raise
                except KeyError:  # (MemoryStore's)
                    raise ChunkMissing(cid) from None
                dst.StoreChunk(Chunk(cid, data))
            except BaseException:
                stop.set()
                raise

        todo = (row.tobytes() for row in ids)
        if n <= 1:
            for cid in todo:
                one(cid)
        else:
            with ThreadPoolExecutor(max_workers=n) as workers:
                for _ in workers.map(one, todo):
                    pass
    finally:
        if pb is not None:
            pb.Finish()


class Cache:
    """Cache (cache.go:9-63): a store ``s`` behind a local WriteStore ``l``.  A
    chunk is looked for in ``l`` first; one fetched from ``s`` is stored in
    ``l`` too.  With two :class:`DeviceStore` s of one context the fetch is a
    dsx_store_copy ``s -> l``, and :func:`desync_amd.AssembleBlob` fills ``l``
    with one copy of everything its plan needs before it reads ``l`` in place.
    A local ``DeviceStore(evict=True)`` makes it a bounded cache: a fetch that
    does not fit evicts the least recently used chunks of ``l`` first (the
    reference's cache grows without bound and is cleaned by ``desync prune``)."""

    def __init__(self, s, l):  # noqa: E741 (the reference's field names)
        self.s, self.l = s, l

    def GetChunk(self, cid) -> bytes:
        cid = bytes(cid)
        try:
            return self.l.GetChunk(cid)
        except KeyError:  # (ChunkMissing is one)
            pass
        if _on_device(self.s, self.l):
            Copy([cid], self.s, self.l)
            return self.l.GetChunk(cid)
        try:
            data = self.s.GetChunk(cid)
        except ChunkMissing:
            raise
        except KeyError:
            raise ChunkMissing(cid) from None
        self.l.StoreChunk(Chunk(cid, data))
        return data

    def HasChunk(self, cid) -> bool:
        cid = bytes(cid)
        return bool(self.l.HasChunk(cid)) or bool(self.s.HasChunk(cid))

    def StoreChunk(self, chunk):
        """Stores into the local store (the store behind it is read-only here)."""
        self.l.StoreChunk(chunk)

    def Close(self):
        for store in (self.l, self.s):
            close = getattr(store, "Close", None) or getattr(store, "close", None)
            if close is not None:
                close()

    def __str__(self):
        return f"store:{self.s} with cache {self.l}"


def NewCache(s, l) -> Cache:  # noqa: E741
    """NewCache (cache.go:18-22)."""
    return Cache(s, l)


__all__ = ["Copy", "Cache", "NewCache"]
