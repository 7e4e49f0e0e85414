"""A chunk store in HBM: what desync puts between the write and the read side.

Reference interface:
    Store, WriteStore, PruneStore         (store.go:21-39)
    LocalStore with Uncompressed: true    (local.go, store.go:98-99)
    LocalStore.Verify, with repair        (local.go:103-161)
    LocalStore.RemoveChunk, Prune         (local.go:69-75, :163-202)
    Copy                                  (copy.go:9-58)
    desync prune's merge of the indexes   (cmd/desync/prune.go:71-81)
    ChunkStorage.StoreChunk               (chunkstorage.go:44-67)
    ChopFile                              (chop.go:14-81)
    ChunkMissing                          (errors.go:5-17)

:class:`DeviceStore` is a deduplicating, tightly packed arena of chunk bytes
on the GPU, keyed by chunk ID (dsx_store_*).  It is filled from a
blob resident in HBM by kernels (``put``: which chunks are new, where they go
and the copy, without a host round trip per chunk) and read in place by
dsx_assemble (:func:`desync_amd.AssembleBlob` with such a store fetches
nothing through the host; ``read_ranges`` reads byte ranges of an indexed blob
out of it in one call, readseeker.py).  ``Prune`` / ``RemoveChunk`` / ``Verify(repair=True)``
remove chunks and compact the arena where it lies (dsx_store_prune), giving
the room back to later puts.  ``CopyFrom`` appends chunks of another store of the
same context (dsx_store_copy; copy.py has ``Copy`` and ``Cache``), and ``Grow``
moves the store into a new capacity with it.
``DeviceStore(track=True)`` keeps one use stamp per entry (dsx_store_track);
``Touch`` says what counts as a use, ``Evict`` removes the least recently used
chunks until a requested room is free (dsx_store_evict: the victims are chosen
on the GPU, then the arena is compacted as a prune compacts it), and
``DeviceStore(evict=True)`` does that by itself when a put or a copy does not
fit: a store of fixed size that is a bounded cache.
``Seal`` / ``PutSealed`` convert its chunks to and from the records of a store
with ``encryption: true`` (XChaCha20-Poly1305 on the GPU, encrypt.py), and
``WriteLocal`` / ``ReadLocal`` save and reload it in LocalStore's layout, plain
or sealed.  Out of scope: compression (zstd), AES-256-GCM, a second context.
"""
from __future__ import annotations

import ctypes
import os
import tempfile
import threading

import numpy as np

from . import _lib, digest
from ._lib import DSX_ENDS_DEVICE, DsxError, lib
from .errors import ChunkInvalid, ChunkMissing
from .info import _host_ids, _ids_arg, _is_device
from .make import _digest_code

OFF_NONE = 0xFFFFFFFFFFFFFFFF  # locate's offset of an ID the store does not hold


def _check(rc, ctx):
    """check() with the context's detail for argument and capacity errors too."""
    if rc < 0:
        d = lib().dsx_last_error(ctx.h) if rc in (_lib.DSX_E_INVAL, _lib.DSX_E_CAPACITY) else None
        if d:
            raise DsxError(rc, d.decode())
        _lib.check(rc, ctx.h)
    return rc


TMP_CHUNK_PREFIX = ".tmp-cacnk"  # local.go:18


def chunk_file_name(base, cid, extension=""):
    """LocalStore.nameFromID (local.go:234-239) -> (directory, file path) of the
    chunk with the 32-byte ID ``cid`` in a store at ``base``."""
    sid = bytes(cid).hex()
    d = os.path.join(base, sid[0:4])
    return d, os.path.join(d, sid) + extension


def chunk_id_from_filename(name, extension=""):
    """chunkIDFromFilename (types.go:44-54): the 32-byte ID a chunk file's name
    carries, or None if the name is not an ID plus ``extension``."""
    if extension:
        if not name.endswith(extension):
            return None
        name = name[:-len(extension)]
    if len(name) != 64:
        return None
    try:
        return bytes.fromhex(name)
    except ValueError:
        return None


def _local_converters(converters):
    """The converters WriteLocal / ReadLocal can apply: none, or one AEAD layer."""
    from .encrypt import AEADConverter, Compressor, Converters
    conv = Converters(converters)
    if any(isinstance(c, Compressor) for c in conv):
        raise ValueError("a compressed store cannot be written or read: zstd is not available "
                         "(use Uncompressed: true)")
    if len(conv) > 1 or (conv and not isinstance(conv[0], AEADConverter)):
        raise ValueError("converters must be empty or one AEAD converter")
    return conv


def _umask():
    try:
        with open("/proc/self/status") as f:
            for line in f:
                if line.startswith("Umask:"):
                    return int(line.split()[1], 8)
    except OSError:
        pass
    return 0o022


def _blob_arg(blob):
    """-> (device pointer, length, object to keep alive) of a device tensor or
    a ``(pointer, length)`` pair."""
    if isinstance(blob, tuple):
        return int(blob[0]), int(blob[1]), None
    if _is_device(blob):
        if not blob.is_contiguous():
            raise ValueError("a blob must be contiguous")
        return blob.data_ptr(), blob.numel() * blob.element_size(), blob
    raise TypeError("a blob is a device tensor or a (device pointer, length) pair")


class DeviceStore:
    """A WriteStore in HBM (dsx_store_t) of up to ``max_chunks`` chunks and
    ``arena_bytes`` bytes, belonging to one context.

    ``HasChunk(id)``, ``StoreChunk(chunk)`` and ``GetChunk(id)`` are the
    reference's interface, one chunk per call (StoreChunk uploads the host
    bytes: the slow path, kept so that ChunkStorage and ChunkStream work with
    it).  ``put`` / ``put_index`` store every chunk of a blob resident in HBM
    in one call.  Every call holds the store's lock: ChunkStream's workers call
    StoreChunk from several threads, and a context is not thread-safe.

    ``track``: the store keeps a use stamp per entry from the start
    (:meth:`Track` turns it on later; it cannot be turned off).  ``evict``
    (implies ``track``): ``put``, ``put_index``, ``StoreChunk`` and ``CopyFrom``
    that get DSX_E_CAPACITY evict the least recently used chunks for exactly
    the missing room, with the call's own IDs pinned, and repeat the call once;
    if the eviction cannot make the room the capacity error is raised and the
    store is unchanged."""

    def __init__(self, arena_bytes, max_chunks, ctx=None, device=0, track=False, evict=False):
        self.ctx = ctx or _lib.default_context(device)
        self.h = None
        self._lock = threading.RLock()
        self.tracked = False
        self.evict = bool(evict)
        h = ctypes.c_void_p()
        _check(lib().dsx_store_create(self.ctx.h, int(arena_bytes), int(max_chunks), ctypes.byref(h)),
               self.ctx)
        self.h = h
        if track or evict:
            self.Track()

    # ---- the fill state ------------------------------------------------------------
    def counts(self):
        """dsx_store_counts_t as a dict: chunks, bytes, max_chunks, arena_bytes."""
        with self._lock:
            c = _lib.StoreCounts()
            _lib.check(lib().dsx_store_count(self.h, ctypes.byref(c)))
            return {k: getattr(c, k) for k, _ in _lib.StoreCounts._fields_}

    def __len__(self):
        return self.counts()["chunks"]

    def arena(self):
        """-> (device pointer of the arena, bytes in use): the store buffer of
        dsx_assemble with DSX_STORE_DEVICE.  The pointer holds until :meth:`Grow`."""
        with self._lock:
            p, used = ctypes.c_void_p(), ctypes.c_uint64()
            _lib.check(lib().dsx_store_arena(self.h, ctypes.byref(p), ctypes.byref(used)))
            return p.value or 0, used.value

    def entries(self):
        """-> (ids (chunks, 32) uint8, ends uint64): the stored IDs and their
        cumulative arena ends, in arena order."""
        with self._lock:
            n = self.counts()["chunks"]
            ids = np.empty((n, 32), dtype=np.uint8)
            ends = np.empty(n, dtype=np.uint64)
            if n:
                _check(lib().dsx_store_entries(self.ctx.h, self.h, 0, n, ids.ctypes.data,
                                               ends.ctypes.data, 0), self.ctx)
            return ids, ends

    # ---- use tracking and eviction ------------------------------------------------------
    def _state_check(self, rc):
        if rc == _lib.DSX_E_STATE:
            d = lib().dsx_last_error(self.ctx.h)
            raise DsxError(rc, d.decode() if d else "")
        return _check(rc, self.ctx)

    def Track(self):
        """dsx_store_track: one use stamp per entry from now on (the entries
        already there start at 0).  Idempotent; cannot be turned off."""
        with self._lock:
            self._state_check(lib().dsx_store_track(self.ctx.h, self.h))
            self.tracked = True

    def Touch(self, ids, stamp=None, n=None):
        """dsx_store_touch: counts the chunks ``ids`` (as for :class:`IDSet`: host
        or device; an :class:`Index` too) as used now, or at the caller's own
        logical time ``stamp`` (> 0).  IDs the store does not hold are no error
        -> their number."""
        from .index import Index
        if isinstance(ids, Index):
            ids = _host_ids(ids)
        iptr, n, flags, _keep = _ids_arg(ids, n)
        miss = ctypes.c_uint64()
        with self._lock:
            self._state_check(lib().dsx_store_touch(self.ctx.h, self.h, ctypes.c_void_p(iptr), n,
                                                    _lib.DSX_STAMP_NOW if stamp is None else int(stamp),
                                                    ctypes.byref(miss), flags))
        return miss.value

    def stamps(self):
        """dsx_store_stamps -> (the entries' stamps as np.uint64, the clock)."""
        with self._lock:
            n = self.counts()["chunks"]
            out = np.empty(n, dtype=np.uint64)
            clock = ctypes.c_uint64()
            self._state_check(lib().dsx_store_stamps(self.ctx.h, self.h, 0, n, out.ctypes.data,
                                                     ctypes.byref(clock), 0))
            return out, clock.value

    def Evict(self, need_bytes=0, need_chunks=0, pin=None, window=0, dry=False, n_pin=None, ids=True):
        """dsx_store_evict: removes the least recently used chunks, in ascending
        (stamp, entry number), until ``need_bytes`` bytes and ``need_chunks``
        chunks are free, and compacts the arena in place.  Chunks whose ID is in
        ``pin`` (as for :class:`IDSet`: host or device) are never removed.
        ``dry`` selects and reports without changing the store.  Returns the
        dsx_store_evict_totals_t as a dict plus ``"ids"``, the evicted IDs as an
        ``(evicted, 32)`` array in their old entry order.  Room that cannot be
        made raises DsxError (DSX_E_CAPACITY) with ``.totals`` (evictable,
        evictable_bytes, pinned) and leaves the store unchanged.  Arena offsets
        taken before are stale afterwards, as after a prune.  ``ids=False``: the
        victims' IDs are not read back (no ``"ids"`` in the result)."""
        if pin is None:
            iptr, n_pin, flags, _keep = 0, 0, 0, None
        else:
            iptr, n_pin, flags, _keep = _ids_arg(pin, n_pin)
        if dry:
            flags |= _lib.DSX_EVICT_DRY
        tot = _lib.StoreEvictTotals()
        with self._lock:
            cap = self.counts()["chunks"] if ids else 0
            out = np.empty((max(1, cap), 32), dtype=np.uint8) if ids else None
            rc = lib().dsx_store_evict(self.ctx.h, self.h, int(need_bytes), int(need_chunks),
                                       ctypes.c_void_p(iptr), n_pin, out.ctypes.data if ids else None, cap,
                                       int(window), ctypes.byref(tot), flags)
            totals = {k: getattr(tot, k) for k, _ in _lib.StoreEvictTotals._fields_ if k != "reserved"}
            try:
                self._state_check(rc)
            except DsxError as e:
                e.totals = totals
                raise
        if ids:
            totals["ids"] = out[:totals["evicted"]].copy()
        return totals

    def _make_room(self, err, chunks, nbytes, pin, n_pin):
        """A put or a copy got DSX_E_CAPACITY (``err``): evicts for exactly what it
        lacks, its own IDs pinned.  Raises ``err`` if that room cannot be made."""
        try:
            self.Evict(need_bytes=nbytes, need_chunks=chunks, pin=pin, n_pin=n_pin, ids=False)
        except DsxError as e:
            if e.code == _lib.DSX_E_CAPACITY:
                raise err from None
            raise

    # ---- the write side --------------------------------------------------------------
    def put(self, blob, ids, ends, start=0, n=None):
        """dsx_store_put: stores the chunks [start, ends[0]), [ends[0], ends[1]),
        ... of ``blob`` (a device tensor or a ``(pointer, length)`` pair) under
        ``ids`` (as for :class:`IDSet`: host or device).  ``ends`` is a host
        array, a device tensor of uint64 or an integer device pointer.  The IDs
        are trusted.  Returns the totals as a dict: total, stored,
        stored_bytes, present, repeats.  A put that does not fit raises
        DsxError (DSX_E_CAPACITY) with ``.totals`` what it would have stored,
        and leaves the store unchanged."""
        ptr, length, _keep_blob = _blob_arg(blob)
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
        tot = _lib.StorePutTotals()
        with self._lock:
            for attempt in (0, 1):
                rc = lib().dsx_store_put(self.ctx.h, self.h, ctypes.c_void_p(ptr), length,
                                         ctypes.c_void_p(iptr), ctypes.c_void_p(eptr), int(start), n,
                                         ctypes.byref(tot), flags)
                totals = {k: getattr(tot, k) for k, _ in _lib.StorePutTotals._fields_}
                try:
                    _check(rc, self.ctx)
                except DsxError as e:
                    e.totals = totals
                    if e.code != _lib.DSX_E_CAPACITY or not self.evict or attempt:
                        raise
                    self._make_room(e, totals["stored"], totals["stored_bytes"],
                                    iptr if flags & _lib.DSX_IDS_DEVICE else _keep_ids, n)
                    continue
                break
        return totals

    def put_index(self, blob, index):
        """``put`` of the blob an :class:`Index` describes (its chunks start at 0)."""
        from .extract import _index_arrays
        ids, ends = _index_arrays(index)
        return self.put(blob, ids, ends, 0)

    def StoreChunk(self, chunk):
        """WriteStore.StoreChunk: uploads the chunk's bytes and puts them as one
        chunk (a chunk the store holds is skipped)."""
        import torch
        data = bytes(chunk.Data())
        cid = bytes(chunk.ID())
        with self._lock:
            dev = f"cuda:{self.ctx.device}"
            if data:
                t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
                torch.cuda.synchronize(t.device)  # (torch's stream, not the context's)
            else:
                t = torch.empty(0, dtype=torch.uint8, device=dev)
            self.put((t.data_ptr(), len(data)), np.frombuffer(cid, dtype=np.uint8).reshape(1, 32),
                     np.array([len(data)], dtype=np.uint64))

    # ---- the read side ---------------------------------------------------------------
    def locate(self, ids, n=None):
        """dsx_store_locate -> (offs, sizes, n_missing): the arena offset
        (``OFF_NONE`` if the store does not hold the ID) and stored size (0 if
        missing) per ID, as np.uint64."""
        iptr, n, flags, _keep = _ids_arg(ids, n)
        offs = np.empty(n, dtype=np.uint64)
        sizes = np.empty(n, dtype=np.uint64)
        miss = ctypes.c_uint64()
        with self._lock:
            _check(lib().dsx_store_locate(self.ctx.h, self.h, ctypes.c_void_p(iptr), n,
                                          offs.ctypes.data, sizes.ctypes.data, ctypes.byref(miss),
                                          flags), self.ctx)
        return offs, sizes, miss.value

    def chunk_ids(self, blob, ends, start=0, n=None, algo=None, device_out=False):
        """:func:`chunk_ids_known` against this store, under its lock
        -> (ids, known_off, totals)."""
        with self._lock:
            return chunk_ids_known(self, blob, ends, start, n, algo, device_out)

    def HasChunk(self, cid) -> bool:
        cid = bytes(cid)
        miss = ctypes.c_uint64()
        with self._lock:
            _check(lib().dsx_store_locate(self.ctx.h, self.h, cid, 1, None, None, ctypes.byref(miss), 0),
                   self.ctx)
        return miss.value == 0

    def GetChunk(self, cid) -> bytes:
        """Store.GetChunk: the chunk's bytes, copied out of the arena;
        :class:`ChunkMissing` if the store does not hold it."""
        cid = bytes(cid)
        with self._lock:
            offs, sizes, miss = self.locate([cid])
            if miss:
                raise ChunkMissing(cid)
            if self.tracked:
                self.Touch([cid])
            size = int(sizes[0])
            out = np.empty(size, dtype=np.uint8)
            if size:
                base, _ = self.arena()
                _lib.check(lib().dsx_copy(self.ctx.h, out.ctypes.data,
                                          ctypes.c_void_p(base + int(offs[0])), size), self.ctx.h)
            return out.tobytes()

    def read_ranges(self, index, ranges, out=None):
        """:func:`desync_amd.read_ranges` of this store, under its lock: the byte
        ranges ``ranges`` of the blob ``index`` (an :class:`Index` or a
        :class:`DeviceIndex`) describes, in one dsx_read_ranges call
        -> (device tensor, totals).  A read stamps nothing in a tracked store:
        ``Touch(index)`` when a read should count as a use."""
        from .readseeker import read_ranges
        with self._lock:
            return read_ranges(index, self, ranges, out=out)

    def resolve(self, ids, segs, n=None):
        """dsx_store_resolve on a plan's structured segment array (in place)
        -> (n_missing, n_wrong_size, first_bad)."""
        iptr, n, flags, _keep = _ids_arg(ids, n)
        miss, wrong, bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        with self._lock:
            _check(lib().dsx_store_resolve(self.ctx.h, self.h, ctypes.c_void_p(iptr), n,
                                           ctypes.c_void_p(segs.ctypes.data), len(segs),
                                           ctypes.byref(miss), ctypes.byref(wrong), ctypes.byref(bad),
                                           flags), self.ctx)
        return miss.value, wrong.value, bad.value

    def Verify(self, algo=None, repair=False):
        """LocalStore.Verify (local.go:103-161): re-hashes every stored chunk in
        the arena and returns the IDs of those that do not hash to their ID (an
        empty list for a sound store).  ``algo`` defaults to the package-global
        Digest.  With ``repair`` the bad chunks are then removed, all in one
        prune; without it nothing is removed."""
        with self._lock:
            bad = self.verify_entries(algo)
            if not bad:
                return []
            ids, _ = self.entries()
            if repair:
                self._prune(ids[bad], remove=True)
            return [ids[e].tobytes() for e in bad]

    def verify_entries(self, algo=None):
        """Verify() as ascending entry numbers."""
        with self._lock:
            n = self.counts()["chunks"]
            bad = np.empty(max(1, n), dtype=np.uint32)
            n_bad = ctypes.c_uint64()
            _check(lib().dsx_store_verify(self.ctx.h, self.h, _digest_code(algo), bad.ctypes.data, n,
                                          ctypes.byref(n_bad)), self.ctx)
            return bad[:n_bad.value].tolist()

    # ---- retention -------------------------------------------------------------------
    def _prune(self, ids, remove=False, window=0, n=None):
        iptr, n, flags, _keep = _ids_arg(ids, n)
        if remove:
            flags |= _lib.DSX_PRUNE_REMOVE
        tot = _lib.StorePruneTotals()
        with self._lock:
            _check(lib().dsx_store_prune(self.ctx.h, self.h, ctypes.c_void_p(iptr), n, int(window),
                                         ctypes.byref(tot), flags), self.ctx)
        return {k: getattr(tot, k) for k, _ in _lib.StorePruneTotals._fields_}

    def Prune(self, ids, window=0, n=None):
        """PruneStore.Prune (local.go:163-202): removes every chunk whose ID is
        not among ``ids`` and compacts the arena in place (dsx_store_prune).
        ``ids`` is an iterable of 32-byte IDs, an ``(n, 32)`` array, device
        memory (as for :class:`IDSet`), an :class:`Index`, or a list of
        indexes, whose IDs are merged as ``desync prune`` merges them
        (prune.go:71-81).  Returns the totals as a dict: entries, kept,
        kept_bytes, removed, removed_bytes, moved, moved_bytes, unmatched.
        Arena offsets taken before (``locate``, a resolved plan) are stale
        afterwards.  ``window`` bounds the compaction's scratch (0: the default)."""
        from .index import Index
        if isinstance(ids, (list, tuple)) and ids and all(isinstance(i, Index) for i in ids):
            ids = np.concatenate([_host_ids(i) for i in ids])
        return self._prune(ids, False, window, n)

    def RemoveChunk(self, cid):
        """LocalStore.RemoveChunk (local.go:69-75): removes one chunk;
        :class:`ChunkMissing` if the store does not hold it."""
        cid = bytes(cid)
        if len(cid) != 32:
            raise ValueError("a chunk ID is 32 bytes")
        if not self._prune([cid], remove=True)["removed"]:
            raise ChunkMissing(cid)

    # ---- copying between stores, growing (copy.go) ------------------------------------------
    def CopyFrom(self, src, ids=None, n=None):
        """dsx_store_copy: appends the chunks of ``src`` (a :class:`DeviceStore`
        of the same context) that ``ids`` names and this store does not hold, in
        the order of their first occurrence, without a host round trip.  ``ids``
        is as for :class:`IDSet` (host, or device memory with ``n``); ``None``
        means every entry of ``src`` (DSX_COPY_ALL).  Returns the totals as a
        dict: total, copied, copied_bytes, present, repeats, missing,
        first_missing.  All or nothing: with ``missing`` > 0 nothing was copied
        (``first_missing`` is the lowest position in ``ids`` of an ID neither
        store holds; :func:`desync_amd.Copy` raises :class:`ChunkMissing` for
        it), and a copy that does not fit raises DsxError (DSX_E_CAPACITY) with
        ``.totals`` what it would have copied; the store is unchanged either way."""
        if not isinstance(src, DeviceStore):
            raise TypeError("CopyFrom takes a DeviceStore (desync_amd.Copy copies from any store)")
        if ids is None:
            iptr, n, flags, _keep = 0, 0, _lib.DSX_COPY_ALL, None
        else:
            iptr, n, flags, _keep = _ids_arg(ids, n)
        tot = _lib.StoreCopyTotals()
        first, second = sorted((self, src), key=id)  # (one lock order for every pair)
        with first._lock, second._lock:
            for attempt in (0, 1):
                rc = lib().dsx_store_copy(self.ctx.h, self.h, src.h, ctypes.c_void_p(iptr), n,
                                          ctypes.byref(tot), flags)
                totals = {k: getattr(tot, k) for k, _ in _lib.StoreCopyTotals._fields_ if k != "reserved"}
                try:
                    _check(rc, self.ctx)
                except DsxError as e:
                    e.totals = totals
                    if e.code != _lib.DSX_E_CAPACITY or not self.evict or attempt:
                        raise
                    if ids is None:  # (every entry of src: its IDs, copied inside HBM)
                        pin, n_pin, _pin_keep = src._device_ids()
                    else:
                        pin, n_pin = (iptr if flags & _lib.DSX_IDS_DEVICE else _keep), n
                    self._make_room(e, totals["copied"], totals["copied_bytes"], pin, n_pin)
                    continue
                break
        return totals

    def _device_ids(self):
        """-> (device pointer, count, the tensor that holds them): the entries'
        IDs in a device tensor, copied there without crossing to the host."""
        import torch
        n = self.counts()["chunks"]
        t = torch.empty((max(1, n), 32), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
        torch.cuda.synchronize(t.device)  # (torch's stream, not the context's)
        if n:
            _check(lib().dsx_store_entries(self.ctx.h, self.h, 0, n, ctypes.c_void_p(t.data_ptr()), None,
                                           _lib.DSX_OUT_DEVICE), self.ctx)
        return t.data_ptr(), n, t

    def Grow(self, arena_bytes, max_chunks):
        """Gives the store a new capacity: creates a store of ``arena_bytes``
        and ``max_chunks``, copies every entry into it in entry order
        (dsx_store_copy with DSX_COPY_ALL: the same entries, ends and arena
        bytes), and destroys the old one.  If the new capacity is below the
        current fill the copy raises DsxError (DSX_E_CAPACITY) and the store
        stays as it was.  The arena's address changes: offsets taken before
        (``arena``, ``locate``, a resolved plan) are stale afterwards, as after
        a prune.  Needs the memory of both stores while it runs.  A tracked store
        stays tracked and keeps its stamps, its clock and so its use order.
        Returns the copy's totals."""
        with self._lock:
            h = ctypes.c_void_p()
            _check(lib().dsx_store_create(self.ctx.h, int(arena_bytes), int(max_chunks), ctypes.byref(h)),
                   self.ctx)
            if self.tracked:  # (the copy of every entry into an empty tracked store carries the stamps)
                rc = lib().dsx_store_track(self.ctx.h, h)
                if rc < 0:
                    lib().dsx_store_destroy(self.ctx.h, h)
                    _check(rc, self.ctx)
            tot = _lib.StoreCopyTotals()
            rc = lib().dsx_store_copy(self.ctx.h, h, self.h, None, 0, ctypes.byref(tot), _lib.DSX_COPY_ALL)
            totals = {k: getattr(tot, k) for k, _ in _lib.StoreCopyTotals._fields_ if k != "reserved"}
            try:
                _check(rc, self.ctx)
            except DsxError as e:
                lib().dsx_store_destroy(self.ctx.h, h)
                e.totals = totals
                raise
            old, self.h = self.h, h
            lib().dsx_store_destroy(self.ctx.h, old)
        return totals

    # ---- storage converters and persistence (encrypt.go, local.go) -------------------------
    def _entry_end(self, e):
        """The arena end of entry e (0 for e < 0)."""
        if e < 0:
            return 0
        end = np.empty(1, dtype=np.uint64)
        _check(lib().dsx_store_entries(self.ctx.h, self.h, int(e), 1, None, end.ctypes.data, 0), self.ctx)
        return int(end[0])

    def Seal(self, converter, first=0, n=None, nonces=None):
        """Seals the entries [first, first + n) where they lie in the arena, with
        the store's device ends (dsx_aead_seal, DSX_ENDS_DEVICE): what a store with
        ``encryption: true`` writes for them.  ``nonces``: n * 24 bytes, or None
        for fresh random ones (as the reference draws one per chunk).  Returns
        (the record buffer, a device tensor of uint8; the record ends as
        np.uint64): record i is ``buffer[ends[i-1]:ends[i]]``."""
        import torch
        from .encrypt import AEADConverter, aead_seal
        if not isinstance(converter, AEADConverter):
            raise TypeError("Seal takes an AEAD converter (NewXChaCha20Poly1305)")
        with self._lock:
            chunks = self.counts()["chunks"]
            n = chunks - first if n is None else int(n)
            if first < 0 or n < 0 or first + n > chunks:
                raise ValueError(f"entries [{first}, {first + n}) of {chunks}")
            dev = f"cuda:{self.ctx.device}"
            if not n:
                return torch.empty(0, dtype=torch.uint8, device=dev), np.empty(0, dtype=np.uint64)
            start, end = self._entry_end(first - 1), self._entry_end(first + n - 1)
            d_ends = torch.empty(n, dtype=torch.int64, device=dev)
            _check(lib().dsx_store_entries(self.ctx.h, self.h, int(first), n, None,
                                           ctypes.c_void_p(d_ends.data_ptr()), _lib.DSX_OUT_DEVICE), self.ctx)
            cap = end - start + _lib.DSX_AEAD_OVERHEAD * n
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            base, used = self.arena()
            _, rec_ends = aead_seal(converter.key, base, used, d_ends.data_ptr(), start, n, nonces,
                                    ctx=self.ctx, out=(out.data_ptr(), cap))
            return out, rec_ends

    def PutSealed(self, records, rec_ends, ids, converter, verify=True):
        """Opens the records ``records[rec_ends[i-1]:rec_ends[i]]`` (a device tensor
        or a ``(pointer, length)`` pair; what :meth:`Seal` returns) into a scratch
        blob and puts the plaintexts under ``ids``.  A record that fails
        authentication raises :class:`AuthenticationError` naming the entries
        (``.entries``) before anything is put; with ``verify`` the plaintexts are
        re-hashed and compared with ``ids`` first (``ChunkInvalid``).  The store is
        unchanged on any failure.  Returns the put totals."""
        from .encrypt import ERR_OPEN, AEADConverter, AuthenticationError, aead_open
        from .make import chunk_ids
        if not isinstance(converter, AEADConverter):
            raise TypeError("PutSealed takes an AEAD converter (NewXChaCha20Poly1305)")
        ptr, length, _keep = _blob_arg(records)
        ids = _host_ids(ids)
        rec_ends = np.ascontiguousarray(rec_ends, dtype=np.uint64)
        if len(ids) != rec_ends.size:
            raise ValueError(f"{len(ids)} IDs but {rec_ends.size} record ends")
        with self._lock:
            plain, ends, bad = aead_open(converter.key, ptr, length, rec_ends, 0, ctx=self.ctx)
            if bad:
                shown = ", ".join(str(b) for b in bad[:8]) + (", ..." if len(bad) > 8 else "")
                raise AuthenticationError(f"{ERR_OPEN}: {len(bad)} of {rec_ends.size} records "
                                          f"(entries {shown})", bad)
            total = int(ends[-1]) if ends.size else 0
            if verify and ends.size:
                got = chunk_ids(plain.data_ptr(), total, ends, 0, ctx=self.ctx,
                                algo=_digest_code(digest.Digest.Algorithm()))
                got = np.frombuffer(b"".join(got), dtype=np.uint8).reshape(-1, 32)
                wrong = np.flatnonzero(np.any(got != ids, axis=1))
                if wrong.size:
                    i = int(wrong[0])
                    raise ChunkInvalid(ids[i].tobytes(), got[i].tobytes())
            return self.put((plain.data_ptr(), total), ids, ends, 0)

    def WriteLocal(self, base, converters=()):
        """Writes every entry as a chunk file of a LocalStore at ``base``
        (local.go:78-98, :234-239): ``<base>/<hex[0:4]>/<hex><extension>``, through
        a temporary file and a rename, directories 0755 and files 0644 (before
        the umask).  ``converters`` is empty -- plain chunks, the
        ``Uncompressed: true`` store -- or one AEAD converter, whose records are
        made on the GPU in one call (:meth:`Seal`).  A :class:`Compressor` is
        refused: zstd is not available.  Returns the number of files written."""
        from .encrypt import _download
        conv = _local_converters(converters)
        ext = conv.storageExtension()
        with self._lock:
            ids, ends = self.entries()
            if conv:
                buf, ends = self.Seal(conv[0])
                data = _download(self.ctx, buf.data_ptr(), int(ends[-1]) if ends.size else 0)
            else:
                ptr, used = self.arena()
                data = _download(self.ctx, ptr, used)
        prev = 0
        for cid, end in zip(ids, ends):
            d, p = chunk_file_name(base, cid.tobytes(), ext)
            os.makedirs(d, mode=0o755, exist_ok=True)
            fd, tmp = tempfile.mkstemp(prefix=TMP_CHUNK_PREFIX, dir=d)
            try:
                with os.fdopen(fd, "wb") as f:
                    f.write(data[prev:int(end)].tobytes())
                os.chmod(tmp, 0o644 & ~_umask())
                os.rename(tmp, p)
            except BaseException:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise
            prev = int(end)
        return len(ids)

    def ReadLocal(self, base, converters=(), ids=None, verify=True):
        """Puts the chunks of the LocalStore at ``base`` into this store: every
        file whose name is a chunk ID plus the converters' extension (others are
        skipped, as local.go:148-150 does: they may belong to other settings), or
        exactly ``ids`` (:class:`ChunkMissing` for an absent one).  Sealed records
        are opened on the GPU in one call (:meth:`PutSealed`): a record that does
        not authenticate -- another key -- raises and leaves the store unchanged.
        With ``verify`` the chunks are re-hashed against their file names.
        Returns the put totals."""
        from .encrypt import _upload
        conv = _local_converters(converters)
        ext = conv.storageExtension()
        if ids is None:
            found = []
            for root, _dirs, files in sorted(os.walk(base)):
                for name in sorted(files):
                    cid = chunk_id_from_filename(name, ext)
                    if cid is not None:
                        found.append((cid, os.path.join(root, name)))
        else:
            found = []
            for cid in _host_ids(ids):
                cid = cid.tobytes()
                p = chunk_file_name(base, cid, ext)[1]
                if not os.path.exists(p):
                    raise ChunkMissing(cid)
                found.append((cid, p))
        parts = []
        for _cid, p in found:
            with open(p, "rb") as f:
                parts.append(f.read())
        cids = np.frombuffer(b"".join(c for c, _ in found), dtype=np.uint8).reshape(-1, 32)
        ends = np.cumsum([len(b) for b in parts], dtype=np.uint64) if parts else np.empty(0, np.uint64)
        blob = b"".join(parts)
        with self._lock:
            dev = _upload(self.ctx, blob)
            if conv:
                return self.PutSealed((dev.data_ptr(), len(blob)), ends, cids, conv[0], verify=verify)
            if verify and len(parts):
                from .make import chunk_ids
                got = chunk_ids(dev.data_ptr(), len(blob), ends, 0, ctx=self.ctx,
                                algo=_digest_code(digest.Digest.Algorithm()))
                got = np.frombuffer(b"".join(got), dtype=np.uint8).reshape(-1, 32)
                wrong = np.flatnonzero(np.any(got != cids, axis=1))
                if wrong.size:
                    i = int(wrong[0])
                    raise ChunkInvalid(cids[i].tobytes(), got[i].tobytes())
            return self.put((dev.data_ptr(), len(blob)), cids, ends, 0)

    # ---- life ------------------------------------------------------------------------
    def close(self):
        with self._lock:
            if self.h is not None:
                if self.ctx.h:  # (a closed context has freed its stores)
                    lib().dsx_store_destroy(self.ctx.h, self.h)
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


def chunk_ids_known(store, blob, ends, start=0, n=None, algo=None, device_out=False):
    """dsx_chunk_ids_known: the IDs of the chunks [start, ends[0]), [ends[0],
    ends[1]), ... of ``blob`` (a device tensor or a ``(pointer, length)`` pair)
    and where ``store`` holds them, in one call.  A chunk whose bytes equal a
    stored entry's bytes gets that entry's ID by comparison; the others are
    hashed and then looked up (make.go:223, chunkstorage.go:44-67).

    ``ends`` is a host array, a device tensor of uint64, or an integer device
    pointer with ``n``.  ``algo`` defaults to the package-global Digest and must
    be the digest the store was filled with.  Returns ``(ids, known_off,
    totals)``: ``ids`` as ``(n, 32)`` uint8 and ``known_off`` as uint64
    (``OFF_NONE`` where the store lacks the ID), both exactly what dsx_chunk_ids
    and ``store.locate`` give -- numpy arrays, or device tensors with
    ``device_out`` (uint8 and int64) -- and the dsx_known_totals_t as a dict."""
    ptr, length, _keep_blob = _blob_arg(blob)
    flags = 0
    if isinstance(ends, int):
        if n is None:
            raise ValueError("a device pointer to the ends needs n")
        eptr, n, _keep_ends = ends, int(n), None
        flags |= DSX_ENDS_DEVICE
    elif _is_device(ends):
        if ends.element_size() != 8 or not ends.is_contiguous():
            raise ValueError("device ends must be contiguous uint64")
        n = ends.numel() if n is None else int(n)
        eptr, _keep_ends = ends.data_ptr(), ends
        flags |= DSX_ENDS_DEVICE
    else:
        _keep_ends = np.ascontiguousarray(ends, dtype=np.uint64)
        n = _keep_ends.size if n is None else int(n)
        if n > _keep_ends.size:
            raise ValueError(f"n = {n} but {_keep_ends.size} chunk ends")
        eptr = _keep_ends.ctypes.data
    if device_out:
        import torch
        dev = f"cuda:{store.ctx.device}"
        ids = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        offs = torch.empty(n, dtype=torch.int64, device=dev)
        iptr, optr = ids.data_ptr(), offs.data_ptr()
        flags |= _lib.DSX_OUT_DEVICE
    else:
        ids = np.empty((n, 32), dtype=np.uint8)
        offs = np.empty(n, dtype=np.uint64)
        iptr, optr = ids.ctypes.data, offs.ctypes.data
    tot = _lib.KnownTotals()
    with store._lock:
        rc = lib().dsx_chunk_ids_known(store.ctx.h, store.h, ctypes.c_void_p(ptr), length, int(start),
                                       ctypes.c_void_p(eptr), n, _digest_code(algo),
                                       ctypes.c_void_p(iptr), ctypes.c_void_p(optr),
                                       ctypes.byref(tot), flags)
        if rc == _lib.DSX_E_STATE:
            d = lib().dsx_last_error(store.ctx.h)
            raise DsxError(rc, d.decode() if d else "")
        _check(rc, store.ctx)
    totals = {k: getattr(tot, k) for k, _ in _lib.KnownTotals._fields_ if k != "reserved"}
    return ids, offs, totals


def ChopBlob(index, blob, store, verify=True, known=False):
    """ChopFile (chop.go:14-81) for a blob in HBM: stores every chunk of
    ``index`` out of ``blob`` (a device tensor or a ``(pointer, length)``
    pair) into ``store``, a :class:`DeviceStore`.

    With ``verify`` every chunk is first re-hashed where it lies
    (dsx_chunk_ids, NewChunkWithID's check, chunk.go:37-73) and compared with
    the index; the first mismatch raises ``ChunkInvalid(id, sum)``.  Then comes
    one ``put``.  Unlike ChopFile, whose workers may already have stored
    earlier chunks when one turns out invalid, nothing is stored when a chunk
    is invalid: the check of the whole blob comes before the put.  With
    ``known`` the re-hash is dsx_chunk_ids_known against ``store``: a chunk whose
    bytes the store already holds is compared with them instead of hashed, with
    the same IDs as the result.  Returns the put totals as a dict."""
    from .extract import _index_arrays
    from .make import chunk_ids
    ids, ends = _index_arrays(index)
    ptr, length, _keep = _blob_arg(blob)
    if len(ends) and int(ends[-1]) > length:
        raise EOFError("unexpected EOF")  # (io.ReadFull on a file shorter than its index)
    if verify and len(ends):
        if known:
            got = store.chunk_ids((ptr, length), ends, 0)[0]
        else:
            with store._lock:
                got = chunk_ids(ptr, length, ends, 0, ctx=store.ctx,
                                algo=_digest_code(digest.Digest.Algorithm()))
            got = np.frombuffer(b"".join(got), dtype=np.uint8).reshape(-1, 32)
        bad = np.flatnonzero(np.any(got != ids, axis=1))
        if bad.size:
            i = int(bad[0])
            raise ChunkInvalid(ids[i].tobytes(), got[i].tobytes())
    return store.put((ptr, length), ids, ends, 0)


def ChopBlobs(blobs, store, min_size, avg_size, max_size, known=False):
    """``desync make -s`` over many blobs in HBM: :func:`IndexFromBlobs` (one
    cut call and one hash call for all of them), then one ``put`` of every
    chunk into ``store``, a :class:`DeviceStore`.  ``blobs`` as for
    IndexFromBlobs (a list is packed first, which costs a copy).  The IDs were
    just computed from the bytes, so nothing is re-hashed.  With ``known`` the
    IDs come from dsx_chunk_ids_known against ``store`` (chunks it already holds
    are compared, not hashed); the indexes and the store are the same either
    way.  Returns the list of indexes, one per blob (``store.counts()`` has the
    fill state)."""
    from .make import _index_blobs
    with store._lock:
        indexes, ptr, length, ends, ids, _keep = _index_blobs(blobs, min_size, avg_size, max_size,
                                                              store.ctx, store if known else None)
        if len(ends):
            store.put((ptr, length), ids, ends, 0)
    return indexes


__all__ = ["DeviceStore", "ChopBlob", "ChopBlobs", "chunk_ids_known", "OFF_NONE", "chunk_file_name", "chunk_id_from_filename"]
