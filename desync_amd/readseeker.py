"""Byte ranges of an indexed blob read out of a chunk store in HBM.

Reference interface:
    NewIndexReadSeeker, IndexPos.Read / Seek     (readseeker.go)
    desync cat -o OFFSET -l LENGTH               (cmd/desync/cat.go:95-105)

The reference serves a read one chunk at a time: bisect the index, fetch the
chunk (or take the null chunk from memory), check its size, copy.  Here many
ranges are one call (dsx_read_ranges): kernels find the chunks
each range touches, look them up in the :class:`DeviceStore`'s ID table, check
their sizes and gather the bytes, without the index, the store's offsets or a
segment list crossing to the host.  :class:`DeviceIndex` keeps an index's IDs
and chunk ends in HBM, so a second read of the same index uploads nothing but
the ranges.  Out of scope: seeds as a source, ranges in device memory, reads
across two stores, a FUSE mount, compressed or sealed stores (``PutSealed``
first).
"""
from __future__ import annotations

import contextlib
import ctypes
import io

import numpy as np

from . import _lib
from ._lib import DSX_ENDS_DEVICE, DsxError, lib
from .digest import NewNullChunk
from .errors import ChunkMissing
from .index import Index
from .info import _ids_arg, _is_device

BAD_NONE = 0xFFFFFFFF  # first_bad_range / first_bad_chunk: none
_CAT_STEP = 64 << 20   # Cat copies this many bytes a read


def _check(rc, ctx):
    """check() with the context's detail for argument and state errors too."""
    if rc < 0:
        d = lib().dsx_last_error(ctx.h) if rc in (_lib.DSX_E_INVAL, _lib.DSX_E_STATE) else None
        if d:
            raise DsxError(rc, d.decode())
        _lib.check(rc, ctx.h)
    return rc


def ranges_array(ranges):
    """-> an (n, 3) uint64 array of {off, len, dst_off}.  ``ranges`` is a list (or
    array) of ``(off, len)``, which are packed back to back in the output, or of
    ``(off, len, dst_off)``."""
    a = np.asarray(ranges, dtype=np.uint64)
    if a.size == 0:
        return np.empty((0, 3), dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] not in (2, 3):
        raise ValueError("ranges are (off, len) or (off, len, dst_off)")
    if a.shape[1] == 2:
        dst = np.cumsum(a[:, 1], dtype=np.uint64) - a[:, 1]
        a = np.column_stack([a, dst])
    return np.ascontiguousarray(a, dtype=np.uint64)


def read_plan(ends, ranges, start=0):
    """dsx_read_plan: the (range, chunk) pairs of a read as a structured array
    with the fields chunk_off, dst_off, bytes, range, chunk -- the arithmetic
    the kernels run, on the host and without a context."""
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    rg = ranges_array(ranges)
    dt = np.dtype([("chunk_off", "<u8"), ("dst_off", "<u8"), ("bytes", "<u8"), ("range", "<u4"),
                   ("chunk", "<u4")])
    assert dt.itemsize == ctypes.sizeof(_lib.ReadPiece)
    n = ctypes.c_uint64()
    out = np.empty(0, dtype=dt)
    rc = lib().dsx_read_plan(ends.ctypes.data, int(start), ends.size, rg.ctypes.data, len(rg),
                             None, 0, ctypes.byref(n))
    if rc == _lib.DSX_E_CAPACITY:
        out = np.empty(n.value, dtype=dt)
        rc = lib().dsx_read_plan(ends.ctypes.data, int(start), ends.size, rg.ctypes.data, len(rg),
                                 out.ctypes.data, len(out), ctypes.byref(n))
    _lib.check(rc)
    return out


def _out_arg(out):
    if isinstance(out, tuple):
        return int(out[0]), int(out[1])
    if _is_device(out):
        if not out.is_contiguous():
            raise ValueError("the output must be contiguous")
        return out.data_ptr(), out.numel() * out.element_size()
    raise TypeError("the output is a device tensor or a (device pointer, length) pair")


def read_ranges_raw(store, ids, ends, ranges, out, start=0, null_id=None, null_size=0, n=None):
    """dsx_read_ranges as it is: ``ids`` as for :class:`IDSet` (host or device),
    ``ends`` a host array, a device tensor of uint64 or an integer device
    pointer, ``ranges`` as for :func:`ranges_array`, ``out`` a device tensor or a
    ``(pointer, length)`` pair.  Returns the totals as a dict and raises for
    nothing but a refused call: the counts are the answer."""
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
    rg = ranges_array(ranges)
    optr, olen = _out_arg(out)
    null = None
    if null_id is not None:
        null = bytes(null_id)
        if len(null) != 32:
            raise ValueError("a chunk ID is 32 bytes")
    tot = _lib.ReadTotals()
    with store._lock:
        _check(lib().dsx_read_ranges(store.ctx.h, store.h, ctypes.c_void_p(iptr), ctypes.c_void_p(eptr),
                                     int(start), n, null, int(null_size), rg.ctypes.data, len(rg),
                                     ctypes.c_void_p(optr), olen, ctypes.byref(tot), flags), store.ctx)
    return {k: getattr(tot, k) for k, _ in _lib.ReadTotals._fields_}


class DeviceIndex:
    """An index's chunk IDs and chunk ends uploaded once to the context's GPU:
    what :func:`read_ranges` and the seeker hand to dsx_read_ranges with
    DSX_IDS_DEVICE | DSX_ENDS_DEVICE.  The null chunk is
    ``NewNullChunk(index.Index.ChunkSizeMax)``, as NewIndexReadSeeker's."""

    def __init__(self, index: Index, ctx=None, device=0):
        from .encrypt import _upload
        from .extract import _index_arrays
        self.ctx = ctx or _lib.default_context(device)
        self.index = index
        self.ids, self.ends = _index_arrays(index)
        self.n = len(self.ends)
        self.length = int(self.ends[-1]) if self.n else 0
        self.null = NewNullChunk(index.Index.ChunkSizeMax)
        self.d_ids = _upload(self.ctx, self.ids.tobytes())
        self.d_ends = _upload(self.ctx, np.ascontiguousarray(self.ends, dtype=np.uint64).tobytes())

    def Length(self):
        return self.length

    def close(self):
        self.d_ids = self.d_ends = None


def read_ranges(index, store, ranges, out=None, ctx=None):
    """Reads the byte ranges ``ranges`` of the blob ``index`` describes out of
    ``store``, a :class:`DeviceStore`, in one call (dsx_read_ranges).

    ``index`` is an :class:`Index` (uploaded for this call) or a
    :class:`DeviceIndex` (nothing but the ranges is uploaded).  ``ranges`` is a
    list of ``(off, len)``, packed back to back in the output, or of ``(off, len,
    dst_off)`` with ascending, non-overlapping destination windows.  ``out`` is a
    uint8 device tensor to write into, or None for a new one that just holds the
    windows.  Returns ``(the device tensor, the totals as a dict)``.

    All or nothing: a chunk the store does not hold raises
    :class:`ChunkMissing`, a stored size that differs from the index's (or a
    null-chunk ID with another size than the null chunk's)
    ``ValueError("unexpected size for chunk <hex id>")`` (readseeker.go:123-126)
    for the lowest such chunk, and a range that leaves the blob ValueError; the
    output is then untouched.  A chunk with the null chunk's ID is read as zeros
    without asking the store (readseeker.go:106-107)."""
    import torch

    ctx = ctx or store.ctx
    if ctx is not store.ctx:
        raise ValueError("the store belongs to another context")
    di = index if isinstance(index, DeviceIndex) else None
    if di is not None and di.ctx is not ctx:
        raise ValueError("the DeviceIndex belongs to another context")
    rg = ranges_array(ranges)
    if out is None:
        need = int((rg[:, 2] + rg[:, 1]).max()) if len(rg) else 0
        out = torch.empty(need, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    with store._lock:
        if di is None:
            di = DeviceIndex(index, ctx)
        tot = read_ranges_raw(store, di.d_ids.data_ptr(), di.d_ends.data_ptr(), rg, out, 0, di.null.ID,
                              len(di.null.Data), n=di.n)
        _raise_for(tot, di.ids, di.null, di.length, rg, store.HasChunk)
    return out, tot


def _raise_for(tot, ids, null, length, rg, has_chunk):
    """The reference's errors for a read's totals."""
    if tot["beyond"]:
        r = next(i for i, (off, ln, _) in enumerate(rg.tolist()) if off + ln > length)
        raise ValueError(f"range {r} [{int(rg[r, 0])}, {int(rg[r, 0] + rg[r, 1])}) is beyond the blob's "
                         f"{length} bytes")
    if tot["missing"] or tot["wrong_size"]:
        cid = bytes(ids[tot["first_bad_chunk"]])
        if cid != null.ID and not has_chunk(cid):
            raise ChunkMissing(cid)
        raise ValueError(f"unexpected size for chunk {cid.hex()}")


class IndexPos(io.RawIOBase):
    """IndexPos (readseeker.go): a position inside the blob an index describes,
    read out of ``Store``.  ``Seek`` / ``Read`` mirror the reference;
    ``ReadAt``, ``read_device`` and the :mod:`io` raw-stream methods (``read``,
    ``readinto``, ``readall``, ``seek``, ``tell``) make it a file object, so
    ``io.BufferedReader(seeker)`` and ``shutil.copyfileobj`` work.

    ``Store`` is a :class:`DeviceStore`, or any object with
    ``read_ranges(index, ranges) -> (bytes-like or device tensor, totals)``.  A
    read is one dsx_read_ranges call however many chunks it spans; nothing is
    cached between reads, so a store pruned or grown in between is read as it
    is."""

    def __init__(self, index: Index, store):
        super().__init__()
        self.Store = store
        self.Index = index
        self.Length = index.Length()
        self.pos = 0
        self._src = None  # what Store.read_ranges is given: a DeviceIndex for a DeviceStore

    # ---- readseeker.go -----------------------------------------------------------------
    def Seek(self, offset, whence=io.SEEK_SET):
        """Seek (readseeker.go:131-152) -> the new position.  Errors are
        ValueError with the reference's text and leave the position unchanged:
        "invalid whence", "unable to seek before start of file", and beyond the
        end "seek found chunk ending at position X, desired position is Y".
        Exactly ``Length`` is fine.  An empty index has no chunk to find: the
        position is tracked and beyond 0 EOFError is raised, as the reference
        returns io.EOF (:62-65, :148-150)."""
        offset = int(offset)
        if whence == io.SEEK_SET:
            new = offset
        elif whence == io.SEEK_CUR:
            new = self.pos + offset
        elif whence == io.SEEK_END:
            new = self.Length + offset
        else:
            raise ValueError("invalid whence")
        if new < 0:
            raise ValueError("unable to seek before start of file")
        if len(self.Index.Chunks) == 0:
            self.pos = new
            if new > self.Length:
                raise EOFError("EOF")
            return new
        if new > self.Length:
            raise ValueError(f"seek found chunk ending at position {self.Length}, desired position is {new}")
        self.pos = new
        return new

    def _source(self):
        if self._src is None:
            from .store import DeviceStore
            self._src = DeviceIndex(self.Index, self.Store.ctx) if isinstance(self.Store, DeviceStore) \
                else self.Index
        return self._src

    def _fetch(self, off, n, device=False):
        with getattr(self.Store, "_lock", None) or contextlib.nullcontext():  # (a context is not thread-safe)
            got, _tot = self.Store.read_ranges(self._source(), [(off, n)])
            if device or not _is_device(got):
                return got
            from .encrypt import _download
            return _download(self.Store.ctx, got.data_ptr(), n)

    def _clip(self, off, n):
        return max(0, min(int(n), self.Length - off))

    def Read(self, n):
        """Read (readseeker.go:154-180) -> up to ``n`` bytes from the position,
        which moves behind them: fewer at the end of the blob, ``b""`` at or
        past it (io.EOF).  An error (:class:`ChunkMissing`, "unexpected size
        for chunk") leaves the position where it was."""
        n = self._clip(self.pos, n)
        if n == 0:
            return b""
        data = bytes(memoryview(self._fetch(self.pos, n)))
        self.pos += n
        return data

    def ReadAt(self, off, n):
        """io.ReaderAt: up to ``n`` bytes from ``off``; the position stays."""
        off = int(off)
        if off < 0:
            raise ValueError("unable to seek before start of file")
        n = self._clip(off, n)
        return bytes(memoryview(self._fetch(off, n))) if n else b""

    def read_device(self, n):
        """``Read`` without the host copy: a uint8 device tensor (of the
        store's context) of up to ``n`` bytes; empty at the end."""
        n = self._clip(self.pos, n)
        got = self._fetch(self.pos, n, device=True)
        self.pos += n
        return got

    # ---- io.RawIOBase --------------------------------------------------------------------
    def readable(self):
        return True

    def seekable(self):
        return True

    def seek(self, offset, whence=io.SEEK_SET):
        return self.Seek(offset, whence)

    def tell(self):
        return self.pos

    def read(self, size=-1):
        if size is None or size < 0:
            return self.readall()
        return self.Read(size)

    def readall(self):
        return self.Read(max(0, self.Length - self.pos))

    def readinto(self, b):
        data = self.Read(len(b))
        b[:len(data)] = data
        return len(data)


def NewIndexReadSeeker(index: Index, store) -> IndexPos:
    """NewIndexReadSeeker (readseeker.go:27-39)."""
    return IndexPos(index, store)


def Cat(index: Index, store, offset=0, length=0, out=None):
    """``desync cat -o offset -l length`` (cmd/desync/cat.go:95-105): seeks to
    ``offset`` and copies ``length`` bytes, or with ``length == 0`` everything
    up to the end, to the writer ``out`` (returns the number of bytes written)
    or, without one, into the bytes returned.  Fewer bytes than ``length > 0``
    asks for raise EOFError after what exists was written, as io.CopyN
    returns io.EOF."""
    rs = NewIndexReadSeeker(index, store)
    rs.Seek(int(offset), io.SEEK_SET)
    length = int(length)
    parts, done = [], 0
    while length <= 0 or done < length:
        data = rs.Read(_CAT_STEP if length <= 0 else min(_CAT_STEP, length - done))
        if not data:
            break
        done += len(data)
        if out is None:
            parts.append(data)
        else:
            out.write(data)
    if length > 0 and done < length:
        raise EOFError("EOF")
    return b"".join(parts) if out is None else done


__all__ = ["read_ranges", "read_ranges_raw", "read_plan", "ranges_array", "DeviceIndex", "IndexPos",
           "NewIndexReadSeeker", "Cat", "BAD_NONE"]
