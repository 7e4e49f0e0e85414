"""The streaming chunker ABI on the GPU through the seeded scripts of
stream_ref.py: pushes of odd sizes, SYNC commits that put a batch seam at any
byte, pops, pop_many and unpop, Advance, flush, chunk IDs switched at restarts,
the end of a stream, context reuse, the product batches with the host buffer's
moves and grows, and the dense redo inside a stream.  After every call the
model says what it may return; chunk bytes, IDs and the window are compared
with the script's data.  Everything runs on the product library, on contexts
of this file's own."""
import ctypes
import time

import numpy as np
import pytest

import stream_ref as sr

pytestmark = pytest.mark.gpu

PATTERN64 = 0xC3C3C3C3C3C3C3C3
SMALL_SCRIPTS = [n for n in sr.NAMES if n != "S7" and not n.startswith("S8")]


def _L():
    from desync_amd import _lib
    return _lib


def _bytes_at(ptr, n):
    if not ptr or not n:
        return np.empty(0, np.uint8)
    return np.frombuffer((ctypes.c_ubyte * n).from_address(ptr), np.uint8)


class GpuBackend:
    """The raw dsx_stream_* calls on one context as the driver's backend."""

    def __init__(self, ctx):
        self.ctx, self.h, self.L = ctx, ctx.h, _L().lib()
        self.ptr = ctypes.c_void_p()

    def begin(self, mn, av, mx):
        from desync_amd.chunker import Params
        return self.L.dsx_stream_begin(self.h, ctypes.byref(Params(mn, av, mx).c))

    def end(self):
        return self.L.dsx_stream_end(self.h)

    def buffer(self, want):
        self.ptr = ctypes.c_void_p()
        return self.L.dsx_stream_buffer(self.h, want, ctypes.byref(self.ptr))

    def commit_bytes(self, data, flags):
        if len(data):
            ctypes.memmove(self.ptr.value, data.ctypes.data, len(data))
        return self.L.dsx_stream_commit(self.h, len(data), flags)

    def commit(self, n, flags):
        return self.L.dsx_stream_commit(self.h, n, flags)

    def push(self, data, eof):
        return self.L.dsx_stream_push(self.h, data.ctypes.data if len(data) else None, len(data), eof)

    def _id(self):
        p = self.L.dsx_stream_chunk_id(self.h)
        return ctypes.string_at(p, 32) if p else None

    def pop(self):
        start, size = ctypes.c_uint64(PATTERN64), ctypes.c_uint64(PATTERN64)
        rc = self.L.dsx_stream_pop(self.h, ctypes.byref(start), ctypes.byref(size))
        if rc != 1:
            return rc, start.value, size.value, None, None
        return rc, start.value, size.value, _bytes_at(self.L.dsx_stream_chunk_data(self.h), size.value), self._id()

    def pop_many(self, cap, with_ids):
        ends = (ctypes.c_uint64 * (cap + 1))(*([PATTERN64] * (cap + 1)))
        ids = (ctypes.c_uint8 * (32 * cap + 32))(*([0xC3] * (32 * cap + 32))) if with_ids else None
        start, n = ctypes.c_uint64(PATTERN64), ctypes.c_uint64(PATTERN64)
        rc = self.L.dsx_stream_pop_many(self.h, ends, ids, cap, ctypes.byref(start), ctypes.byref(n))
        k = n.value
        assert k <= cap and ends[cap] == PATTERN64 and all(e == PATTERN64 for e in ends[k:]), "pop_many wrote beyond n"
        if with_ids:
            assert bytes(ids[32 * k:]) == b"\xc3" * (32 * (cap - k) + 32), "pop_many wrote IDs beyond n"
        if rc != 1:
            return rc, start.value, list(ends[:k]), None, None
        raw = bytes(ids[:32 * k]) if with_ids else b""
        return (rc, start.value, list(ends[:k]), [raw[32 * i:32 * i + 32] for i in range(k)] if with_ids else None,
                _bytes_at(self.L.dsx_stream_chunk_data(self.h), ends[k - 1] - start.value))

    def unpop(self, pos):
        return self.L.dsx_stream_unpop(self.h, pos)

    def window(self):
        base, pos, n = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        assert self.L.dsx_stream_window(self.h, ctypes.byref(base), ctypes.byref(pos), ctypes.byref(n)) == 0
        return base.value or 0, pos.value, _bytes_at(base.value, n.value)

    def advance(self, n):
        return self.L.dsx_stream_advance(self.h, n)

    def flush(self):
        start, size = ctypes.c_uint64(PATTERN64), ctypes.c_uint64(PATTERN64)
        rc = self.L.dsx_stream_flush(self.h, ctypes.byref(start), ctypes.byref(size))
        chunk = _bytes_at(self.L.dsx_stream_chunk_data(self.h), size.value if rc == 0 else 0)
        return rc, start.value, size.value, chunk, self._id()

    def ids(self, algo):
        return self.L.dsx_stream_ids(self.h, algo)

    def done(self):
        return self.L.dsx_stream_done(self.h)

    def dense_fallbacks(self):
        return int(self.ctx.stats().dense_fallbacks)


@pytest.fixture(scope="module")
def sctx():
    ctx = _L().Context(0)
    yield ctx
    ctx.close()


def run(name, ctx):
    sc = sr.script(name)  # (built, on the model, before the clock starts)
    t0 = time.perf_counter()
    try:
        model = sr.drive(GpuBackend(ctx), sc)
    finally:
        assert _L().lib().dsx_stream_end(ctx.h) == 0
    print(f"{name}: {len(sc['ops'])} ops in {time.perf_counter() - t0:.2f} s on the GPU; host buffer {model.room}")
    return model


@pytest.mark.parametrize("name", SMALL_SCRIPTS)
def test_script(sctx, name):
    """S1-S6 on one context, one after the other: every script leaves it with
    dsx_stream_end, whatever state the one before left the buffers in."""
    run(name, sctx)


def test_product_batches_and_host_buffer():
    """S7 on a fresh context (its host buffer starts at 32 MiB): the feeding
    calls of the two runs must show the buffer moved down, grown, and left
    alone, and every chunk's bytes right after each."""
    ctx = _L().Context(0)
    try:
        model = run("S7", ctx)
    finally:
        ctx.close()
    assert all(model.room[k] >= 1 for k in ("move", "grow", "neither")), model.room
    assert model.room["grow"] >= 2, model.room  # (the first allocation is one; run 2's is the other)


@pytest.mark.parametrize("name", [n for n in sr.NAMES if n.startswith("S8")])
def test_dense_redo_in_a_stream(sctx, name):
    """S8: dense_fallbacks must rise while the tile's batch, which continues a
    chain, is collected (the model's dense_check op)."""
    assert GpuBackend(sctx).dense_fallbacks() is not None
    run(name, sctx)
