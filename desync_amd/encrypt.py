"""Storage converters: what a chunk store applies between a chunk and its file.

Reference interface:
    converter, Converters, Compressor        (converter.go)
    aeadConverter, NewXChaCha20Poly1305,
    NewAES256GCM, EncryptionKeySize          (encrypt.go)
    StoreOptions.StorageConverters           (store.go:124-170)

The XChaCha20-Poly1305 converter runs on the GPU (dsx_aead_seal / dsx_aead_open,
DESIGN.md 4.8): ``toStorage`` / ``fromStorage`` convert one chunk given as host
bytes, as the reference's do, and :func:`aead_seal` / :func:`aead_open` convert
every chunk of a device-resident blob in one call
(:meth:`desync_amd.DeviceStore.Seal` / ``PutSealed`` use them).  A record is
``nonce(24) || ciphertext || tag(16)``.

Not built: AES-256-GCM (GHASH is a carry-less multiplication, which gfx950 has
no instruction for) and zstd (:class:`Compressor` only carries its extension, so
that a configuration naming it is recognised and refused where data would have
to pass through it).
"""
from __future__ import annotations

import binascii
import ctypes
import hashlib
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import DSX_AEAD_NONCE, DSX_AEAD_OVERHEAD, DSX_ENDS_DEVICE, DsxError, lib

EncryptionKeySize = 32

ERR_NO_NONCE = "no nonce prefix found in chunk, not encrypted or wrong algorithm"
ERR_OPEN = "chacha20poly1305: message authentication failed"


class AuthenticationError(ValueError):
    """An AEAD Open failed.  ``entries``: the numbers of the failed records of a
    many-record call."""

    def __init__(self, msg=ERR_OPEN, entries=()):
        super().__init__(msg)
        self.entries = list(entries)


def _check(rc, ctx):
    if rc < 0:
        d = lib().dsx_last_error(ctx.h) if rc in (_lib.DSX_E_INVAL, _lib.DSX_E_CAPACITY, _lib.DSX_E_IO) else None
        if d:
            raise DsxError(rc, d.decode())
        _lib.check(rc, ctx.h)
    return rc


def validateKey(key):
    if len(key) != EncryptionKeySize:
        raise ValueError(f"encryption key must be {EncryptionKeySize} bytes, got {len(key)}")


def _device_bytes(ctx, n):
    import torch
    return torch.empty(max(1, int(n)), dtype=torch.uint8, device=f"cuda:{ctx.device}")


def _upload(ctx, data):
    """Host bytes -> a device tensor, through the context (dsx_copy)."""
    t = _device_bytes(ctx, len(data))
    if data:
        buf = np.frombuffer(data, dtype=np.uint8)
        _lib.check(lib().dsx_copy(ctx.h, ctypes.c_void_p(t.data_ptr()), buf.ctypes.data, len(data)), ctx.h)
    return t


def _download(ctx, ptr, n):
    out = np.empty(int(n), dtype=np.uint8)
    if n:
        _lib.check(lib().dsx_copy(ctx.h, out.ctypes.data, ctypes.c_void_p(int(ptr)), int(n)), ctx.h)
    return out


def aead_seal(key, src, src_len, ends, start=0, n=None, nonces=None, ctx=None, out=None,
              algo=_lib.DSX_AEAD_XCHACHA20_POLY1305):
    """dsx_aead_seal: seals the chunks [start, ends[0]), [ends[0], ends[1]), ... of
    the device memory ``src`` (a pointer) under ``key``.  ``ends`` is a host array,
    or a device tensor of uint64 / an integer device pointer with ``n``
    (DSX_ENDS_DEVICE).  ``nonces``: n * 24 bytes, or None for fresh random ones.
    ``out``: a ``(pointer, capacity[, owner])`` tuple, or None with host ends: a
    new device tensor of exactly the records' size.
    Returns (the record buffer -- the new tensor, the owner or the pointer --
    and the record ends as np.uint64)."""
    ctx = ctx or _lib.default_context(0)
    validateKey(key)
    flags = 0
    if isinstance(ends, int):
        if n is None:
            raise ValueError("a device pointer needs n, the number of chunks")
        eptr, keep, n = ends, None, int(n)
        flags |= DSX_ENDS_DEVICE
    elif hasattr(ends, "data_ptr"):
        n = ends.numel() if n is None else int(n)
        eptr, keep = ends.data_ptr(), ends
        flags |= DSX_ENDS_DEVICE
    else:
        keep = np.ascontiguousarray(ends, dtype=np.uint64)
        n = keep.size if n is None else int(n)
        eptr = keep.ctypes.data
    if nonces is not None:
        nonces = bytes(nonces)
        if len(nonces) != DSX_AEAD_NONCE * n:
            raise ValueError(f"{n} chunks need {DSX_AEAD_NONCE * n} nonce bytes, got {len(nonces)}")
    if out is None:
        if flags & DSX_ENDS_DEVICE:
            raise ValueError("device ends need out=(pointer, capacity)")
        total = int(keep[-1]) - int(start) if n else 0
        buf = _device_bytes(ctx, total + DSX_AEAD_OVERHEAD * n)
        optr, ocap = buf.data_ptr(), total + DSX_AEAD_OVERHEAD * n
    else:
        buf = out[2] if len(out) > 2 else None
        optr, ocap = int(out[0]), int(out[1])
    rec_ends = np.empty(n, dtype=np.uint64)
    _check(lib().dsx_aead_seal(ctx.h, int(algo), bytes(key), ctypes.c_void_p(int(src)), int(src_len),
                               ctypes.c_void_p(eptr), int(start), n, nonces, ctypes.c_void_p(optr),
                               ocap, rec_ends.ctypes.data, flags), ctx)
    return (buf if buf is not None else optr), rec_ends


def aead_open(key, rec, rec_len, rec_ends, start=0, ctx=None, algo=_lib.DSX_AEAD_XCHACHA20_POLY1305):
    """dsx_aead_open: opens the records [start, rec_ends[0]), ... of the device
    memory ``rec`` (a pointer).  Returns (the plaintext buffer, a device tensor;
    the plaintext ends as np.uint64; the ascending numbers of the bad records).
    The plaintext of a bad record is zero-filled."""
    ctx = ctx or _lib.default_context(0)
    validateKey(key)
    rec_ends = np.ascontiguousarray(rec_ends, dtype=np.uint64)
    n = rec_ends.size
    sizes = np.diff(np.concatenate([[np.uint64(start)], rec_ends]).astype(np.int64)) if n else np.zeros(0, np.int64)
    total = int(np.maximum(sizes - DSX_AEAD_OVERHEAD, 0).sum()) if n else 0
    buf = _device_bytes(ctx, total)
    out_ends = np.empty(n, dtype=np.uint64)
    bad = np.empty(max(1, n), dtype=np.uint32)
    n_bad = ctypes.c_uint64()
    _check(lib().dsx_aead_open(ctx.h, int(algo), bytes(key), ctypes.c_void_p(int(rec)), int(rec_len),
                               rec_ends.ctypes.data, int(start), n, ctypes.c_void_p(buf.data_ptr()),
                               total, out_ends.ctypes.data, bad.ctypes.data, n, ctypes.byref(n_bad), 0),
           ctx)
    return buf, out_ends, bad[:n_bad.value].tolist()


class AEADConverter:
    """aeadConverter (encrypt.go:24-113): seals a chunk with a fresh random nonce
    and prepends it; opens what it sealed."""

    def __init__(self, algorithm, key, ctx=None):
        self.algorithm = algorithm
        self.key = bytes(key)
        # the leading 4 bytes of SHA-256(key): chunks under different keys can
        # share a store (encrypt.go:65-72)
        self.extension = f".{algorithm}-{hashlib.sha256(self.key).digest()[:4].hex()}"
        self._ctx = ctx

    @property
    def ctx(self):
        return self._ctx or _lib.default_context(0)

    def toStorage(self, data, nonce=None) -> bytes:
        data = bytes(data)
        ctx = self.ctx
        src = _upload(ctx, data)
        out, ends = aead_seal(self.key, src.data_ptr(), len(data), [len(data)], 0, nonces=nonce, ctx=ctx)
        return _download(ctx, out.data_ptr(), int(ends[0])).tobytes()

    def fromStorage(self, data) -> bytes:
        data = bytes(data)
        if len(data) < DSX_AEAD_NONCE:
            raise ValueError(ERR_NO_NONCE)
        ctx = self.ctx
        rec = _upload(ctx, data)
        out, ends, bad = aead_open(self.key, rec.data_ptr(), len(data), [len(data)], 0, ctx=ctx)
        if bad:
            raise AuthenticationError()
        return _download(ctx, out.data_ptr(), int(ends[0])).tobytes()

    def equal(self, other) -> bool:
        return isinstance(other, AEADConverter) and self.algorithm == other.algorithm and self.key == other.key

    def storageExtension(self) -> str:
        return self.extension


def NewXChaCha20Poly1305(key, ctx=None) -> AEADConverter:
    """encrypt.go:35-46."""
    validateKey(key)
    return AEADConverter("xchacha20-poly1305", key, ctx)


def NewAES256GCM(key):
    """encrypt.go:48-63.  Validates the key as the reference does, then refuses:
    the AES-256-GCM converter is not built."""
    validateKey(key)
    raise NotImplementedError(
        "the aes-256-gcm converter is not built: GHASH needs a carry-less multiplication, "
        "which gfx950 has no instruction for; use xchacha20-poly1305 (the default)")


class Compressor:
    """converter.go:85-108.  Only its extension and ``equal``: zstd is not
    available here, so data cannot pass through it."""

    def toStorage(self, data):
        raise NotImplementedError("zstd is not available: a compressed store cannot be written")

    def fromStorage(self, data):
        raise NotImplementedError("zstd is not available: a compressed store cannot be read")

    def equal(self, other) -> bool:
        return isinstance(other, Compressor)

    def storageExtension(self) -> str:
        return ".cacnk"


class Converters(tuple):
    """converter.go:11-63: the layers between a chunk and its storage form, applied
    in order towards storage and backwards from it."""

    def __new__(cls, layers=()):
        return super().__new__(cls, layers)

    def toStorage(self, data):
        for layer in self:
            data = layer.toStorage(data)
        return data

    def fromStorage(self, data):
        for layer in reversed(self):
            data = layer.fromStorage(data)
        return data

    def commonPrefix(self, other) -> int:
        n = 0
        while n < len(self) and n < len(other) and self[n].equal(other[n]):
            n += 1
        return n

    def storageExtension(self) -> str:
        return "".join(layer.storageExtension() for layer in self)


@dataclass
class StoreOptions:
    """The converter settings of store.go:55-107."""

    Uncompressed: bool = False
    Encryption: bool = False
    EncryptionAlgorithm: str = ""
    EncryptionKey: str = ""

    def EncryptionConfigured(self) -> bool:
        return bool(self.Encryption or self.EncryptionKey != "" or self.EncryptionAlgorithm != "")

    def StorageConverters(self) -> Converters:
        """store.go:130-164, the checks in the reference's order with its messages."""
        c = []
        if not self.Uncompressed:
            c.append(Compressor())
        if not self.Encryption and self.EncryptionConfigured():
            raise ValueError("encryption-key or encryption-algorithm configured without setting "
                             "encryption to true")
        if self.Encryption:
            if self.EncryptionKey == "":
                raise ValueError("no encryption key configured")
            try:
                key = binascii.unhexlify(self.EncryptionKey)
            except (binascii.Error, ValueError) as e:
                raise ValueError(f"invalid encryption key, expected hex-encoded 256-bit key: {e}") from None
            if self.EncryptionAlgorithm in ("", "xchacha20-poly1305"):
                new = NewXChaCha20Poly1305
            elif self.EncryptionAlgorithm == "aes-256-gcm":
                new = NewAES256GCM
            else:
                raise ValueError(f'unsupported encryption algorithm "{self.EncryptionAlgorithm}"')
            c.append(new(key))
        return Converters(c)


__all__ = ["EncryptionKeySize", "NewXChaCha20Poly1305", "NewAES256GCM", "AEADConverter", "Compressor",
           "Converters", "StoreOptions", "AuthenticationError", "aead_seal", "aead_open"]
