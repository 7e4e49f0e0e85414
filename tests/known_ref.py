"""The model of dsx_chunk_ids_known in hashlib and a dict: the IDs, the offsets
dsx_store_locate gives, how many chunks the store holds, and a restatement of
the fingerprint windows (desync_amd/csrc/dsx_known_geom.h) for planting
collisions."""
import hashlib

import numpy as np

OFF_NONE = 0xFFFFFFFFFFFFFFFF
WINDOW = 32


def digest(data, algo="sha512_256"):
    return hashlib.new(algo, data).digest()


def known_windows(size):
    """-> [(offset, length)]: the bytes of a chunk of `size` bytes its
    fingerprint reads: the first and last min(size, 32) and, from 96 bytes on,
    the 32 at size // 2 - 16."""
    e = min(size, WINDOW)
    w = [(0, e), (size - e, e)]
    if size >= 3 * WINDOW:
        w.append((size // 2 - WINDOW // 2, WINDOW))
    return w


def in_windows(size, pos):
    return any(o <= pos < o + n for o, n in known_windows(size))


def chunks_of(raw, ends, start=0):
    prev = start
    for e in ends:
        yield raw[prev:int(e)]
        prev = int(e)


class StoreModel:
    """A DeviceStore as a dict: ID -> arena offset, appended in put order."""

    def __init__(self, algo="sha512_256"):
        self.algo, self.off, self.used = algo, {}, 0

    def put(self, raw, ends, start=0):
        for c in chunks_of(raw, ends, start):
            i = digest(c, self.algo)
            if i not in self.off:
                self.off[i] = self.used
                self.used += len(c)

    def answer(self, raw, ends, start=0):
        """-> (ids (n, 32) uint8, known_off uint64, recognised): `recognised`
        is the number of chunks whose ID the store holds (what the call reports
        while no fingerprint bucket is oversized)."""
        ids = [digest(c, self.algo) for c in chunks_of(raw, ends, start)]
        offs = np.array([self.off.get(i, OFF_NONE) for i in ids], dtype=np.uint64)
        arr = np.frombuffer(b"".join(ids), dtype=np.uint8).reshape(-1, 32)
        return arr, offs, sum(i in self.off for i in ids)
