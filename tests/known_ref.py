"""The model of dsx_chunk_ids_known in hashlib and a dict: the IDs, the offsets
dsx_store_locate gives, how many chunks the store holds, a restatement of
the fingerprint windows (desync_amd/csrc/dsx_known_geom.h) for planting
collisions, and the fixtures of test_gpu_known_paths.py.

The call's contract for callers is "a store whose IDs are those of its bytes".
The model also takes a *marked* store, whose entries carry IDs that are not the
hashes of their bytes.  That is a test device, not a use of the call:
dsx_store_put trusts its IDs, so a chunk the call recognises by comparison then
carries the entry's marker, a chunk it hashes carries hashlib's digest, and the
two paths can be told apart in ids[].  The model therefore looks a chunk up by
its bytes first (the entry's ID, whatever it is) and, where no entry has its
bytes, by the ID of its hash.  No two entries of a modelled store may hold equal
bytes under different IDs: which of them the call would answer is not
determined."""
import functools
import hashlib
import struct

import numpy as np

OFF_NONE = 0xFFFFFFFFFFFFFFFF
WINDOW = 32
ALGOS = ("sha512_256", "sha256")  # hashlib's names, indexed by DSX_DIGEST_*


def algo_name(algo):
    """hashlib's name of a digest given as a DSX_DIGEST_* code, as the
    package's name ("sha512-256") or as hashlib's."""
    if isinstance(algo, (int, np.integer)):
        return ALGOS[int(algo)]
    name = algo.replace("-", "_")
    assert name in ALGOS, algo
    return name


def digest(data, algo="sha512_256"):
    return hashlib.new(algo_name(algo), data).digest()


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


def id_rows(ids):
    """A list of 32-byte IDs as an (n, 32) uint8 array."""
    return np.frombuffer(b"".join(ids), dtype=np.uint8).reshape(-1, 32)


class StoreModel:
    """A DeviceStore as two dicts, appended in put order: ID -> arena offset
    and bytes -> ID.  An entry's ID is the hash of its bytes under `algo`
    unless the put names another (a marked store, see the module)."""

    def __init__(self, algo="sha512_256"):
        self.algo, self.off, self.by_bytes, self.used = algo_name(algo), {}, {}, 0

    def put(self, raw, ends, start=0, ids=None):
        """dsx_store_put: the first occurrence of an ID is stored.  `ids`: one
        32-byte ID per chunk (rows or byte strings), default their hashes."""
        for k, c in enumerate(chunks_of(raw, ends, start)):
            c = bytes(c)
            i = digest(c, self.algo) if ids is None else bytes(bytearray(ids[k]))
            assert len(i) == 32
            if i not in self.off:
                self.off[i] = self.used
                self.used += len(c)
                assert self.by_bytes.setdefault(c, i) == i, "equal bytes under two IDs"

    def answer(self, raw, ends, start=0):
        """-> (ids (n, 32) uint8, known_off uint64, recognised): by the bytes
        first (the ID of the entry that holds them), then by the hash's ID.
        `recognised` is the number of chunks whose bytes the store holds (what
        the call reports while no fingerprint bucket is oversized); the others
        are hashed."""
        ids, rec = [], 0
        for c in chunks_of(raw, ends, start):
            i = self.by_bytes.get(bytes(c))
            rec += i is not None
            ids.append(digest(c, self.algo) if i is None else i)
        offs = np.array([self.off.get(i, OFF_NONE) for i in ids], dtype=np.uint64)
        return id_rows(ids), offs, rec


# ---- the fixtures of test_gpu_known_paths.py ---------------------------------------------
# Every SHA-2 padding case up to 4,097 bytes (test_gpu_parity._tricky_ends from
# 8 bytes on: a chunk starts with its 8-byte number), the bare number, and one
# byte past a page.
PAD_SIZES = (8, 15, 16, 17, 55, 56, 57, 63, 64, 65, 111, 112, 113, 119, 120, 127, 128, 129, 191, 192,
             255, 256, 257, 1000, 4096, 4097)
BIG_SIZE, BIG_AT = 70000, 777
N_LIARS, N_OTHERS = 3, 32


def marker(i):
    """The ID of chunk number i in a marked store: the hash of nothing."""
    return b"\xEE" * 8 + struct.pack("<Q", i) + b"\x11" * 16


def small_sizes(n):
    """Three chunks of four cycle through PAD_SIZES (3 and the 26 sizes share
    no factor, so every stride of chunk numbers meets every size), the fourth
    is 8 + i % 57, and one chunk is longer than a 64 KiB tile."""
    sizes, p = [], 0
    for i in range(n):
        if i % 4 != 3:
            sizes.append(PAD_SIZES[p % len(PAD_SIZES)])
            p += 1
        else:
            sizes.append(8 + i % 57)
    sizes[BIG_AT] = BIG_SIZE
    return sizes


def tiny_sizes(n):
    return [8 + i % 57 for i in range(n)]


def numbered_bytes(sizes, first, seed):
    """Seeded random chunks of `sizes` (each >= 8), chunk k starting with
    LE64(first + k): all distinct, and distinct at the first fingerprint
    window -> (one bytes object, ends)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert sizes.min() >= 8
    ends = np.cumsum(sizes)
    body = np.random.default_rng(seed).integers(0, 256, int(ends[-1]), dtype=np.uint8)
    at = (ends - sizes)[:, None] + np.arange(8)
    body[at] = (first + np.arange(len(sizes), dtype="<u8")).view(np.uint8).reshape(-1, 8)
    return body.tobytes(), ends.astype(np.uint64)


class PathBlob:
    """The blob of n numbered chunks and hashlib's IDs of them."""

    def __init__(self, n, sizes):
        self.n, self.sizes, self._hashes = n, list(sizes), {}
        self.raw, self.ends = numbered_bytes(self.sizes, 0, [20250611, n])
        self.starts = np.concatenate([[0], self.ends[:-1]]).astype(np.int64)

    def chunk(self, i):
        return self.raw[int(self.starts[i]):int(self.ends[i])]

    def hashes(self, algo):
        """(n, 32): computed once per digest, and not to be written to."""
        name = algo_name(algo)
        if name not in self._hashes:
            self._hashes[name] = id_rows([digest(c, name) for c in chunks_of(self.raw, self.ends)])
        return self._hashes[name]


@functools.lru_cache(maxsize=None)
def small_blob(n):
    return PathBlob(n, small_sizes(n))


@functools.lru_cache(maxsize=None)
def tiny_blob(n):
    return PathBlob(n, tiny_sizes(n))


# name -> the recognised chunk numbers of a blob of n chunks (n > 1,024 + 100)
PATTERNS = {
    "every-second": lambda n: range(0, n, 2),
    "first-1024": lambda n: range(1024),               # every static lane starts on an untaken chunk
    "last-hashed": lambda n: range(n - 1),             # work = 1
    "first-hashed": lambda n: range(1, n),             # work = 1
    "lone-63": lambda n: [i for i in range(n) if i != 63],   # a hashed run of one chunk: the last lane
    "lone-64": lambda n: [i for i in range(n) if i != 64],   # of a wave, the first and the second of
    "lone-65": lambda n: [i for i in range(n) if i != 65],   # the next
    "run-64": lambda n: range(320, 384),               # one whole wave's static share recognised
    "none": lambda n: [],                              # a mask of all ones
}


class MarkedStore:
    """What to put so that exactly the chunks `recognised` of `blob` are
    recognised, and what the call must then answer under `algo`.

    The entries, behind a junk entry of odd length and in a shuffled order:
    the recognised chunks under marker(i); N_OTHERS chunks the blob lacks (the
    sizes of its first chunks, numbered from n + 1,000) under their markers;
    and up to N_LIARS entries that lie the other way: the ID is the true hash
    of a hashed chunk X, the bytes are others, one byte longer.  X is hashed
    and must then be found at that entry's offset."""

    def __init__(self, blob, recognised, algo, check_sizes=True):
        n = blob.n
        self.blob, self.algo = blob, algo_name(algo)
        self.recognised = np.asarray(sorted(recognised), dtype=np.int64)
        mask = np.ones(n, dtype=bool)
        mask[self.recognised] = False
        self.hashed = np.flatnonzero(mask)
        assert len(self.recognised) + len(self.hashed) == n and len(self.hashed) >= 1
        if check_sizes and len(self.hashed) >= 100:  # every padding case is hashed
            got = {blob.sizes[i] for i in self.hashed}
            assert got >= set(PAD_SIZES) and (BIG_SIZE in got or BIG_AT in self.recognised), sorted(got)
        rng = np.random.default_rng([n, len(self.recognised), int(self.recognised.sum())])
        self.lied = [int(x) for x in self.hashed[np.linspace(0, len(self.hashed) - 1,
                                                             min(N_LIARS, len(self.hashed))).astype(np.int64)]]
        self.lied = sorted(set(self.lied))
        other_raw, other_ends = numbered_bytes(blob.sizes[:N_OTHERS], n + 1000, [n, 1])
        liar_raw, liar_ends = numbered_bytes([blob.sizes[x] + 1 for x in self.lied], n + 2000, [n, 2])
        entries = [(marker(1 << 40), rng.integers(0, 256, 13, dtype=np.uint8).tobytes())]
        rest = [(marker(int(i)), blob.chunk(i)) for i in self.recognised]
        rest += [(marker(n + 1000 + k), c) for k, c in enumerate(chunks_of(other_raw, other_ends))]
        rest += [(digest(blob.chunk(x), self.algo), c) for x, c in zip(self.lied, chunks_of(liar_raw, liar_ends))]
        entries += [rest[k] for k in rng.permutation(len(rest))]
        self.ids = id_rows([i for i, _ in entries])
        self.raw = b"".join(c for _, c in entries)
        self.ends = np.cumsum([len(c) for _, c in entries], dtype=np.uint64)
        assert len({i for i, _ in entries}) == len(entries) == len({c for _, c in entries})
        self.model = StoreModel(self.algo)
        self.model.put(self.raw, self.ends, ids=self.ids)
        assert len(self.model.off) == len(entries)

    def want(self):
        """-> (ids, known_off): the model's answer, which must be path-exact:
        a marker and an offset for a recognised chunk, the hash and OFF_NONE
        (or a liar's offset) for a hashed one."""
        ids, off, rec = self.model.answer(self.blob.raw, self.blob.ends)
        assert rec == len(self.recognised)
        r, h = self.recognised, self.hashed
        assert np.array_equal(ids[r], id_rows([marker(int(i)) for i in r]) if len(r) else ids[r])
        assert np.array_equal(ids[h], self.blob.hashes(self.algo)[h])
        assert np.all(off[r] != OFF_NONE) and len(set(off[r].tolist())) == len(r)
        found = off[h] != OFF_NONE
        assert h[found].tolist() == self.lied
        return ids, off
