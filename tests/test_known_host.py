"""dsx_chunk_ids_known without a GPU: the ABI, the NULL-context refusal, the
package names, and the arithmetic of its kernels.

The fingerprint windows and the compare's tiles are pure functions in
desync_amd/csrc/dsx_known_geom.h; tests/known_model.cpp is a stand-alone host
program over them, built here with the host sanitizers (it is a program of its
own: nothing is loaded into python).

The second half checks the test devices themselves: the blobs, the mask
patterns and the marked stores test_gpu_known_paths.py runs (known_ref.py), and
the model's lookup by bytes and then by ID against a brute-force restatement.
"""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import known_ref
from desync_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "dsx.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_symbol_is_exported_bound_and_declared():
    assert "dsx_chunk_ids_known" in _lib.EXPORTS
    L = _lib.lib()
    f = L.dsx_chunk_ids_known
    assert f.restype is ctypes.c_int and len(f.argtypes) == 12
    txt = _header()
    assert re.search(r"\bint\s+dsx_chunk_ids_known\s*\(\s*dsx_ctx_t\s*\*\s*ctx\s*,\s*const\s+dsx_store_t\s*\*", txt)
    assert L.dsx_abi_version() == 5
    # the header cites what the call replaces
    raw = open(HDR).read()
    doc = raw[raw.index("chunk IDs by comparison"):raw.index("int dsx_chunk_ids_known(")]
    for cite in ("make.go:223", "chunkstorage.go:44-67", "dsx_chunk_ids", "dsx_store_locate",
                 "dsx_store_verify"):
        assert cite in doc, cite


def test_totals_struct_matches_the_header():
    assert ctypes.sizeof(_lib.KnownTotals) == 80
    names = [n for n, _ in _lib.KnownTotals._fields_]
    assert names == ["chunks", "recognised", "recognised_bytes", "hashed", "hashed_bytes", "pairs",
                     "compared_bytes", "fp_false", "untried", "reserved"]
    txt = open(HDR).read()
    body = txt[txt.index("typedef struct dsx_known_totals"):txt.index("} dsx_known_totals_t")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == names


def test_constants_match_the_header_and_the_geometry():
    txt = _header()
    geom = open(os.path.join(REPO, "desync_amd", "csrc", "dsx_known_geom.h")).read()
    for name, const, value in (("DSX_KNOWN_TILE", "kTile", _lib.DSX_KNOWN_TILE),
                               ("DSX_KNOWN_TRIES", "kTries", _lib.DSX_KNOWN_TRIES),
                               ("DSX_KNOWN_PROBES", "kProbes", _lib.DSX_KNOWN_PROBES)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, txt).group(1)) == value
        assert int(re.search(r"\b%s\s*=\s*(\d+)\s*;" % const, geom).group(1)) == value
    assert _lib.DSX_OFF_NONE == known_ref.OFF_NONE == 2 ** 64 - 1


def test_null_context_is_refused_before_hip():
    """Without a GPU any HIP call would fail with another code."""
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the context is NULL
    ends = (ctypes.c_uint64 * 2)(5, 9)
    ids = (ctypes.c_uint8 * 64)()
    tot = _lib.KnownTotals()
    rc = L.dsx_chunk_ids_known(None, fake, fake, 9, 0, ends, 2, 0, ids, None, ctypes.byref(tot), 0)
    assert rc == _lib.DSX_E_INVAL
    assert L.dsx_chunk_ids_known(None, None, None, 0, 0, None, 0, 0, None, None, None, 0) == _lib.DSX_E_INVAL


def test_package_names():
    import inspect

    import desync_amd
    assert "chunk_ids_known" in desync_amd.__all__
    assert desync_amd.chunk_ids_known is desync_amd.store.chunk_ids_known
    assert callable(desync_amd.DeviceStore.chunk_ids)
    # the opt-in keywords are off by default
    assert inspect.signature(desync_amd.IndexFromBlobs).parameters["known"].default is None
    assert inspect.signature(desync_amd.ChopBlobs).parameters["known"].default is False
    assert inspect.signature(desync_amd.ChopBlob).parameters["known"].default is False


def test_model_windows():
    for size in list(range(0, 301)) + [65535, 65536, 65537, 131089]:
        w = known_ref.known_windows(size)
        assert sum(n for _, n in w) <= 96
        assert all(0 <= o and o + n <= size for o, n in w)
        assert len(w) == (3 if size >= 96 else 2)
    assert known_ref.known_windows(4096) == [(0, 32), (4064, 32), (2032, 32)]
    assert not known_ref.in_windows(4096, 40) and known_ref.in_windows(4096, 2040)


def _compiler():
    for name in ("g++", "c++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    path = "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(path), "no host C++ compiler"
    return path


def test_known_model(tmp_path):
    """For every size 0-300 and around 1x, 2x and 3x the tile the fingerprint's
    windows lie inside the chunk and total at most 96 bytes (the sanitizer
    watches a buffer of exactly the chunk's size), a flip changes the
    fingerprint exactly inside a window, and for random pair lists the
    compare's tiles partition the pair bytes exactly (tests/known_model.cpp)."""
    cxx = _compiler()
    exe = str(tmp_path / "known_model")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(REPO, "desync_amd", "csrc"),
           os.path.join(REPO, "tests", "known_model.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "known model ok: 364 sizes, 304 pair lists", r.stdout[-1000:]


# ---- the marked store and the fixtures of test_gpu_known_paths.py ---------------------------
SMALL_N = (1500, 2500)


@pytest.mark.parametrize("n", SMALL_N)
def test_path_blob(n):
    blob = known_ref.small_blob(n)
    chunks = list(known_ref.chunks_of(blob.raw, blob.ends))
    assert len(chunks) == n == len(set(chunks))  # all distinct ...
    assert len({c[:8] for c in chunks}) == n     # ... already at the number in front
    assert all(c[:8] == i.to_bytes(8, "little") for i, c in enumerate(chunks))
    assert [len(c) for c in chunks] == blob.sizes
    for need in (8, 55, 56, 63, 64, 111, 112, 119, 120, 127, 128, 129, 4096, 4097):
        assert need in known_ref.PAD_SIZES
    assert set(known_ref.PAD_SIZES) <= set(blob.sizes) and blob.sizes.count(70000) == 1
    assert all(z == 8 + i % 57 for i, z in enumerate(blob.sizes) if i % 4 == 3)
    assert 400 << 10 < len(blob.raw) < 1 << 20  # about a MiB
    for algo, name in ((0, "sha512_256"), (1, "sha256")):
        h = blob.hashes(algo)
        assert h.shape == (n, 32) and not h.flags.writeable
        for i in (0, 1, known_ref.BIG_AT, n - 1):
            assert h[i].tobytes() == hashlib.new(name, chunks[i]).digest()
    assert blob.hashes(0) is blob.hashes("sha512-256") and not np.array_equal(blob.hashes(0), blob.hashes(1))


PLANNED = {"every-second": lambda n: n // 2, "first-1024": lambda n: n - 1024, "last-hashed": lambda n: 1,
           "first-hashed": lambda n: 1, "lone-63": lambda n: 1, "lone-64": lambda n: 1, "lone-65": lambda n: 1,
           "run-64": lambda n: n - 64, "none": lambda n: n}


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("pattern", sorted(known_ref.PATTERNS))
@pytest.mark.parametrize("n", SMALL_N)
def test_marked_store(n, pattern, algo):
    """The builder's claims: the planned counts, every padding length among the
    hashed chunks, markers that are no hashes, and a path-exact answer."""
    blob = known_ref.small_blob(n)
    ms = known_ref.MarkedStore(blob, known_ref.PATTERNS[pattern](n), algo)
    assert set(PLANNED) == set(known_ref.PATTERNS)
    assert len(ms.hashed) == PLANNED[pattern](n) and len(ms.recognised) == n - len(ms.hashed)
    assert sorted(ms.hashed.tolist() + ms.recognised.tolist()) == list(range(n))
    if len(ms.hashed) >= 100:
        assert {blob.sizes[i] for i in ms.hashed} >= set(known_ref.PAD_SIZES)
    else:
        assert len(ms.hashed) == 1
    assert {"lone-63": [63], "lone-64": [64], "lone-65": [65], "last-hashed": [n - 1],
            "first-hashed": [0]}.get(pattern, ms.hashed.tolist()) == ms.hashed.tolist()
    if pattern == "first-1024":
        # the grid is sized by the hashed chunks: at 1,500 every static lane starts on an
        # untaken chunk, at 2,500 the first 1,024 of 1,536 do
        lanes = 256 * -(-len(ms.hashed) // 256)
        assert ms.hashed.min() == 1024 and (lanes <= 1024) == (n == 1500) and lanes <= 1536
    assert len(ms.lied) == min(3, len(ms.hashed)) and set(ms.lied) <= set(ms.hashed.tolist())
    # no marker is a hash, of either digest, of a chunk or of an entry
    hashes = {r.tobytes() for a in (0, 1) for r in blob.hashes(a)}
    hashes |= {known_ref.digest(c, a) for a in (0, 1) for c in known_ref.chunks_of(ms.raw, ms.ends)}
    markers = {known_ref.marker(i) for i in range(n + 3000)} | {known_ref.marker(1 << 40)}
    assert len(markers) == n + 3001 and not markers & hashes
    stored = [r.tobytes() for r in ms.ids]
    assert sum(i in markers for i in stored) == len(stored) - len(ms.lied)
    assert len(stored) == 1 + len(ms.recognised) + known_ref.N_OTHERS + len(ms.lied)
    # the liars: the hash of a hashed chunk over other bytes of another size
    ends = [0] + ms.ends.tolist()
    for x in ms.lied:
        e = stored.index(blob.hashes(algo)[x].tobytes())
        assert ends[e + 1] - ends[e] == blob.sizes[x] + 1
    ids, off = ms.want()
    for i in ms.recognised[:50]:
        e = stored.index(known_ref.marker(int(i)))
        assert ids[i].tobytes() == stored[e] and off[i] == ends[e]
        assert ms.raw[ends[e]:ends[e + 1]] == blob.chunk(i)
    for i in ms.hashed[:50]:
        assert ids[i].tobytes() == known_ref.digest(blob.chunk(i), algo)
        assert (off[i] != known_ref.OFF_NONE) == (int(i) in ms.lied)
    assert ends[1] == 13  # the junk entry: no recognised chunk at offset 0


def test_big_plan():
    """The plan of test_big at 256 CUs, on a tenth of the chunks."""
    lanes = 256 * 4 * 256
    n = -(-(lanes + 16384) * 8 // 7) + 8
    assert 318000 < n < 321000 and n // 8 <= len(range(3, n, 8)) <= n // 8 + 1
    assert n - len(range(3, n, 8)) >= lanes + 16384 > 256 * 64 * 2
    assert 11_000_000 < sum(known_ref.tiny_sizes(n)) < 13_000_000  # about 12 MB
    m = n // 10
    ms = known_ref.MarkedStore(known_ref.tiny_blob(m), range(3, m, 8), 1, check_sizes=False)
    ids, off = ms.want()
    assert ids.shape == (m, 32) and int((off != known_ref.OFF_NONE).sum()) == len(range(3, m, 8)) + 3


def brute_force(entries, chunks, algo):
    """The model restated: a linear scan over the entries comparing bytes,
    then one comparing IDs."""
    ids, offs, rec = [], [], 0
    for c in chunks:
        for i, data, _ in entries:
            if data == c:
                rec += 1
                break
        else:
            i = hashlib.new(algo, c).digest()
        ids.append(i)
        for j, _, o in entries:
            if j == i:
                offs.append(o)
                break
        else:
            offs.append(known_ref.OFF_NONE)
    return ids, offs, rec


def test_model_against_brute_force():
    """200 random small cases: honest, marked and lying entries, repeated IDs
    in a put (the first occurrence is stored), chunks the store holds, lacks,
    and holds only by ID; both digests; a start behind a pad."""
    rng = np.random.default_rng(411)
    seen = {"marked": 0, "by_id": 0, "hashed": 0, "repeat": 0}
    for case in range(200):
        algo = known_ref.ALGOS[case % 2]
        alphabet = [rng.integers(0, 4, int(rng.integers(0, 4)), dtype=np.uint8).tobytes() + bytes([k])
                    for k in range(24)] + [b""]
        model, entries, used, held = known_ref.StoreModel(algo), [], 0, {}
        for _ in range(int(rng.integers(0, 3))):  # puts
            picks = rng.integers(0, 18, int(rng.integers(0, 12)))
            data = [alphabet[k] for k in picks]
            ids = []
            for k, c in zip(picks, data):
                r = rng.random()
                if c in held:  # equal bytes keep their ID: a store never holds them under two
                    ids.append(held[c])
                    seen["repeat"] += 1
                elif r < 0.3:
                    ids.append(known_ref.marker(int(k)))
                elif r < 0.45:  # a liar: the hash of a chunk the store will not hold
                    ids.append(hashlib.new(algo, alphabet[18 + int(k) % 6]).digest())
                else:
                    ids.append(hashlib.new(algo, c).digest())
                if ids[-1] in {i for i, _, _ in entries} | set(ids[:-1]) and c not in held:
                    ids[-1] = known_ref.marker(1000 + len(entries) + len(ids))  # (an ID names one entry)
                held.setdefault(c, ids[-1])
                if ids[-1] not in {i for i, _, _ in entries}:
                    entries.append((ids[-1], c, used))
                    used += len(c)
            pad = int(rng.integers(0, 5))
            raw = bytes(pad) + b"".join(data)
            ends = pad + np.cumsum([len(c) for c in data], dtype=np.int64)
            arg = None if all(i == hashlib.new(algo, c).digest() for i, c in zip(ids, data)) else \
                (known_ref.id_rows(ids) if rng.random() < 0.5 else ids)
            model.put(raw, ends, pad, ids=arg)
        assert model.used == used and list(model.off.items()) == [(i, o) for i, _, o in entries]
        chunks = [alphabet[k] for k in rng.integers(0, 25, int(rng.integers(0, 30)))]
        pad = int(rng.integers(0, 5))
        raw = bytes(pad) + b"".join(chunks)
        ends = pad + np.cumsum([len(c) for c in chunks], dtype=np.int64)
        ids, offs, rec = model.answer(raw, ends, pad)
        want_ids, want_offs, want_rec = brute_force(entries, chunks, algo)
        assert [r.tobytes() for r in ids] == want_ids and offs.tolist() == want_offs and rec == want_rec
        assert ids.shape == (len(chunks), 32) and offs.dtype == np.uint64
        markers = {known_ref.marker(k) for k in range(1100)}
        seen["marked"] += sum(i in markers for i in want_ids)
        seen["by_id"] += sum(o != known_ref.OFF_NONE and c not in held for o, c in zip(want_offs, chunks))
        seen["hashed"] += len(chunks) - rec
    assert min(seen.values()) >= 20, seen
