"""dsx_chunk_ids_known without a GPU: the ABI, the NULL-context refusal, the
package names, and the arithmetic of its kernels.

The fingerprint windows and the compare's tiles are pure functions in
desync_amd/csrc/dsx_known_geom.h; tests/known_model.cpp is a stand-alone host
program over them, built here with the host sanitizers (it is a program of its
own: nothing is loaded into python).
"""
import ctypes
import os
import re
import shutil
import subprocess

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
