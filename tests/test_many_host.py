"""dsx_cut_device_many without a GPU: the ABI, the refusals and the plan.

The plan (which blobs share a scan launch, which take the one-blob path) is a
pure function in desync_amd/csrc/dsx_many_plan.h; tests/many_plan_model.cpp is
a stand-alone host program over it, built here with the host sanitizers (it is
a program of its own: nothing is loaded into python).
"""
import ctypes
import os
import re
import shutil
import subprocess

from desync_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "dsx.h")


def test_symbol_is_exported_bound_and_declared():
    assert "dsx_cut_device_many" in _lib.EXPORTS
    L = _lib.lib()
    f = L.dsx_cut_device_many
    assert f.restype is ctypes.c_int and len(f.argtypes) == 13
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"\bint\s+dsx_cut_device_many\s*\(", txt)
    assert "dsx_many_opts_t" in txt and "dsx_many_totals_t" in txt
    assert L.dsx_abi_version() == 5


def test_struct_sizes_match_the_header():
    # dsx_many_opts_t: 2 + 2 uint64; dsx_many_totals_t: 8 uint64
    assert ctypes.sizeof(_lib.ManyOpts) == 32
    assert ctypes.sizeof(_lib.ManyTotals) == 64
    assert [n for n, _ in _lib.ManyTotals._fields_] == [
        "blobs", "empty_blobs", "chunks", "groups", "batched_blobs", "single_blobs", "redone_blobs",
        "reserved"]
    txt = open(HDR).read()
    body = txt[txt.index("typedef struct dsx_many_totals"):txt.index("} dsx_many_totals_t")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.ManyTotals._fields_]


def test_refusals_come_before_hip():
    """Every refusal returns DSX_E_INVAL before HIP is touched (without a GPU a
    HIP call would fail with another code); tests/test_gpu_many.py repeats them
    with a context and reads dsx_last_error."""
    import desync_amd
    L = _lib.lib()
    E = _lib.DSX_E_INVAL
    p = desync_amd.Params(2048, 8192, 32768)
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the context is NULL
    n = ctypes.c_uint64()
    ends = (ctypes.c_uint64 * 2)(5, 9)
    dec = (ctypes.c_uint64 * 2)(9, 5)
    opts = _lib.ManyOpts()

    def call(ctx, blob, length, be, nb, pp, n_out, o=None, flags=0):
        return L.dsx_cut_device_many(ctx, blob, length, be, nb, pp, None, 0, n_out, None, o, None,
                                     flags)

    pb, nb_ = ctypes.byref(p.c), ctypes.byref(n)
    assert call(None, fake, 9, ends, 2, pb, nb_) == E          # NULL ctx
    assert call(None, fake, 9, ends, 2, None, nb_) == E        # NULL p
    assert call(None, fake, 9, ends, 2, pb, None) == E         # NULL n_out
    assert call(None, fake, 9, None, 2, pb, nb_) == E          # NULL blob_ends with blobs
    assert call(None, fake, 9, dec, 2, pb, nb_) == E           # decreasing ends
    assert call(None, fake, 10, ends, 2, pb, nb_) == E         # last end != len
    assert call(None, fake, 9, None, 0, pb, nb_) == E          # bytes but no blob
    opts.reserved[1] = 1
    assert call(None, fake, 9, ends, 2, pb, nb_, ctypes.byref(opts)) == E
    opts = _lib.ManyOpts(0, (8 << 30) + 1)
    assert call(None, fake, 9, ends, 2, pb, nb_, ctypes.byref(opts)) == E
    assert call(None, fake, 9, ends, 2, pb, nb_, None, _lib.DSX_NO_SYNC | _lib.DSX_OUT_DEVICE) == E
    assert call(None, None, 0, None, 0, pb, nb_) == E          # (the empty call needs a context too)


def _compiler():
    for name in ("g++", "c++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    path = "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(path), "no host C++ compiler"
    return path


def test_plan_model(tmp_path):
    """Items tile the blob list in order, no group exceeds group_bytes, every
    blob >= big_blob is single, a blob over group_bytes is single, empty blobs
    cost nothing, and the plan is right for 0 blobs, 1 blob and empty blobs
    only (tests/many_plan_model.cpp)."""
    cxx = _compiler()
    exe = str(tmp_path / "many_plan_model")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(REPO, "desync_amd", "csrc"),
           os.path.join(REPO, "tests", "many_plan_model.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "many plan model ok: 400 sweep plans", r.stdout[-1000:]
