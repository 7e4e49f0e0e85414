"""The scan geometry of a piece on the CPU.

tests/scan_geom_model.cpp is a stand-alone host program over
desync_amd/csrc/dsx_scan_geom.h, the header enqueue_piece (dsx_engine.cpp)
takes every piece's lane segments, regions, list capacity, line-grid origin
and launch grid from.  It compares scan_geom() field by field with a table
recorded for the smallest shapes on each side of every branch (short pieces,
the one-trip / two-trip switch, delta and the 96-B-row kernel, shift0, the
1 GiB and 8 GiB pieces, the two-size threshold, DSX_TAIL_SPLIT, the tuning
overrides, the dense path, the rcap clamp), checks over a seeded sweep the
invariants the kernels and pc_region_base / pc_region_of rely on, and pins the
rule tests/test_gpu_seam_record.py::_geometry restates.  This test builds it
without a sanitizer; the program's header gives the flags of a sanitizer build
by hand.  Nothing is loaded into python.
"""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for name in ("g++", "c++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    path = "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(path), "no host C++ compiler"
    return path


def test_scan_geometry_matches_recorded_table(tmp_path):
    cxx = _compiler()
    exe = str(tmp_path / "scan_geom_model")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
            "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "desync_amd", "csrc"),
            os.path.join(REPO, "tests", "scan_geom_model.cpp"), "-o", exe]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == \
        "scan geometry model ok: 53 rows, 4000 sweep pieces, 2052 rule points", r.stdout[-1000:]
