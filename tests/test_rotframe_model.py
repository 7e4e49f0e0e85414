"""The rotating frame of scanl_kernel<ROTF> on the CPU.

tests/rotframe_model.cpp is a stand-alone host program over
desync_amd/csrc/dsx_rotframe.h, the header the kernel takes its slot,
rotation and phase-register arithmetic from.  For 64 lanes it runs the
rotating-frame recurrence with the kernel's lookup schedule over a 48-byte
warm-up (random for lanes 0..31, a zero window for lanes 32..63) and
2*384 + 96 random bytes, and compares x at every position with the direct
Buzhash of the last 48 bytes (include/dsx_buzhash_table.h); it also checks
that in each of the 32 phases the 64 lanes read 64 distinct LDS banks and
that the v_perm_b32 selector builds the table offset.  The program's header
gives the -fsanitize=address,undefined command line it is also meant for;
nothing is loaded into python.
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


def test_rotating_frame_matches_direct_buzhash(tmp_path):
    cxx = _compiler()
    exe = str(tmp_path / "rotframe_model")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
            "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "desync_amd", "csrc"),
            os.path.join(REPO, "tests", "rotframe_model.cpp"), "-o", exe]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rotframe model ok: 64 lanes x 864 positions" in r.stdout, r.stdout[-1000:]
