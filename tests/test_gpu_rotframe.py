"""scanl_kernel in the rotating frame (DSX_SCAN_ROTF=1) cuts
exactly where the oracle and the parent kernel (DSX_SCAN_ROTF=0) cut.

The cases, each run with both settings in ONE child process (the setting is
read when a context is created):
  u64      64 MiB + 777 B uniform at avg 64 KiB: the one-size instantiation,
           a few regions per wave slot, a partial last lane segment, queue draws
  u16/u256 the same blob at avg 16 KiB (d is even: the rotate form of the rare
           path, which needs the true x and not the rotated g) and 256 KiB
  two      4 GiB - 999 B uniform: the smallest piece of the two-size (TWO)
           instantiation with tail regions (tests/test_gpu_variants.py's shape)
  zeros    32 MiB of zeros: every hash is the same and forced cuts dominate, so
           a frame one position off at a trip, handoff or region border shows
  stream   16 MiB + 4097 B through NewChunker: three pieces (8 MiB batches)
           with carried cuts, min_pos behind the first piece's start and no
           halo at the chain origin
  golden   tests/golden/chunker.input against chunker.index
The library is the one DSX_SCAN_ROTF is registered for in desync_amd/_lib.py
(the product library, or the diagnostic build).
"""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, AVG, MAX = 16 << 10, 64 << 10, 256 << 10
CASES = ("u64", "u16", "u256", "two", "zeros", "stream", "golden")


def _library():
    from desync_amd import _lib
    if "DSX_SCAN_ROTF" in _lib.PRODUCT_ENV:
        return os.path.join(REPO, "desync_amd", "libdsx.so")
    assert "DSX_SCAN_ROTF" in _lib.DIAG_ENV
    return os.path.join(REPO, "desync_amd", "libdsx_diag.so")


def test_rotating_frame_cuts_equal_oracle_and_parent():
    path = _library()
    assert os.path.exists(path), path + " missing: __graft_entry__.build() makes it"
    with open(path, "rb") as f:
        assert b"DSX_SCAN_ROTF" in f.read(), "the library does not read DSX_SCAN_ROTF"
    env = dict(os.environ, DSX_LIB_PATH=path, PYTHONPATH=REPO)
    env.pop("DSX_SCAN_ROTF", None)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for name in CASES:
        assert f"case {name} ok" in r.stdout, r.stdout[-3000:]


def _main():
    import torch

    import desync_amd
    from desync_amd import _lib
    from oracle import oracle as o
    L = _lib.lib()

    ctxs = {}
    for rotf in ("0", "1"):
        os.environ["DSX_SCAN_ROTF"] = rotf
        ctxs[rotf] = _lib.Context(0)
    os.environ.pop("DSX_SCAN_ROTF", None)

    def both(name, run, want):
        got = {k: np.asarray(run(c), dtype=np.uint64) for k, c in ctxs.items()}
        want = np.asarray(want, dtype=np.uint64)
        assert np.array_equal(got["1"], want), f"{name}: the rotating frame differs from the oracle"
        assert np.array_equal(got["0"], got["1"]), f"{name}: the two kernels differ"
        print(f"case {name} ok ({want.size} cuts)", flush=True)

    def device_cuts(t, n, mn, av, mx):
        return lambda c: desync_amd.cut_device(t.data_ptr(), n, mn, av, mx, ctx=c)

    try:
        blob = o.synth_uniform(21, 0, (64 << 20) + 777)
        t = torch.from_numpy(blob.copy()).to("cuda")
        for name, av in (("u64", 64 << 10), ("u16", 16 << 10), ("u256", 256 << 10)):
            mn, mx = av // 4, av * 4
            both(name, device_cuts(t, blob.size, mn, av, mx), o.chunk_stream(blob, mn, av, mx))
        del t

        n = (4 << 30) - 999
        t = torch.empty(n, dtype=torch.uint8, device="cuda")
        _lib.check(L.dsx_gen_uniform(ctxs["0"].h, ctypes.c_void_p(t.data_ptr()), 0, n, 7), ctxs["0"].h)
        torch.cuda.synchronize()
        host = t.cpu().numpy()
        before = {k: c.stats().pieces for k, c in ctxs.items()}
        both("two", device_cuts(t, n, MIN, AVG, MAX),
             o.chunk_parallel(host, MIN, AVG, MAX, o.default_threads()))
        for k, c in ctxs.items():  # (one piece: the two-size region geometry)
            assert c.stats().pieces - before[k] == 1
        del t, host

        z = np.zeros(32 << 20, np.uint8)
        t = torch.from_numpy(z).to("cuda")
        both("zeros", device_cuts(t, z.size, MIN, AVG, MAX), o.chunk_stream(z, MIN, AVG, MAX))
        del t

        s = o.synth_uniform(22, 0, (16 << 20) + 4097)
        sb = s.tobytes()

        def stream(c):
            ch = desync_amd.NewChunker(io.BytesIO(sb), MIN, AVG, MAX, ctx=c)
            return [start + len(b) for start, b in ch]
        both("stream", stream, o.chunk_stream(s, MIN, AVG, MAX))

        with open(os.path.join(REPO, "tests", "golden", "chunker.input"), "rb") as f:
            g = np.frombuffer(f.read(), np.uint8)
        with open(os.path.join(REPO, "tests", "golden", "chunker.index"), "rb") as f:
            want = o.decode_caibx(f.read())["ends"]
        t = torch.from_numpy(g.copy()).to("cuda")
        both("golden", device_cuts(t, g.size, MIN, AVG, MAX), want)
    finally:
        for c in ctxs.values():
            c.close()


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    _main()
