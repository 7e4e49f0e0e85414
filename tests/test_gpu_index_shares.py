"""The one-window share schedule of IndexFromFile on the GPU: every chunk ID
is hashed exactly once by the GPU's shares, the tail feeder or the digest
after the read (dsx_index_plan.h index_schedule), at the geometries where the
three once disagreed.

Until round 7 a planned share that no scan point below the end of the file
could fire had already given the feeder its cut, while the digest after the
read used the cut after the last share: the last segment's chunks with a
length between the two got no ID, and dsx_index_fd / dsx_index_host returned
whatever the context's ID buffer held, with return code 0.  That needs a read
slot large against the file (DSX_INDEX_SLOT, a product setting); every other
test runs the default 32 MiB slot.

Stale IDs are made wrong, not accidentally right: before every call whose
IDs are checked, the same entry point runs on the same context over a blob
of the same length from another generator seed (84, no other test's), so an
ID the checked call does not write is the primer's.

Product library: 352 MiB + 4321 B at 28 feeder threads (two planned shares,
at ~176 MiB with cut 90112 and ~264 MiB with cut 45056; the cut after them
28672) through a 288 MiB slot (the second share cannot fire: chunks after
288 MiB with a length in (28672, 45056] went unhashed), a slot above the file
(88 MiB pieces and one of 4321 B: the second share fires at 352 MiB, 4321 B
before the end) and the default slot.

Diagnostic library (one child process, DSX_LIB_PATH): the same shapes at
80 MiB, the read-time model shrunk with DSX_SHARE_NS=10, DSX_SHARE_SLACK,
DSX_FEED_MID, DSX_FINE_TAIL=0 and DSX_FEED_THREADS=28.

stats.host_tail_chunks must equal the count the schedule's per-segment cuts
give on the reference chain, for dsx_index_fd and dsx_index_host; in the
diagnostic child also for dsx_ids_fd and dsx_ids_host, under run_ids's own
schedule (ids_schedule) at this process's measured SHA rate
(dsx_diag_host_ns_per_byte), which its last cut is planned from.
"""
import concurrent.futures as cf
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import index_sched as S  # noqa: E402
from oracle import oracle as o  # noqa: E402

pytestmark = pytest.mark.gpu

MIN, AVG, MAX = 16 * 1024, 64 * 1024, 256 * 1024
MiB = 1 << 20
SEED, PRIMER_SEED = 81, 84
N = (352 << 20) + 4321
THREADS = 28  # feeder threads: DSX_HOST_THREADS=32 less the 4 readers; DSX_FEED_THREADS in the child


def _avx512():
    flags = open("/proc/cpuinfo").read()
    return "avx512f" in flags and "avx512bw" in flags


def _reference(data):
    """(ends, IDs) of the reference chain: oracle.chunk_parallel, hashlib."""
    ref = o.chunk_parallel(data, MIN, AVG, MAX, o.default_threads())
    starts = np.concatenate([[0], ref[:-1]]).astype(np.uint64)
    mv = memoryview(data)

    def h(i):
        return hashlib.new("sha512_256", mv[int(starts[i]):int(ref[i])]).digest()

    with cf.ThreadPoolExecutor(o.default_threads()) as pool:
        want = list(pool.map(h, range(ref.size), chunksize=256))
    return ref, want


def _first_mismatch(got, want, ref):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"first wrong ID at chunk {i}, length {int(ref[i]) - (int(ref[i - 1]) if i else 0)}"
    return None


def _check_four(ctx, data, path, primer, primer_path, ref, want, sched, algo="sha512-256", log=None,
                ids_want=None):
    """dsx_index_fd, dsx_index_host, dsx_ids_fd and dsx_ids_host on `ctx`,
    each after the same entry point over the primer: the cut list is the
    reference's, every ID hashlib's, and (sched given) the host hashed exactly
    the chunks above their segment's cut; (ids_want given) dsx_ids_* had the
    host hash exactly that many chunks."""
    import desync_amd
    n_want = None if sched is None else S.host_chunks(sched, ref)
    if sched is not None:
        assert n_want is not None, "a reference chunk ends on a segment boundary: pick another seed"

    def on_fd(p, fn):
        fd = os.open(p, os.O_RDONLY)
        try:
            return fn(fd)
        finally:
            os.close(fd)

    def check_ids(name, ids):
        got = [bytes(x) for x in ids]
        assert len(got) == len(want), (name, len(got), len(want))
        assert got == want, f"{name}: {_first_mismatch(got, want, ref)}"

    for name, prime, call in (
            ("index_fd", lambda: on_fd(primer_path, lambda fd: desync_amd.index_fd(fd, MIN, AVG, MAX, algo=algo, ctx=ctx)),
             lambda: on_fd(path, lambda fd: desync_amd.index_fd(fd, MIN, AVG, MAX, algo=algo, ctx=ctx))),
            ("index_host", lambda: desync_amd.index_host(primer, MIN, AVG, MAX, algo=algo, ctx=ctx),
             lambda: desync_amd.index_host(data, MIN, AVG, MAX, algo=algo, ctx=ctx))):
        # (the primer's own chain may have fewer chunks than the reference's:
        # its IDs over the reference's list first, so that every index of the
        # context's ID buffer holds a primer ID before the checked call)
        desync_amd.ids_host(primer, 0, ref, algo=algo, ctx=ctx)
        prime()
        t0 = time.perf_counter()
        ends, ids = call()
        dt = time.perf_counter() - t0
        n_host = ctx.stats().host_tail_chunks
        if log is not None:
            log.append(f"{name} {dt * 1e3:.0f} ms host {n_host} (want {n_want})")
        assert np.array_equal(ends, ref), name
        check_ids(name, ids)
        if n_want is not None:
            assert n_host == n_want, (name, n_host, n_want)
    # VerifyIndex's IDs of the same list; the primer run over the same list
    # (any contiguous list within the blob is one), so it writes every index
    for name, prime, call in (
            ("ids_fd", lambda: on_fd(primer_path, lambda fd: desync_amd.ids_fd(fd, 0, ref, algo=algo, ctx=ctx)),
             lambda: on_fd(path, lambda fd: desync_amd.ids_fd(fd, 0, ref, algo=algo, ctx=ctx))),
            ("ids_host", lambda: desync_amd.ids_host(primer, 0, ref, algo=algo, ctx=ctx),
             lambda: desync_amd.ids_host(data, 0, ref, algo=algo, ctx=ctx))):
        prime()
        check_ids(name, call())
        n_host = ctx.stats().host_tail_chunks
        if log is not None:
            log.append(f"{name} host {n_host} (want {ids_want})")
        if ids_want is not None:
            assert n_host == ids_want, (name, n_host, ids_want)


# ------------------------------------------------------------ product library
@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    """The 352 MiB + 4321 B blob and its primer, in memory and on disk, with
    the reference chain and IDs (computed once for the three cases)."""
    d = tmp_path_factory.mktemp("shares")
    out = {}
    for key, seed in (("data", SEED), ("primer", PRIMER_SEED)):
        blob = o.synth_uniform_c(seed, 0, N)
        path = str(d / key)
        blob.tofile(path)
        out[key], out[key + "_path"] = blob, path
    out["ref"], out["want"] = _reference(out["data"])
    yield out
    for key in ("data_path", "primer_path"):
        os.unlink(out[key])


# slot -> (the scan points the shares fire at, 0: dropped; the last scan point below len)
_PRODUCT = {
    "slot-288MiB": (288 << 20, [288 * MiB, 0], 288 * MiB),
    "slot-1GiB": (1 << 30, [264 * MiB, 352 * MiB], 352 * MiB),
    "default-slot": (None, [192 * MiB, 288 * MiB], 352 * MiB),
}


@pytest.mark.parametrize("case", list(_PRODUCT))
def test_index_shares_large_slot(traced, monkeypatch, case):
    """The issue's traced geometries on the product library (the module's
    docstring).  A large slot pins 8 x min(slot, file) of host memory for the
    life of the context (2.25 GiB at 288 MiB, 2.75 GiB above the file), so
    the context is closed in `finally`."""
    from desync_amd import _lib
    slot, fires, last_scan = _PRODUCT[case]
    monkeypatch.setenv("DSX_HOST_THREADS", "32")
    if slot:
        monkeypatch.setenv("DSX_INDEX_SLOT", str(slot))
    else:
        monkeypatch.delenv("DSX_INDEX_SLOT", raising=False)
    # the shape this case is for, from the diagnostic library's exports (it
    # reads none of the settings above; the product constants are its defaults)
    sched = None
    lib = S.diag_lib()
    if lib is not None:
        import ctypes
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        at, cut = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)()
        n = lib.dsx_diag_index_plan(N, MAX, THREADS, ctypes.byref(a), ctypes.byref(b), at, cut, 8)
        assert (n, a.value, b.value, list(cut[:n])) == (2, 28672, 28672, [90112, 45056])
        ends = [x + y for x, y in S.pieces(lib, N, slot or 32 << 20, 1 << 30)]
        sched = S.schedule(lib, N, slot or 32 << 20, 1 << 30, THREADS)
        below = [x for x in sched["scan"] if x < N]
        assert set(sched["scan"]) <= set(ends) and below[-1] == last_scan
        # slot-288MiB: both shares are due by the one scan point below len,
        # which the first takes: none is left for the second
        if case == "slot-288MiB":
            assert below == [last_scan] and at[0] < at[1] <= last_scan
        assert [f for _, _, f in sched["shares"]] == fires
        assert S.violations(sched, N) == []
    ctx = _lib.Context(0)
    try:
        _check_four(ctx, traced["data"], traced["data_path"], traced["primer"], traced["primer_path"],
                    traced["ref"], traced["want"], sched if _avx512() else None)
    finally:
        ctx.close()


# ------------------------------------------------- diagnostic library, 80 MiB
_DIAG_BASE = {"DSX_SHARE_NS": "10", "DSX_FEED_THREADS": "28", "DSX_FINE_TAIL": "0"}
_N80, _N80X, _N160 = 80 * MiB + 4321, 80 * MiB + 8193, 160 * MiB + 4321
# name -> (settings, length, DSX_INDEX_SLOT, DSX_INDEX_WINDOW, algo,
#          the planned shares' scan points (0: dropped), the segments' feeder cuts)
_DIAG = {
    # shares due at 40 and 60 MiB, scan points 64 MiB and len
    "two-due-at-one-point": (_DIAG_BASE, _N80, 64 * MiB, None, "sha512-256", [64 * MiB, 0], [90112, 28672]),
    # at 40, 60 and 70 MiB, scan points 72 MiB and len
    "three-due-at-one-point": (dict(_DIAG_BASE, DSX_SHARE_SLACK="300"), _N80, 72 * MiB, None, "sha512-256",
                               [72 * MiB, 0, 0], [122880, 28672]),
    # scan points 48 MiB and len: the share at 60 MiB is due after the last one below len
    "due-after-last-point": (_DIAG_BASE, _N80, 48 * MiB, None, "sha512-256", [48 * MiB, 0], [90112, 28672]),
    # 1/2 of 80 MiB + 8193 B is the slot: due exactly at a scan point; the
    # second fires at twice that, one byte before the end
    "due-exactly-at-a-point": (dict(_DIAG_BASE, DSX_FEED_MID="0.5,0.75"), _N80X, 40 * MiB + 4096, None,
                               "sha512-256", [40 * MiB + 4096, 80 * MiB + 8192], [90112, 45056, 28672]),
    # the first cut is max: the GPU takes the first segment whole
    "first-cut-is-max": ({"DSX_SHARE_NS": "10", "DSX_FEED_THREADS": "28", "DSX_SHARE_SLACK": "2000",
                          "DSX_FEED_MID": "0.5,0.75"}, _N80, None, None, "sha512-256",
                         [48 * MiB, 64 * MiB], [262144, 245760, 28672]),
    # two windows of 96 MiB (80 MiB rounded up to the 48 MiB slot), the shares
    # in the last, on side streams 1..: side stream 0 has the first window's digest
    "two-windows": (dict(_DIAG_BASE, DSX_SHARE_SLACK="100"), _N160, 48 * MiB, 80 * MiB, "sha512-256",
                    [144 * MiB, 0], [81920, 28672]),
    # SHA-256: no feeder, no shares
    "sha256-control": (_DIAG_BASE, _N80, 64 * MiB, None, "sha256", [], [S.NONE]),
}


@pytest.fixture(scope="module")
def diag_child():
    """All diagnostic cases in one child process on libdsx_diag.so."""
    assert os.path.exists(S.DIAG), "libdsx_diag.so missing: __graft_entry__.build() makes it"
    env = {k: v for k, v in os.environ.items() if not k.startswith("DSX_")}
    env.update(DSX_LIB_PATH=S.DIAG, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__)], env=env, capture_output=True,
                       text=True, timeout=300, cwd=REPO)
    return r


@pytest.mark.parametrize("case", list(_DIAG))
def test_index_shares_diag(diag_child, case):
    r = diag_child
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(f"case {case}: ")]
    assert line, f"exit {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-3000:]
    print(line[0])
    assert line[0].startswith(f"case {case}: ok"), line[0]


def _main():
    import tempfile

    from desync_amd import _lib
    assert os.path.basename(_lib.LIB_PATH).startswith("libdsx_diag")
    lib = S.diag_lib()
    avx = _avx512()
    with tempfile.TemporaryDirectory() as d:
        blobs = {}
        for key, seed in (("data", SEED), ("primer", PRIMER_SEED)):
            blobs[key] = o.synth_uniform_c(seed, 0, _N160)
        refs = {}
        for name, (settings, n, slot, window, algo, fires, cuts) in _DIAG.items():
            t0 = time.perf_counter()
            log = []
            try:
                for k in [k for k in os.environ if k.startswith("DSX_") and k != "DSX_LIB_PATH"]:
                    del os.environ[k]
                os.environ.update(settings)
                if slot:
                    os.environ["DSX_INDEX_SLOT"] = str(slot)
                if window:
                    os.environ["DSX_INDEX_WINDOW"] = str(window)
                # the shape, from the schedule export under this environment
                sched = S.schedule(lib, n, slot or 32 << 20, window or 1 << 30, THREADS,
                                   host_tail=-1 if algo == "sha512-256" else 0)
                assert S.violations(sched, n) == [], S.violations(sched, n)
                assert [f for _, _, f in sched["shares"]] == fires, sched["shares"]
                assert [s[2] for s in sched["segs"]] == cuts, sched["segs"]
                if name == "due-exactly-at-a-point":
                    assert sched["shares"][0][0] == sched["shares"][0][2]
                if name == "due-after-last-point":
                    assert sched["shares"][1][0] > [x for x in sched["scan"] if x < n][-1]
                if name == "first-cut-is-max":
                    assert sched["segs"][0][2] >= MAX and sched["segs"][0][3] == 0
                if name == "two-windows":
                    assert sched["last_ws"] == 96 * MiB and sched["side0"] == 1
                if n not in refs:
                    data, primer = blobs["data"][:n], blobs["primer"][:n]
                    paths = [os.path.join(d, f"{k}{n}") for k in ("data", "primer")]
                    data.tofile(paths[0])
                    primer.tofile(paths[1])
                    refs[n] = (data, primer, paths, {})
                data, primer, paths, by_algo = refs[n]
                if algo not in by_algo:
                    ref, want = _reference(data)
                    if algo == "sha256":
                        want = [hashlib.sha256(data[(int(ref[i - 1]) if i else 0):int(ref[i])]).digest()
                                for i in range(ref.size)]
                    by_algo[algo] = (ref, want)
                ref, want = by_algo[algo]
                # run_ids's schedule of the reference list under this
                # environment, at this process's SHA rate (None: a chunk ends
                # exactly where a share lands, or no AVX-512)
                ids_want = None
                if avx or algo == "sha256":
                    isched = S.ids_schedule(lib, 0, ref, slot or 32 << 20, window or 1 << 30, THREADS,
                                            host_tail=-1, tail_on=algo == "sha512-256",
                                            host_ns=lib.dsx_diag_host_ns_per_byte())
                    assert S.ids_violations(isched, 0, ref, THREADS, -1, algo == "sha512-256",
                                            lib.dsx_diag_host_ns_per_byte()) == []
                    ids_want = S.ids_host_chunks(isched, 0, ref)
                ctx = _lib.Context(0)
                try:
                    _check_four(ctx, data, paths[0], primer, paths[1], ref, want,
                                sched if avx or algo == "sha256" else None, algo=algo, log=log,
                                ids_want=ids_want)
                finally:
                    ctx.close()
                print(f"case {name}: ok {time.perf_counter() - t0:.2f} s; " + "; ".join(log), flush=True)
            except AssertionError as e:
                print(f"case {name}: FAILED {str(e)[:600]!r}; " + "; ".join(log), flush=True)
            # (anything else -- a HIP error among them -- ends the child: no
            # further case runs on a context that failed)


if __name__ == "__main__":
    _main()
