"""The take mask of dsx_chunk_ids_known (DigestArgs.take) on every digest
path, both digests, against a marked store (known_ref.py): the chunks planned
to be recognised lie in the store under marker IDs that are no hashes, so ids[]
says which path produced each ID.  A recognised chunk must carry its marker and
the entry's arena offset; a hashed chunk hashlib's digest and OFF_NONE, or the
offset of the entry that claims its hash.  A digest kernel that runs on an
untaken chunk turns a marker into a hash, one that drops a taken chunk leaves
its row unwritten; either fails here.

Every chunk starts with its number, so every fingerprint bucket holds one
entry and the chunks recognised are exactly the planned ones: the totals are
asserted as conditions (an entry the sketch failed to insert would turn a
marker into a hash as well).

The paths (launch_digest reads the settings from the context, which reads them
when it is created; `work` is the number of hashed chunks):

  pc            DSX_DIGEST_PC=1                    n = 1,500  digest_pc_kernel
  wave-index    DSX_DIGEST_PC=0 DSX_DIGEST_LPT=0   n = 2,500  digest_kernel in index order: untaken
                                                              static lanes refill by single atomics
  wave-noorder  DSX_DIGEST_PC=0 DSX_DIGEST_LPT=1   n = 1,500  the same, no order below 8 * 256 chunks
  wave-order    DSX_DIGEST_PC=0 DSX_DIGEST_LPT=1   n = 2,500  count, scan and scatter with the mask;
                                                              the order ends at 0xFFFFFFFF
  auto-big      nothing set                        n ~ 320 K  what a 4 GiB blob runs: digest_kernel,
                                                              order, mask, more hashed chunks than lanes
  index-big     DSX_DIGEST_PC=0 DSX_DIGEST_LPT=0   n ~ 320 K  the queue refill without an order
"""
import functools

import numpy as np
import pytest

import known_ref
from known_ref import OFF_NONE, PATTERNS, MarkedStore

pytestmark = pytest.mark.gpu

SETTINGS = ("DSX_DIGEST_PC", "DSX_DIGEST_LPT")
SMALL = {  # path -> (settings, chunks)
    "pc": ({"DSX_DIGEST_PC": "1"}, 1500),
    "wave-index": ({"DSX_DIGEST_PC": "0", "DSX_DIGEST_LPT": "0"}, 2500),
    "wave-noorder": ({"DSX_DIGEST_PC": "0", "DSX_DIGEST_LPT": "1"}, 1500),
    "wave-order": ({"DSX_DIGEST_PC": "0", "DSX_DIGEST_LPT": "1"}, 2500),
}
BIG = {
    "auto-big": {},
    "index-big": {"DSX_DIGEST_PC": "0", "DSX_DIGEST_LPT": "0"},
}
ORDER_FROM = 8 * 256  # launch_digest: the longest-first order from 8 * kDigestThreads chunks on
assert SMALL["wave-noorder"][1] < ORDER_FROM <= SMALL["wave-order"][1]
ALGOS = [0, 1]  # DSX_DIGEST_SHA512_256, DSX_DIGEST_SHA256
ALGO_IDS = ["sha512-256", "sha256"]


def _torch():
    import torch
    return torch


def to_dev(arr):
    t = _torch().from_numpy(np.frombuffer(arr, np.uint8).copy()).to("cuda:0")
    _torch().cuda.synchronize()  # (torch's stream is not the context's)
    return t


@pytest.fixture(scope="module")
def path_ctx(request):
    """A context of its own per path: the settings are read at its creation."""
    from desync_amd import _lib
    env = SMALL[request.param][0] if request.param in SMALL else BIG[request.param]
    with pytest.MonkeyPatch.context() as mp:
        for k in SETTINGS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        ctx = _lib.Context(0)
    yield request.param, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def small_case(n, pattern, algo):
    blob = known_ref.small_blob(n)
    ms = MarkedStore(blob, PATTERNS[pattern](n), algo)
    return ms, ms.want()


@functools.lru_cache(maxsize=None)
def big_case(n, algo):
    blob = known_ref.tiny_blob(n)
    ms = MarkedStore(blob, range(3, n, 8), algo, check_sizes=False)
    return ms, ms.want()


@functools.lru_cache(maxsize=None)
def dev_blob(blob):
    return to_dev(blob.raw)


def first_rows(a, b):
    bad = np.flatnonzero(np.any(a != b, axis=1) if a.ndim == 2 else a != b)
    return [(int(i), bytes(a[i]).hex() if a.ndim == 2 else int(a[i]),
             bytes(b[i]).hex() if b.ndim == 2 else int(b[i])) for i in bad[:4]], len(bad)


def run_case(ctx, ms, want, algo, device=False):
    """Fills a store with ms's entries, calls once and compares everything."""
    import desync_amd
    from desync_amd import _lib
    blob = ms.blob
    want_ids, want_off = want
    store = desync_amd.DeviceStore(len(ms.raw) + 4096, len(ms.ends) + 64, ctx=ctx)
    try:
        t = store.put(to_dev(ms.raw), ms.ids, ms.ends)
        assert t["stored"] == len(ms.ends) and store.counts()["bytes"] == ms.model.used
        ends = to_dev(blob.ends.tobytes()).view(_torch().int64) if device else blob.ends
        # the context's ID scratch, which the call fills and copies out, first holds the other
        # digest's IDs: a row the call leaves unwritten is then wrong (a null mask, same settings)
        other = desync_amd.chunk_ids(dev_blob(blob).data_ptr(), len(blob.raw), blob.ends, 0, ctx=ctx, algo=1 - algo)
        assert b"".join(other) == blob.hashes(1 - algo).tobytes()
        ids, off, tot = store.chunk_ids(dev_blob(blob), ends, 0, algo=algo, device_out=device)
        if device:
            _torch().cuda.synchronize()
            ids, off = ids.cpu().numpy(), off.cpu().numpy().view(np.uint64)
        print(tot)
        assert tot["chunks"] == blob.n
        assert tot["hashed"] == len(ms.hashed) and tot["recognised"] == len(ms.recognised), tot
        assert tot["untried"] == 0 and tot["fp_false"] == 0, tot
        assert tot["hashed_bytes"] == sum(blob.sizes[i] for i in ms.hashed)
        assert tot["recognised_bytes"] + tot["hashed_bytes"] == len(blob.raw)
        assert np.array_equal(ids, want_ids), first_rows(ids, want_ids)
        assert np.array_equal(off, want_off), first_rows(off, want_off)
        assert np.array_equal(off, store.locate(ids)[0])
        assert int((off == OFF_NONE).sum()) == len(ms.hashed) - len(ms.lied)
        assert _lib.DSX_OFF_NONE == OFF_NONE
    finally:
        store.close()


@pytest.mark.parametrize("algo", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("path_ctx", list(SMALL), indirect=True)
def test_small(path_ctx, pattern, algo):
    """Host ends, host outputs."""
    path, ctx = path_ctx
    ms, want = small_case(SMALL[path][1], pattern, algo)
    run_case(ctx, ms, want, algo)


@pytest.mark.parametrize("algo", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("path_ctx", list(SMALL), indirect=True)
def test_small_device_ends_and_outputs(path_ctx, algo):
    """DSX_ENDS_DEVICE | DSX_OUT_DEVICE: the kernels write the caller's buffers."""
    path, ctx = path_ctx
    ms, want = small_case(SMALL[path][1], "every-second", algo)
    run_case(ctx, ms, want, algo, device=True)


@pytest.mark.parametrize("algo", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("path_ctx", list(BIG), indirect=True)
def test_big(path_ctx, algo):
    """Chunks of 8-64 bytes, one in eight recognised, and more hashed chunks
    than digest_kernel's grid has lanes: at most 4 workgroups of 256 per CU
    (SHA-256's occupancy before the mask's registers; SHA-512/256 holds 2), so
    every lane takes further chunks from the queue, through order[] or not."""
    _, ctx = path_ctx
    lanes = _torch().cuda.get_device_properties(0).multi_processor_count * 4 * 256
    n = -(-(lanes + 16384) * 8 // 7) + 8
    ms, want = big_case(n, algo)
    assert len(ms.hashed) >= lanes + 16384
    assert len(ms.hashed) > 2 * 64 * lanes // 1024  # (beyond digest_pc_kernel's automatic range)
    run_case(ctx, ms, want, algo)
