"""dsx_cut_device_many on the GPU: many blobs packed in one buffer, one call.

The expectation is always the oracle's Chunker.Next loop per blob
(oracle.chunk_stream of the blob's bytes alone) plus the blob's start,
concatenated in blob order; each data set's expectation is computed once.
"""
import ctypes
import functools
import io

import numpy as np
import pytest

from oracle import oracle as o

pytestmark = pytest.mark.gpu

KiB, MiB = 1024, 1 << 20
SMALL = (2 * KiB, 8 * KiB, 32 * KiB)
DFLT = (16 * KiB, 64 * KiB, 256 * KiB)


def torch_dev(arr):
    import torch
    t = torch.from_numpy(np.array(arr, dtype=np.uint8, copy=True)).to("cuda")
    torch.cuda.synchronize()
    return t


def expected(data, blob_ends, params):
    """-> (ends, first) of the per-blob oracle."""
    ends, first, b0 = [], [0], 0
    for b1 in (int(x) for x in blob_ends):
        e = o.chunk_stream(data[b0:b1], *params) + np.uint64(b0) if b1 > b0 else np.empty(0, np.uint64)
        ends.append(e)
        first.append(first[-1] + e.size)
        b0 = b1
    return (np.concatenate(ends) if ends else np.empty(0, np.uint64)), np.array(first, dtype=np.uint64)


def many(dctx, t, blob_ends, params, **kw):
    import desync_amd
    return desync_amd.cut_device_many(t.data_ptr(), t.numel(), blob_ends, *params, ctx=dctx, **kw)


def check_lists(got, want, blob_ends):
    ends, first, totals = got
    wends, wfirst = want
    assert ends.size == wends.size, (ends.size, wends.size)
    bad = np.flatnonzero(ends != wends)
    assert bad.size == 0, (int(bad[0]), int(ends[bad[0]]), int(wends[bad[0]]))
    assert np.array_equal(first, wfirst)
    be = np.asarray(blob_ends, dtype=np.uint64)
    lens = np.diff(np.concatenate([np.zeros(1, np.uint64), be]))
    # blob_first is consistent and every non-empty blob's end is in the list
    assert first[0] == 0 and first[-1] == ends.size and np.all(np.diff(first.astype(np.int64)) >= 0)
    assert np.array_equal(np.diff(first.astype(np.int64)) > 0, lens > 0)
    assert np.all(np.isin(be[lens > 0], ends)) and np.all(np.diff(ends.astype(np.int64)) > 0)
    assert totals["blobs"] == be.size and totals["empty_blobs"] == int((lens == 0).sum())
    assert totals["chunks"] == ends.size
    assert totals["batched_blobs"] + totals["single_blobs"] + totals["empty_blobs"] == be.size


# ------------------------------------------------------------------ 1. edge lengths
def test_edge_lengths(dctx):
    mn, av, mx = SMALL
    lens = [0, 0, 1, 47, 48, 49, mn - 1, mn, mn + 1, mn + 48, av, mx - 1, mx, mx + 1,
            -(2 * mx + mn), -(2 * mx + mn + 1), 0, 100_003, 0]  # (negative: that many zeros)
    rng = np.random.default_rng(11)
    parts = [np.zeros(-n, np.uint8) if n < 0 else rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    data = np.concatenate(parts)
    be = np.cumsum([abs(n) for n in lens]).astype(np.uint64)
    want = expected(data, be, SMALL)
    got = many(dctx, torch_dev(data), be, SMALL)
    check_lists(got, want, be)
    first = got[1]
    assert first[0] == first[1] == first[2] == 0 and first[-1] == first[-2]  # empty first / last blobs
    # the blobs of zeros: forced cuts every max, then the tail rule
    z = 14
    assert np.array_equal(got[0][first[z]:first[z + 1]] - be[z - 1], [mx, 2 * mx, 2 * mx + mn])
    assert np.array_equal(got[0][first[z + 1]:first[z + 2]] - be[z], [mx, 2 * mx, 2 * mx + mn + 1])


# ------------------------------------------------------------------ 2. planted boundaries
def test_planted_boundaries(dctx):
    """Blob boundaries placed around candidates of the whole buffer: a blob
    starting at c-min-1 must cut at c (the first position its chain tests), one
    starting at c-min must not, one starting at c-20 sees a candidate at c
    whose window straddles the boundary, and blobs end at c, c-1 and c+1."""
    mn, av, mx = SMALL
    data = o.synth_uniform(21, 0, 4 * MiB)
    cands = o.candidates(data, *SMALL).astype(np.int64)
    offs = (-mn - 1, -mn, -20, 0, -1, 1)
    picked, bounds = [], []
    for k in range(60):  # ten candidates per kind
        c = int(cands[np.searchsorted(cands, 40_000 + 68_000 * k)])
        picked.append(c)
        bounds.append(c + offs[k % 6])
    assert all(b > a for a, b in zip(bounds, bounds[1:])) and bounds[-1] < data.size
    be = np.array(bounds + [data.size], dtype=np.uint64)
    want = expected(data, be, SMALL)
    whole = o.chunk_stream(data, *SMALL)
    assert not np.array_equal(whole, want[0])  # a call that ignores blob_ends cannot pass
    for k, c in enumerate(picked):
        if k % 6 == 0:
            assert want[0][want[1][k + 1]] == c        # the blob after boundary k cuts at c first
        if k % 6 == 1:
            assert c not in want[0]                    # c == start + min: not eligible
    # the scan does see candidates in (B0, B0 + 47]: garbage the chain never asks for
    junk = [b for b in bounds if np.any((cands > b) & (cands <= b + 47))]
    assert junk, "no candidate straddles a boundary: the test does not plant what it claims"
    got = many(dctx, torch_dev(data), be, SMALL)
    check_lists(got, want, be)


# ------------------------------------------------------------------ 3. many small
@functools.lru_cache(maxsize=None)
def small_set():
    rng = np.random.default_rng(3)
    lens = np.exp(rng.uniform(0.0, np.log(256 * KiB), 3000)).astype(np.uint64)
    lens = np.clip(lens, 1, 256 * KiB)
    be = np.cumsum(lens).astype(np.uint64)
    data = o.synth_uniform(3, 0, int(be[-1]))
    return data, be, {p: expected(data, be, p) for p in (DFLT, SMALL)}


@pytest.mark.parametrize("params", [DFLT, SMALL], ids=["16:64:256", "2:8:32"])
def test_many_small(dctx, params):
    import torch
    data, be, want = small_set()
    t = torch_dev(data)
    got = many(dctx, t, be, params)
    check_lists(got, want[params], be)
    assert got[2]["batched_blobs"] + got[2]["empty_blobs"] == got[2]["blobs"] == 3000
    assert got[2]["single_blobs"] == 0 and got[2]["groups"] == 1
    # device output
    cap = data.size // params[0] + be.size
    d_out = torch.zeros(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n, first, totals = many(dctx, t, be, params, out_ptr=d_out.data_ptr(), out_cap=cap)
    ends = d_out[:n].cpu().numpy().view(np.uint64)
    check_lists((ends, first, totals), want[params], be)


# ------------------------------------------------------------------ 4. plan paths
def test_plan_paths_at_small_sizes(dctx):
    """big_blob = 1 MiB and group_bytes = 4 MiB: several groups, single blobs
    between them, blob ends exactly on multiples of 4 MiB."""
    rng = np.random.default_rng(4)
    lens = [int(x) for x in np.exp(rng.uniform(np.log(64), np.log(256 * KiB), 500))]
    for at, n in ((40, 1 * MiB), (170, 3 * MiB), (171, 0), (300, 2 * MiB + 12345), (480, MiB - 1)):
        lens.insert(at, n)
    # trim the blob that crosses 4 MiB and the one that crosses 12 MiB to end there
    be, total = [], 0
    marks = [4 * MiB, 12 * MiB]
    for n in lens:
        if marks and total < marks[0] < total + n:
            n = marks.pop(0) - total
        total += n
        be.append(total)
    assert not marks and 4 * MiB in be and 12 * MiB in be
    be = np.array(be, dtype=np.uint64)
    lens = np.diff(np.concatenate([np.zeros(1, np.uint64), be]))
    data = o.synth_uniform(44, 0, int(be[-1]))
    want = expected(data, be, DFLT)
    t = torch_dev(data)
    got = many(dctx, t, be, DFLT, big_blob=1 * MiB, group_bytes=4 * MiB)
    check_lists(got, want, be)
    dflt = many(dctx, t, be, DFLT)
    check_lists(dflt, want, be)
    assert np.array_equal(got[0], dflt[0]) and np.array_equal(got[1], dflt[1])
    assert got[2]["groups"] > 1 and dflt[2]["groups"] == 1
    assert got[2]["single_blobs"] == int((lens >= 1 * MiB).sum()) == 3
    assert dflt[2]["single_blobs"] == 0


# ------------------------------------------------------------------ 5. fallback
def test_fallback_dense_blob(dctx):
    """test_periodic_dense_candidates' data (a candidate every 48 bytes) as one
    blob between random ones: the batched path cannot hold it."""
    P = o.params(*DFLT)
    rng = np.random.default_rng(1)
    while True:  # a 48-byte block whose periodic window hash is a candidate
        blk = rng.integers(0, 256, 48, dtype=np.uint8)
        if o.window_hash(bytes(blk)) % P.d == P.d - 1:
            break
    parts = [rng.integers(0, 256, 200_001, dtype=np.uint8), np.tile(blk, (3 * MiB) // 48),
             rng.integers(0, 256, 300_007, dtype=np.uint8)]
    data = np.concatenate(parts)
    be = np.cumsum([p.size for p in parts]).astype(np.uint64)
    got = many(dctx, torch_dev(data), be, DFLT)
    print("dense blob: totals", got[2])
    check_lists(got, expected(data, be, DFLT), be)


def test_fallback_small_avg(dctx):
    """avg 192, the smallest of test_random_avg_sweep: 9 MiB as blobs of 3 MiB,
    100 KiB, 500 KiB and the rest."""
    params = (48, 192, 768)
    data = o.synth_uniform(5, 0, 9 * MiB)
    lens = [3 * MiB] + [100 * KiB] * 20 + [500 * KiB] * 4
    lens.append(data.size - sum(lens))
    be = np.cumsum(lens).astype(np.uint64)
    got = many(dctx, torch_dev(data), be, params)
    print("avg 192: totals", got[2])
    check_lists(got, expected(data, be, params), be)


# ------------------------------------------------------------------ 6. capacity and reuse
def test_capacity_and_reuse(dctx):
    import desync_amd
    from desync_amd import _lib
    data, be, want = small_set()
    be, n_bytes = be[:200], int(be[199])
    data = data[:n_bytes]
    wends, wfirst = expected(data, be, SMALL)
    t = torch_dev(data)
    one = o.chunk_stream(data, *SMALL)
    assert np.array_equal(desync_amd.cut_device(t.data_ptr(), n_bytes, *SMALL, ctx=dctx), one)
    # cap = needed - 1
    p = desync_amd.Params(*SMALL)
    out = np.full(wends.size, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    n = ctypes.c_uint64()
    rc = _lib.lib().dsx_cut_device_many(dctx.h, ctypes.c_void_p(t.data_ptr()), n_bytes,
                                        be.ctypes.data, be.size, ctypes.byref(p.c), out.ctypes.data,
                                        wends.size - 1, ctypes.byref(n), None, None, None, 0)
    assert rc == _lib.DSX_E_CAPACITY and n.value == wends.size
    assert np.all(out == np.uint64(0xA5A5A5A5A5A5A5A5))  # a failing call leaves the host buffer alone
    check_lists(many(dctx, t, be, SMALL), (wends, wfirst), be)
    assert np.array_equal(desync_amd.cut_device(t.data_ptr(), n_bytes, *SMALL, ctx=dctx), one)
    # one blob equals cut_device; no blob at all is no chunk
    ends, first, totals = many(dctx, t, np.array([n_bytes], dtype=np.uint64), SMALL)
    assert np.array_equal(ends, one) and list(first) == [0, one.size]
    ends, first, totals = desync_amd.cut_device_many(0, 0, np.empty(0, np.uint64), *SMALL, ctx=dctx)
    assert ends.size == 0 and list(first) == [0] and totals["chunks"] == 0
    ends, first, totals = desync_amd.cut_device_many(0, 0, np.zeros(3, np.uint64), *SMALL, ctx=dctx)
    assert ends.size == 0 and list(first) == [0, 0, 0, 0] and totals["empty_blobs"] == 3


def test_refusals_with_a_context(dctx):
    """The refusals of tests/test_many_host.py with a real context: DSX_E_INVAL
    and a dsx_last_error text, and the context works afterwards."""
    import desync_amd
    from desync_amd import _lib
    t = torch_dev(np.arange(9, dtype=np.uint8))
    for be, length, kw in (([9, 5], 9, {}), ([5, 8], 9, {}), ([], 9, {}), ([5, 9], 9, {"group_bytes": (8 << 30) + 1})):
        with pytest.raises(_lib.DsxError) as e:
            desync_amd.cut_device_many(t.data_ptr(), length, np.array(be, dtype=np.uint64), *SMALL,
                                       ctx=dctx, **kw)
        assert e.value.code == _lib.DSX_E_INVAL and "cut_device_many" in str(e.value)
    ends, _, _ = desync_amd.cut_device_many(t.data_ptr(), 9, np.array([5, 9], dtype=np.uint64), *SMALL,
                                            ctx=dctx)
    assert list(ends) == [5, 9]


# ------------------------------------------------------------------ 7. downstream
def test_device_ends_feed_chunk_ids(dctx):
    import torch
    from desync_amd import _lib
    data, be, want = small_set()
    be, n_bytes = be[:300], int(be[299])
    data = data[:n_bytes]
    wends, _ = expected(data, be, DFLT)
    t = torch_dev(data)
    cap = n_bytes // DFLT[0] + be.size
    d_ends = torch.zeros(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n, _, _ = many(dctx, t, be, DFLT, out_ptr=d_ends.data_ptr(), out_cap=cap)
    assert n == wends.size
    ids = np.zeros((n, 32), dtype=np.uint8)
    _lib.check(_lib.lib().dsx_chunk_ids(dctx.h, ctypes.c_void_p(t.data_ptr()), n_bytes, 0,
                                        ctypes.c_void_p(d_ends.data_ptr()), n, ids.ctypes.data,
                                        _lib.DSX_ENDS_DEVICE, _lib.DSX_DIGEST_SHA512_256), dctx.h)
    assert [r.tobytes() for r in ids] == o.chunk_ids(data, wends)


def _encoded(index):
    b = io.BytesIO()
    index.WriteTo(b)
    return b.getvalue()


def test_index_from_blobs_and_chop_blobs(dctx, golden):
    import desync_amd
    b1, b2 = golden("blob1"), golden("blob2")
    rnd = o.synth_uniform(77, 0, 300 * KiB).tobytes()
    blobs = [b1, b"", b2, rnd]
    idx = desync_amd.IndexFromBlobs(blobs, *SMALL, ctx=dctx)
    assert len(idx) == 4
    assert _encoded(idx[0]) == golden("blob1.caibx")
    assert _encoded(idx[2]) == golden("blob2.caibx")
    assert len(_encoded(idx[1])) == 104 and _encoded(idx[1]) == o.make_caibx(b"", *SMALL)
    assert _encoded(idx[3]) == o.make_caibx(rnd, *SMALL)
    # a device tensor in the list, and the packed form with a (pointer, length) pair
    t = torch_dev(np.frombuffer(b1 + b2 + rnd, np.uint8))
    be = np.cumsum([len(b1), 0, len(b2), len(rnd)]).astype(np.uint64)
    for form in ([torch_dev(np.frombuffer(b1, np.uint8)), b"", b2, rnd], (t, be),
                 ((t.data_ptr(), t.numel()), be)):
        again = desync_amd.IndexFromBlobs(form, *SMALL, ctx=dctx)
        assert [_encoded(i) for i in again] == [_encoded(i) for i in idx]
    # desync make -s over the blobs, then extract each from the store
    need = len(b1) + len(b2) + len(rnd)
    with desync_amd.DeviceStore(need, sum(len(i.Chunks) for i in idx), ctx=dctx) as store:
        chopped = desync_amd.ChopBlobs(blobs, store, *SMALL)
        assert [_encoded(i) for i in chopped] == [_encoded(i) for i in idx]
        for index, blob in zip(chopped, blobs):
            out, _ = desync_amd.AssembleBlob(index, store, null_seed=False, ctx=dctx)
            assert out.cpu().numpy().tobytes() == blob
