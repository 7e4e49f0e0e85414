"""tests/test_gpu_cut_capacity.py's table is not vacuous (no GPU): the fence
and the checks catch a deliberately wrong "library" written in Python, the
restated stitch geometry puts every case on the side of 256 / 2048 segments
that the table claims, the oracle confirms the cases' claims about their
lists, and caps(n) holds both sides of the edge for every case's n.
"""
import numpy as np
import pytest

import cut_cap_ref as cc
from cut_cap_ref import DSX_E_CAPACITY, DSX_OK, FencedOut, caps, check, check_fences, check_untouched


# ------------------------------------------------------ a library in Python
def fake_cut(fenced, want, bug=None):
    """dsx_cut_device's contract on a host FencedOut, with one bug at a time."""
    out = fenced.mem[fenced.guard:]
    n, cap = want.size, fenced.cap
    fits = n < cap if bug == "lt" else n <= cap
    if fits or bug == "ignores_cap":
        out[:n] = want
    elif bug == "one_past_cap":
        out[:cap + 1] = want[:cap + 1]
    elif bug == "partial_on_failure":
        out[:cap] = want[:cap]
    if bug == "front":
        fenced.mem[fenced.guard - 1] = 0
    if bug == "tail" and fits:
        out[n] = want[-1]
    if not fits:
        return (DSX_OK if bug == "ok_when_short" else DSX_E_CAPACITY), (n - 1 if bug == "count" else n)
    return DSX_OK, n


def run_fake(bug, where="host"):
    want = cc.zero_runs().want
    for cap in caps(want.size, 386):
        f = FencedOut(386, cap, "host")
        f.host_rule = where == "host"  # ("device": what a failed call leaves below cap is open)
        rc, n = fake_cut(f, want, bug)
        check(f, rc, n, want, str(bug))


def test_an_honest_library_passes():
    run_fake(None)
    run_fake("partial_on_failure", where="device")  # below cap after a failure: not asserted


@pytest.mark.parametrize("bug,needle", [
    ("one_past_cap", "at or past cap"), ("ignores_cap", "at or past cap"), ("count", ""),
    ("ok_when_short", ""), ("lt", ""), ("front", "front guard"), ("tail", "behind the list"),
    ("partial_on_failure", "host output of a failed call")])
def test_every_bug_is_caught(bug, needle):
    with pytest.raises(AssertionError) as e:
        run_fake(bug)
    assert needle in str(e.value)


def test_each_bug_is_caught_at_the_cap_it_belongs_to():
    """'lt' shows only at cap == n, 'one_past_cap' at every short cap."""
    want = cc.zero_runs().want
    n = want.size

    def fails(bug, cap):
        f = FencedOut(386, cap, "host")
        try:
            check(f, *fake_cut(f, want, bug), want)
        except AssertionError:
            return True
        return False

    assert [c for c in caps(n, 386) if fails("lt", c)] == [n]
    assert [c for c in caps(n, 386) if fails("one_past_cap", c)] == [0, 1, n // 3, n - 1]
    assert [c for c in caps(n, 386) if fails("count", c)] == [0, 1, n // 3, n - 1]


def test_fence_layout_and_helpers():
    f = FencedOut(100, 7, "host")
    assert f.guard >= f.upper and f.mem.size == 2 * f.guard + f.upper
    assert f.ptr.value == f.mem.ctypes.data + 8 * f.guard and f.ptr_or_null.value == f.ptr.value
    assert FencedOut(100, 0, "host").ptr_or_null is None
    assert np.all(f.mem == np.uint64(cc.SENTINEL)) and cc.SENTINEL > 1 << 63
    check_untouched(f)
    check_fences(f, 50)
    f.mem[f.guard + 6] = 1
    check_fences(f, 50)  # (below cap)
    with pytest.raises(AssertionError):
        check_untouched(f)
    f.mem[f.guard + 7] = 1
    with pytest.raises(AssertionError):
        check_fences(f, 50)
    # a writer that ignores cap writes at most `upper` entries from the pointer on
    for upper in (1, 63, 64, 65, 2818051):
        g = max(upper, 64)
        assert g >= upper and g + upper <= 2 * g + upper


# --------------------------------------------------------- the geometry rule
def test_geometry_sides():
    """Which kernels end each case's piece (launch_stitch's thresholds)."""
    assert cc.stitch_seg(8 * cc.MiB, 256 * cc.KiB) == 1 << 20
    assert cc.stitch_seg(8 * cc.MiB, 768, 65536) == 65536
    assert cc.stitch_seg(8 << 30, 256 * cc.KiB) == 2 << 20      # (4096 segments: DESIGN.md 4.2)
    for case, lo, hi in ((cc.fast_short(), 1, 256), (cc.fast_long(), 1, 256), (cc.zero_runs(), 1, 256),
                         (cc.gather_clean(), 2049, 4096), (cc.gather_suspect(), 2049, 4096)):
        assert lo <= case.nseg <= hi, case.nseg
        assert cc.backend(case.nseg) == ("finish" if hi <= 2048 else "fixup_fast+gather")
    assert cc.nseg(2048 * 65536, 768, 65536) == 2048 and cc.nseg(2048 * 65536 + 1, 768, 65536) == 2049
    assert cc.backend(2048) == "finish" and cc.backend(2049) == "fixup_fast+gather"
    assert cc.backend(8, finish=False) == "fixup_fast+gather"
    assert cc.backend(8, finish=False, fixup_fast=False) == "fixup+gather"
    assert cc.backend(9217) == "fixup+gather"
    # the dense retry's pieces of the 70 MiB tile: each a finish_kernel launch
    L, mx = cc.DENSE_LEN, cc.DFLT[2]
    pieces = [(P, min(cc.DENSE_PIECE, L - P)) for P in range(0, L, cc.DENSE_PIECE)]
    assert len(pieces) == 3
    assert [cc.piece_nseg(P, n, L, mx) for P, n in pieces] == [32, 33, 7]
    # 8 GiB + 64 MiB: an 8 GiB piece in 2 MiB segments, then 64 MiB + max in 1 MiB segments
    L = cc.TWO_PIECES_LEN
    assert cc.piece_nseg(0, cc.PIECE_MAX, L, mx) == 4096
    assert cc.piece_nseg(cc.PIECE_MAX, L - cc.PIECE_MAX, L, mx) == 65
    assert cc.backend(4096) == "fixup_fast+gather" and cc.backend(65) == "finish"
    # the queued calls and the shards: one piece, finish_kernel
    for case, _ in cc.queued_blobs():
        assert cc.backend(case.nseg) == "finish"


# ------------------------------------------------------- the oracle's claims
def test_list_claims():
    short, long_ = cc.fast_short(), cc.fast_long()
    assert cc.cuts_per_segment(short.want, 1 << 20).max() <= 64
    assert cc.cuts_per_segment(long_.want, 65536).max() > 64
    # the zero run of the suspect gather case: forced cuts every max, off every segment start
    sus = cc.gather_suspect()
    z = sus.want[(sus.want > cc.ZEROS_AT + 2 * 768) & (sus.want <= cc.ZEROS_AT + cc.ZEROS_LEN)]
    assert np.all(np.diff(z.astype(np.int64)) == 768) and z.size > 8000
    assert z[0] % 256 != 0  # (a chain from a segment start k * 65536 cuts at k * 65536 + j * 768)
    # the dense tile: the counts at the piece ends split the list in three
    dense = cc.dense_pieces()
    cap_list, at = cc.dense_caps(dense)
    assert 0 < at[0] < at[1] < dense.n
    assert dense.want[at[0] - 1] <= cc.DENSE_PIECE < dense.want[at[0]]
    assert dense.want[at[1] - 1] <= 2 * cc.DENSE_PIECE < dense.want[at[1]]
    for c in at:
        assert {c - 1, c, c + 1} <= set(cap_list)
    assert set(caps(dense.n, dense.upper)) <= set(cap_list)
    # the shards: every rank has cuts and the ranks' lists add up to the chain
    for sh in (cc.shards_uniform(), cc.shards_zero_run()):
        assert all(w.size >= 6 for w in sh.want)
        assert np.array_equal(np.concatenate(sh.want), cc.o.chunk_stream(sh.data, *sh.params))
    # many: the fallback blob is the dense tile; blob_first ends at the count
    for m in (cc.many_plan(), cc.many_fallback()):
        assert m.first[-1] == m.n and m.first.size == m.blob_ends.size + 1


def test_caps_hold_the_edge():
    cases = [(c.n, c.upper) for c in (cc.fast_short(), cc.fast_long(), cc.zero_runs(), cc.gather_clean(),
                                      cc.gather_suspect(), cc.dense_pieces(), cc.dense_small(),
                                      cc.many_plan(), cc.many_fallback())]
    for sh in (cc.shards_uniform(), cc.shards_zero_run()):
        cases.append((sh.want[1].size, sh.upper[1]))
    for n, upper in cases:
        c = caps(n, upper)
        assert {0, 1, n // 3, n - 1, n, n + 1, upper} == set(c) and max(c) == upper
        assert sum(1 for x in c if x < n) >= 4  # four distinct short caps
    for case, short in cc.queued_blobs():
        assert case.n + 1 <= case.upper
