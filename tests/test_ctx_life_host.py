"""The context's chain-state contract on the CPU (tests/ctx_life_ref.py).

include/dsx.h, "One chain state per context": a chain call inside an
unfinished stream is refused, dsx_stream_begin with uncollected queued calls
is refused, a chain call between dsx_shard_local and its resolve makes the
shard stale, neutral calls run anywhere.  Here: the rule itself under the host
sanitizers (tests/chain_owner_model.cpp over csrc/dsx_chain_owner.h), the
scripts' conditions, the model driven by itself, and three broken libraries
that every script must catch at the first op they affect.  The GPU runs the
same scripts in tests/test_gpu_ctx_life.py.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ctx_life_ref as r
from ctx_life_ref import E_CAPACITY, E_STATE, OK

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_owner_model(tmp_path):
    """dsx_chain_owner.h alone, built with -fsanitize=address,undefined: every
    sequence of up to five events against the contract restated from the
    history of events; the first difference is a non-zero exit."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "chain_owner_model")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "desync_amd", "csrc"),
           os.path.join(REPO, "tests", "chain_owner_model.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.splitlines()[-1].startswith("chain owner model ok: 1419857 sequences"), res.stdout[-1000:]


def test_the_guard_comes_after_the_argument_refusals():
    """Without a context no chain entry point reaches the owner: DSX_E_INVAL,
    as before (no GPU is touched)."""
    from desync_amd import _lib
    L = _lib.lib()
    p = _lib.Params()
    assert L.dsx_params_init(4096, 16384, 65536, ctypes.byref(p)) == 0
    n = ctypes.c_uint64()
    E = _lib.DSX_E_INVAL
    assert L.dsx_cut_device(None, None, 0, ctypes.byref(p), None, 0, ctypes.byref(n), 0) == E
    assert L.dsx_cut_device_many(None, None, 0, None, 0, ctypes.byref(p), None, 0, ctypes.byref(n), None,
                                 None, None, 0) == E
    assert L.dsx_cut_host(None, None, 0, ctypes.byref(p), None, 0, ctypes.byref(n)) == E
    assert L.dsx_index_host(None, None, 0, ctypes.byref(p), 0, None, None, 0, ctypes.byref(n)) == E
    assert L.dsx_cut_fd(None, 0, 0, 0, ctypes.byref(p), None, 0, ctypes.byref(n)) == E
    assert L.dsx_index_fd(None, 0, 0, 0, ctypes.byref(p), 0, None, None, 0, ctypes.byref(n)) == E
    assert L.dsx_shard_local(None, None, 0, 0, 0, 0, ctypes.byref(p), None, 0) == E
    assert L.dsx_shard_resolve(None, None, 1, 0, None, None, 0, ctypes.byref(n), 0) == E
    assert L.dsx_shard_resolve_async(None, None, 1, 0, None, 0, None) == E
    assert L.dsx_shard_collect(None, None, None, None, ctypes.byref(n)) == E
    assert L.dsx_stream_begin(None, ctypes.byref(p)) == E
    assert L.dsx_result(None, ctypes.byref(n)) == E


# ------------------------------------------------------------------- inputs
def test_pool_and_shard_geometry():
    P = r.pool()
    assert [P.blobs[b].size for b in ("u256k", "u1m", "u3m", "tiny", "empty")] == [
        256 * r.KiB, r.MiB + 12345, 3 * r.MiB + 1, 1000, 0]
    assert P.want("tiny", "B").tolist() == [1000] and P.want("empty", "A").size == 0
    assert P.stream.size == 20 * r.MiB + 5 and -(-P.stream.size // r.BATCH) == 3
    # an odd split; both shards hold the longest intruder of a round
    (s0, n0), (s1, n1) = P.shard_geo
    assert s1 % 2 == 1 and s0 + n0 == s1 and s1 + n1 == r.SHARD_LEN
    assert min(n0, n1) >= max(P.blobs[b].size for b in r._Gen.SAFE)
    assert all(w.size >= 2 for w in P.shard_want)
    assert np.array_equal(np.concatenate(P.shard_want), r.o.chunk_stream(P.shard, *r.PSETS[r.SHARD_PSET]))
    # the seam converges in one round on the CPU: no script needs a resync
    assert P.shard_converges()
    # the dense tile is what a queued call redoes; the lists the failing ops shorten have two cuts
    assert P.want("dense", "D").size >= 2
    for b in ("u1m", "u3m", "zero"):
        for ps in ("A", "B"):
            assert P.want(b, ps).size >= 2


def test_many_plan_restated():
    """The four dsx_cut_device_many variants launch one, two and three scans,
    and one takes the one-blob path between two groups."""
    g = r._Gen(1)
    got = []
    for v in range(4):
        op = g.many_op(variant=v)
        _, be, ends, first, groups, singles = r.pool().many(op)
        assert first[-1] == ends.size and be[-1] == sum(r.pool().blobs[b].size for b in op["blobs"])
        got.append((groups, singles))
    assert got == [(1, 0), (2, 0), (3, 0), (2, 1)]


@pytest.mark.parametrize("seed", r.SEEDS)
def test_scripts_are_deterministic(seed):
    a = r.script(seed)
    r.script.cache_clear()
    b = r.script(seed)
    assert a == b and len(a) == r.NOPS
    assert len({repr(r.script(s)) for s in r.SEEDS}) == len(r.SEEDS)


def _union(key):
    out = {}
    for s in r.SEEDS:
        for k, v in r.conditions(s)[key].items():
            out[k] = out.get(k, 0) + v
    return out


def test_conditions_over_the_seed_set():
    assert 6 <= len(r.SEEDS) <= 8
    cs = [r.conditions(s) for s in r.SEEDS]
    assert all(c["nops"] == 60 for c in cs)
    pairs = set().union(*(c["pairs"] for c in cs))
    want = {(a, b) for a in r.CHAIN_KINDS for b in r.CHAIN_KINDS}
    assert pairs >= want, sorted(want - pairs)
    chain = _union("intruder_chain")
    assert all(chain.get(k, 0) >= 2 for k in r.CHAIN_KINDS), chain
    neutral = _union("intruder_neutral")
    assert all(neutral.get(k, 0) >= 1 for k in r.NEUTRAL_KINDS), neutral
    refused = _union("refused_in_carried_stream")
    assert all(refused.get(k, 0) >= 1 for k in r.CHAIN_KINDS), refused
    inside = _union("neutral_in_stream")
    assert all(inside.get(k, 0) >= 1 for k in r.NEUTRAL_KINDS), inside
    two = _union("sync_with_two_queued")
    assert all(two.get(k, 0) >= 1 for k in r.SYNC_KINDS), two
    assert sum(c["dense_queued_with_later"] for c in cs) >= 2
    assert sum(c["begin_refused_for_queue"] for c in cs) >= 1
    assert max(c["max_queue"] for c in cs) == r.QUEUE_DEPTH
    # dsx_cut_device_many: one, two and three scans, and the one-blob path
    scans = set().union(*(c["scans"] for c in cs))
    assert {g for g, _ in scans} >= {1, 2, 3} and any(s for _, s in scans), scans
    # the direct path and the recovery after a stale round
    assert sum(c["direct_resolves"] for c in cs) >= len(r.SEEDS)
    assert sum(c["recoveries"] for c in cs) >= len(r.SEEDS)


@pytest.mark.parametrize("seed", r.SEEDS)
def test_conditions_of_each_script(seed):
    c = r.conditions(seed)
    assert c["stale_refusals"] >= 1 and c["stream_refusals"] >= 1 and c["max_queue"] >= 4
    # every failing op (a short cut, a short queued call's result, a refused many) is followed
    # directly by a chain op
    assert c["failing"] >= 3 and c["failing_then_chain"] == c["failing"]
    # what runs between a local and its resolve stays inside the shard's list
    # even for a library that does not refuse it
    assert c["bounds_ok"]


# ------------------------------------------------------- the model, driven
@pytest.mark.parametrize("seed", r.SEEDS)
def test_model_backend_drives_clean(seed):
    log = []
    n = r.drive(r.ModelBackend(), r.script(seed), log=log)
    assert n >= r.NOPS + 2  # (the periodic cuts ran where the model allows them)
    codes = {rc for _, _, rc, _ in log}
    assert {OK, E_STATE, E_CAPACITY, r.E_INVAL} <= codes


# ------------------------------------------------------ three broken libraries
class _NoStaleModel(r.Model):
    """A library without the owner: a chain call leaves a waiting shard `valid`."""

    def _chain(self):
        if self.shard is not None:
            self.shard["clobbered"] = True


class ResolveEmitsTheLastCallsCuts(r.ModelBackend):
    """dsx_shard_resolve launches its emit over whatever the last chain call
    left in the context's state and staging list (the library before the owner)."""

    def __init__(self):
        self.m = _NoStaleModel()

    def apply(self, op):
        exp = self.m.predict(op)
        got = r.realize(self.m, op, exp)
        if op["op"] in r.RESOLVES and exp.rc == OK and self.m.shard.get("clobbered"):
            got["list"] = self.m.last_list
            got["n"] = int(self.m.last_list.size)
        self.m.commit(op, exp, got)
        return got


class _NoStreamGuardModel(r.Model):
    def predict(self, op):
        if op["op"] in r.CHAIN_KINDS and self.stream_unfinished() and not op.get("bad"):
            s, self.stream = self.stream, None
            try:
                exp = super().predict(op)
            finally:
                self.stream = s
            exp["intruded"] = True
            return exp
        return super().predict(op)


class StreamContinuesFromTheIntrudersCarry(r.ModelBackend):
    """A chain call inside a stream runs, and the next batch continues from
    the chain position it left."""

    def __init__(self):
        self.m = _NoStreamGuardModel()
        self.off = 0

    def apply(self, op):
        exp = self.m.predict(op)
        got = r.realize(self.m, op, exp)
        if exp.get("intruded"):
            self.off = 1
            stream, self.m.stream = self.m.stream, None
            self.m.commit(op, exp, got)
            self.m.stream = stream
            return got
        if op["op"] == "stream_pop_all" and self.off:
            got["list"] = got["list"] + np.uint64(self.off)
        if op["op"] == "stream_begin" and exp.rc == OK:
            self.off = 0
        self.m.commit(op, exp, got)
        return got


class ResultAnswersWithTheNewestCall(r.ModelBackend):
    """dsx_result reads the context's current chain state instead of the
    oldest queued call's published slot."""

    def apply(self, op):
        exp = self.m.predict(op)
        got = r.realize(self.m, op, exp)
        if op["op"] == "result" and len(self.m.queue) >= 2:
            q = self.m.queue[-1]
            w = self.m.P.want(q["blob"], q["pset"])
            got["n"], got["rc"] = int(w.size), E_CAPACITY if q.get("short") else OK
        self.m.commit(op, exp, got)
        return got


def _first_affected(ops, fake):
    """The first op at which the broken library must differ, from the script
    and a model that keeps the contract."""
    m = r.Model()
    for pos, op in enumerate(ops):
        exp = m.predict(op)
        k = op["op"]
        if fake is ResolveEmitsTheLastCallsCuts and k in ("shard_resolve", "shard_resolve_async",
                                                         "shard_collect"):
            if m.shard is not None and m.shard["stale"] and exp.rc == E_STATE:
                return pos
        if fake is StreamContinuesFromTheIntrudersCarry and k in r.CHAIN_KINDS:
            if exp.rc == E_STATE and exp.err == "stream":
                return pos
        if fake is ResultAnswersWithTheNewestCall and k == "result" and len(m.queue) >= 2:
            old, new = m.queue[0], m.queue[-1]
            if (m.P.want(old["blob"], old["pset"]).size, bool(old.get("short"))) != (
                    m.P.want(new["blob"], new["pset"]).size, bool(new.get("short"))):
                return pos
        m.commit(op, exp, r.realize(m, op, exp))
    return None


@pytest.mark.parametrize("seed", r.SEEDS)
@pytest.mark.parametrize("fake", [ResolveEmitsTheLastCallsCuts, StreamContinuesFromTheIntrudersCarry,
                                  ResultAnswersWithTheNewestCall])
def test_driver_catches_a_broken_library(fake, seed):
    ops = r.script(seed)
    at = _first_affected(ops, fake)
    assert at is not None, "the script never reaches what this library gets wrong"
    with pytest.raises(r.Mismatch) as e:
        r.drive(fake(), ops)
    assert e.value.pos == at and not e.value.extra, str(e.value)
