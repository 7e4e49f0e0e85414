"""The stream scripts on the model alone (stream_ref.py): the generators are
deterministic, every script contains the rare sequences it exists for, the
pure-Python stream passes every script, the SYNC-seam method holds at every
SYNC point of every script (what a non-final scan confirms is a prefix of the
whole stream's cuts, namely those at or before the fed position), and the
driver notices a stream that is wrong: four deliberately broken backends are
each caught at the first op they affect."""
import numpy as np
import pytest

import stream_ref as sr
from stream_ref import Mismatch, ModelBackend, drive, record, script


def canon(v):
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, (list, tuple)):
        return tuple(canon(x) for x in v)
    if isinstance(v, dict):
        return tuple((k, canon(x)) for k, x in sorted(v.items()))
    return v


@pytest.fixture(scope="module")
def models():
    """Every script once on the ModelBackend -> its model (counters, SYNC points)."""
    return {name: drive(ModelBackend(), script(name)) for name in sr.NAMES}


@pytest.mark.parametrize("name", sr.NAMES)
def test_script_is_deterministic(name):
    a = script(name)
    b = sr.SCRIPTS[name]()
    assert a is not b and a["ops"] == b["ops"] and len(a["ops"]) > 10
    assert canon(a["data"]) == canon(b["data"])


def test_model_backend_passes_every_script(models):
    assert sorted(models) == sr.NAMES
    for name in sr.NAMES:
        log = []
        drive(ModelBackend(), script(name), log=log)
        assert len(log) == len(script(name)["ops"]) and log == record(ModelBackend(), script(name))


def test_sync_seam_method(models):
    """confirmable(H) is a prefix of o.chunk_stream of the rest of the data,
    and equals the whole stream's cuts <= H (H itself when it is a cut), at
    every SYNC point of every script."""
    points = 0
    for name, m in models.items():
        data = script(name)["data"]
        for key, prm, origin, fed in sorted(set(m.sync_points)):
            if fed <= origin:
                continue
            arr = data[key]
            conf = [origin + x for x in sr.confirmable_of(arr[origin:fed], prm)]
            rest = [origin + x for x in sr.final_of(arr[origin:], prm)]
            assert conf == rest[:len(conf)], (name, key, origin, fed)
            ext = np.concatenate([arr[origin:], np.zeros(2 * prm[2], np.uint8)])
            whole = [origin + x for x in sr.final_of(ext, prm)]
            assert conf == [c for c in whole if c <= fed], (name, key, origin, fed)
            points += 1
    assert points > 250


# ---- every script holds what it exists for -------------------------------------------------------
def test_s1_conditions(models):
    m, prm = models["S1"], sr.SMALL
    c = m.c
    assert c["sync_on_hash_cut"] == 3 and c["sync_on_max_cut"] == 2, c
    assert c["sync_before_cut"] >= 5 and c["sync_after_cut"] >= 5, c
    assert c["flush"] + c["adv_zero"] + c["adv_exact"] + c["adv_past"] == 15, c   # one restart per case
    assert c["flush"] == 5 and c["adv_past"] == 5, c
    assert set(sr.odd_sizes(prm)) <= m.sizes and sr.odd_sizes(prm) == (0, 1, 47, 48, 49, 63, 1024, 1025)
    assert len(script("S1")["data"]["d"]) > 1 << 20 and m.c["pop_many_ids"] == 0


@pytest.mark.parametrize("seed,prm,total", sr.S2_CASES)
def test_s2_conditions(models, seed, prm, total):
    sc, m = script(f"S2-{seed}"), models[f"S2-{seed}"]
    assert 150 <= len(sc["ops"]) <= 160 and abs(len(sc["data"]["d"]) - total) < 64
    kinds = {op["op"] for op in sc["ops"]}
    assert {"begin", "end", "push", "fill", "pop", "pop_many", "drain", "unpop", "advance", "flush", "ids"} <= kinds
    assert m.caps <= {0, 1, 2, 7, 128} and len(m.caps) >= 3, m.caps
    assert m.c["want_gt_n"] >= 1 and m.c["flush"] >= 1, m.c
    assert m.c["refused_ids"] + m.c["refused_begin"] + m.c["refused_pop_many_ids"] >= 2, m.c


def test_s2_together(models):
    c = {k: sum(models[f"S2-{s}"].c[k] for s, _, _ in sr.S2_CASES) for k in sr.COUNTERS}
    assert c["unpop_mid"] >= 2 and c["pop_after_unpop"] >= 2, c
    assert c["pop_many_ids"] >= 10 and c["pop_many_no_ids"] >= 5 and c["pop_many_plain"] >= 10, c
    assert c["refused_ids"] and c["refused_begin"] and c["refused_pop_many_ids"], c
    assert c["adv_zero"] + c["adv_zero_ids"] >= 2 and c["adv_inside"] + c["adv_inside_ids"] >= 2, c
    assert c["adv_past"] + c["adv_past_ids"] + c["adv_past_3max"] + c["adv_past_3max_ids"] >= 2, c
    assert c["ids_toggle_at_restart"] >= 2, c


@pytest.mark.parametrize("algo", (sr.SHA512_256, sr.SHA256))
def test_s3_conditions(models, algo):
    m = models[f"S3-{algo}"]
    c = m.c
    assert c["chunk_3_batches_ids"] >= 8, c          # the chunks of the two zero runs, 20 KiB per batch
    assert c["single_byte_batch"] >= 1, c
    assert c["pop_many_ids"] >= 5 and c["pop_many_no_ids"] >= 5, c
    assert c["ids_on"] == 3 and c["ids_off"] == 1 and c["ids_toggle_at_restart"] == 2, c
    assert c["flush"] == 2 and c["adv_exact"] + c["adv_zero"] == 1, c
    assert c["refused_ids"] >= 1 and c["unpop_mid"] + c["unpop_start"] >= 1 and c["pop_after_unpop"] >= 1, c
    algos = [op["algo"] for op in script(f"S3-{algo}")["ops"] if op["op"] == "ids"]
    assert {0, 1, -1} == set(algos)                  # both digests in either script
    assert 2.5 * (1 << 20) < len(script(f"S3-{algo}")["data"]["d"]) <= 3 << 20


def test_s4_conditions(models):
    m = models["S4"]
    c = m.c
    for tag in ("", "_ids"):
        for k in ("adv_zero", "adv_inside", "adv_exact", "adv_past_1", "adv_past_3max", "adv_eof_inside",
                  "adv_eof_past", "adv_before_first", "adv_after_unpop"):
            assert c[k + tag] >= 1, (k + tag, c)
        assert c["adv_past_1" + tag] == 2 and c["adv_past_3max" + tag] == 3, c
    assert m.skip_commits == {1, 2, 5}               # the skipped bytes over 1, 2 and 5 commits
    assert c["adv_on_pending_skip"] == 4 and c["unpop_mid"] >= 2 and c["want_gt_n"] >= 2, c


def test_s5_conditions(models):
    c = models["S5"].c
    assert c["eof_after_sync_all"] == 3 and c["eof_after_sync_all_ids"] == 6, c   # (two of each on a forced cut)
    assert c["eof_one_byte"] == 3 and c["empty_stream"] == 3 and c["shorter_than_min"] == 3, c
    assert c["sync_on_max_cut"] == 3 and c["begin_after_done"] >= 3, c
    for k in ("push", "fill", "buffer", "commit"):
        assert c["refused_after_eof_" + k] == 9, (k, c)
    ops = script("S5")["ops"]
    assert sum(op["op"] == "done" for op in ops) >= 30


def test_s6_conditions(models):
    c = models["S6"].c
    ops = script("S6")["ops"]
    assert [tuple(op["params"]) for op in ops if op["op"] == "begin"] == \
        [sr.DEFAULT, sr.SMALL, sr.SMALL, sr.DEFAULT, sr.SMALL]
    assert c["begin"] == 3 and c["refused_begin"] == 2 and c["begin_after_done"] == 1, c
    assert c["begin_other_params"] == 1 and c["ids_on"] == 1 and c["pop_many_ids"] >= 19, c
    first_end = [op["op"] for op in ops].index("end")
    assert [op["op"] for op in ops[first_end:first_end + 4]] == ["end", "begin", "ids", "fill"]
    # the second stream's first batch has 70 times the cuts of the first stream's largest (2 MiB)
    assert ops[first_end + 3]["n"] // sr.SMALL[0] > 70 * ((1 << 21) // sr.DEFAULT[0])


def test_s7_conditions(models):
    sc = script("S7")
    ops = sc["ops"]
    assert len(sc["data"]["p"]) == (44 << 20) + 13
    feeds = [op for op in ops if op["op"] in ("push", "fill")]
    assert all(1 << 20 <= op["n"] <= 3 << 20 for op in feeds if op["lo"] + op["n"] < (44 << 20) + 13)
    assert sum(op["op"] == "fill" for op in ops) == 1  # the one SYNC, right before the 32 MiB buffer overflows
    i = next(i for i, op in enumerate(ops) if op["op"] == "fill")
    nxt = next(op for op in ops[i + 1:] if op["op"] == "push")
    assert ops[i]["lo"] + ops[i]["n"] <= 4 * sr.BATCH < nxt["lo"] + nxt["n"]
    second = [op["op"] for op in ops].index("end") + 1
    assert ops[second]["op"] == "begin"
    first_drain = next(i for i in range(second, len(ops)) if ops[i]["op"] == "drain")
    assert ops[first_drain - 1]["lo"] + ops[first_drain - 1]["n"] >= 40 << 20 > ops[first_drain - 1]["lo"]


@pytest.mark.parametrize("algo", (-1, sr.SHA512_256))
def test_s8_conditions(models, algo):
    sc = script(f"S8-{algo}")
    ops = [op["op"] for op in sc["ops"]]
    i = ops.index("dense_mark")
    assert ops[i - 2:i + 3] == ["fill", "drain", "dense_mark", "fill", "dense_check"]
    assert sc["ops"][i - 2]["flags"] == sr.F_SYNC and sc["ops"][i - 2]["n"] == 1 << 20
    assert sc["ops"][i + 1]["lo"] == 1 << 20 and sc["ops"][i + 1]["n"] == (3 << 20) // 48 * 48
    assert ("ids" in ops) == (algo >= 0)


# ---- the driver must be able to fail -------------------------------------------------------------
class ConfirmsFedEarly(ModelBackend):
    """A non-final scan that ends the chain's open chunk at the fed position."""

    def confirmed(self, arr):
        cuts = super().confirmed(arr)
        return cuts if cuts and cuts[-1] == len(arr) else cuts + [len(arr)]


class UnpopLosesIds(ModelBackend):
    """An unpop that queues the cuts again without their IDs."""

    def requeue_id(self, cid):
        pass


class ForgetsSkip(ModelBackend):
    """An Advance beyond the held bytes whose debt the first commit clears."""

    def dropped(self, n):
        d = super().dropped(n)
        self.skip = 0
        return d


class StaleFlushId(ModelBackend):
    """A flush that leaves the ID of the last popped chunk in place."""

    def flush_id(self):
        return self.last_id if self.has_id else None


MUTATIONS = {
    "confirms_fed_early": (ConfirmsFedEarly, sr.NAMES),
    "unpop_loses_ids": (UnpopLosesIds, ["S3-0", "S3-1", "S4", "S6", "S8-0"]),
    "forgets_skip": (ForgetsSkip, ["S4"]),
    "stale_flush_id": (StaleFlushId, ["S2-2", "S2-4", "S3-0", "S3-1"]),
}
CASES = [(m, name) for m, (_, names) in sorted(MUTATIONS.items()) for name in names if name != "S7"]


@pytest.mark.parametrize("mutation,name", CASES)
def test_driver_detects_a_broken_stream(mutation, name):
    """The first op at which the broken stream's results differ from the true
    one's (both recorded without the model) is the op the driver names."""
    sc = script(name)
    true, broken = record(ModelBackend(), sc), record(MUTATIONS[mutation][0](), sc)
    want = next(i for i, (a, b) in enumerate(zip(true, broken)) if a != b)
    with pytest.raises(Mismatch) as e:
        drive(MUTATIONS[mutation][0](), sc)
    assert e.value.pos == want, str(e.value)
    text = str(e.value)
    assert f"{name}, op {want}:" in text and "last five ops:" in text
    assert f"[{want}] " + sr.describe(sc["ops"][want]) in text
