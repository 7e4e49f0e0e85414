"""oracle/seam.py's shard_local with the blob's candidates handed in (cands=:
one o.candidates call for many shards, and the C chain rule for a shard that
ends the blob) is shard_local's plain path: the same record, chain and
candidate list, over a spread of starts, shards that end the blob and shards
that end inside it.  tests/test_gpu_seam_record.py's tiling relies on it."""
import numpy as np
import pytest

from oracle import oracle as o
from oracle import seam as oseam


@pytest.mark.parametrize("prm", [(48, 256, 8192), (1024, 4096, 16384), (16 << 10, 64 << 10, 256 << 10)])
def test_shard_local_with_blob_candidates(prm):
    mn, av, mx = prm
    data = o.synth_uniform(21, 0, (2 << 20) + 777)
    total = data.size
    cands = o.candidates(data, mn, av, mx)
    starts = [0, 1, 47, 48, 49, 63, 64, 65, 4097, 53305, int(cands[3]), int(cands[3]) - 1,
              total // 2 + 3, total - 100000, total - mn - 1, total - mn, total - 1, total]
    for start in starts:
        for length in sorted({total - start, min(total - start, 300001), min(total - start, mn), 0}):
            want = oseam.shard_local(data, start, length, total, mn, av, mx)
            got = oseam.shard_local(data, start, length, total, mn, av, mx, cands=cands)
            assert got[0] == want[0], (start, length)
            assert list(got[1]) == list(want[1]), (start, length)
            assert np.array_equal(got[2], want[2]), (start, length)
