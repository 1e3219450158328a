"""bench.py --dump-outputs: the sample written is the lists themselves, in
topic order, whatever positions the call put them at (the pairs form leaves
gaps and places the spans in launch order), and stays inside its budget."""
import numpy as np
import torch

import bench


def _case(n=1000, seed=1):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 7, n)
    lists = [rng.integers(0, 2**32, c, dtype=np.uint64).astype(np.uint32) for c in cnt]
    buf = np.zeros(int(cnt.sum()) + 3 * n, np.uint32)
    starts = np.zeros(n, np.int64)
    p = 0
    for i in rng.permutation(n):   # spans out of topic order, a gap before each
        p += 3
        starts[i] = p
        buf[p:p + cnt[i]] = lists[i]
        p += cnt[i]
    err = (rng.integers(0, 50, n) == 0).astype(np.uint8)
    return cnt, lists, starts, buf, err


def test_dump_outputs_sample_is_the_lists_in_topic_order(tmp_path, monkeypatch):
    cnt, lists, starts, buf, err = _case()
    n, half = len(cnt), len(cnt) // 2
    v = torch.from_numpy(buf.view(np.int32))
    parts = [(torch.from_numpy(starts[lo:hi]), torch.from_numpy(cnt[lo:hi]), v, torch.from_numpy(err[lo:hi]))
             for lo, hi in ((0, half), (half, n))]   # two sub-batches of one step
    seen = []
    for budget in (bench.DUMP_VALUES, 500):
        monkeypatch.setattr(bench, "DUMP_VALUES", budget)
        d = tmp_path / str(budget)
        bench.dump_outputs(str(d), parts, int(cnt.sum()))
        got = {f.stem: np.load(f) for f in d.iterdir()}
        assert sorted(got) == ["counts", "err", "topics", "total_hits", "values"]
        idx = got["topics"].astype(np.int64)
        assert (np.diff(idx) > 0).all() and got["values"].size <= budget
        assert np.array_equal(got["counts"], cnt[idx].astype(np.float64))
        assert np.array_equal(got["values"], np.concatenate([lists[i] for i in idx]).astype(np.float64))
        assert np.array_equal(got["err"], err[idx].astype(np.float32))
        assert got["values"].dtype == np.float64 and got["err"].dtype == np.float32
        assert got["total_hits"].tolist() == [float(cnt.sum())]
        seen.append(idx)
    assert seen[0].size == n and 0 < seen[1].size < n
    assert np.isin(seen[1], seen[0]).all()
    # the same arguments give the same sample
    bench.dump_outputs(str(tmp_path / "again"), parts, int(cnt.sum()))
    assert np.array_equal(np.load(tmp_path / "again" / "topics.npy"), seen[1].astype(np.float64))
