"""The post-pass kernels driven directly: k_segsort_small / k_segsort_big
(tm_sort_segments) and k_merge_shards (tm_merge_shards) on synthetic CSRs
built in numpy, exact against numpy -- no index content involved.

The sort has four size regimes (tm_kernels.hip): one lane per segment up to
SS_SMALL = 32 values; a bitonic sort in LDS up to SS_LDS = 8192; LDS-sorted
chunks plus one merge level in global memory up to 16384; above that the global
half-cleaner loop.  The lengths below sit on both sides of every threshold and
of the powers of two in between, with full-range u32 values (a signed compare
sorts 0x80000000 before 0x7FFFFFFF).  More long segments than the big kernel's
grid (SS_GRID_BIG = 512) make its blocks loop; a run with no long segment
between two with many checks the device-side list counter's reset.

The merge stages the shards' offsets in LDS for up to MERGE_LDS_WORLD = 16
shards and reads them in place beyond that; one wave takes MERGE_TOPICS = 16
topics, so n around the multiples of 16 puts the final offset in a wave of its
own (t0 == n) or at a wave's end (t1 == n).

References: np.sort per segment; for TM_ORDER_UNIQUE np.unique per segment,
then 0xFFFFFFFF padding, plus the distinct count (test_gpu_parity._sorted_ref's
contract); test_gpu_parity._merge_ref for the merge.
"""
import numpy as np
import pytest

from emqx_amd import _native, shard
from test_gpu_parity import _merge_ref

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF
EDGES = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE)
CANARY = 0xC0FFEE11
LENGTHS = (0, 1, 2, 31, 32, 33, 34, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 16383, 16384,
           16385, 24577, 32768, 32769, 70001)
FILLS = ("random", "ascending", "descending", "equal", "seven")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def index(torch_dev):
    """an empty index: tm_sort_segments needs a handle for its workspace only"""
    return _native.Index()


# ------------------------------------------------------------------ the sort

def _fill(rng, length, kind, with_pad):
    """`length` u32 values of one fill; the signed-range edges are in every fill that has room for them"""
    top = PAD if with_pad else PAD - 1
    if kind == "equal":
        return np.full(length, EDGES[length % 4] if length % 5 else top, np.uint32)
    if kind == "seven":
        pool = np.array(list(EDGES) + [top, 0x7FFFFFFE, 0x80000001], np.uint32)
        return pool[rng.integers(0, 7, length)]
    v = rng.integers(0, top + 1, length, dtype=np.uint64).astype(np.uint32)
    spots = rng.permutation(length)[:5]
    v[spots] = np.array(list(EDGES) + [top], np.uint32)[:len(spots)]
    if kind == "ascending":
        v = np.sort(v)
    elif kind == "descending":
        v = np.sort(v)[::-1].copy()
    return v


def _csr(segments):
    hit = np.zeros(len(segments) + 1, np.uint64)
    hit[1:] = np.cumsum([len(s) for s in segments], dtype=np.uint64)
    vals = np.concatenate(segments).astype(np.uint32) if segments else np.zeros(0, np.uint32)
    return hit, vals


def _ref(hit, vals, n, cap, unique):
    """The contract: every segment t < n that ends at or below cap sorted
    (UNIQUE: its distinct values, then padding; the distinct count), every
    other value unchanged and a count of 0 for a segment ending beyond cap."""
    out = vals.copy()
    cnt = np.zeros(n, np.uint32)
    for t in range(n):
        o, e = int(hit[t]), int(hit[t + 1])
        if e > cap:
            continue
        seg = np.sort(vals[o:e])
        if unique:
            u = np.unique(seg)
            cnt[t] = len(u)
            seg = np.concatenate([u, np.full(len(seg) - len(u), PAD, np.uint32)])
        out[o:e] = seg
    return out, cnt


def _run_sort(torch, ix, hit, vals, n, cap, order, tail=64):
    """tm_sort_segments on device copies -> (the whole value buffer with its
    canary tail, the counts with theirs or None)"""
    d_hit = torch.from_numpy(hit.view(np.int64).copy()).cuda()
    buf = np.concatenate([vals, np.full(tail, CANARY, np.uint32)])
    d_vals = torch.from_numpy(buf.view(np.int32).copy()).cuda()
    d_cnt = None
    if order == _native.TM_ORDER_UNIQUE:
        d_cnt = torch.full((n + tail,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.sort_segments(n, d_hit.data_ptr(), d_vals.data_ptr(), cap, order, None if d_cnt is None else d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_hit.cpu().numpy().view(np.uint64), hit), "the offsets were written"
    return d_vals.cpu().numpy().view(np.uint32), None if d_cnt is None else d_cnt.cpu().numpy().view(np.uint32)


def _check_sort(torch, ix, hit, vals, n, cap, what):
    """SORTED and UNIQUE of one CSR, exact, canaries included"""
    got, _ = _run_sort(torch, ix, hit, vals, n, cap, _native.TM_ORDER_SORTED)
    exp, _ = _ref(hit, vals, n, cap, False)
    total = len(vals)
    bad = np.nonzero(got[:total] != exp)[0]
    assert len(bad) == 0, f"{what} SORTED: {len(bad)} values differ, first at {bad[0]} " \
                          f"(segment {np.searchsorted(hit, bad[0], 'right') - 1})"
    assert (got[total:] == CANARY).all(), f"{what} SORTED: wrote past the values"
    got, cnt = _run_sort(torch, ix, hit, vals, n, cap, _native.TM_ORDER_UNIQUE)
    exp, ecnt = _ref(hit, vals, n, cap, True)
    bad = np.nonzero(got[:total] != exp)[0]
    assert len(bad) == 0, f"{what} UNIQUE: {len(bad)} values differ, first at {bad[0]} " \
                          f"(segment {np.searchsorted(hit, bad[0], 'right') - 1})"
    assert (got[total:] == CANARY).all(), f"{what} UNIQUE: wrote past the values"
    assert np.array_equal(cnt[:n], ecnt), f"{what} UNIQUE: distinct counts differ"
    assert (cnt[n:] == 7).all(), f"{what} UNIQUE: wrote past the counts"


def _threshold_segments(with_pad):
    rng = np.random.default_rng(0x5E65)
    segs = [_fill(rng, n, kind, with_pad) for n in LENGTHS for kind in FILLS]
    order = rng.permutation(len(segs))
    return [segs[i] for i in order]


def test_sort_every_size_regime_and_fill(torch_dev, index):
    """every length in LENGTHS with every fill, segments in shuffled order"""
    for with_pad, order in ((True, _native.TM_ORDER_SORTED), (False, _native.TM_ORDER_UNIQUE)):
        segs = _threshold_segments(with_pad)
        hit, vals = _csr(segs)
        n, total = len(segs), len(vals)
        assert sorted(len(s) for s in segs) == sorted(LENGTHS * len(FILLS))
        for e in EDGES + ((PAD,) if with_pad else ()):
            assert (vals == e).any()
        assert with_pad or not (vals == PAD).any()
        got, cnt = _run_sort(torch_dev, index, hit, vals, n, total, order)
        exp, ecnt = _ref(hit, vals, n, total, order == _native.TM_ORDER_UNIQUE)
        for t in range(n):   # segment by segment, to name the length that failed
            o, e = int(hit[t]), int(hit[t + 1])
            assert np.array_equal(got[o:e], exp[o:e]), f"order {order}: segment {t} of {e - o} values differs"
        assert (got[total:] == CANARY).all(), "wrote past hit[n]"
        if cnt is not None:
            assert np.array_equal(cnt[:n], ecnt) and (cnt[n:] == 7).all()
    # UNIQUE's input run through SORTED too (and the other way round is not
    # possible: 0xFFFFFFFF is UNIQUE's padding)
    _check_sort(torch_dev, index, hit, vals, n, total, "no-pad set")


def _many_long(seed, n_long=600, n_short=2000):
    """n_long segments of 33-40 values among n_short of 0-32: more long segments than SS_GRID_BIG;
    segment 0 is a long one"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(33, 41, n_long), rng.integers(0, 33, n_short)])
    rng.shuffle(lens)
    first_long = int(np.nonzero(lens > 32)[0][0])
    lens[0], lens[first_long] = lens[first_long], lens[0]
    kinds = ("random", "random", "seven", "descending")
    return [_fill(rng, int(c), kinds[i % 4], False) for i, c in enumerate(lens)]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2600])
def test_sort_more_long_segments_than_blocks(torch_dev, index, n):
    """600 long segments (> SS_GRID_BIG: the big kernel's blocks loop) among
    2,000 short ones, the first n segments sorted: the rest stays as it was"""
    segs = _many_long(11)
    hit, vals = _csr(segs)
    assert len(segs) == 2600 and sum(len(s) > 32 for s in segs) == 600 and len(segs[0]) > 32
    got, _ = _run_sort(torch_dev, index, hit, vals, n, len(vals), _native.TM_ORDER_SORTED)
    assert np.array_equal(got[int(hit[n]):len(vals)], vals[int(hit[n]):]), "segments past n were touched"
    _check_sort(torch_dev, index, hit, vals, n, len(vals), f"n = {n}")


def test_sort_list_counter_resets_between_runs(torch_dev, index):
    """many long segments, none, many again on one index and stream: the last
    block of the big kernel resets the device-side list of long segments"""
    rng = np.random.default_rng(5)
    none = _csr([_fill(rng, int(c), "random", False) for c in rng.integers(0, 33, 2000)])
    for k, (hit, vals) in enumerate((_csr(_many_long(21)), none, _csr(_many_long(22)), none, _csr(_many_long(23, 513, 100)))):
        _check_sort(torch_dev, index, hit, vals, len(hit) - 1, len(vals), f"run {k}")


def test_sort_cap_leaves_later_segments_alone(torch_dev, index):
    """cap = hit[k]: segments ending at or below cap are sorted, every segment
    ending beyond it is unchanged with a distinct count of 0; short and long
    segments (every regime) on both sides of k.  TM_ORDER_TRAVERSAL leaves
    the whole buffer unchanged."""
    rng = np.random.default_rng(9)
    segs = _many_long(31, 40, 120)
    for at in (5, 60, 100, 150):
        segs.insert(at, _fill(rng, 9000, "random", False))
        segs.insert(at + 1, _fill(rng, 20000, "descending", False))
    hit, vals = _csr(segs)
    n = len(segs)
    for k in (n // 2, 62, 6, n - 1):
        cap = int(hit[k])
        assert 0 < cap < len(vals)
        got, cnt = _run_sort(torch_dev, index, hit, vals, n, cap, _native.TM_ORDER_UNIQUE)
        beyond = np.nonzero(hit[1:] > cap)[0]
        assert len(beyond) and (cnt[beyond] == 0).all()
        lo = int(hit[beyond[0]])
        assert np.array_equal(got[lo:len(vals)], vals[lo:]), f"cap = hit[{k}]: a segment ending beyond cap changed"
        _check_sort(torch_dev, index, hit, vals, n, cap, f"cap = hit[{k}]")
    got, _ = _run_sort(torch_dev, index, hit, vals, n, len(vals), _native.TM_ORDER_TRAVERSAL)
    assert np.array_equal(got[:len(vals)], vals) and (got[len(vals):] == CANARY).all()


# ----------------------------------------------------------------- the merge

MERGE_LENS = (0, 0, 1, 63, 64, 65, 200)


def _shards(seed, world, n):
    """-> (all_offs i64 [world, n+1], all_vals i32 [world, stride], stride):
    per-(shard, topic) lengths from MERGE_LENS, some shards entirely empty (world >= 3),
    full-range values, stride larger than any shard's total"""
    rng = np.random.default_rng(seed)
    lens = np.array(MERGE_LENS)[rng.integers(0, len(MERGE_LENS), (world, n))] if n else np.zeros((world, 0), np.int64)
    if world > 2:   # (two shards stay both live: their order in the merged list is then checked)
        lens[rng.permutation(world)[:max(world // 4, 1)]] = 0
    all_offs = np.zeros((world, n + 1), np.int64)
    all_offs[:, 1:] = np.cumsum(lens, axis=1)
    stride = int(all_offs[:, -1].max()) + 5
    all_vals = rng.integers(0, 1 << 32, (world, stride), dtype=np.uint64).astype(np.uint32)
    all_vals[0, :4][:min(stride, 4)] = np.array(EDGES, np.uint32)[:min(stride, 4)]
    return all_offs, all_vals.view(np.int32), stride


def _run_merge(torch, all_offs, all_vals, stride, cap, null_out=False, tail=32):
    """tm_merge_shards on device copies -> (out_hit with its canary tail,
    out values with theirs: `cap` slots then the tail)"""
    world, n1 = all_offs.shape
    d_offs = torch.from_numpy(all_offs.copy()).cuda()
    d_vals = torch.from_numpy(all_vals.copy()).cuda()
    d_hit = torch.full((n1 + tail,), -77, dtype=torch.int64, device="cuda")
    d_out = torch.from_numpy(np.full(cap + tail, CANARY, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    _native.merge_shards(world, n1 - 1, d_offs.data_ptr(), d_vals.data_ptr(), stride, d_hit.data_ptr(),
                         None if null_out else d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_hit.cpu().numpy(), d_out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("world", [1, 2, 3, 8, 15, 16, 17, 33])
def test_merge_worlds_and_wave_boundaries(torch_dev, world):
    """offsets staged in LDS (world <= 16) and read in place (17, 33), n around
    the multiples of MERGE_TOPICS: all n + 1 offsets and every value exact"""
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000):
        all_offs, all_vals, stride = _shards(1000 * world + n, world, n)
        assert stride > all_offs[:, -1].max() and (world < 3 or (all_offs[:, -1] == 0).any())
        r_hit, r_vals = _merge_ref(all_offs, all_vals)
        total = int(r_hit[-1])
        hit, out = _run_merge(torch_dev, all_offs, all_vals, stride, total)
        assert np.array_equal(hit[:n + 1], r_hit), f"world {world} n {n}: offsets differ"
        assert (hit[n + 1:] == -77).all(), f"world {world} n {n}: wrote past out_hit[n]"
        assert np.array_equal(out[:total], r_vals.view(np.uint32)), f"world {world} n {n}: values differ"
        assert (out[total:] == CANARY).all(), f"world {world} n {n}: wrote past the total"


@pytest.mark.parametrize("world", [3, 17])
def test_merge_cap_truncates(torch_dev, world):
    """cap below the total: out_hit is complete, the values below cap are
    exact, nothing at or beyond cap is written (cap 0 with a null out too)"""
    n = 70
    all_offs, all_vals, stride = _shards(77 + world, world, n)
    r_hit, r_vals = _merge_ref(all_offs, all_vals)
    total = int(r_hit[-1])
    mid = n // 2 + int(np.argmax(np.diff(r_hit)[n // 2:] > 7))   # a topic with room for a cap inside its list
    inside = int(r_hit[mid]) + 7
    assert total > 200 and r_hit[mid] < inside < r_hit[mid + 1]
    for cap, null_out in ((0, True), (0, False), (1, False), (inside, False), (total - 1, False), (total, False)):
        hit, out = _run_merge(torch_dev, all_offs, all_vals, stride, cap, null_out)
        assert np.array_equal(hit[:n + 1], r_hit) and (hit[n + 1:] == -77).all(), f"cap {cap}: offsets"
        if null_out:
            assert (out == CANARY).all()
            continue
        assert np.array_equal(out[:cap], r_vals.view(np.uint32)[:cap]), f"cap {cap}: values below cap differ"
        assert (out[cap:] == CANARY).all(), f"cap {cap}: wrote at or beyond cap"


def test_merge_then_sort_world_17(torch_dev, index):
    """shard.merge, then tm_sort_segments on the merged CSR == np.sort of each
    topic's concatenated lists"""
    torch = torch_dev
    world, n = 17, 100
    all_offs, all_vals, stride = _shards(4242, world, n)
    m_hit, m_vals = shard.merge(torch.from_numpy(all_offs).cuda(), torch.from_numpy(all_vals).cuda(), stride)
    torch.cuda.synchronize()
    index.sort_segments(n, m_hit.data_ptr(), m_vals.data_ptr(), m_vals.numel())
    torch.cuda.synchronize()
    u = all_vals.view(np.uint32)
    exp = [np.sort(np.concatenate([u[r, all_offs[r, t]:all_offs[r, t + 1]] for r in range(world)])) for t in range(n)]
    e_hit, e_vals = _csr(exp)
    assert max(len(s) for s in exp) > 32 * 17
    assert np.array_equal(m_hit.cpu().numpy().view(np.uint64), e_hit)
    assert np.array_equal(m_vals.cpu().numpy().view(np.uint32)[:len(e_vals)], e_vals)
