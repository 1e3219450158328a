"""tm_aggre_dev driven directly: synthetic bucketed (topic, value) arrays built
in numpy, exact against the numpy definition in include/tmatch.h -- no index
content involved (the pattern of test_gpu_fanout.py).

The pass runs on G = TM_DEBUG_FANOUT_GRID one-wave blocks; block k owns the
positions [k * chunk, (k + 1) * chunk), chunk = ceil(E / G) rounded up to 64,
E = min(dest_offsets[n_dests + 1], cap).  Up to E = 64 G a block owns one
64-entry step, so a pair at positions 63 / 64 straddles two blocks; from
64 G + 1 on the chunk is 128: 63 / 64 then straddles two steps of block 0 and
127 / 128 two blocks.  The inputs hold exactly E entries (one spare word keeps
an empty tensor from being a null pointer), every output buffer is filled with
a sentinel that must survive at and past K, and the inputs are compared after
the run.
"""
import numpy as np
import pytest

from emqx_amd import _native

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CANARY = 0xC0FFEE11
OFFS_CANARY = -77
TAIL = 64


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def index(torch_dev):
    """an empty index: tm_aggre_dev needs a handle for its scratch (and its own table) only"""
    ix = _native.Index()
    yield ix
    torch_dev.cuda.synchronize()
    ix.close()


@pytest.fixture(scope="module")
def G(index):
    g = index.debug_get(_native.TM_DEBUG_FANOUT_GRID)
    assert g >= 64 and g % 64 == 0
    return g


# ------------------------------------------------------------- the reference

def _ref(doff, t, v, cap, fof, n_dests):
    """the header's numpy definition -> (out_doff u64[n_dests + 2], topic u32[K], value u32[K])"""
    doff = doff.astype(np.int64)
    E = min(int(doff[n_dests + 1]), cap)
    t, v = t[:E], v[:E]
    f = np.full(E, NONE, np.uint32)
    inr = v.astype(np.int64) < len(fof)
    f[inr] = fof[v[inr]]
    keep = np.ones(E, bool)
    if E > 1:
        keep[1:] = ~((t[1:] == t[:-1]) & (f[1:] == f[:-1]) & (f[1:] != NONE))
    heads = doff[:n_dests + 1]
    keep[heads[heads < E]] = True
    keep[min(int(doff[n_dests]), E):] = True
    before = np.concatenate([[0], np.cumsum(keep)])
    return before[np.minimum(doff, E)].astype(np.uint64), t[keep], v[keep]


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def _dev(torch, a):
    return torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)]).view(np.int32 if a.itemsize == 4 else np.int64)).cuda()


class Run:
    """one tm_aggre_dev call's device buffers (kept alive until checked)"""

    def __init__(self, torch, ix, doff, t, v, n_dests, fof, cap=None, stream=None):
        doff = np.asarray(doff, np.uint64)
        t, v = np.asarray(t, np.uint32), np.asarray(v, np.uint32)
        assert len(doff) == n_dests + 2 and len(t) == len(v)
        cap = len(t) if cap is None else cap
        E = min(int(doff[-1]), cap)
        assert E <= len(t)
        t, v = t[:E].copy(), v[:E].copy()   # no position at or past E exists
        self.torch, self.args, self.E = torch, (doff, t, v, cap, fof, n_dests), E
        with torch.cuda.stream(stream) if stream is not None else _Null():
            self.d_doff, self.d_t, self.d_v = _dev(torch, doff), _dev(torch, t), _dev(torch, v)
            self.d_fof = None if fof is None else _dev(torch, np.asarray(fof, np.uint32))
            self.o_doff = torch.full((n_dests + 2 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.o_t = torch.from_numpy(np.full(E + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
            self.o_v = torch.from_numpy(np.full(E + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
            ix.aggre_dev(n_dests, self.d_doff.data_ptr(), self.d_t.data_ptr(), self.d_v.data_ptr(), cap,
                         self.o_doff.data_ptr(), self.o_t.data_ptr(), self.o_v.data_ptr(),
                         None if fof is None else self.d_fof.data_ptr(), 0 if fof is None else len(fof),
                         torch.cuda.current_stream().cuda_stream)

    def check(self, what, table=None):
        """exact outputs, sentinels at and past K, inputs unmodified -> K"""
        doff, t, v, cap, fof, n_dests = self.args
        self.torch.cuda.synchronize()
        e_doff, e_t, e_v = _ref(doff, t, v, cap, np.asarray(fof if table is None else table, np.uint32), n_dests)
        K = len(e_t)
        g_doff = self.o_doff.cpu().numpy()
        g_t, g_v = self.o_t.cpu().numpy().view(np.uint32), self.o_v.cpu().numpy().view(np.uint32)
        assert np.array_equal(g_doff[:n_dests + 2].view(np.uint64), e_doff), f"{what}: bucket offsets differ"
        assert int(e_doff[-1]) == K
        assert (g_doff[n_dests + 2:] == OFFS_CANARY).all(), f"{what}: wrote past out_dest_offsets[n_dests + 1]"
        bad = np.nonzero((g_t[:K] != e_t) | (g_v[:K] != e_v))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {K} entries differ, first at {bad[0]}"
        assert (g_t[K:] == CANARY).all() and (g_v[K:] == CANARY).all(), f"{what}: wrote at or past K"
        assert np.array_equal(self.d_doff.cpu().numpy().view(np.uint64)[:-1], doff), f"{what}: the offsets were written"
        assert np.array_equal(self.d_t.cpu().numpy().view(np.uint32)[:-1], t), f"{what}: the topics were written"
        assert np.array_equal(self.d_v.cpu().numpy().view(np.uint32)[:-1], v), f"{what}: the values were written"
        return K


# ---------------------------------------------------------------- the inputs

def _doff(sizes):
    d = np.zeros(len(sizes) + 1, np.uint64)
    d[1:] = np.cumsum(np.asarray(sizes, np.int64), dtype=np.uint64)
    return d


def _runs(lengths, none_every=0):
    """entries in runs: run r has topic r // 3 and filter r (so neighbouring runs
    never compare equal), value p names filter_of[p]; -> (t, v, filter_of)"""
    lengths = np.asarray(lengths, np.int64)
    r = np.repeat(np.arange(len(lengths)), lengths)
    fof = r.astype(np.uint32)
    if none_every:
        fof[r % none_every == none_every - 1] = NONE
    return (r // 3).astype(np.uint32), np.arange(len(r), dtype=np.uint32), fof


def _random(E, n_dests, seed, empty_ends=0):
    """E entries in random runs of 1 .. 5 (a few long), one run in eight without a filter, the
    values a permutation, the bucket bounds random (duplicates cross them) with empty buckets
    at both ends"""
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < E:
        lens.append(int(rng.choice([1, 1, 1, 2, 3, 5, 70])))
    t, _, fof_by_pos = _runs(lens, none_every=8)
    t, fof_by_pos = t[:E], fof_by_pos[:E]
    v = rng.permutation(E).astype(np.uint32)
    fof = np.zeros(E, np.uint32)
    fof[v] = fof_by_pos
    used = max(n_dests + 1 - 2 * empty_ends, 1)
    cuts = np.sort(rng.integers(0, E + 1, used - 1)) if used > 1 else np.zeros(0, np.int64)
    inner = np.diff(np.concatenate([[0], cuts, [E]]))
    lead = min(empty_ends, n_dests + 1 - used)
    sizes = np.concatenate([np.zeros(lead, np.int64), inner, np.zeros(n_dests + 1 - used - lead, np.int64)])
    return _doff(sizes), t, v, fof


# ------------------------------------------------------------------ the tests

def test_entry_counts_around_steps_and_chunks(torch_dev, index, G):
    for E in (0, 1, 63, 64, 65, 64 * G - 1, 64 * G, 64 * G + 1):
        doff, t, v, fof = _random(E, 3, seed=E)
        K = Run(torch_dev, index, doff, t, v, 3, fof).check(f"E={E}")
        assert E == 0 or 0 < K <= E and (E < 60 or K < E)


def test_pairs_straddling_steps_and_blocks(torch_dev, index, G):
    for E, at in ((200, 64), (64 * G, 64), (64 * G, 64 * (G - 1)), (64 * G + 1, 64), (64 * G + 1, 128),
                  (64 * G + 1, 64 * G)):
        lens = np.ones(E - 1, np.int64)
        lens[at - 1] = 2            # the run covers positions at - 1 and at
        t, v, fof = _runs(lens)
        assert len(t) == E and fof[at] == fof[at - 1] and t[at] == t[at - 1]
        K = Run(torch_dev, index, _doff([E, 0]), t, v, 1, fof).check(f"E={E} pair at {at}")
        assert K == E - 1


def test_run_lengths(torch_dev, index):
    lens = [2, 1, 3, 1, 64, 1, 65, 1, 200, 2, 3, 64, 65, 200]
    t, v, fof = _runs(lens)
    K = Run(torch_dev, index, _doff([len(t), 0]), t, v, 1, fof).check("runs")
    assert K == len(lens)


def test_one_run_and_no_duplicates(torch_dev, index, G):
    for E in (5000, 64 * G + 777):
        t, v, fof = _runs([E])
        assert Run(torch_dev, index, _doff([E, 0]), t, v, 1, fof).check("everything one run") == 1
        t, v, fof = _runs(np.ones(E, np.int64))
        r = Run(torch_dev, index, _doff([E // 2, E - E // 2, 0]), t, v, 2, fof)
        assert r.check("no duplicates") == E
        assert np.array_equal(r.o_t.cpu().numpy().view(np.uint32)[:E], t)


def test_what_is_never_dropped(torch_dev, index):
    E = 300
    same_f = (np.arange(E, dtype=np.uint32), np.arange(E, dtype=np.uint32), np.full(E, 7, np.uint32))
    same_t = (np.zeros(E, np.uint32), np.arange(E, dtype=np.uint32), np.arange(E, dtype=np.uint32))
    both_none = (np.zeros(E, np.uint32), np.arange(E, dtype=np.uint32), np.full(E, NONE, np.uint32))
    for what, (t, v, fof) in (("equal filter, different topic", same_f), ("equal topic, different filter", same_t),
                              ("no filter known", both_none)):
        assert Run(torch_dev, index, _doff([E, 0]), t, v, 1, fof).check(what) == E
    # values at or past filter_len have no filter: those entries stay, the others of the run go
    t, v, fof = np.zeros(E, np.uint32), np.arange(E, dtype=np.uint32), np.full(100, 5, np.uint32)
    assert Run(torch_dev, index, _doff([E, 0]), t, v, 1, fof).check("v >= filter_len") == 1 + 200
    # a null table of length 0: nothing has a filter
    assert Run(torch_dev, index, _doff([E, 0]), t, v, 1, np.zeros(0, np.uint32)).check("empty table") == E


def test_bucket_bounds_and_the_unrouted_bucket(torch_dev, index):
    # one run of 400 equal entries over buckets of 100, 0, 0, 150, 50 and an unrouted bucket of 100
    t, v, fof = _runs([400])
    sizes = [100, 0, 0, 150, 50, 100]
    r = Run(torch_dev, index, _doff(sizes), t, v, 5, fof)
    assert r.check("one run over every bucket") == 3 + 100
    assert r.o_doff.cpu().numpy()[:7].tolist() == [0, 1, 1, 1, 2, 3, 103]
    # the same (topic, filter) as last entry of bucket b and first of b + 1: both kept
    t, v, fof = _runs(np.ones(200, np.int64))
    fof[100] = fof[99]
    t[100] = t[99]
    assert Run(torch_dev, index, _doff([100, 100, 0]), t, v, 2, fof).check("pair across a bound") == 200
    assert Run(torch_dev, index, _doff([99, 101, 0]), t, v, 2, fof).check("pair inside a bucket") == 199
    assert Run(torch_dev, index, _doff([0, 99, 101]), t, v, 2, fof).check("pair in the unrouted bucket") == 200


@pytest.mark.parametrize("n_dests", [1, 2, 255, 256, 65536])
def test_destination_counts_with_empty_buckets(torch_dev, index, n_dests):
    for seed, E, ends in ((1, 20_000, 0), (2, 20_000, n_dests // 3), (3, 50, n_dests // 3)):
        doff, t, v, fof = _random(E, n_dests, seed=seed * 100_003 + n_dests, empty_ends=ends)
        K = Run(torch_dev, index, doff, t, v, n_dests, fof).check(f"n_dests={n_dests} E={E} empty ends {ends}")
        assert 0 < K <= E
    # every routed bucket empty but the last; and every entry unrouted
    t, v, fof = _runs([3] * 100)
    assert Run(torch_dev, index, _doff([0] * (n_dests - 1) + [300, 0]), t, v, n_dests, fof).check("last bucket") == 100
    assert Run(torch_dev, index, _doff([0] * n_dests + [300]), t, v, n_dests, fof).check("all unrouted") == 300


def test_cap_below_the_total(torch_dev, index, G):
    doff, t, v, fof = _random(64 * G + 500, 4, seed=77)
    for cap in (64 * G + 499, 64 * G, 1000, 1, 0):
        Run(torch_dev, index, doff, t, v, 4, fof, cap=cap).check(f"cap={cap}")


def test_small_after_large_and_three_streams(torch_dev, index, G):
    big = _random(64 * G * 2 + 33, 300, seed=5)
    small = _random(77, 300, seed=6)
    a = Run(torch_dev, index, *big[:3], 300, big[3])
    b = Run(torch_dev, index, *small[:3], 300, small[3])
    a.check("large")
    b.check("small after large")
    streams = [torch_dev.cuda.Stream() for _ in range(3)]
    ins = [_random(30_000 + 1000 * k, (3, 300, 40)[k], seed=10 + k) for k in range(3)]
    runs = []
    for rep in range(3):
        for k, s in enumerate(streams):
            runs.append((Run(torch_dev, index, *ins[k][:3], (3, 300, 40)[k], ins[k][3], stream=s), f"stream {k} rep {rep}"))
    for r, what in runs:
        r.check(what)
    for s in streams:
        index.release_stream(s.cuda_stream)


def test_the_index_own_table(torch_dev):
    ix = _native.Index()
    E = 1000
    t = np.zeros(E, np.uint32)
    v = np.arange(E, dtype=np.uint32)
    doff = _doff([E, 0])
    table = np.full(E, NONE, np.uint32)
    assert Run(torch_dev, ix, doff, t, v, 1, None).check("never set", table=table) == E
    table[:500] = 9
    ix.set_route_filters(np.arange(500), table[:500])
    assert Run(torch_dev, ix, doff, t, v, 1, None).check("500 set", table=table) == 1 + 500
    table[:] = 9                                   # grown
    ix.set_route_filters(np.arange(500, E), table[500:])
    assert Run(torch_dev, ix, doff, t, v, 1, None).check("grown", table=table) == 1
    table[700] = 11                                # one entry changed
    ix.set_route_filters([700], [11])
    assert Run(torch_dev, ix, doff, t, v, 1, None).check("one changed", table=table) == 3
    table[300] = NONE                              # one set back
    ix.set_route_filters([300], [NONE])
    assert Run(torch_dev, ix, doff, t, v, 1, None).check("one unset", table=table) == 5
    # beyond the table: no filter
    v2 = v + 500
    assert Run(torch_dev, ix, doff, t, v2, 1, None).check("past the table", table=table) == 1 + 2 + 500
    ix.close()


def test_bad_arguments(torch_dev, index):
    lib, h = index._lib, index._h
    d = torch_dev.zeros(16, dtype=torch_dev.int64, device="cuda").data_ptr()
    E = _native.TM_EINVAL
    assert lib.tm_aggre_dev(h, 0, d, d, d, 4, None, 0, d, d, d, None) == E
    assert lib.tm_aggre_dev(h, 65537, d, d, d, 4, None, 0, d, d, d, None) == E
    assert lib.tm_aggre_dev(h, 1, None, d, d, 4, None, 0, d, d, d, None) == E
    assert lib.tm_aggre_dev(h, 1, d, None, d, 4, None, 0, d, d, d, None) == E
    assert lib.tm_aggre_dev(h, 1, d, d, d, 4, None, 0, None, d, d, None) == E
    assert lib.tm_aggre_dev(h, 1, d, d, d, 4, None, 0, d, d, None, None) == E
    assert lib.tm_set_route_filters(h, 1, None, None) == E
