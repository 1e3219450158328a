"""tm_dispatch_dev driven directly: synthetic bucketed (topic, value) arrays and
explicit subscriber tables built in numpy, exact against the numpy definition
in include/tmatch.h -- no index content involved (the pattern of
test_gpu_aggre.py).

The counting and offset passes run on G = TM_DEBUG_FANOUT_GRID one-wave blocks
over the bucket's M entries (chunk = ceil(M / G) rounded up to 64), the
expansion on the same grid over the W = min(T, out_cap) output positions
(ochunk = ceil(W / G) rounded up to 64): up to 64 G of either a block owns one
64-wide step, from 64 G + 1 on two.  The inputs hold exactly E entries and the
pool exactly pool_len words (one spare word keeps an empty tensor from being a
null pointer); every output buffer is filled with a sentinel that must survive
at and past W, past off[M] and past head[1]; the inputs are compared after the
run.
"""
import numpy as np
import pytest

from emqx_amd import _native

pytestmark = pytest.mark.gpu

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
    """an empty index: tm_dispatch_dev needs a handle for its scratch (and its own table) only"""
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

def _ref(doff, t, v, cap, n_dests, bucket, span, pool, out_cap):
    """the header's numpy definition -> (M, T, off u64[M + 1], topic, value, sub: the first W)"""
    doff = doff.astype(np.int64)
    E = min(int(doff[n_dests + 1]), cap)
    q0, q1 = min(int(doff[bucket]), E), min(int(doff[bucket + 1]), E)
    M = q1 - q0
    t, v = t[q0:q1], v[q0:q1]
    span = span.astype(np.int64)
    span_len = len(span) // 2
    pos, cnt = np.zeros(M, np.int64), np.zeros(M, np.int64)
    inr = v.astype(np.int64) < span_len
    pos[inr], cnt[inr] = span[2 * v[inr].astype(np.int64)], span[2 * v[inr].astype(np.int64) + 1]
    cnt[pos + cnt > len(pool)] = 0
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    T = int(off[M])
    W = min(T, out_cap)
    if T <= 1 << 22:
        src = np.repeat(np.arange(M), cnt)[:W]
    else:   # (the same thing without T words of memory: the last j with off[j] <= p)
        src = np.searchsorted(off, np.arange(W), side="right") - 1
    r = np.arange(W) - off[src]
    return M, T, off.astype(np.uint64), t[src], v[src], pool[pos[src] + r] if W else np.zeros(0, np.uint32)


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def _dev(torch, a):
    return torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)]).view(np.int32 if a.itemsize == 4 else np.int64)).cuda()


class Run:
    """one tm_dispatch_dev call's device buffers (kept alive until checked)"""

    def __init__(self, torch, ix, doff, t, v, n_dests, bucket, span, pool, cap=None, out_cap=None, offsets=True,
                 stream=None, expect=None):
        """span / pool None: the index's own table, `expect` = the (span, pool) the host model has now"""
        doff = np.asarray(doff, np.uint64)
        t, v = np.asarray(t, np.uint32), np.asarray(v, np.uint32)
        assert len(doff) == n_dests + 2 and len(t) == len(v)
        cap = len(t) if cap is None else cap
        E = min(int(doff[-1]), cap)
        assert E <= len(t)
        t, v = t[:E].copy(), v[:E].copy()   # no position at or past E exists
        own = span is None
        rspan, rpool = expect if own else (np.asarray(span, np.uint32), np.asarray(pool, np.uint32))
        M, T = _ref(doff, t, v, cap, n_dests, bucket, rspan, rpool, 0)[:2]
        out_cap = T if out_cap is None else out_cap
        self.exp = _ref(doff, t, v, cap, n_dests, bucket, rspan, rpool, out_cap)
        self.torch, self.ins, self.out_cap, self.offsets = torch, (doff, t, v), out_cap, offsets
        W = min(T, out_cap)
        with torch.cuda.stream(stream) if stream is not None else _Null():
            self.d_doff, self.d_t, self.d_v = _dev(torch, doff), _dev(torch, t), _dev(torch, v)
            self.d_span = None if own else _dev(torch, rspan)
            self.d_pool = None if own else _dev(torch, rpool)
            self.o_head = torch.full((2 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.o_off = torch.full((M + 1 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.o_t, self.o_v, self.o_s = (torch.from_numpy(np.full(W + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
                                            for _ in range(3))
            ix.dispatch_dev(n_dests, self.d_doff.data_ptr(), bucket, self.d_t.data_ptr(), self.d_v.data_ptr(), cap,
                            self.o_head.data_ptr(), self.o_t.data_ptr(), self.o_v.data_ptr(), self.o_s.data_ptr(), out_cap,
                            d_out_offsets=self.o_off.data_ptr() if offsets else None,
                            d_sub_span=None if own else self.d_span.data_ptr(), span_len=0 if own else len(rspan) // 2,
                            d_sub_pool=None if own else self.d_pool.data_ptr(), pool_len=0 if own else len(rpool),
                            stream=torch.cuda.current_stream().cuda_stream)
        self.span, self.pool = (None, None) if own else (rspan, rpool)

    def check(self, what):
        """exact outputs, sentinels, inputs unmodified -> (M, T)"""
        doff, t, v = self.ins
        self.torch.cuda.synchronize()
        M, T, off, e_t, e_v, e_s = self.exp
        W = min(T, self.out_cap)
        head = self.o_head.cpu().numpy()
        print(f"{what}: M={M} T={T} W={W} head={head[:2].tolist()}")
        assert head[:2].view(np.uint64).tolist() == [M, T], f"{what}: head is {head[:2].tolist()}, not {[M, T]}"
        assert (head[2:] == OFFS_CANARY).all(), f"{what}: wrote past head[1]"
        g_off = self.o_off.cpu().numpy()
        if self.offsets:
            assert np.array_equal(g_off[:M + 1].view(np.uint64), off), f"{what}: delivery offsets differ"
            assert (g_off[M + 1:] == OFFS_CANARY).all(), f"{what}: wrote past d_out_offsets[M]"
        else:
            assert (g_off == OFFS_CANARY).all()
        g_t, g_v, g_s = (x.cpu().numpy().view(np.uint32) for x in (self.o_t, self.o_v, self.o_s))
        bad = np.nonzero((g_t[:W] != e_t) | (g_v[:W] != e_v) | (g_s[:W] != e_s))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {W} deliveries differ, first at {bad[0]}"
        for g in (g_t, g_v, g_s):
            assert (g[W:] == CANARY).all(), f"{what}: wrote at or past W"
        assert np.array_equal(self.d_doff.cpu().numpy().view(np.uint64)[:-1], doff), f"{what}: the offsets were written"
        assert np.array_equal(self.d_t.cpu().numpy().view(np.uint32)[:-1], t), f"{what}: the topics were written"
        assert np.array_equal(self.d_v.cpu().numpy().view(np.uint32)[:-1], v), f"{what}: the values were written"
        if self.span is not None:
            assert np.array_equal(self.d_span.cpu().numpy().view(np.uint32)[:-1], self.span), f"{what}: the spans were written"
            assert np.array_equal(self.d_pool.cpu().numpy().view(np.uint32)[:-1], self.pool), f"{what}: the pool was written"
        return M, T


# ---------------------------------------------------------------- the inputs

def _doff(sizes):
    d = np.zeros(len(sizes) + 1, np.uint64)
    d[1:] = np.cumsum(np.asarray(sizes, np.int64), dtype=np.uint64)
    return d


def _table(lengths, seed=0, gap=3):
    """value i has a list of lengths[i] distinct ids, the lists `gap` words apart in the pool
    and in shuffled order -> (span u32[2 n], pool)"""
    lengths = np.asarray(lengths, np.int64)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(lengths))
    span = np.zeros(2 * len(lengths), np.uint32)
    at = 1
    for i in order:
        span[2 * i], span[2 * i + 1] = at, lengths[i]
        at += int(lengths[i]) + gap
    pool = (np.arange(at, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(seed)
    return span, pool


def _entries(M, seed, lens=(0, 1, 2, 3)):
    """M entries in one bucket: value q has a list of a length drawn from lens; topics ascend"""
    rng = np.random.default_rng(seed)
    span, pool = _table(rng.choice(lens, M), seed)
    return (np.arange(M, dtype=np.uint32) // 2), rng.permutation(M).astype(np.uint32), span, pool


# ------------------------------------------------------------------ the tests

def test_entry_counts_around_steps_and_chunks(torch_dev, index, G):
    for M in (0, 1, 63, 64, 65, 64 * G, 64 * G + 1):
        t, v, span, pool = _entries(M, seed=M + 1)
        m, T = Run(torch_dev, index, _doff([M, 0]), t, v, 1, 0, span, pool).check(f"M={M}")
        assert m == M and (M < 60 or 0 < T < 3 * M)


def test_a_list_across_blocks(torch_dev, index, G):
    # one entry of 1000 subscribers among single ones: W <= 64 G, every block one step
    lens = np.ones(500, np.int64)
    lens[123] = 1000
    span, pool = _table(lens, seed=3)
    t, v = np.arange(500, dtype=np.uint32), np.arange(500, dtype=np.uint32)
    assert Run(torch_dev, index, _doff([500, 0]), t, v, 1, 0, span, pool).check("1000 among ones") == (500, 1499)
    assert 1499 <= 64 * G
    # 5 entries of 60,000 each: two steps a block (when 300,000 > 64 G), every list over hundreds of blocks
    span, pool = _table([60_000] * 5, seed=4)
    t, v = np.arange(5, dtype=np.uint32) + 7, np.arange(5, dtype=np.uint32)
    assert Run(torch_dev, index, _doff([5, 0]), t, v, 1, 0, span, pool).check("5 x 60000") == (5, 300_000)


def test_empty_entries(torch_dev, index):
    # more than 64 consecutive empty entries between two non-empty ones, empty first and last entries
    lens = np.zeros(300, np.int64)
    lens[[40, 241]] = 5, 70     # 200 empty entries between them
    span, pool = _table(lens, seed=5)
    t, v = np.arange(300, dtype=np.uint32), np.arange(300, dtype=np.uint32)
    assert Run(torch_dev, index, _doff([300, 0]), t, v, 1, 0, span, pool).check("200 empty between") == (300, 75)
    lens[:] = 0
    span, pool = _table(lens, seed=6)
    assert Run(torch_dev, index, _doff([300, 0]), t, v, 1, 0, span, pool).check("all empty") == (300, 0)
    # the same value twice in a row (and the same topic): its list twice
    span, pool = _table([3, 2, 4], seed=7)
    t, v = np.array([9, 9, 9, 9], np.uint32), np.array([1, 0, 0, 2], np.uint32)
    assert Run(torch_dev, index, _doff([4, 0]), t, v, 1, 0, span, pool).check("a value twice") == (4, 12)


def test_truncation(torch_dev, index):
    t, v, span, pool = _entries(3000, seed=8, lens=(0, 1, 2, 3, 40))
    doff = _doff([1000, 1500, 500])
    M, T = Run(torch_dev, index, doff, t, v, 2, 1, span, pool).check("whole")
    assert M == 1500 and T > 1500
    for out_cap in (0, 1, T - 1, T, T + 5):
        Run(torch_dev, index, doff, t, v, 2, 1, span, pool, out_cap=out_cap).check(f"out_cap={out_cap}")
    # a cut inside a long list
    span2, pool2 = _table([100, 100, 100], seed=9)
    for out_cap in (150, 64, 65):
        r = Run(torch_dev, index, _doff([3, 0]), [4, 5, 6], [0, 1, 2], 1, 0, span2, pool2, out_cap=out_cap)
        assert r.check(f"cut inside a list at {out_cap}") == (3, 300)
    # cap below doff[bucket + 1], below doff[bucket], and 0
    for cap, m in ((2499, 1499), (1700, 700), (1000, 0), (999, 0), (0, 0)):
        assert Run(torch_dev, index, doff, t, v, 2, 1, span, pool, cap=cap).check(f"cap={cap}")[0] == m


def test_buckets(torch_dev, index):
    t, v, span, pool = _entries(2000, seed=10)
    doff = _doff([300, 0, 900, 0, 800])   # n_dests = 4: buckets 0 .. 3 and the unrouted one
    for bucket, m in ((0, 300), (2, 900), (1, 0), (3, 0), (4, 800)):
        assert Run(torch_dev, index, doff, t, v, 4, bucket, span, pool).check(f"bucket {bucket}")[0] == m
    doff = _doff([0] * 65536 + [2000])
    assert Run(torch_dev, index, doff, t, v, 65536, 65536, span, pool).check("bucket 65536")[0] == 2000
    assert Run(torch_dev, index, doff, t, v, 65536, 40000, span, pool).check("an empty bucket of 65536")[0] == 0


def test_defensive_rules(torch_dev, index):
    span, pool = _table([2, 3, 4, 5], seed=11, gap=0)    # lists at 1, .. in shuffled order; the pool ends with the last
    t = np.arange(8, dtype=np.uint32)
    v = np.array([0, 1, 7, 2, 4, 3, 0xFFFFFFFF, 1], np.uint32)   # 7, 4, 2^32 - 1: v >= span_len
    assert Run(torch_dev, index, _doff([8, 0]), t, v, 1, 0, span, pool).check("v >= span_len") == (8, 2 + 3 + 4 + 5 + 3)
    # a span that ends past the pool is empty; one that ends exactly at it is not
    last = int(np.argmax(span[0::2]))
    assert int(span[2 * last]) + int(span[2 * last + 1]) == len(pool)
    short = pool[:-1].copy()
    r = Run(torch_dev, index, _doff([8, 0]), t, v, 1, 0, span, short)
    assert r.check("pos + cnt > pool_len")[1] == 2 + 3 + 4 + 5 + 3 - int(span[2 * last + 1]) * (2 if last == 1 else 1)
    # the 64-bit sum: 0xFFFFFFF0 + 0x20 wraps to 0x10 in 32 bits
    span3 = np.array([1, 2, 0xFFFFFFF0, 0x20, 4, 1], np.uint32)
    pool64 = np.arange(64, dtype=np.uint32) * np.uint32(7)
    r = Run(torch_dev, index, _doff([3, 0]), [0, 1, 2], [0, 1, 2], 1, 0, span3, pool64)
    assert r.check("pos + cnt past 2^32") == (3, 3)
    # no table at all
    assert Run(torch_dev, index, _doff([3, 0]), [0, 1, 2], [0, 1, 2], 1, 0, np.zeros(0, np.uint32),
               np.zeros(0, np.uint32)).check("empty table") == (3, 0)


def test_a_total_past_32_bits(torch_dev, index):
    n = 1 << 20
    span = np.array([0, n], np.uint32)
    pool = np.arange(n, dtype=np.uint32) * np.uint32(2246822519)
    t, v = np.arange(5000, dtype=np.uint32), np.zeros(5000, np.uint32)
    r = Run(torch_dev, index, _doff([5000, 0]), t, v, 1, 0, span, pool, out_cap=1000)
    assert r.check("T = 5000 * 2^20") == (5000, 5000 << 20)
    assert 5000 << 20 > 1 << 32


def test_offsets_given_and_null_give_the_same_deliveries(torch_dev, index, G):
    t, v, span, pool = _entries(64 * G + 777, seed=12, lens=(0, 1, 1, 2, 3, 200))
    doff = _doff([len(t), 0])
    a = Run(torch_dev, index, doff, t, v, 1, 0, span, pool, offsets=True)
    b = Run(torch_dev, index, doff, t, v, 1, 0, span, pool, offsets=False)
    assert a.check("offsets given") == b.check("offsets NULL")
    for x, y in ((a.o_t, b.o_t), (a.o_v, b.o_v), (a.o_s, b.o_s)):
        assert torch_dev.equal(x, y)


# ---- the index's own table

def _model_table(model, nvals):
    """the host model {value: [ids]} as an explicit (span, pool)"""
    span = np.zeros(2 * nvals, np.uint32)
    words = []
    at = 0
    for val in range(nvals):
        ids = model.get(val, [])
        span[2 * val], span[2 * val + 1] = at, len(ids)
        words.extend(ids)
        at += len(ids)
    return span, np.asarray(words, np.uint32)


def test_the_index_own_table(torch_dev):
    ix = _native.Index()
    nv = 6000
    E = 400
    t = np.arange(E, dtype=np.uint32)
    v = np.concatenate([np.arange(200), np.arange(200) + 5800]).astype(np.uint32)
    doff = _doff([E, 0])
    model = {}

    def run(what, **kw):
        return Run(torch_dev, ix, doff, t, v, 1, 0, None, None, expect=_model_table(model, nv), **kw).check(what)

    assert run("never set") == (E, 0)
    model.update({i: [1000 + i, 2000 + i] for i in range(100)})
    ix.set_subscribers(list(model), list(model.values()))
    assert run("100 set") == (E, 200)
    model[5] = list(range(50, 90))          # longer
    model[6] = [77]                         # shorter
    model[7] = []                           # empty
    ix.set_subscribers([5, 6, 7], [model[5], model[6], model[7]])
    assert run("longer, shorter, empty") == (E, 200 + 38 - 1 - 2)
    ix.set_subscribers([8, 8, 9, 8], [[1], [2, 3, 4], [5], [6, 7]])   # a value twice (three times) in one call
    model[8], model[9] = [6, 7], [5]
    assert run("a value twice in one call") == (E, 200 + 38 - 1 - 2 - 1)
    # growth past the first allocation of the spans (values up to 5999) and of the pool
    grown = {i: [i * 3 + k for k in range(1 + i % 5)] for i in range(5800, 6000)}
    grown[150] = list(range(10_000, 19_000))
    model.update(grown)
    ix.set_subscribers(list(grown), list(grown.values()))
    assert run("grown")[1] > 9000
    ix.set_subscribers([150], [[]])
    model[150] = []
    run("after the long list went", offsets=False)
    ix.close()


def test_updates_between_dispatches_on_two_streams(torch_dev):
    ix = _native.Index()
    rng = np.random.default_rng(2024)
    nv, E = 300, 600
    t = np.arange(E, dtype=np.uint32) // 3
    v = rng.integers(0, nv + 20, E).astype(np.uint32)     # a few values past every span
    doff = _doff([100, E - 100, 0])
    streams = [torch_dev.cuda.Stream() for _ in range(2)]
    model, runs, next_id = {}, [], 1
    for step in range(3000):
        val = int(rng.integers(0, nv))
        kind = rng.random()
        n = 0 if kind < 0.3 else int(rng.integers(1, 4)) if kind < 0.97 else int(rng.integers(300, 1500))
        model[val] = list(range(next_id, next_id + n))
        next_id += n
        ix.set_subscribers([val], [model[val]])
        if step % 50 == 49:
            k = (step // 50) % 2
            runs.append((Run(torch_dev, ix, doff, t, v, 2, 1, None, None, expect=_model_table(model, nv),
                             stream=streams[k], offsets=bool(k)), f"step {step} stream {k}"))
    for r, what in runs:
        r.check(what)
    # long lists set and cleared: more garbage than lists, whatever the history left
    ix.set_subscribers(list(range(200)), [list(range(500))] * 200)
    ix.set_subscribers(list(range(200)), [[]] * 200)
    for val in range(200):
        model[val] = []
    Run(torch_dev, ix, doff, t, v, 2, 1, None, None, expect=_model_table(model, nv)).check("after the compaction")
    assert ix.debug_get(_native.TM_DEBUG_SUB_COMPACTIONS) > 0
    for s in streams:
        ix.release_stream(s.cuda_stream)
    ix.close()


def test_bad_arguments(torch_dev, index):
    lib, h = index._lib, index._h
    d = torch_dev.zeros(16, dtype=torch_dev.int64, device="cuda").data_ptr()
    E = _native.TM_EINVAL

    def call(n_dests=1, doff=d, bucket=0, t=d, v=d, cap=4, span=None, span_len=0, pool=None, pool_len=0, head=d,
             o_t=d, o_v=d, o_s=d, out_cap=4):
        return lib.tm_dispatch_dev(h, n_dests, doff, bucket, t, v, cap, span, span_len, pool, pool_len, head, None, o_t,
                                   o_v, o_s, out_cap, None)

    assert call(n_dests=0) == E and call(n_dests=65537) == E
    assert call(bucket=2) == E and call(n_dests=7, bucket=8) == E
    assert call(doff=None) == E and call(t=None) == E and call(v=None) == E and call(head=None) == E
    assert call(o_t=None) == E and call(o_v=None) == E and call(o_s=None) == E
    assert call(span=d, span_len=1, pool=None, pool_len=3) == E
    assert call() == _native.TM_OK and call(n_dests=7, bucket=7) == _native.TM_OK
    torch_dev.cuda.synchronize()
    one = np.zeros(1, np.uint32)
    offs = np.array([3, 1], np.uint64)
    assert lib.tm_set_subscribers(h, 1, None, None, None) == E
    assert lib.tm_set_subscribers(h, 1, one.ctypes.data, offs.ctypes.data, one.ctypes.data) == E   # decreasing
    assert lib.tm_set_subscribers(h, 0, None, None, None) == _native.TM_OK
