"""tm_fanout_dev_pairs: the route fan-out of a batch given as per-topic (first
position, count) pairs, exact against its definition (include/tmatch.h):

    eff_t = 0 if pos_t >= cap else min(cnt_t, cap - pos_t)
    hit'[t] = sum of eff_u for u < t (64-bit), vals'[hit'[t] + j] = values[pos_t + j]
    outputs = tm_fanout_dev(n, hit', vals', cap, ...), i.e. the first
    E = min(hit'[n], cap) entries under np.argsort(bucket, kind="stable")

Synthetic pairs built in numpy (the pattern of test_gpu_fanout.py, whose small
helpers are copied here), then a real index matched both ways.  G =
TM_DEBUG_FANOUT_GRID one-wave blocks own chunks of ceil(E / G) entries rounded
up to 64, so totals around 64 * G sit on both sides of one step; the topics'
offsets are scanned in tiles of at least 256 topics, at most 1024 tiles, so
n = 70001 takes several tiles with a ragged last one.  Every output carries a
canary tail of 64 words; the inputs are checked unmodified.
"""
import random

import numpy as np
import pytest

from emqx_amd import _native, workload as wl

pytestmark = pytest.mark.gpu

CANARY = 0xC0FFEE11
OFFS_CANARY = -77
TAIL = 64
U32 = 1 << 32
FF = 0xFFFFFFFF
BOTH = (16, 300)   # one pass, two passes


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def index(torch_dev):
    """an empty index: the fan-out needs a handle for its scratch (and its own table) only"""
    return _native.Index()


@pytest.fixture(scope="module")
def G(index):
    g = index.debug_get(_native.TM_DEBUG_FANOUT_GRID)
    assert g >= 64 and g % 64 == 0
    return g


# ------------------------------------------------------------- the reference

def _buckets(vals, dest_of, n_dests):
    v = vals.astype(np.int64)
    b = np.full(len(v), n_dests, np.int64)
    inr = v < len(dest_of)
    d = dest_of[v[inr]].astype(np.int64)
    b[inr] = np.where(d < n_dests, d, n_dests)
    return b


def _virtual_csr(pairs, values, n, cap):
    """the definition's (E, topic u32[E], value u32[E]): the first E entries of the virtual CSR"""
    cap = min(cap, U32 - 1)
    pos, cnt = pairs[:n, 0].astype(np.int64), pairs[:n, 1].astype(np.int64)
    eff = np.where(pos >= cap, 0, np.minimum(cnt, cap - pos))
    hit = np.zeros(n + 1, np.int64)   # (n * cap stays far below 2^63 here)
    hit[1:] = np.cumsum(eff)
    E = int(min(hit[n], cap))
    clipped = np.minimum(hit, E)
    take = np.diff(clipped)           # a topic's entries below E
    topic = np.repeat(np.arange(n, dtype=np.int64), take)
    j = np.arange(E, dtype=np.int64) - np.repeat(clipped[:-1], take)
    at = pos[topic] + j
    assert E == 0 or at.max() < cap
    return E, topic.astype(np.uint32), values[at] if E else np.zeros(0, np.uint32)


def _ref(pairs, values, n, cap, dest_of, n_dests):
    """-> (dest_offsets u64[n_dests + 2], topic u32[E], value u32[E])"""
    E, topic, v = _virtual_csr(pairs, values, n, cap)
    b = _buckets(v, dest_of, n_dests)
    order = np.argsort(b, kind="stable")
    offs = np.zeros(n_dests + 2, np.uint64)
    offs[1:] = np.cumsum(np.bincount(b, minlength=n_dests + 1))
    return offs, topic[order], v[order]


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


class Run:
    """one tm_fanout_dev_pairs call's device buffers (kept alive until checked).
    pairs: int64 [n, 2]; values: u32, exactly max(cap, 1) words on the device;
    tail: what follows the 2 n pair words (the producers write a total and an
    extent there; the call must not care)"""

    def __init__(self, torch, ix, pairs, values, n, cap, n_dests, dest_of, stream=None, tail=(FF, FF)):
        assert len(values) >= cap
        self.torch, self.args = torch, (pairs, values, n, cap, dest_of, n_dests)
        self.flat = np.concatenate([pairs[:n].reshape(-1), np.asarray(tail, np.int64)]).astype(np.uint32)
        self.dvals = values[:cap] if len(values) > cap else values
        self.E = E = _virtual_csr(pairs, values, n, cap)[0]
        with torch.cuda.stream(stream) if stream is not None else _Null():
            self.d_pairs = torch.from_numpy(self.flat.view(np.int32).copy()).cuda()
            self.d_vals = torch.from_numpy(np.ascontiguousarray(self.dvals).view(np.int32).copy()).cuda() \
                if len(self.dvals) else torch.zeros(1, dtype=torch.int32, device="cuda")
            self.d_tab = None if dest_of is None else \
                torch.from_numpy(np.concatenate([dest_of, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
            self.d_offs = torch.full((n_dests + 2 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.d_topic = torch.from_numpy(np.full(E + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
            self.d_value = torch.from_numpy(np.full(E + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
            assert self.d_pairs.data_ptr() % 8 == 0
            s = torch.cuda.current_stream().cuda_stream
            ix.fanout_dev_pairs(n, self.d_pairs.data_ptr(), self.d_vals.data_ptr(), cap, n_dests,
                                self.d_offs.data_ptr(), self.d_topic.data_ptr(), self.d_value.data_ptr(),
                                None if dest_of is None else self.d_tab.data_ptr(),
                                0 if dest_of is None else len(dest_of), s)

    def outputs(self):
        self.torch.cuda.synchronize()
        return (self.d_offs.cpu().numpy(), self.d_topic.cpu().numpy().view(np.uint32),
                self.d_value.cpu().numpy().view(np.uint32))

    def check(self, what, table=None):
        """exact outputs, canary tails, inputs unmodified"""
        pairs, values, n, cap, dest_of, n_dests = self.args
        g_offs, g_topic, g_value = self.outputs()
        offs, topic, value = _ref(pairs, values, n, cap, dest_of if table is None else table, n_dests)
        E = self.E
        assert len(topic) == E
        assert np.array_equal(g_offs[:n_dests + 2].view(np.uint64), offs), f"{what}: bucket offsets differ"
        assert int(g_offs[n_dests + 1]) == E
        assert (g_offs[n_dests + 2:] == OFFS_CANARY).all(), f"{what}: wrote past dest_offsets[n_dests + 1]"
        bad = np.nonzero((g_topic[:E] != topic) | (g_value[:E] != value))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {E} entries differ, first at {bad[0]}: " \
                              f"({g_topic[bad[0]]}, {g_value[bad[0]]}) for ({topic[bad[0]]}, {value[bad[0]]})"
        assert (g_topic[E:] == CANARY).all() and (g_value[E:] == CANARY).all(), f"{what}: wrote past min(total, cap)"
        assert np.array_equal(self.d_pairs.cpu().numpy().view(np.uint32), self.flat), f"{what}: the pairs were written"
        if len(self.dvals):
            assert np.array_equal(self.d_vals.cpu().numpy().view(np.uint32), self.dvals), f"{what}: the values were written"
        return g_offs[:n_dests + 2], g_topic[:E], g_value[:E]


def _csr_fanout(torch, ix, hit, vals, n, cap, n_dests, dest_of):
    """tm_fanout_dev on the plain CSR -> (dest_offsets, topic, value) on the host"""
    E = min(int(hit[n]), cap)
    d_hit = torch.from_numpy(hit.view(np.int64).copy()).cuda()
    d_vals = torch.from_numpy(np.concatenate([vals, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
    d_tab = torch.from_numpy(np.concatenate([dest_of, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
    d_offs = torch.zeros(n_dests + 2, dtype=torch.int64, device="cuda")
    d_topic = torch.zeros(E + 1, dtype=torch.int32, device="cuda")
    d_value = torch.zeros(E + 1, dtype=torch.int32, device="cuda")
    ix.fanout_dev(n, d_hit.data_ptr(), d_vals.data_ptr(), cap, n_dests, d_offs.data_ptr(), d_topic.data_ptr(),
                  d_value.data_ptr(), d_tab.data_ptr(), len(dest_of), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_offs.cpu().numpy(), d_topic.cpu().numpy().view(np.uint32)[:E], d_value.cpu().numpy().view(np.uint32)[:E]


# ---------------------------------------------------------------- the inputs

def _hit(lens):
    hit = np.zeros(len(lens) + 1, np.uint64)
    hit[1:] = np.cumsum(np.asarray(lens, np.int64), dtype=np.uint64)
    return hit


def _spread(rng, n, total):
    """`total` entries over n topics at random (many topics empty when total < n)"""
    if n == 0:
        return np.zeros(0, np.int64)
    return np.bincount(rng.integers(0, n, total), minlength=n).astype(np.int64)


def _table(rng, n_dests, length, stray=0.05):
    """dest_of[length]: ids over the whole range (both digits vary), n_dests - 1
    and 0 present, a few entries >= n_dests (0xFFFFFFFF among them)"""
    t = rng.integers(0, n_dests, length, dtype=np.int64).astype(np.uint32)
    bad = rng.random(length) < stray
    t[bad] = rng.integers(n_dests, U32, int(bad.sum()), dtype=np.int64).astype(np.uint32)
    t[rng.integers(0, length, 3)] = FF
    t[0], t[length - 1] = n_dests - 1, 0
    return t


def _values(rng, total, dest_len, beyond=0.03):
    """values hitting the table's first and last entry, a few beyond it"""
    v = rng.integers(0, dest_len, total, dtype=np.int64)
    far = rng.random(total) < beyond
    v[far] = rng.integers(dest_len, U32, int(far.sum()), dtype=np.int64)
    if total >= 2:
        v[rng.integers(0, total)], v[rng.integers(0, total)] = 0, dest_len - 1
    return v.astype(np.uint32)


LAYOUTS = ("csr", "reverse", "permuted")


def _layout(rng, lens, vals, kind):
    """the CSR (lens, vals) as spans -> (pairs int64 [n, 2], values u32[cap], cap).
    csr: in topic order and contiguous; reverse: contiguous in reverse topic
    order; permuted: a random order with 0-130 words of garbage before, between
    and after the spans.  An empty topic's pos is arbitrary: 0xFFFFFFFF, cap,
    beyond cap or inside another topic's span."""
    lens = np.asarray(lens, np.int64)
    n, total = len(lens), int(lens.sum())
    hit = _hit(lens).astype(np.int64)
    if kind == "csr":
        pos, cap = hit[:-1].copy(), total
    elif kind == "reverse":
        pos, cap = total - hit[1:], total
    else:
        order = rng.permutation(n)
        gaps = rng.integers(0, 131, n + 1)
        step = lens[order] + gaps[1:]
        start = gaps[0] + np.concatenate([[0], np.cumsum(step)])
        pos = np.zeros(n, np.int64)
        pos[order] = start[:-1]
        cap = int(start[-1])
    values = rng.integers(0, U32, cap, dtype=np.int64).astype(np.uint32)   # garbage wherever no span lies
    at = np.repeat(pos, lens) + np.arange(total) - np.repeat(hit[:-1], lens)
    values[at] = vals
    empty = np.nonzero(lens == 0)[0]
    pos[empty] = np.resize(np.array([FF, cap, cap + 5, max(cap // 2, 0), 0], np.int64), len(empty))
    return np.stack([pos, lens], axis=1) if n else np.zeros((0, 2), np.int64), values, cap


def _check_layouts(torch, ix, lens, n_dests, rng, what, kinds=LAYOUTS, table_len=5000):
    """every layout of the same lists: equal to the definition and to tm_fanout_dev on the plain CSR"""
    n, total = len(lens), int(np.sum(lens))
    tab = _table(rng, n_dests, table_len)
    vals = _values(rng, total, len(tab))
    c_offs, c_topic, c_value = _csr_fanout(torch, ix, _hit(lens), vals, n, total, n_dests, tab)
    for kind in kinds:
        pairs, values, cap = _layout(rng, lens, vals, kind)
        offs, topic, value = Run(torch, ix, pairs, values, n, cap, n_dests, tab).check(f"{what}, {kind}, n_dests {n_dests}")
        assert np.array_equal(offs, c_offs) and np.array_equal(topic, c_topic) and np.array_equal(value, c_value), \
            f"{what}, {kind}, n_dests {n_dests}: differs from tm_fanout_dev on the CSR"


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 70001])
def test_span_layouts_equal_the_csr(torch_dev, index, G, n):
    """in topic order, reversed and permuted with gaps: the same outputs as tm_fanout_dev on the CSR"""
    rng = np.random.default_rng(200 + n)
    for total in ((0, 65, 64 * G + 1) if n else (0,)):
        lens = _spread(rng, n, total)
        for n_dests in BOTH:
            _check_layouts(torch_dev, index, lens, n_dests, rng, f"n {n} total {total}")


def test_totals_around_the_chunk_step(torch_dev, index, G):
    """64 G - 1, 64 G, 64 G + 1 entries (the chunk on both sides of one step), fewer than G, and one
    topic with 3/4 of about 260k entries (longer than any chunk)"""
    rng = np.random.default_rng(11)
    for total in (64 * G - 1, 64 * G, 64 * G + 1, G - 3):
        for n_dests in BOTH:
            _check_layouts(torch_dev, index, _spread(rng, 1500, total), n_dests, rng, f"total {total}", kinds=("permuted",))
    total = 260_000
    big = _spread(rng, 3000, total // 4)
    big[1000] += total - total // 4
    assert big.max() > 100 * (((total + G - 1) // G + 63) // 64 * 64)
    for n_dests in BOTH:
        _check_layouts(torch_dev, index, big, n_dests, rng, "one long topic")
    alone = np.array([0, 0, 3 * 64 * G + 5, 0], np.int64)
    _check_layouts(torch_dev, index, alone, 16, rng, "one long topic alone")


def _with_empty_runs(rng, n, total):
    """random lengths with runs of 1, 63, 64, 65 and 200 empty topics at the start, in the middle and at the end"""
    runs = (1, 63, 64, 65, 200)
    lens = 1 + _spread(rng, n, total - n)
    at = 0
    for r in runs:   # the start: run, one topic, run, ...
        lens[at:at + r] = 0
        at += r + 1
    at = n // 2
    for r in runs:
        lens[at:at + r] = 0
        at += r + 3
    at = n
    for r in runs:   # ... one topic, run at the very end
        lens[at - r:at] = 0
        at -= r + 1
    assert lens[0] == 0 and lens[-1] == 0 and lens[1] > 0
    return lens


def test_empty_topics_with_arbitrary_positions(torch_dev, index, G):
    """runs of empty topics across the 64-offset window, at the start, the middle and the end; their pos
    is 0xFFFFFFFF, cap, beyond cap, or inside another span; all topics empty"""
    rng = np.random.default_rng(12)
    lens = _with_empty_runs(rng, 3000, 40_000)
    pairs, _, cap = _layout(rng, lens, np.zeros(int(lens.sum()), np.uint32), "permuted")
    ep = pairs[lens == 0, 0]
    assert (ep == FF).any() and (ep == cap).any() and (ep > cap).any() and ((ep < cap) & (ep > 0)).any()
    for n_dests in BOTH:
        _check_layouts(torch_dev, index, lens, n_dests, rng, "empty runs")
        _check_layouts(torch_dev, index, np.zeros(700, np.int64), n_dests, rng, "all empty", kinds=("permuted",))


@pytest.mark.parametrize("n_dests", BOTH)
def test_cap_below_the_spans(torch_dev, index, G, n_dests):
    """a span cut by cap, one starting exactly at cap, spans wholly beyond, cnt = 0xFFFFFFFF below cap;
    d_values holds exactly cap words"""
    rng = np.random.default_rng(60 + n_dests)
    n, total = 1200, 64 * G + 777
    lens = 1 + _spread(rng, n, total - n)
    tab = _table(rng, n_dests, 3000)
    vals = _values(rng, total, len(tab))
    pairs, values, full = _layout(rng, lens, vals, "permuted")
    by_pos = np.argsort(pairs[:, 0])
    mid = n // 2   # a span in the middle of the memory order, at least 2 long
    while pairs[by_pos[mid], 1] < 2:
        mid += 1
    k = by_pos[mid]
    cut = int(pairs[k, 0] + pairs[k, 1] // 2)
    for cap, what in ((cut, "cut in the middle"), (int(pairs[k, 0]), "starting exactly at cap"), (0, "cap 0"), (1, "cap 1"),
                      (full - 1, "one word short"), (full, "all of it")):
        beyond = (pairs[:, 0] > cap).sum()
        assert what in ("one word short", "all of it") or beyond > 100
        Run(torch_dev, index, pairs, values, n, cap, n_dests, tab).check(f"{what}, n_dests {n_dests}")
    huge = pairs.copy()
    huge[k, 1] = FF          # reaches cap: the same entries as the cut span
    huge[by_pos[3], 1] = FF  # and one near the start, running over its neighbours up to cap
    Run(torch_dev, index, huge, values, n, cut, n_dests, tab).check(f"cnt 0xFFFFFFFF, n_dests {n_dests}")
    e1 = _virtual_csr(pairs, values, n, cut)[0]
    e2 = _virtual_csr(huge, values, n, cut)[0]
    assert e1 < e2 == cut   # (the long span alone fills the virtual CSR up to cap)


@pytest.mark.parametrize("n_dests", BOTH)
def test_overlapping_and_repeated_spans(torch_dev, index, G, n_dests):
    """spans that overlap and repeat, their effective counts summing far past cap: the virtual CSR is
    clipped at cap, nothing is written outside the outputs"""
    rng = np.random.default_rng(70 + n_dests)
    n, cap = 900, 64 * G + 100
    tab = _table(rng, n_dests, 3000)
    values = _values(rng, cap, len(tab))
    pos = rng.integers(0, cap + 50, n)
    cnt = rng.integers(0, 3000, n)
    pos[100:110], cnt[100:110] = pos[100], cnt[100] + 1   # the same span ten times
    cnt[5], cnt[6] = FF, cap
    pos[7] = 0
    pairs = np.stack([pos, cnt], axis=1).astype(np.int64)
    eff = np.where(pos >= cap, 0, np.minimum(cnt, cap - pos))
    assert eff.sum() > 3 * cap
    r = Run(torch_dev, index, pairs, values, n, cap, n_dests, tab)
    assert r.E == cap
    r.check(f"overlapping spans, n_dests {n_dests}")
    # few enough that the sum stays below cap: every span read, the repeated ones twice
    small = pairs[95:125].copy()
    small[:, 1] = np.minimum(small[:, 1], 500)
    r = Run(torch_dev, index, small, values, len(small), cap, n_dests, tab)
    assert 0 < r.E < cap
    r.check(f"repeated spans below cap, n_dests {n_dests}")


def test_garbage_after_the_pairs_changes_nothing(torch_dev, index, G):
    """d_pairs[2 n] and [2 n + 1] (a producer's total and extent) are not read: 0xFFFFFFFF, zeros and
    the true total give the same outputs"""
    rng = np.random.default_rng(13)
    lens = _spread(rng, 2000, 64 * G + 9)
    for n_dests in BOTH:
        tab = _table(rng, n_dests, 4000)
        vals = _values(rng, int(lens.sum()), len(tab))
        pairs, values, cap = _layout(rng, lens, vals, "permuted")
        outs = [Run(torch_dev, index, pairs, values, len(lens), cap, n_dests, tab, tail=tail).check(f"tail {tail}")
                for tail in ((FF, FF), (0, 0), (int(lens.sum()), cap))]
        for o in outs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))


@pytest.mark.parametrize("n_dests", [1, 255, 256, 257, 65536])
def test_destination_counts(torch_dev, index, G, n_dests):
    """the pass boundary (256 / 257 buckets) and the largest ids, on the permuted layout"""
    rng = np.random.default_rng(n_dests)
    total = 2 * 64 * G + 99
    lens = _spread(rng, 1500, total)
    tab = _table(rng, n_dests, 200_000)
    vals = _values(rng, total, len(tab))
    b = _buckets(vals, tab, n_dests)
    assert (b == n_dests - 1).any() and (b == n_dests).any() and (b == 0).any()
    pairs, values, cap = _layout(rng, lens, vals, "permuted")
    Run(torch_dev, index, pairs, values, len(lens), cap, n_dests, tab).check(f"n_dests {n_dests}")


def test_large_then_small_on_one_stream(torch_dev, index, G):
    """a large run, then small ones, on one stream without a release in between: nothing of the large
    run's tables, scratch or offsets shows in the small ones"""
    rng = np.random.default_rng(14)
    for n_dests in BOTH + (65536,):
        tab = _table(rng, n_dests, 4000)
        for total, n in ((6 * 64 * G + 5, 9000), (100, 50), (0, 50), (G + 3, 7000), (6 * 64 * G + 5, 100), (1, 1)):
            lens = _spread(rng, n, total)
            pairs, values, cap = _layout(rng, lens, _values(rng, total, len(tab)), "permuted")
            Run(torch_dev, index, pairs, values, n, cap, n_dests, tab).check(f"total {total} after a larger run, n_dests {n_dests}")


def test_three_streams_in_flight(torch_dev, index, G):
    """three streams, different inputs and pass counts, queued before any is waited for"""
    torch = torch_dev
    rng = np.random.default_rng(15)
    streams = [torch.cuda.Stream() for _ in range(3)]
    runs = []
    for rnd in range(3):
        for k, st in enumerate(streams):
            n_dests = (16, 300, 65536)[(k + rnd) % 3]
            total = (4 * 64 * G + 11, 64 * G - 1, 3000)[k]
            lens = _spread(rng, 500 + 1000 * k, total)
            tab = _table(rng, n_dests, 2000 + k)
            pairs, values, cap = _layout(rng, lens, _values(rng, total, len(tab)), "permuted")
            runs.append((Run(torch, index, pairs, values, len(lens), cap, n_dests, tab, stream=st),
                         f"stream {k} round {rnd} n_dests {n_dests}"))
    for r, what in runs:
        r.check(what)
    for st in streams:
        index.release_stream(st.cuda_stream)


def test_own_table(torch_dev):
    """d_dest_of == NULL: the table of tm_set_dests, uploaded in stream order before the fan-out; a
    second set_dests is seen by the next call"""
    torch = torch_dev
    ix = _native.Index()
    rng = np.random.default_rng(16)
    total = 40_000
    lens = _spread(rng, 700, total)
    vals = rng.integers(0, 6000, total, dtype=np.int64).astype(np.uint32)
    vals[:3] = (4999, 5000, FF)
    pairs, values, cap = _layout(rng, lens, vals, "permuted")
    for n_dests in BOTH:
        Run(torch, ix, pairs, values, 700, cap, n_dests, None).check("no table yet", table=np.zeros(0, np.uint32))
    host = np.full(5000, FF, np.uint32)
    ids = np.setdiff1d(np.arange(5000), np.concatenate([[17], np.arange(4000, 4100)])).astype(np.uint32)
    host[ids] = rng.integers(0, 300, len(ids))
    ix.set_dests(ids, host[ids])
    for n_dests in BOTH:
        Run(torch, ix, pairs, values, 700, cap, n_dests, None).check(f"own table, n_dests {n_dests}", table=host)
    st = torch.cuda.Stream()
    chg = np.array([0, 17, 4050, 4999, 5500], np.uint32)
    host = np.concatenate([host, np.full(501, FF, np.uint32)])
    host[chg] = (299, 5, 6, 0, 15)
    ix.set_dests(chg, host[chg])
    for n_dests in BOTH:
        Run(torch, ix, pairs, values, 700, cap, n_dests, None, stream=st).check(f"after a second set_dests, n_dests {n_dests}",
                                                                                table=host)
    ix.close()


def test_einval_before_any_device_work(torch_dev, index):
    """n_dests 0 or above 65536, null required pointers, d_pairs at 4 modulo 8, n >= 2^32 - 1: TM_EINVAL,
    nothing written"""
    lib, h = index._lib, index._h
    d = torch_dev.full((64,), OFFS_CANARY, dtype=torch_dev.int64, device="cuda")
    p = d.data_ptr()
    assert p % 8 == 0
    E = _native.TM_EINVAL
    f = lib.tm_fanout_dev_pairs
    assert f(h, 1, p, p, 8, p, 8, 0, p, p, p, None) == E
    assert f(h, 1, p, p, 8, p, 8, _native.MAX_DESTS + 1, p, p, p, None) == E
    assert f(h, 1, None, p, 8, p, 8, 4, p, p, p, None) == E
    assert f(h, 1, p, p, 8, p, 8, 4, None, p, p, None) == E
    assert f(h, 1, p, None, 8, p, 8, 4, p, p, p, None) == E
    assert f(h, 1, p, p, 8, p, 8, 4, p, None, p, None) == E
    assert f(h, 1, p, p, 8, p, 8, 4, p, p, None, None) == E
    assert f(h, 1, p + 4, p, 8, p, 8, 4, p, p, p, None) == E
    assert b"aligned" in lib.tm_last_error(h)
    assert f(h, U32 - 1, p, p, 8, p, 8, 4, p, p, p, None) == E
    torch_dev.cuda.synchronize()
    assert (d.cpu().numpy() == OFFS_CANARY).all()


# ------------------------------------------------- end to end on a real index

def _items(strings):
    blob, offs = _native.pack_strings(strings)
    return wl.ItemSet(blob, offs, np.arange(len(strings), dtype=np.uint32), np.zeros(len(strings), np.uint8))


OVERFLOW = [b"#", b"+/#", b"a/#", b"+/+/#", b"a/+/#", b"a/b/#", b"+/b/#", b"+/+/+", b"a/+/+", b"a/b/+", b"a/b/c"]
DEEP = b"/".join([b"z"] * 12)


@pytest.fixture(scope="module")
def routed(torch_dev):
    """a few thousand filters: a/b/c is matched by 11 distinct ones (more than the walk's 8 value runs:
    the overflow list), the z/... topics are 12 and 14 levels deep (the tail kernel's spans)"""
    filters = OVERFLOW + [DEEP, DEEP + b"/#", DEEP + b"/+/+", b"z/+/z/+/z/+/z/+/z/+/z/#", b"z/#"]
    filters += [b"dev/%d/+/t" % i for i in range(1200)] + [b"dev/+/%d/#" % i for i in range(1200)]
    filters += [b"dev/%d/#" % i for i in range(0, 1200, 3)] + [b"grp/%d/+" % i for i in range(600)]
    fs = _items(filters)
    ix = _native.Index()
    ix.apply(np.ones(len(fs), np.uint8), fs.blob, fs.offs, fs.vals)
    r = random.Random(21)

    def topic():
        k = r.random()
        if k < 0.15:
            return b"a/b/c"
        if k < 0.25:
            return DEEP if k < 0.2 else DEEP + b"/x/y"
        if k < 0.30:
            return b"nomatch"
        if k < 0.33:
            return b"bad/+/level"   # badarg: no hits
        if k < 0.40:
            return b"grp/%d/m" % r.randrange(700)
        return b"dev/%d/%d/t" % (r.randrange(1300), r.randrange(1300))
    return ix, len(filters), topic


def _match_csr(torch, ix, ts):
    n = len(ts)
    d_blob = torch.from_numpy(ts.blob.copy()).cuda()
    d_offs = torch.from_numpy(ts.offs.view(np.int64).copy()).cuda()
    cap = 16 * n
    d_hit = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_vals = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_err = torch.zeros(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ix.match_batch_dev(n, d_blob.data_ptr(), d_offs.data_ptr(), d_hit.data_ptr(), d_vals.data_ptr(), cap, d_err.data_ptr(), s)
    torch.cuda.synchronize()
    hit = d_hit.cpu().numpy()
    assert int(hit[n]) <= cap
    return d_blob, d_offs, d_hit, d_vals, hit


def _fan(torch, call, n, total, n_dests, *front):
    d_offs = torch.full((n_dests + 2 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
    d_topic = torch.from_numpy(np.full(total + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
    d_value = torch.from_numpy(np.full(total + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
    call(n, *front, n_dests, d_offs.data_ptr(), d_topic.data_ptr(), d_value.data_ptr())
    torch.cuda.synchronize()
    return d_offs.cpu().numpy(), d_topic.cpu().numpy().view(np.uint32), d_value.cpu().numpy().view(np.uint32)


def test_matched_batch_both_forms(torch_dev, routed):
    """40,000 topics (several regions) matched into a CSR and into pairs, both fanned out with the same
    table: identical bucket offsets, topics and values"""
    torch = torch_dev
    ix, nvals, topic = routed
    ts = _items([topic() for _ in range(40_000)])
    n = len(ts)
    d_blob, d_offs, d_hit, d_vals, hit = _match_csr(torch, ix, ts)
    total, most = int(hit[n]), int(np.diff(hit).max())
    assert most >= 11 and total > n
    cap = 8 * (total + 64 * most)   # enough for any layout (include/tmatch.h)
    d_pairs = torch.full((2 * n + 2,), -1, dtype=torch.int32, device="cuda")
    d_pv = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    d_err = torch.zeros(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_pv.data_ptr(), cap,
                             d_err.data_ptr(), s)
    torch.cuda.synchronize()
    p = d_pairs.cpu().numpy().view(np.uint32)
    assert int(p[2 * n]) == total
    assert int(p[2 * n + 1]) <= cap, "values dropped with the capacity that is enough for any layout"
    live_pos = p[0:2 * n:2][p[1:2 * n:2] > 0].astype(np.int64)
    assert (np.diff(live_pos) < 0).any() and (p[1:2 * n:2] == 0).any(), "spans in topic order or no empty topic: too easy"
    rng = np.random.default_rng(22)
    for n_dests in BOTH:
        tab = _table(rng, n_dests, nvals)
        d_tab = torch.from_numpy(tab.view(np.int32)).cuda()
        a = _fan(torch, lambda n, hitp, valp, cp, nd, o, t, v: ix.fanout_dev(n, hitp, valp, cp, nd, o, t, v, d_tab.data_ptr(), nvals, s),
                 n, total, n_dests, d_hit.data_ptr(), d_vals.data_ptr(), total)
        b = _fan(torch, lambda n, pp, valp, cp, nd, o, t, v: ix.fanout_dev_pairs(n, pp, valp, cp, nd, o, t, v, d_tab.data_ptr(), nvals, s),
                 n, total, n_dests, d_pairs.data_ptr(), d_pv.data_ptr(), cap)
        assert int(a[0][n_dests + 1]) == total
        for x, y, name in zip(a, b, ("bucket offsets", "topics", "values")):
            assert np.array_equal(x, y), f"n_dests {n_dests}: the {name} of the two forms differ"
        assert (a[1][total:] == CANARY).all() and (b[2][total:] == CANARY).all()
    assert np.array_equal(d_pairs.cpu().numpy().view(np.uint32), p)


def test_small_form_pairs(torch_dev, routed):
    """tm_match_batch32_pairs' output (2 n + 1 words) of a 3,000-topic batch, uploaded, against the CSR
    fan-out of the same batch"""
    torch = torch_dev
    ix, nvals, topic = routed
    items = [topic() for _ in range(3000)]
    blob, offs = _native.pack_strings(items)
    n = len(items)
    hit, vals, _ = ix.match_batch(blob, offs)
    total = int(hit[n])
    cap = 64 * n + 64
    pb = ix.host_array(len(blob) + 16, np.uint8)
    pb[:len(blob)] = blob
    po = ix.host_array(n + 1, np.uint32)
    po[:] = offs.astype(np.uint32)
    out = (ix.host_array(2 * n + 1, np.uint32), ix.host_array(cap, np.uint32), ix.host_array(n, np.uint8))
    pairs, pvals, _ = ix.match_batch32_pairs(pb, po, out)
    assert int(pairs[2 * n]) == total and int((pairs[0:2 * n:2].astype(np.int64) + pairs[1:2 * n:2]).max()) <= cap
    d_pairs = torch.from_numpy(pairs.view(np.int32).copy()).cuda()
    d_pv = torch.from_numpy(pvals.view(np.int32).copy()).cuda()
    d_hit = torch.from_numpy(hit.view(np.int64).copy()).cuda()
    d_vals = torch.from_numpy(np.concatenate([vals, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(23)
    for n_dests in BOTH:
        tab = _table(rng, n_dests, nvals)
        d_tab = torch.from_numpy(tab.view(np.int32)).cuda()
        a = _fan(torch, lambda n, hitp, valp, cp, nd, o, t, v: ix.fanout_dev(n, hitp, valp, cp, nd, o, t, v, d_tab.data_ptr(), nvals, s),
                 n, total, n_dests, d_hit.data_ptr(), d_vals.data_ptr(), total)
        b = _fan(torch, lambda n, pp, valp, cp, nd, o, t, v: ix.fanout_dev_pairs(n, pp, valp, cp, nd, o, t, v, d_tab.data_ptr(), nvals, s),
                 n, total, n_dests, d_pairs.data_ptr(), d_pv.data_ptr(), cap)
        for x, y, name in zip(a, b, ("bucket offsets", "topics", "values")):
            assert np.array_equal(x, y), f"n_dests {n_dests}: the {name} of the two forms differ"
