"""The route fan-out driven directly: tm_fanout_dev on synthetic CSRs built in
numpy, exact against np.argsort(bucket, kind="stable") -- no index content
involved (the pattern of test_gpu_postpass.py).

A pass runs on G = TM_DEBUG_FANOUT_GRID one-wave blocks; block k owns the
positions [k * chunk, (k + 1) * chunk), chunk = ceil(E / G) rounded up to 64,
E = min(hit[n], cap).  So totals around 64 * G put the chunk size on both sides
of one step, totals below G leave most blocks empty, and a topic holding 3/4 of
the entries is longer than any chunk.  A first pass finds topics from the
offsets with a 64-entry window: runs of 1, 63, 64, 65 and 200 empty topics at
the start, in the middle and at the end cross it.  n_dests + 1 <= 256 buckets
take one pass, more take two (low digit, then high, through per-stream
scratch): 255 / 256 / 257 sit on that boundary, 65535 / 65536 fill the high
digit (bucket ids >= 2^15, and the 17-bit id 65536 of the unrouted bucket).
Every output buffer carries a canary tail.
"""
import numpy as np
import pytest

from emqx_amd import _native

pytestmark = pytest.mark.gpu

CANARY = 0xC0FFEE11
OFFS_CANARY = -77
TAIL = 64
U32 = 1 << 32


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def index(torch_dev):
    """an empty index: tm_fanout_dev needs a handle for its scratch (and its own table) only"""
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


def _ref(hit, vals, n, cap, dest_of, n_dests):
    """-> (dest_offsets u64[n_dests + 2], topic u32[E], value u32[E]) for E = min(hit[n], cap)"""
    E = min(int(hit[n]), cap)
    lens = np.diff(hit[:n + 1].astype(np.int64))
    topic = np.repeat(np.arange(n, dtype=np.uint32), lens)[:E]
    v = vals[:E]
    b = _buckets(v, dest_of, n_dests)
    order = np.argsort(b, kind="stable")
    offs = np.zeros(n_dests + 2, np.uint64)
    offs[1:] = np.cumsum(np.bincount(b, minlength=n_dests + 1))
    return offs, topic[order], v[order]


class Run:
    """one tm_fanout_dev call's device buffers (kept alive until checked)"""

    def __init__(self, torch, ix, hit, vals, n, cap, n_dests, dest_of, stream=None):
        self.torch, self.args = torch, (hit, vals, n, cap, dest_of, n_dests)
        E = min(int(hit[n]), cap)
        self.E = E
        with torch.cuda.stream(stream) if stream is not None else _Null():
            self.d_hit = torch.from_numpy(hit.view(np.int64).copy()).cuda()
            self.d_vals = torch.from_numpy(np.concatenate([vals, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
            self.d_tab = None if dest_of is None else \
                torch.from_numpy(np.concatenate([dest_of, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
            self.d_offs = torch.full((n_dests + 2 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.d_topic = torch.from_numpy(np.full(E + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
            self.d_value = torch.from_numpy(np.full(E + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
            s = torch.cuda.current_stream().cuda_stream
            ix.fanout_dev(n, self.d_hit.data_ptr(), self.d_vals.data_ptr(), cap, n_dests, self.d_offs.data_ptr(),
                          self.d_topic.data_ptr(), self.d_value.data_ptr(),
                          None if dest_of is None else self.d_tab.data_ptr(), 0 if dest_of is None else len(dest_of), s)

    def check(self, what, table=None):
        """exact outputs, canary tails, inputs unmodified"""
        hit, vals, n, cap, dest_of, n_dests = self.args
        self.torch.cuda.synchronize()
        offs, topic, value = _ref(hit, vals, n, cap, dest_of if table is None else table, n_dests)
        E = self.E
        g_offs = self.d_offs.cpu().numpy()
        g_topic = self.d_topic.cpu().numpy().view(np.uint32)
        g_value = self.d_value.cpu().numpy().view(np.uint32)
        assert np.array_equal(g_offs[:n_dests + 2].view(np.uint64), offs), f"{what}: bucket offsets differ"
        assert (g_offs[n_dests + 2:] == OFFS_CANARY).all(), f"{what}: wrote past dest_offsets[n_dests + 1]"
        bad = np.nonzero((g_topic[:E] != topic) | (g_value[:E] != value))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {E} entries differ, first at {bad[0]}: " \
                              f"({g_topic[bad[0]]}, {g_value[bad[0]]}) for ({topic[bad[0]]}, {value[bad[0]]})"
        assert (g_topic[E:] == CANARY).all() and (g_value[E:] == CANARY).all(), f"{what}: wrote past min(total, cap)"
        assert np.array_equal(self.d_hit.cpu().numpy().view(np.uint64), hit), f"{what}: the offsets were written"
        assert np.array_equal(self.d_vals.cpu().numpy().view(np.uint32)[:len(vals)], vals), f"{what}: the values were written"


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def _check(torch, ix, hit, vals, n_dests, dest_of, what, cap=None):
    n = len(hit) - 1
    Run(torch, ix, hit, vals, n, len(vals) if cap is None else cap, n_dests, dest_of).check(what)


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
    t[rng.integers(0, length, 3)] = 0xFFFFFFFF
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


BOTH = (16, 300)   # one pass, two passes


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 70001])
def test_topic_counts_and_totals(torch_dev, index, G, n):
    """every n with every total around the step (64) and the grid (64 * G), entries spread at random"""
    rng = np.random.default_rng(100 + n)
    totals = (0, 1, 63, 64, 65, G - 1, 64 * G - 1, 64 * G, 64 * G + 1, 5 * 64 * G + 17) if n else (0,)
    for total in totals:
        lens = _spread(rng, n, total)
        hit = _hit(lens)
        for n_dests in BOTH:
            tab = _table(rng, n_dests, 5000)
            _check(torch_dev, index, hit, _values(rng, total, len(tab)), n_dests, tab, f"n {n} total {total} n_dests {n_dests}")


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


def test_segment_layouts(torch_dev, index, G):
    """all empty; empty runs around the window size at the start, the middle
    and the end; one topic with 3/4 of the entries; every topic of length 1"""
    rng = np.random.default_rng(7)
    n, total = 3000, 64 * G + 4321
    big = _spread(rng, n, total // 4)
    big[n // 3] += total - total // 4
    layouts = {"all empty": np.zeros(n, np.int64), "empty runs": _with_empty_runs(rng, n, total),
               "one long topic": big, "all of length 1": np.ones(n, np.int64),
               "all of length 1, many": np.ones(64 * G + 65, np.int64),
               "one long topic alone": np.array([0, 0, 3 * G * 64 + 5, 0], np.int64)}
    chunk = ((total + G - 1) // G + 63) // 64 * 64
    assert big.max() > 100 * chunk
    for name, lens in layouts.items():
        hit = _hit(lens)
        for n_dests in BOTH:
            tab = _table(rng, n_dests, 777)
            _check(torch_dev, index, hit, _values(rng, int(hit[-1]), len(tab)), n_dests, tab, f"{name}, n_dests {n_dests}")


@pytest.mark.parametrize("n_dests", [1, 2, 255, 256, 257, 4096, 65535, 65536])
def test_destination_counts(torch_dev, index, G, n_dests):
    """the pass boundary (256 / 257 buckets) and the largest ids; both digits vary, id n_dests - 1 occurs"""
    rng = np.random.default_rng(n_dests)
    total = 2 * 64 * G + 99
    hit = _hit(_spread(rng, 1500, total))
    tab = _table(rng, n_dests, 200_000)
    vals = _values(rng, total, len(tab))
    b = _buckets(vals, tab, n_dests)
    assert (b == n_dests - 1).any() and (b == n_dests).any() and (b == 0).any()
    if n_dests > 256:
        assert len(np.unique(b & 0xFF)) > 200 and len(np.unique(b >> 8)) >= min(n_dests >> 8, 200)
    if n_dests >= 65535:
        assert (b >= 1 << 15).sum() > total // 4
    _check(torch_dev, index, hit, vals, n_dests, tab, f"n_dests {n_dests}")


def test_unrouted_through_both_routes(torch_dev, index):
    """v >= dest_len with full-range u32 values and a short table; dest_of[v] >= n_dests, 0xFFFFFFFF included;
    an empty table (dest_len 0)"""
    rng = np.random.default_rng(3)
    total = 50_000
    hit = _hit(_spread(rng, 900, total))
    vals = rng.integers(0, U32, total, dtype=np.int64).astype(np.uint32)
    vals[:4] = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
    vals[rng.integers(0, total, 5000)] = rng.integers(0, 40, 5000)
    for n_dests in BOTH + (65536,):
        tab = np.arange(40, dtype=np.uint32) % 7
        tab[5], tab[6], tab[7], tab[8] = n_dests, n_dests + 1, 0x80000000, 0xFFFFFFFF
        b = _buckets(vals, tab, n_dests)
        assert (b == n_dests).sum() > total // 2 and (b < n_dests).sum() > 1000
        _check(torch_dev, index, hit, vals, n_dests, tab, f"short table, n_dests {n_dests}")
        _check(torch_dev, index, hit, vals, n_dests, np.zeros(0, np.uint32), f"empty table, n_dests {n_dests}")
        allbad = np.full(40, 0xFFFFFFFF, np.uint32)
        _check(torch_dev, index, hit, vals % 40, n_dests, allbad, f"every entry >= n_dests, n_dests {n_dests}")


def test_one_bucket_and_descending_buckets(torch_dev, index, G):
    """every entry in one bucket (the order must stay the input's); buckets strictly descending with position"""
    rng = np.random.default_rng(4)
    total = 64 * G + 1000
    hit = _hit(_spread(rng, 2000, total))
    vals = rng.integers(0, 1000, total, dtype=np.int64).astype(np.uint32)
    for n_dests, only in ((16, 11), (255, 254), (300, 299), (65536, 65535), (65536, 0x8000)):
        _check(torch_dev, index, hit, vals, n_dests, np.full(1000, only, np.uint32), f"all in bucket {only} of {n_dests}")
    for n_dests, total in ((255, 255), (256, 257), (5000, 5000), (65536, 65536)):
        hit = _hit(_spread(rng, 300, total))
        vals = np.arange(total, dtype=np.uint32)
        tab = (total - 1 - np.arange(total)).astype(np.uint32)   # position p -> bucket total - 1 - p
        r = Run(torch_dev, index, hit, vals, 300, total, n_dests, tab)
        r.check(f"descending buckets, n_dests {n_dests}")
        assert np.array_equal(r.d_value.cpu().numpy().view(np.uint32)[:total], vals[::-1])


@pytest.mark.parametrize("n_dests", BOTH)
def test_cap_below_total(torch_dev, index, G, n_dests):
    """positions >= cap are neither counted nor written (the canaries after
    min(total, cap) survive), the inputs are not modified"""
    rng = np.random.default_rng(50 + n_dests)
    total = 3 * 64 * G + 77
    lens = _spread(rng, 1200, total)
    hit = _hit(lens)
    tab = _table(rng, n_dests, 3000)
    vals = _values(rng, total, len(tab))
    inside = int(hit[600]) + int(lens[600]) // 2   # a cap inside a topic's list
    for cap in (0, 1, 63, 64, 65, 64 * G, inside, total - 1, total, total + 1000):
        _check(torch_dev, index, hit, vals, n_dests, tab, f"cap {cap} of {total}, n_dests {n_dests}", cap=cap)


def test_large_then_small_on_one_stream(torch_dev, index, G):
    """a large run, then small ones, on one stream without a release in between: nothing of the
    large run's tables, totals or scratch shows in the small ones"""
    rng = np.random.default_rng(6)
    for n_dests in BOTH + (65536,):
        tab = _table(rng, n_dests, 4000)
        for total, n in ((6 * 64 * G + 5, 9000), (100, 50), (0, 50), (G + 3, 7000), (6 * 64 * G + 5, 100), (1, 1)):
            hit = _hit(_spread(rng, n, total))
            _check(torch_dev, index, hit, _values(rng, total, len(tab)), n_dests, tab,
                   f"total {total} after a larger run, n_dests {n_dests}")


def test_three_streams_in_flight(torch_dev, index, G):
    """three streams, different inputs and pass counts, queued before any is waited for"""
    torch = torch_dev
    rng = np.random.default_rng(8)
    streams = [torch.cuda.Stream() for _ in range(3)]
    runs = []
    for rnd in range(3):
        for k, st in enumerate(streams):
            n_dests = (16, 300, 65536)[(k + rnd) % 3]
            total = (4 * 64 * G + 11, 64 * G - 1, 3000)[k]
            hit = _hit(_spread(rng, 500 + 1000 * k, total))
            tab = _table(rng, n_dests, 2000 + k)
            runs.append((Run(torch, index, hit, _values(rng, total, len(tab)), len(hit) - 1, total, n_dests, tab, stream=st),
                         f"stream {k} round {rnd} n_dests {n_dests}"))
    for r, what in runs:
        r.check(what)
    for st in streams:
        index.release_stream(st.cuda_stream)


def test_own_table(torch_dev):
    """d_dest_of == NULL: the table of tm_set_dests -- before any set_dests every
    value is unrouted; a second set_dests changing a few values is seen by the
    next fan-out; a value never set is unrouted"""
    torch = torch_dev
    ix = _native.Index()
    rng = np.random.default_rng(9)
    total = 40_000
    hit = _hit(_spread(rng, 700, total))
    vals = rng.integers(0, 6000, total, dtype=np.int64).astype(np.uint32)
    vals[:3] = (4999, 5000, 0xFFFFFFFF)
    for n_dests in BOTH:
        Run(torch, ix, hit, vals, 700, total, n_dests, None).check("no table yet", table=np.zeros(0, np.uint32))
    # values 0 .. 4999 set, except 17 and 4000 .. 4099; 5000 and above never
    host = np.full(5000, 0xFFFFFFFF, np.uint32)
    ids = np.setdiff1d(np.arange(5000), np.concatenate([[17], np.arange(4000, 4100)])).astype(np.uint32)
    host[ids] = rng.integers(0, 300, len(ids))
    ix.set_dests(ids, host[ids])
    for n_dests in BOTH:   # (16: ids 16 .. 299 are >= n_dests there)
        Run(torch, ix, hit, vals, 700, total, n_dests, None).check(f"own table, n_dests {n_dests}", table=host)
    assert (_buckets(vals, host, 300) == 300).sum() > 100
    # a few changed, one beyond the host table's end, on another stream
    st = torch.cuda.Stream()
    chg = np.array([0, 17, 4050, 4999, 5500], np.uint32)
    host = np.concatenate([host, np.full(501, 0xFFFFFFFF, np.uint32)])
    host[chg] = (299, 5, 6, 0, 15)
    ix.set_dests(chg, host[chg])
    for n_dests in BOTH:
        Run(torch, ix, hit, vals, 700, total, n_dests, None, stream=st).check(f"after a second set_dests, n_dests {n_dests}",
                                                                              table=host)
    ix.set_dests(np.array([17], np.uint32), np.array([0xFFFFFFFF], np.uint32))   # back to unrouted
    host[17] = 0xFFFFFFFF
    Run(torch, ix, hit, vals, 700, total, 16, None).check("a destination taken away", table=host)
    ix.close()


def test_einval_before_any_device_work(torch_dev, index):
    """n_dests 0 or above 65536, null required pointers: TM_EINVAL, nothing written"""
    lib, h = index._lib, index._h
    d = torch_dev.full((64,), OFFS_CANARY, dtype=torch_dev.int64, device="cuda")
    p = d.data_ptr()
    E = _native.TM_EINVAL
    assert lib.tm_fanout_dev(h, 1, p, p, 8, p, 8, 0, p, p, p, None) == E
    assert lib.tm_fanout_dev(h, 1, p, p, 8, p, 8, _native.MAX_DESTS + 1, p, p, p, None) == E
    assert lib.tm_fanout_dev(h, 1, None, p, 8, p, 8, 4, p, p, p, None) == E
    assert lib.tm_fanout_dev(h, 1, p, p, 8, p, 8, 4, None, p, p, None) == E
    assert lib.tm_fanout_dev(h, 1, p, None, 8, p, 8, 4, p, p, p, None) == E
    assert lib.tm_fanout_dev(h, 1, p, p, 8, p, 8, 4, p, None, p, None) == E
    assert lib.tm_fanout_dev(h, 1, p, p, 8, p, 8, 4, p, p, None, None) == E
    assert lib.tm_set_dests(h, 1, None, None) == E
    offs = np.zeros(2, np.uint64)
    out = np.zeros(8, np.uint64)
    P = _native._ptr
    assert lib.tm_route_batch(h, 1, None, P(offs), 0, P(out), P(out), P(out), 2, None) == E
    assert lib.tm_route_batch(h, 1, None, P(offs), _native.MAX_DESTS + 1, P(out), P(out), P(out), 2, None) == E
    assert lib.tm_route_batch(h, 1, None, None, 4, P(out), P(out), P(out), 2, None) == E
    assert lib.tm_route_batch(h, 1, None, P(offs), 4, None, P(out), P(out), 2, None) == E
    assert lib.tm_route_batch(h, 1, None, P(offs), 4, P(out), None, P(out), 2, None) == E
    torch_dev.cuda.synchronize()
    assert (d.cpu().numpy() == OFFS_CANARY).all()


def test_own_table_gap_below_a_high_value_is_unrouted(torch_dev):
    """set_dests of one low value, a fan-out (the device copy exists), then
    set_dests of one high value only: the values between them were never set,
    so they are unrouted -- the device must not read entries there that the
    host never wrote"""
    torch = torch_dev
    ix = _native.Index()
    rng = np.random.default_rng(10)
    total = 20_000
    hit = _hit(_spread(rng, 300, total))
    vals = rng.integers(0, 3500, total, dtype=np.int64).astype(np.uint32)
    vals[:4] = (10, 11, 500, 3000)
    host = np.full(11, 0xFFFFFFFF, np.uint32)
    host[10] = 3
    ix.set_dests(np.array([10], np.uint32), np.array([3], np.uint32))
    for n_dests in BOTH:
        Run(torch, ix, hit, vals, 300, total, n_dests, None).check(f"one low value, n_dests {n_dests}", table=host)
    host = np.concatenate([host, np.full(2990, 0xFFFFFFFF, np.uint32)])
    host[3000] = 2
    ix.set_dests(np.array([3000], np.uint32), np.array([2], np.uint32))
    for n_dests in BOTH:
        r = Run(torch, ix, hit, vals, 300, total, n_dests, None)
        r.check(f"one high value after it, n_dests {n_dests}", table=host)
        offs = r.d_offs.cpu().numpy()
        assert offs[n_dests + 1] - offs[n_dests] == ((vals != 10) & (vals != 3000)).sum(), "the gap is not unrouted"
    ix.close()
