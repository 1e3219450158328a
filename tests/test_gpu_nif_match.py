"""The NIF core's match half on the real library: c_src/tmatch_nif_core.c's
tmn_pack, tmn_match, tmn_row, tmn_first and tmn_first_row, linked (with the
other six units and tests/native/nif_chain_shim.c) against
emqx_amd/libtmatch.so and run on the device.

The reference is the oracle (oracle/pyoracle.py): a topic's row is the oracle's
list in traversal order, numpy.sort of it in TM_ORDER_SORTED and numpy.unique of
it in TM_ORDER_UNIQUE; tmn_first_row is Oracle.first.  Every row of every batch
is compared, the flags with it.  Only the 65,537-topic batch is compared whole
against Index.match_batch / first_batch (the staged 64-bit calls, which
tests/test_gpu_parity.py pins to the oracle) and in a 2,000-topic sample
against the oracle itself.

The index holds values that several filters share, so a topic's hits contain a
value more than once: unique differs from sorted, and a tmn_row that took the
CSR's next offset for a unique row's end would hand out the padding.
"""
import numpy as np
import pytest

from emqx_amd import _native
from nif_chain import VALUES, Caller, load
from pyoracle import Oracle
from test_gpu_route_batch32 import _routed_filters, _topics

pytestmark = pytest.mark.gpu

VRAM = _native.TM_ALLOC_VRAM
TRAVERSAL, SORTED, UNIQUE = _native.TM_ORDER_TRAVERSAL, _native.TM_ORDER_SORTED, _native.TM_ORDER_UNIQUE
ORDERS = {"traversal": TRAVERSAL, "sorted": SORTED, "unique": UNIQUE}
PLACES = {"pinned": 0, "vram": VRAM}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def nif(tmp_path_factory, gpu):
    return load(tmp_path_factory.mktemp("nifmatch"))


class Both:
    """one table on the device and in the oracle"""

    def __init__(self, filters, values):
        self.ix, self.o = _native.Index(), Oracle()
        blob, offs = _native.pack_strings(filters)
        values = np.asarray(values, np.uint32)
        self.ix.apply(np.ones(len(filters), np.uint8), blob, offs, values)
        self.o.apply(np.ones(len(filters), np.uint8), blob, offs, values)
        self.o.prepare()

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.ix.close()


@pytest.fixture(scope="module")
def table(gpu):
    """test_gpu_route_batch32's filters with values i % 700 (filters share values), and four filters under
    'dup/' that give one topic the value 5 three times"""
    fs = _routed_filters()
    vals = [i % 700 for i in range(len(fs))]
    fs += [b"dup/+/x", b"dup/#", b"dup/y/+", b"dup/y/x"]
    vals += [5, 5, 5, 9]
    t = Both(fs, vals)
    yield t
    t.close()


@pytest.fixture(scope="module")
def fat(gpu):
    """300 values under every topic 't/<i>', 50 of them twice: 20 topics hold 6,000 values, beyond a fresh set's
    first capacity (TMN_IDS_PER_TOPIC per topic + 1024, and the half tmn_get allocates on top)"""
    t = Both([b"#"] * 250 + [b"t/#"] * 50, list(range(250)) + list(range(50)))
    yield t
    t.close()


def batch(n, seed):
    out = _topics(n, seed=seed)
    out[1], out[n // 2], out[n - 1] = b"dup/y/x", b"dup/z/x", b"dup/y/x"
    return out


def expected(o, topics, order):
    """the oracle's rows -> (flags u8[n], counts i64[n], the rows' values one after the other)"""
    flags, rows = np.zeros(len(topics), np.uint8), []
    for i, t in enumerate(topics):
        m = o.matches(t)
        if m is None:
            flags[i] = 1
            m = []
        m = np.asarray(m, np.uint32)
        rows.append(m if order == TRAVERSAL else np.sort(m) if order == SORTED else np.unique(m))
    cnt = np.array([len(r) for r in rows], np.int64)
    return flags, cnt, np.concatenate(rows) if rows else np.zeros(0, np.uint32)


def same_rows(c, o, topics, order):
    flags, cnt, vals = c.rows(len(topics), order)
    eflags, ecnt, evals = expected(o, topics, order)
    assert np.array_equal(flags, eflags), "the rows' flags"
    assert np.array_equal(cnt, ecnt), "the rows' lengths"
    assert np.array_equal(vals, evals), "the rows' values"
    return ecnt


def expected_first(o, topics):
    found, val = np.zeros(len(topics), np.uint8), np.zeros(len(topics), np.uint32)
    for i, t in enumerate(topics):
        r, v = o.first(t)
        found[i] = {1: 1, 0: 0, -1: 2, -2: 3}[r]
        val[i] = v if r == 1 else 0
    return found, val


def same_firsts(c, o, topics):
    found, val = c.firsts(len(topics))
    efound, eval_ = expected_first(o, topics)
    assert np.array_equal(found, efound), "found / none / badarg per topic"
    assert np.array_equal(val[efound == 1], eval_[efound == 1]), "the first value"
    return efound


# ---- B1. the three orders

@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("order", ORDERS)
def test_rows_in_every_order(table, nif, order, place):
    """tmn_match + tmn_row == the oracle's list / numpy.sort / numpy.unique of it, 400 topics, inputs pinned and
    in device memory; 'dup/y/x' holds the value 5 three times"""
    topics = batch(400, seed=21)
    m = np.asarray(table.o.matches(b"dup/y/x"))
    assert len(m) > len(np.unique(m)) and (m == 5).sum() == 3, "no topic with a duplicate value"
    c = Caller(nif, table.ix, PLACES[place])
    try:
        assert c.pack(topics) == 0 and c.input_flags in (0, PLACES[place])
        assert c.match(len(topics), ORDERS[order]) == 0
        cnt = same_rows(c, table.o, topics, ORDERS[order])
        assert cnt.sum() > 500 and (cnt == 0).sum() > 3
        topics = topics[:37]                                     # a smaller batch in the same buffers
        assert c.pack(topics) == 0 and c.match(len(topics), ORDERS[order]) == 0
        same_rows(c, table.o, topics, ORDERS[order])
    finally:
        c.close()


# ---- B2. a forced TM_ECAP rerun in each order

@pytest.mark.parametrize("order", ORDERS)
def test_a_forced_rerun_in_every_order(fat, nif, order):
    """20 topics x 300 values on a fresh set: ONE rerun with room for the exact total, the rows still the oracle's
    (50 values twice per topic: 250 distinct); the same batch again needs none"""
    topics = [b"t/%d" % i for i in range(20)]
    want = nif.shim_ids_per_topic() * len(topics) + 1024
    first = nif.shim_first_cap(fat.ix._h, want)
    total = sum(len(fat.o.matches(t)) for t in topics)
    print(f"planned match-{order}: total={total} capacity={first}")
    assert total == 6000 > first, "the shape does not force a rerun"
    c = Caller(nif, fat.ix, VRAM)
    try:
        assert c.pack(topics) == 0 and c.match(len(topics), ORDERS[order]) == 0
        assert c.reruns == 1 and c.cap(VALUES) >= total
        cnt = same_rows(c, fat.o, topics, ORDERS[order])
        assert cnt.tolist() == [250 if order == "unique" else 300] * 20
        assert c.match(len(topics), ORDERS[order]) == 0 and c.reruns == 1, "the sizes are sticky"
        same_rows(c, fat.o, topics, ORDERS[order])
    finally:
        c.close()


# ---- B3. tmn_first

@pytest.mark.parametrize("place", PLACES)
def test_first_rows(table, nif, place):
    """tmn_first + tmn_first_row == Oracle.first: 1 and the value, 0 for no match, 2 for a '+' / '#' level; with
    inputs in device memory the u64 offsets are the ones tmn_pack kept on the host.  Then on a set whose previous
    call was a tmn_match of a larger batch: the value, flag and offset buffers are reused, stale"""
    topics = batch(300, seed=31)
    c = Caller(nif, table.ix, PLACES[place])
    try:
        assert c.pack(topics) == 0 and c.first(len(topics)) == 0
        found = same_firsts(c, table.o, topics)
        assert all((found == k).sum() > 2 for k in (0, 1, 2)), "found, none and badarg all occur"
        bigger = batch(900, seed=32)
        assert c.pack(bigger) == 0 and c.match(len(bigger), SORTED) == 0
        same_rows(c, table.o, bigger, SORTED)
        small = [b"dup/y/x", b"+/b", b"zzz", b"a1/b1/c1", b"#"] + batch(100, seed=33)
        assert c.pack(small) == 0 and c.first(len(small)) == 0
        found = same_firsts(c, table.o, small)
        assert found[:5].tolist() == [1, 2, 0, 1, 2]
    finally:
        c.close()


# ---- B4. more than 65,536 topics

def test_65537_short_topics(table, nif):
    """tmn_match (traversal) and tmn_first of 65,537 topics: the whole batch against Index.match_batch and
    first_batch, a 2,000-topic sample against the oracle"""
    n = 65537
    rng = np.random.default_rng(65)
    lv = rng.integers(0, 60, (n, 3))
    topics = [b"a%d/b%d/c%d" % (x, y % 45, z % 9) for x, y, z in lv.tolist()]
    topics[7], topics[n - 1], topics[n // 2] = b"dup/y/x", b"dup/y/x", b"a1/+/c1"
    blob, offs = _native.pack_strings(topics)
    hit, vals, err = table.ix.match_batch(blob, offs)
    fval, ffound = table.ix.first_batch(blob, offs)
    sample = np.sort(rng.choice(n, 2000, replace=False))
    sample[0], sample[-1] = 7, n - 1
    some = [topics[i] for i in sample.tolist()]
    eflags, ecnt, evals = expected(table.o, some, TRAVERSAL)
    efound, efirst = expected_first(table.o, some)
    c = Caller(nif, table.ix, VRAM)
    try:
        assert c.pack(topics) == 0 and c.match(n, TRAVERSAL) == 0
        flags, cnt, got = c.rows(n, TRAVERSAL)
        assert np.array_equal(flags, err) and np.array_equal(cnt, np.diff(hit.astype(np.int64)))
        assert np.array_equal(got, vals) and len(got) == int(hit[-1]) > n
        lo = np.concatenate(([0], np.cumsum(cnt)))
        assert np.array_equal(flags[sample], eflags) and np.array_equal(cnt[sample], ecnt)
        at = np.repeat(lo[sample] - np.concatenate(([0], np.cumsum(ecnt)[:-1])), ecnt) + np.arange(int(ecnt.sum()))
        assert np.array_equal(got[at], evals), "the sample's rows against the oracle"
        assert c.first(n) == 0
        found, val = c.firsts(n)
        assert np.array_equal(found, ffound) and np.array_equal(val[ffound == 1], fval[ffound == 1])
        assert np.array_equal(found[sample], efound) and np.array_equal(val[sample][efound == 1], efirst[efound == 1])
    finally:
        c.close()


# ---- B5. an index the one-launch walk refuses

def test_the_33_level_index(gpu, nif):
    """test_index_the_one_launch_walk_refuses's index: tmn_match in traversal order gets the CSR fallback
    converted to (offset, count) pairs -- the rows are the oracle's; sorted and unique as well"""
    deep = b"/".join(b"l%d" % i for i in range(33))
    t = Both([deep, b"l0/#", b"+/l1/#", b"l0/l1/#"], [0, 1, 2, 1])
    topics = [deep, b"l0/l1", b"x/l1/y", b"none", b"l0/+"] * 8
    c = Caller(nif, t.ix, VRAM)
    try:
        for order in (TRAVERSAL, SORTED, UNIQUE):
            assert c.pack(topics) == 0 and c.match(len(topics), order) == 0
            cnt = same_rows(c, t.o, topics, order)
            assert cnt[:5].tolist() == ([4, 3, 1, 0, 0] if order != UNIQUE else [3, 2, 1, 0, 0])
        assert c.first(len(topics)) == 0
        same_firsts(c, t.o, topics)
        assert c.reruns == 0
    finally:
        c.close()
        t.close()


# ---- B6. inputs in device memory or not: the same answers

def test_input_placement_changes_nothing(table, nif):
    """a pool without TM_ALLOC_VRAM, and one with it whose allocation the library may refuse (no large BAR: the
    set's in_flags then falls to 0 for good): either way the set says where its inputs are (shim_input_flags),
    asks for nothing else afterwards (shim_in_flags), and rows and firsts are the oracle's"""
    topics = batch(200, seed=41)
    for flags in (0, VRAM):
        c = Caller(nif, table.ix, flags)
        try:
            assert c.in_flags == flags
            for _ in range(2):
                assert c.pack(topics) == 0
                assert c.input_flags in (0, flags) and c.in_flags == c.input_flags, "a refused placement is not asked for again"
                assert c.match(len(topics), TRAVERSAL) == 0
                same_rows(c, table.o, topics, TRAVERSAL)
                assert c.match(len(topics), UNIQUE) == 0
                same_rows(c, table.o, topics, UNIQUE)
                assert c.first(len(topics)) == 0
                same_firsts(c, table.o, topics)
        finally:
            c.close()
