"""tm_route_batch_ex / tm_route_batch32_ex with TM_ROUTE_AGGRE: aggre/1 applied
on the device to the buckets of a routed micro-batch.

The reference everywhere is the flags-0 call on the same index state and topics
passed through the numpy definition of include/tmatch.h (_aggre) with the filter
table the test shipped; every compared array must be equal element for element,
every output buffer carries a canary tail that must survive at and past K, and
TM_DEBUG_ROUTE_ONE / TM_DEBUG_ROUTE_GRID say which path finished the call: the
one-launch fan-out followed by the one-workgroup compaction (up to FO1_TOPICS
topics, FO1_ENTRIES entries before aggregation, 256 buckets), or the grid
kernels / the staged path.
"""
import ctypes as C
import subprocess
import threading
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.broker import Broker, Message
from emqx_amd.router import Router

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FO1_TOPICS, FO1_ENTRIES = 8192, 16384   # emqx_amd/csrc/tm_dev.h
NONE = 0xFFFFFFFF
CANARY, OFFC, ERRC, TAIL = 0xC0FFEE11, 0xDEADBEEF, 0xEE, 64
ONE, GRID = _native.TM_DEBUG_ROUTE_ONE, _native.TM_DEBUG_ROUTE_GRID
AGG = _native.TM_ROUTE_AGGRE
OK, ECAP = _native.TM_OK, _native.TM_ECAP
N_DESTS = 5   # 3 nodes + 2 groups
P = _native._ptr


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


# ------------------------------------------------------------- the reference

def _aggre(doff, t, v, fof, n_dests):
    """the header's numpy definition on a whole fan-out -> (out_doff u64, topic, value)"""
    doff = doff.astype(np.int64)
    E = int(doff[n_dests + 1])
    assert len(t) == len(v) == E
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


# ------------------------------------------------------------------ the index

def _routes():
    """~300 filters with 1 .. 6 routes each over 3 nodes and 2 groups on 3 nodes each: value =
    the route's position, class ids n1 n2 n3 g1 g2 = 0 .. 4; every 17th route unrouted (its
    filter known), every 19th without a filter id -> (filters, dests, filter ids)"""
    rng = np.random.default_rng(99)
    names = []
    for i in range(300):
        names.append((f"a{i % 50}/+/c{i % 7}", f"a{i % 50}/#", f"+/b{i % 40}/#", f"a{i % 50}/b{i % 40}/+")[i % 4])
    names += [f"a{k % 50}/b{k % 40}/c{k % 7}" for k in range(40)]
    names = list(dict.fromkeys(names))
    options = [(c, n) for c in range(3) for n in (0,)] + [(3, n) for n in range(3)] + [(4, n) for n in range(3)]
    rows = []
    for fi, name in enumerate(names):
        for o in rng.choice(len(options), 1 + fi % 6, replace=False):
            rows.append((name.encode(), options[o][0], fi))
    rows = [rows[i] for i in rng.permutation(len(rows))]   # values in any order within a filter
    fs = [r[0] for r in rows]
    dests = [None if v % 17 == 0 else r[1] for v, r in enumerate(rows)]
    fids = [NONE if v % 19 == 0 else 7 * r[2] + 3 for v, r in enumerate(rows)]   # (ids need not be dense)
    return fs, dests, fids


def _insert(ix, filters, values, dests, fids):
    values = np.asarray(values, np.uint32)
    keep = [i for i, d in enumerate(dests) if d is not None]
    ix.set_dests(values[keep], np.array([dests[i] for i in keep], np.uint32))
    keep = [i for i, f in enumerate(fids) if f != NONE]      # (the others: never set)
    ix.set_route_filters(values[keep], np.array([fids[i] for i in keep], np.uint32))
    blob, offs = _native.pack_strings(filters)
    ix.apply(np.ones(len(filters), np.uint8), blob, offs, values)


def _routed_index(copies=1):
    ix = _native.Index(copies=copies)
    fs, dests, fids = _routes()
    _insert(ix, fs, np.arange(len(fs)), dests, fids)
    ix.fof = np.array(fids, np.uint32)
    return ix


@pytest.fixture(scope="module")
def routed(gpu):
    ix = _routed_index()
    yield ix
    ix.close()


def _topics(n, seed=1):
    rng = np.random.default_rng(seed)
    out = [f"a{rng.integers(0, 60)}/b{rng.integers(0, 45)}/c{rng.integers(0, 9)}".encode() for _ in range(n)]
    for i in range(0, n, 97):
        out[i] = (b"a1/+/c1", b"#", b"a/#/b")[i % 3]          # badarg
    for i in range(5, n, 89):
        out[i] = f"zzz{i}".encode()                          # no route at all (one level)
    return out


class Bufs:
    """one caller's batch buffers: host_array (pinned) or plain numpy; outputs with canary tails"""

    def __init__(self, ix, nmax, bytes_max, dmax, cap_max, pinned=True):
        def alloc(k, dt):
            return ix.host_array(k, dt) if pinned else np.zeros(max(k, 1), dt)
        self.ix, self.cap_max, self.pinned = ix, cap_max, pinned
        self.blob, self.offs = alloc(bytes_max + 48, np.uint8), alloc(nmax + 1, np.uint32)
        self.doff, self.err = alloc(dmax + 2 + TAIL, np.uint32), alloc(nmax + TAIL, np.uint8)
        self.topic, self.vals = alloc(cap_max + TAIL, np.uint32), alloc(cap_max + TAIL, np.uint32)

    def free(self):
        if self.pinned:
            for a in (self.blob, self.offs, self.doff, self.err, self.topic, self.vals):
                self.ix.host_free(a)

    def route(self, topics, n_dests, cap=None, flags=AGG, old=False):
        """-> (rc, dest_offsets, topic[:kept], values[:kept], err[:n]); the canaries checked.
        old: the call without flags (tm_route_batch32)"""
        blob, offs = _native.pack_strings(topics)
        n, nb = len(topics), int(offs[-1])
        cap = self.cap_max if cap is None else cap
        assert cap <= self.cap_max and n + 1 <= len(self.offs) and nb <= len(self.blob)
        self.blob[:nb] = blob[:nb]
        self.offs[:n + 1] = offs
        self.doff[:], self.topic[:], self.vals[:], self.err[:] = OFFC, CANARY, CANARY, ERRC
        ix = self.ix
        args = (ix._h, n, P(self.blob), P(self.offs), n_dests, P(self.doff), P(self.topic), P(self.vals), cap, P(self.err))
        rc = ix._lib.tm_route_batch32(*args) if old else ix._lib.tm_route_batch32_ex(*args, flags)
        assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
        total = int(self.doff[n_dests + 1])
        kept = min(total, cap)
        assert (self.doff[n_dests + 2:] == OFFC).all(), "offsets: canary"
        assert (self.err[n:] == ERRC).all(), "err: canary"
        if rc == ECAP and flags:   # no room for the fan-out: un-aggregated sizes, the entries undefined
            assert total > cap
            assert (self.topic[cap:] == CANARY).all() and (self.vals[cap:] == CANARY).all(), "entries: canary"
            kept = 0
        else:
            assert (rc == ECAP) == (total > cap)
            assert (self.topic[kept:] == CANARY).all() and (self.vals[kept:] == CANARY).all(), "entries: canary"
        return rc, self.doff[:n_dests + 2].copy(), self.topic[:kept].copy(), self.vals[:kept].copy(), \
            self.err[:n].copy()


def _plain(ix, topics, n_dests):
    """the flags-0 result of the staged 64-bit call: (doff u64, topic, value, err)"""
    blob, offs = _native.pack_strings(topics)
    doff, t, v, err = ix.route_batch(blob, offs, n_dests, cap=1 << 16)
    return doff, t.copy(), v.copy(), err.copy()


def _expect(ix, topics, n_dests, fof=None):
    doff, t, v, err = _plain(ix, topics, n_dests)
    a = _aggre(doff, t, v, ix.fof if fof is None else fof, n_dests)
    return a + (err, doff)


def _check(ix, bufs, topics, n_dests, path, exp=None, cap=None):
    """one aggregated call against the reference; path: ONE or GRID must rise by one"""
    exp = exp or _expect(ix, topics, n_dests)
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
    rc, doff, t, v, err = bufs.route(topics, n_dests, cap)
    c1 = (ix.debug_get(ONE), ix.debug_get(GRID))
    assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if path == ONE else (0, 1)), "path"
    assert np.array_equal(err, exp[3]), "err flags"
    if rc == ECAP:
        assert np.array_equal(doff.astype(np.uint64), exp[4]), "TM_ECAP: the un-aggregated bucket sizes"
        return rc, int(exp[0][-1]), int(exp[4][-1])
    assert np.array_equal(doff.astype(np.uint64), exp[0]), "bucket offsets"
    assert np.array_equal(t, exp[1]) and np.array_equal(v, exp[2]), "entries"
    return rc, int(exp[0][-1]), int(exp[4][-1])


@pytest.fixture(scope="module")
def bufs(routed):
    b = Bufs(routed, 8200, 8200 * 24, 256, 40_000)
    yield b
    b.free()


# ---- 1. flags

def test_flags_zero_is_the_old_call(routed, bufs):
    topics = _topics(1000, seed=11)
    for pinned in (bufs, None):
        b = pinned or Bufs(routed, 1000, 1000 * 24, 16, 40_000, pinned=False)
        old = b.route(topics, N_DESTS, flags=0, old=True)
        new = b.route(topics, N_DESTS, flags=0)
        assert old[0] == new[0] == OK and all(x.tobytes() == y.tobytes() for x, y in zip(old[1:], new[1:]))
        old = b.route(topics, N_DESTS, cap=100, flags=0, old=True)
        new = b.route(topics, N_DESTS, cap=100, flags=0)
        assert old[0] == new[0] == ECAP and all(x.tobytes() == y.tobytes() for x, y in zip(old[1:], new[1:]))
    # the 64-bit pair
    ix = routed
    blob, offs = _native.pack_strings(topics)
    outs = []
    for ex in (False, True):
        doff, err = np.full(N_DESTS + 2, 7, np.uint64), np.full(len(topics), ERRC, np.uint8)
        t, v = np.full(40_000, CANARY, np.uint32), np.full(40_000, CANARY, np.uint32)
        args = (ix._h, len(topics), P(blob), P(offs), N_DESTS, P(doff), P(t), P(v), 40_000, P(err))
        assert (ix._lib.tm_route_batch_ex(*args, 0) if ex else ix._lib.tm_route_batch(*args)) == OK
        outs.append((doff, t, v, err))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*outs))
    assert int(outs[0][0][-1]) > 1000


def test_unknown_flag_bits(routed, bufs):
    lib, h = routed._lib, routed._h
    b = bufs
    for flags in (2, 3, 0x80000000):
        args = (h, 0, P(b.blob), P(b.offs), N_DESTS, P(b.doff), P(b.topic), P(b.vals), 10, P(b.err))
        assert lib.tm_route_batch32_ex(*args, flags) == _native.TM_EINVAL
        o64, d64 = np.zeros(1, np.uint64), np.zeros(N_DESTS + 2, np.uint64)
        args = (h, 0, P(b.blob), P(o64), N_DESTS, P(d64), P(b.topic), P(b.vals), 10, P(b.err))
        assert lib.tm_route_batch_ex(*args, flags) == _native.TM_EINVAL


# ---- 2. the in-place path

@pytest.mark.parametrize("topics", [[], [b"zzz"], [b"a1/b1/c1"], [b"a1/+/c1"]],
                         ids=["n0", "n1-nohit", "n1-hit", "n1-badarg"])
def test_tiny_batches(routed, bufs, topics):
    _check(routed, bufs, topics, N_DESTS, ONE)


@pytest.mark.parametrize("n", [63, 64, 65, 1000, 4096])
def test_in_place_shapes(routed, bufs, n):
    topics = _topics(n, seed=n)
    _, K, total = _check(routed, bufs, topics, N_DESTS, ONE)
    assert n // 2 < K < total <= FO1_ENTRIES, "groups on several nodes: something is dropped"


def test_the_staged_64_bit_call(routed):
    topics = _topics(1000, seed=21)
    exp = _expect(routed, topics, N_DESTS)
    blob, offs = _native.pack_strings(topics)
    doff, t, v, err = routed.route_batch(blob, offs, N_DESTS, cap=1 << 16, aggre=True)
    assert np.array_equal(doff, exp[0]) and np.array_equal(t, exp[1]) and np.array_equal(v, exp[2])
    assert np.array_equal(err, exp[3])


@pytest.fixture(scope="module")
def exact(gpu):
    """'#' carries 3 values -- node 0 and group 1 on two nodes --, 'one/x' 1, '$e/x' 1 ('#' does
    not match a '$' topic): a batch of a plain topics, m x 'one/x' and s x '$e/x' has
    E = 3 (a + m) + m + s entries and K = 2 (a + m) + m + s"""
    ix = _native.Index()
    _insert(ix, [b"#", b"#", b"#", b"one/x", b"$e/x"], [0, 1, 2, 3, 4], [0, 1, 1, 0, 1], [5, 5, 5, 6, 8])
    ix.fof = np.array([5, 5, 5, 6, 8], np.uint32)
    b = Bufs(ix, 8200, 8200 * 8, 256, 40_000)
    yield ix, b
    b.free()
    ix.close()


@pytest.mark.parametrize("E", [FO1_ENTRIES - 1, FO1_ENTRIES, FO1_ENTRIES + 1])
def test_entry_bound(exact, E):
    """E before aggregation around FO1_ENTRIES: the first two in one launch each, the third by
    the grid kernels on the lane; and cut by cap on either path"""
    ix, b = exact
    n = 5000
    m = E - 3 * n
    t = [b"p/%d" % i for i in range(n - m)] + [b"one/x"] * m
    rng = np.random.default_rng(E)
    topics = [t[i] for i in rng.permutation(n)]
    path = ONE if E <= FO1_ENTRIES else GRID
    exp = _expect(ix, topics, 2)
    rc, K, total = _check(ix, b, topics, 2, path, exp=exp)
    assert rc == OK and total == E and K == 2 * n + m
    rc, K, total = _check(ix, b, topics, 2, path, exp=exp, cap=E - 1)
    assert rc == ECAP
    rc, K, total = _check(ix, b, topics, 2, path, exp=exp, cap=E)   # room for the fan-out is enough
    assert rc == OK


@pytest.mark.parametrize("E", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_entry_counts_around_the_wave_chunks(exact, E):
    ix, b = exact
    a, m = E // 8, E // 16
    sdol = E - 3 * (a + m) - m
    t = [b"p/%d" % i for i in range(a)] + [b"one/x"] * m + [b"$e/x"] * sdol + [b"$none"] * 37
    rng = np.random.default_rng(E)
    topics = [t[i] for i in rng.permutation(len(t))]
    rc, K, total = _check(ix, b, topics, 2, ONE)
    assert rc == OK and total == E and K == 2 * (a + m) + m + sdol


@pytest.mark.parametrize("n_dests,path", [(255, ONE), (256, GRID)])
def test_destination_counts(routed, n_dests, path):
    b = Bufs(routed, 1100, 1100 * 24, n_dests, 8000)
    try:
        _, K, total = _check(routed, b, _topics(1000, seed=n_dests), n_dests, path)
        assert 500 < K < total
    finally:
        b.free()


def test_plain_numpy_buffers_take_the_staged_path(routed):
    b = Bufs(routed, 600, 600 * 24, 16, 8000, pinned=False)
    _, K, total = _check(routed, b, _topics(500, seed=3), N_DESTS, GRID)
    assert K < total


# ---- 3. capacity

def test_ecap_and_one_sized_retry(routed, bufs):
    topics = _topics(1000, seed=77)
    exp = _expect(routed, topics, N_DESTS)
    K, total = int(exp[0][-1]), int(exp[4][-1])
    assert 500 < K < total
    plain = Bufs(routed, 1000, 1000 * 24, 16, 40_000, pinned=False)
    for b, path in ((bufs, ONE), (plain, GRID)):
        for cap in (total - 1, K, 1, 0):      # even K entries of room are not enough: the fan-out needs `total`
            rc, _, _ = _check(routed, b, topics, N_DESTS, path, exp=exp, cap=cap)
            assert rc == ECAP
        rc, doff, _, _, _ = b.route(topics, N_DESTS, cap=10)
        assert rc == ECAP
        rc, _, _ = _check(routed, b, topics, N_DESTS, path, exp=exp, cap=int(doff[N_DESTS + 1]))   # the sized retry
        assert rc == OK


# ---- 4. read-your-writes

@pytest.mark.parametrize("copies", [1, 2])
def test_a_filter_set_and_inserted_is_routed_at_once(gpu, copies):
    ix = _routed_index(copies)
    b = Bufs(ix, 300, 300 * 24, 16, 8000)
    topics = _topics(200, seed=5) + [b"fresh/x/y"]
    _check(ix, b, topics, N_DESTS, ONE)
    # group 3 on two nodes under one new filter, and a node route of it
    kids = np.array([50_000, 50_001, 50_002], np.uint32)
    ix.set_dests(kids, [3, 3, 1])
    ix.set_route_filters(kids, [123_456, 123_456, 123_456])
    blob, offs = _native.pack_strings([b"fresh/+/y"] * 3)
    ix.apply(np.ones(3, np.uint8), blob, offs, kids)
    fof = np.full(50_003, NONE, np.uint32)
    fof[:len(ix.fof)] = ix.fof
    fof[kids] = 123_456
    exp = _expect(ix, topics, N_DESTS, fof)
    rc, doff, t, v, err = b.route(topics, N_DESTS)
    assert np.array_equal(doff.astype(np.uint64), exp[0]) and np.array_equal(t, exp[1]) and np.array_equal(v, exp[2])
    new = v[t == 200]
    assert sorted(new[new >= 50_000].tolist()) == [50_000, 50_002], "one entry for the group, one for the node"
    # the second member's filter becomes unknown: it equals nothing any more
    ix.set_route_filters([50_001], [NONE])
    fof[50_001] = NONE
    rc, doff, t, v, err = b.route(topics, N_DESTS)
    new = v[t == 200]
    assert sorted(new[new >= 50_000].tolist()) == [50_000, 50_001, 50_002]
    _check(ix, b, topics, N_DESTS, ONE, exp=_expect(ix, topics, N_DESTS, fof))
    b.free()
    ix.close()


# ---- 5. concurrent callers

def test_eight_concurrent_callers(routed):
    batches = [_topics(512, seed=100 + k) for k in range(8)]
    exps = [_expect(routed, tp, N_DESTS) for tp in batches]
    sets = [Bufs(routed, 512, 512 * 24, 16, 8000) for _ in range(8)]
    start, bad = threading.Barrier(8), []

    def caller(k):
        try:
            start.wait()
            for _ in range(30):
                rc, doff, t, v, err = sets[k].route(batches[k], N_DESTS)
                ok = rc == OK and np.array_equal(doff.astype(np.uint64), exps[k][0]) and \
                    np.array_equal(t, exps[k][1]) and np.array_equal(v, exps[k][2]) and np.array_equal(err, exps[k][3])
                if not ok:
                    bad.append(k)
                    return
        except Exception as e:   # noqa: BLE001
            bad.append((k, repr(e)))

    one0 = routed.debug_get(ONE)
    th = [threading.Thread(target=caller, args=(k,)) for k in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not bad
    assert routed.debug_get(ONE) - one0 == 240
    for s in sets:
        s.free()


# ---- 6. the Python layers

NODES = ("n1", "n2", "n3")
GROUPS = (b"g1", b"g2")


@pytest.fixture(scope="module", params=[False, True], ids=["staged", "in-place"])
def router(gpu, request):
    rng = np.random.default_rng(2024)
    r = Router(node="n1", route_in_place=request.param)
    dests = list(NODES) + [(g, n) for g in GROUPS for n in NODES] + [("external", "c1"), ("external", "c2")]
    batch = {}
    for i in range(400):
        f = (f"a{i % 50}/+/c{i % 7}", f"a{i % 50}/#", f"+/b{i % 40}/#", f"a{i % 50}/b{i % 40}/+")[i % 4].encode()
        for d in rng.choice(len(dests), 1 + i % 5, replace=False):
            batch[(f, dests[d])] = ("add", 0, None)
    for k in range(100):   # the bag: exact topics, a group on two nodes among them
        t = f"a{k % 50}/b{k % 40}/c{k % 7}".encode()
        batch[(t, (GROUPS[k % 2], "n1"))] = ("add", 0, None)
        batch[(t, (GROUPS[k % 2], "n3"))] = ("add", 0, None)
        batch[(t, NODES[k % 3])] = ("add", 0, None)
    assert r.do_batch(batch) == {}
    return r


def _messages(n, seed):
    """publish topics, every fifth one an exact topic of the bag"""
    topics = _topics(n, seed=seed)
    for i in range(3, n, 5):
        k = i % 100
        topics[i] = f"a{k % 50}/b{k % 40}/c{k % 7}".encode()
    return topics


def test_router_returns_aggregated_buckets(router):
    topics = _messages(800, seed=31)
    plain = router.match_routes_by_dest(topics, errors="return")
    got = router.match_routes_by_dest(topics, errors="return", aggre=True)
    assert set(got) == set(plain) and set(got.errors) == set(plain.errors)
    fewer = 0
    for cls, rows in plain.items():
        exp, last = [], None
        for i, r in rows:   # one (message, To) per class among the filter matches; the bag's rows all
            wild = b"+" in r.topic or b"#" in r.topic
            if wild and isinstance(r.dest, tuple) and r.dest[0] != "external" and (i, r.topic) == last:
                continue
            last = (i, r.topic) if wild else None
            exp.append((i, r.topic))
        assert sorted((i, r.topic) for i, r in got[cls]) == sorted(exp), f"class {cls!r}"
        fewer += len(rows) - len(got[cls])
    assert fewer > 100


def test_broker_on_device_aggre_delivers_the_same_multiset(router):
    msgs = [Message(t, i) for i, t in enumerate(_messages(800, seed=3))]
    log = Counter()

    def broker(**kw):
        return Broker(router, dispatch=lambda to, m: log.update([("n1", to, m.payload)]) or 1,
                      forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1, **kw)
    res = broker().publish_batch(msgs)
    exp, log = log, Counter()
    plans, errors = broker(aggre_on_device=True).publish_batch_by_dest(msgs)
    assert log == exp and sum(exp.values()) > 1500 and max(exp.values()) == 1
    assert set(errors) == {i for i, r in enumerate(res) if isinstance(r, Exception)}
    bag_group = [k for k in exp if k[0] in GROUPS and b"+" not in k[1] and b"#" not in k[1]]
    assert len(bag_group) > 10, "bag rows with a group destination were delivered (once each)"


# ---- 7. the NIF core on the real library

@pytest.fixture(scope="module")
def nif(tmp_path_factory, gpu):
    out = tmp_path_factory.mktemp("nifaggre") / "libnifaggre.so"
    libdir = ROOT / "emqx_amd"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out),
                    str(ROOT / "c_src" / "tmatch_nif_core.c"), str(ROOT / "c_src" / "tmatch_nif_route.c"),
                    str(ROOT / "c_src" / "tmatch_nif_aggre.c"), str(ROOT / "tests" / "native" / "nif_route_shim.c"),
                    f"-L{libdir}", "-l:libtmatch.so", f"-Wl,-rpath,{libdir}"], check=True)
    _native.load_library()
    lib = C.CDLL(str(out))
    vp, u32 = C.c_void_p, C.c_uint32
    lib.shim_pool_new.restype = vp
    lib.shim_pool_new.argtypes = [vp, u32]
    lib.shim_pool_free.argtypes = [vp]
    lib.tmn_take.restype = vp
    lib.tmn_take.argtypes = [vp]
    lib.tmn_give.argtypes = [vp, vp]
    lib.tmn_pack.argtypes = [vp, vp, u32, vp, vp]
    lib.tmn_route_aggre.argtypes = [vp, vp, u32, u32]
    lib.tmn_route_dest.argtypes = [vp, u32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for f in (lib.shim_vals, lib.shim_route_topics):
        f.argtypes, f.restype = [vp], C.POINTER(u32)
    lib.shim_err.argtypes, lib.shim_err.restype = [vp], C.POINTER(C.c_uint8)
    lib.shim_reruns.argtypes, lib.shim_reruns.restype = [vp], C.c_uint64
    return lib


@pytest.mark.parametrize("in_flags", [0, _native.TM_ALLOC_VRAM], ids=["pinned", "vram"])
def test_nif_core_routes_aggregated_on_the_real_library(routed, nif, in_flags):
    """tmn_pack -> tmn_route_aggre -> tmn_route_dest == the reference, with a forced TM_ECAP
    rerun (more entries before aggregation than the set's first guess)"""
    fat = _native.Index()   # 300 values on '#': 7 classes; the values v and v + 7 of one class share a filter id
    fat_fids = [v // 14 for v in range(300)]
    _insert(fat, [b"#"] * 300, np.arange(300), [v % 7 for v in range(300)], fat_fids)
    fat.fof = np.array(fat_fids, np.uint32)
    for ix, topics, rerun in ((routed, _topics(700, seed=12), 0), (fat, [b"t/%d" % i for i in range(20)], 1)):
        h = ix._h
        pool = nif.shim_pool_new(h, in_flags)   # (vram: the core falls back to pinned memory without a large BAR)
        s = nif.tmn_take(pool)
        n = len(topics)
        exp = _expect(ix, topics, N_DESTS)
        one0 = ix.debug_get(ONE)
        arr = (C.c_char_p * n)(*topics)
        lens = (C.c_uint64 * n)(*[len(t) for t in topics])
        assert nif.tmn_pack(s, h, n, C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p)) == 0
        assert nif.tmn_route_aggre(s, h, n, N_DESTS) == 0
        assert nif.shim_reruns(s) == rerun
        assert ix.debug_get(ONE) - one0 == 1 + rerun, "in place, the rerun too"
        tv, tt, te = nif.shim_vals(s), nif.shim_route_topics(s), nif.shim_err(s)
        for d in range(N_DESTS + 1):
            b, e = C.c_uint64(), C.c_uint64()
            assert nif.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
            assert (b.value, e.value) == (int(exp[0][d]), int(exp[0][d + 1]))
            assert tt[b.value:e.value] == exp[1][b.value:e.value].tolist()
            assert tv[b.value:e.value] == exp[2][b.value:e.value].tolist()
        assert te[:n] == exp[3].tolist()
        assert int(exp[0][-1]) < int(exp[4][-1])
        nif.tmn_give(pool, s)
        nif.shim_pool_free(pool)
    fat.close()
