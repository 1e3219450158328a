"""tm_route_batch32: the 32-bit, in-place route call for a NIF's micro-batches.

The reference everywhere is the unchanged tm_route_batch on the same index and
topics (Index.route_batch); once, independently, numpy.argsort(bucket,
kind="stable") over match_batch's CSR.  Every compared array must be equal
element for element, every output buffer carries a canary tail that must
survive, and TM_DEBUG_ROUTE_ONE / TM_DEBUG_ROUTE_GRID say which fan-out ran:
the one-launch kernel (k_fo_one: one workgroup, up to FO1_TOPICS topics,
FO1_ENTRIES entries, 256 buckets) or the grid kernels / the staged path.

k_fo_one gives each of its 16 waves a chunk of ceil(E / 16) entries rounded up
to 64, so E = 1024 fills every wave's first step exactly and 1025 takes a
second; E = FO1_ENTRIES fills all 16 steps of all waves.

Last, one table of refusals over the six entry points of the route family
(tm_route_batch_ex, tm_dispatch_batch, tm_publish_batch and their 32-bit
forms): TM_EINVAL, no output written, no leg counted, no state word moved, and
tm_last_error names the entry point that was called.
"""
import ctypes as C
import subprocess
import threading
from collections import Counter
from itertools import product
from pathlib import Path

import numpy as np
import pytest

from emqx_amd import _native, topic_index as ti
from emqx_amd.broker import Broker, Message
from emqx_amd.router import Router, dest_class

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FO1_TOPICS, FO1_ENTRIES = 8192, 16384   # emqx_amd/csrc/tm_dev.h
CANARY, OFFC, ERRC, TAIL = 0xC0FFEE11, 0xDEADBEEF, 0xEE, 64
ONE, GRID = _native.TM_DEBUG_ROUTE_ONE, _native.TM_DEBUG_ROUTE_GRID
SMALL = _native.TM_DEBUG_PATH_SMALL
N_DESTS = 5   # 3 nodes + 2 groups
P = _native._ptr


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _insert(ix, filters, values, dests=None):
    values = np.asarray(values, np.uint32)
    if dests is not None:
        keep = [i for i, d in enumerate(dests) if d is not None]
        ix.set_dests(values[keep], np.array([dests[i] for i in keep], np.uint32))
    blob, offs = _native.pack_strings(filters)
    ix.apply(np.ones(len(filters), np.uint8), blob, offs, values)


def _routed_filters():
    fs = []
    for i in range(2000):
        fs.append((f"a{i % 50}/+/c{i % 7}", f"a{i % 50}/#", f"+/b{i % 40}/#", f"a{i % 50}/b{i % 40}/+")[i % 4].encode())
    fs += [f"a{k % 50}/b{k % 40}/c{k % 7}".encode() for k in range(300)]   # exact topics
    # every '+' variant of q/r/s/t and its '#' prefixes: one topic with more than 8 value runs
    for ws in product(*[(w, b"+") for w in (b"q", b"r", b"s", b"t")]):
        fs.append(b"/".join(ws))
        fs.append(b"/".join(ws[:2]) + b"/#")
    return list(dict.fromkeys(fs))


def _routed_dests(nv):
    """most values on the 5 destinations; some never set, some on a destination >= any n_dests
    used here, some spread over 400 ids (routed or not, depending on n_dests)"""
    out = []
    for v in range(nv):
        out.append(None if v % 11 == 0 else 100_000 if v % 13 == 0 else (v // 5) % 400 if v % 5 == 0 else (v // 3) % N_DESTS)
    return out


def _routed_index(copies=1):
    ix = _native.Index(copies=copies)
    fs = _routed_filters()
    _insert(ix, fs, np.arange(len(fs)), _routed_dests(len(fs)))
    return ix


@pytest.fixture(scope="module")
def routed(gpu):
    return _routed_index()


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

    def route(self, topics, n_dests, cap=None, shift=0):
        """-> (rc, dest_offsets, topic[:kept], values[:kept], err[:n]); the canaries checked"""
        blob, offs = _native.pack_strings(topics)
        n, nb = len(topics), int(offs[-1])
        cap = self.cap_max if cap is None else cap
        assert cap <= self.cap_max and n + 1 <= len(self.offs) and nb + shift <= len(self.blob)
        self.blob[shift:shift + nb] = blob[:nb]
        self.offs[:n + 1] = offs
        self.doff[:], self.topic[:], self.vals[:], self.err[:] = OFFC, CANARY, CANARY, ERRC
        ix = self.ix
        rc = ix._lib.tm_route_batch32(ix._h, n, P(self.blob[shift:]), P(self.offs), n_dests, P(self.doff),
                                      P(self.topic), P(self.vals), cap, P(self.err))
        assert rc in (_native.TM_OK, _native.TM_ECAP), ix._lib.tm_last_error(ix._h)
        total = int(self.doff[n_dests + 1])
        kept = min(total, cap)
        assert (rc == _native.TM_ECAP) == (total > cap)
        assert (self.doff[n_dests + 2:] == OFFC).all(), "offsets: canary"
        assert (self.topic[kept:] == CANARY).all() and (self.vals[kept:] == CANARY).all(), "entries: canary"
        assert (self.err[n:] == ERRC).all(), "err: canary"
        return rc, self.doff[:n_dests + 2].copy(), self.topic[:kept].copy(), self.vals[:kept].copy(), \
            self.err[:n].copy()


def _reference(ix, topics, n_dests):
    blob, offs = _native.pack_strings(topics)
    doff, t, v, err = ix.route_batch(blob, offs, n_dests, cap=1 << 16)
    return doff, t.copy(), v.copy(), err.copy()


def _check(ix, bufs, topics, n_dests, path, cap=None, shift=0, ref=None, walks=1):
    """one call against the reference; path: ONE or GRID must rise by one, the other stay put"""
    ref = ref or _reference(ix, topics, n_dests)
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID), ix.debug_get(SMALL))
    rc, doff, t, v, err = bufs.route(topics, n_dests, cap, shift)
    c1 = (ix.debug_get(ONE), ix.debug_get(GRID), ix.debug_get(SMALL))
    assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if path == ONE else (0, 1)), "fan-out path"
    if walks is not None and topics:
        assert c1[2] - c0[2] == walks, "one-launch walks of the call"
    kept = len(t)
    assert np.array_equal(doff.astype(np.uint64), ref[0]), "bucket offsets"
    assert np.array_equal(t, ref[1][:kept]) and np.array_equal(v, ref[2][:kept]), "entries"
    assert np.array_equal(err, ref[3]), "err flags"
    return rc, int(doff[-1])


@pytest.fixture(scope="module")
def bufs(routed):
    b = Bufs(routed, 8200, 8200 * 24, 256, 40_000)
    yield b
    b.free()


# ---- 1. shapes

@pytest.mark.parametrize("topics", [[], [b"zzz"], [b"a1/b1/c1"], [b"a1/+/c1"]],
                         ids=["n0", "n1-nohit", "n1-hit", "n1-badarg"])
def test_tiny_batches(routed, bufs, topics):
    _, total = _check(routed, bufs, topics, N_DESTS, ONE)
    assert (total > 0) == (topics == [b"a1/b1/c1"])


@pytest.mark.parametrize("n", [63, 64, 65, 1000, 4096])
def test_shapes_equal_route_batch(routed, bufs, n):
    topics = _topics(n, seed=n)
    _, total = _check(routed, bufs, topics, N_DESTS, ONE)
    assert total > n // 2 and total <= FO1_ENTRIES


def test_equals_a_stable_argsort_of_the_csr(routed, bufs):
    """independent of tm_route_batch: the stable partition of match_batch's CSR by bucket"""
    topics = _topics(1500, seed=42) + [b"q/r/s/t"]
    blob, offs = _native.pack_strings(topics)
    hit, vals, err = routed.match_batch(blob, offs)
    nv = len(_routed_filters())
    dest_of = np.array([0xFFFFFFFF if d is None else d for d in _routed_dests(nv)], np.uint32)
    b = dest_of[vals].astype(np.int64)
    b[b >= N_DESTS] = N_DESTS
    order = np.argsort(b, kind="stable")
    topic = np.repeat(np.arange(len(topics), dtype=np.uint32), np.diff(hit.astype(np.int64)))
    rc, doff, t, v, err2 = bufs.route(topics, N_DESTS)
    assert rc == _native.TM_OK and np.array_equal(err, err2)
    assert np.array_equal(t, topic[order]) and np.array_equal(v, vals[order])
    exp = np.zeros(N_DESTS + 2, np.int64)
    exp[1:] = np.cumsum(np.bincount(b, minlength=N_DESTS + 1))
    assert np.array_equal(doff.astype(np.int64), exp)
    assert np.diff(exp).min() > 0 and np.diff(hit.astype(np.int64))[-1] > 8   # every bucket used; > 8 runs


# ---- 2. the kernel's bounds: an index whose entry count is exact

@pytest.fixture(scope="module")
def exact(gpu):
    """'#' carries 3 values, 'one/x' 1, '$e/x' 1 ('#' does not match a '$' topic): a batch of
    a plain topics, m x 'one/x', s x '$e/x' and z x '$none' has E = 3 (a + m) + m + s"""
    ix = _native.Index()
    _insert(ix, [b"#", b"#", b"#", b"one/x", b"$e/x"], [0, 1, 2, 3, 4], [0, 1, 2, 0, None])
    b = Bufs(ix, 8200, 8200 * 8, 256, 40_000)
    yield ix, b
    b.free()


def _exact_topics(a=0, m=0, s=0, z=0):
    t = [b"p/%d" % i for i in range(a)] + [b"one/x"] * m + [b"$e/x"] * s + [b"$none"] * z
    rng = np.random.default_rng(len(t))
    return [t[i] for i in rng.permutation(len(t))], 3 * (a + m) + m + s


@pytest.mark.parametrize("E", [FO1_ENTRIES - 1, FO1_ENTRIES, FO1_ENTRIES + 1])
def test_entry_bound(exact, E):
    """E = 3 n + m around FO1_ENTRIES: the first two in one launch, the third by the grid
    kernels on the pairs already matched (one walk, not two)"""
    ix, b = exact
    n = 5000
    topics, e = _exact_topics(a=n - (E - 3 * n), m=E - 3 * n)
    assert e == E and len(topics) == n
    path = ONE if E <= FO1_ENTRIES else GRID
    _, total = _check(ix, b, topics, 3, path, walks=1)
    assert total == E
    rc, total = _check(ix, b, topics, 3, path, cap=100, walks=1)   # and cut by cap on either path
    assert total == E and rc == _native.TM_ECAP


@pytest.mark.parametrize("n", [FO1_TOPICS - 1, FO1_TOPICS, FO1_TOPICS + 1])
def test_topic_bound(exact, n):
    ix, b = exact
    topics, E = _exact_topics(a=100, m=50, s=n - 150 - 1000, z=1000)
    assert len(topics) == n and E < FO1_ENTRIES
    _, total = _check(ix, b, topics, 3, ONE if n <= FO1_TOPICS else GRID)
    assert total == E


@pytest.mark.parametrize("E", [1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049])
def test_entry_counts_around_the_wave_chunks(exact, E):
    ix, b = exact
    topics, e = _exact_topics(a=E // 8, m=E // 16, s=E - 3 * (E // 8 + E // 16) - E // 16, z=37)
    assert e == E
    _, total = _check(ix, b, topics, 3, ONE)
    assert total == E


# ---- 3. destinations

@pytest.mark.parametrize("n_dests,path", [(1, ONE), (2, ONE), (255, ONE), (256, GRID), (65536, GRID)])
def test_destination_counts(routed, n_dests, path):
    b = Bufs(routed, 1100, 1100 * 24, n_dests, 8000)
    try:
        _, total = _check(routed, b, _topics(1000, seed=n_dests), n_dests, path, walks=None)
        assert total > 500
    finally:
        b.free()


def test_all_unrouted_and_all_in_one_bucket(gpu):
    fs = _routed_filters()[:400]
    for dests in (None, [2] * len(fs)):
        ix = _native.Index()
        _insert(ix, fs, np.arange(len(fs)), dests)
        b = Bufs(ix, 600, 600 * 24, 16, 8000)
        _, total = _check(ix, b, _topics(500, seed=9), 4, ONE)
        sizes = np.diff(b.doff[:6].astype(np.int64))
        assert total > 100 and sizes[4 if dests is None else 2] == total
        ix.close()


# ---- 4. capacity

def test_capacity(routed, bufs):
    topics = _topics(1000, seed=77)
    ref = _reference(routed, topics, N_DESTS)
    total = int(ref[0][-1])
    assert total > 500
    for cap in (total, total - 1, 1, 0):
        rc, got = _check(routed, bufs, topics, N_DESTS, ONE, cap=cap, ref=ref)
        assert got == total and rc == (_native.TM_ECAP if total > cap else _native.TM_OK)


# ---- 5. fallbacks

def test_plain_numpy_buffers_take_the_staged_path(routed):
    b = Bufs(routed, 600, 600 * 24, 16, 8000, pinned=False)
    _check(routed, b, _topics(500, seed=3), N_DESTS, GRID, walks=None)


def test_misaligned_blob_takes_the_staged_path(routed, bufs):
    _check(routed, bufs, _topics(500, seed=4), N_DESTS, GRID, shift=1, walks=None)
    _check(routed, bufs, _topics(500, seed=4), N_DESTS, ONE, shift=16)


def test_more_topics_than_one_launch_takes(routed):
    n = 65537
    b = Bufs(routed, n, n * 24, 16, 300_000)
    try:
        blob, offs = _native.pack_strings(_topics(n, seed=6))
        ref = routed.route_batch(blob, offs, N_DESTS, cap=1 << 19)
        _check(routed, b, _topics(n, seed=6), N_DESTS, GRID, ref=ref, walks=None)
    finally:
        b.free()


def test_index_the_one_launch_walk_refuses(gpu):
    """a 33-level filter: deeper than the one-launch kernels' fallback store"""
    ix = _native.Index()
    deep = b"/".join(b"l%d" % i for i in range(33))
    _insert(ix, [deep, b"l0/#", b"+/l1/#"], [0, 1, 2], [0, 1, None])
    b = Bufs(ix, 64, 64 * 200, 16, 1000)
    topics = [deep, b"l0/l1", b"x/l1/y", b"none", b"l0/+"] * 8
    _, total = _check(ix, b, topics, 2, GRID, walks=None)
    assert total == 8 * (3 + 2 + 1)
    ix.close()


def test_deep_topic_and_many_value_runs_in_place(routed, bufs):
    deep = b"/".join(b"d%d" % i for i in range(40))        # deeper than the walk's level store
    long_ = b"a1/" + b"x" * 400                           # longer than the staged topic bytes
    topics = _topics(200, seed=8) + [deep, b"q/r/s/t", long_, b"q/r/s/t", b"q/r/x/t"]
    _, total = _check(routed, bufs, topics, N_DESTS, ONE)
    assert total > 100


# ---- 6. the value scratch grows inside the call

def test_value_scratch_growth(gpu):
    ix = _native.Index()
    _insert(ix, [b"#"] * 300, np.arange(300), [v % 7 for v in range(300)])
    b = Bufs(ix, 1000, 1000 * 8, 16, 310_000)
    topics = [b"t/%d" % i for i in range(1000)]
    b2 = Bufs(ix, 1000, 1000 * 8, 16, 310_000, pinned=False)
    # (first: the first routed batch of the index is the in-place one)
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID), ix.debug_get(SMALL))
    rc, doff, t, v, err = b.route(topics, 5)
    assert rc == _native.TM_OK and int(doff[-1]) == 300_000
    assert (ix.debug_get(ONE) - c0[0], ix.debug_get(GRID) - c0[1]) == (0, 1)
    assert ix.debug_get(SMALL) - c0[2] == 2, "grown and run again, once"
    blob, offs = _native.pack_strings(topics)
    ref = ix.route_batch(blob, offs, 5, cap=300_000)
    assert np.array_equal(doff.astype(np.uint64), ref[0]) and np.array_equal(t, ref[1]) and np.array_equal(v, ref[2])
    assert not err.any() and not ref[3].any()
    _check(ix, b, topics, 5, GRID, ref=ref, walks=1)       # the scratch is kept: one walk now
    _check(ix, b2, topics[:10], 5, GRID, walks=None)
    b.free()
    ix.close()


# ---- 7. read-your-writes

@pytest.mark.parametrize("copies", [1, 2])
def test_read_your_writes(gpu, copies):
    ix = _routed_index(copies)
    b = Bufs(ix, 300, 300 * 24, 16, 8000)
    topics = _topics(200, seed=5) + [b"fresh/x/y"]
    _check(ix, b, topics, N_DESTS, ONE)
    kid = 50_000
    ix.set_dests([kid], [3])
    blob, offs = _native.pack_strings([b"fresh/+/y"])
    ix.apply(np.ones(1, np.uint8), blob, offs, np.array([kid], np.uint32))
    rc, doff, t, v, err = b.route(topics, N_DESTS)
    at = np.flatnonzero(v == kid)
    assert len(at) == 1 and doff[3] <= at[0] < doff[4] and t[at[0]] == 200
    _check(ix, b, topics, N_DESTS, ONE)
    ix.apply(np.zeros(1, np.uint8), blob, offs, np.array([kid], np.uint32))
    rc, doff, t, v, err = b.route(topics, N_DESTS)
    assert not (v == kid).any()
    _check(ix, b, topics, N_DESTS, ONE)
    ix.close()


# ---- 8. concurrent callers

def test_eight_concurrent_callers(routed):
    failed0 = routed.debug_get(_native.TM_DEBUG_FAILED_BATCHES)
    batches = [_topics(512, seed=100 + k) for k in range(8)]
    refs = [_reference(routed, tp, N_DESTS) for tp in batches]
    sets = [Bufs(routed, 512, 512 * 24, 16, 8000) for _ in range(8)]
    start, bad = threading.Barrier(8), []

    def caller(k):
        try:
            start.wait()
            for _ in range(50):
                rc, doff, t, v, err = sets[k].route(batches[k], N_DESTS)
                ok = rc == _native.TM_OK and np.array_equal(doff.astype(np.uint64), refs[k][0]) and \
                    np.array_equal(t, refs[k][1]) and np.array_equal(v, refs[k][2]) and np.array_equal(err, refs[k][3])
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
    assert routed.debug_get(ONE) - one0 == 400
    assert routed.debug_get(_native.TM_DEBUG_FAILED_BATCHES) == failed0
    for s in sets:
        s.free()


# ---- 9. the Python layers

NODES = ("n1", "n2", "n3")
GROUPS = (b"g1", b"g2")


@pytest.fixture(scope="module")
def router(gpu):
    rng = np.random.default_rng(2024)
    r = Router(node="n1", route_in_place=True)
    dests = list(NODES) + [(g, n) for g in GROUPS for n in NODES]
    batch = {}
    for i in range(2000):
        f = (f"a{i % 50}/+/c{i % 7}", f"a{i % 50}/#", f"+/b{i % 40}/#", f"a{i % 50}/b{i % 40}/+")[i % 4].encode()
        for d in rng.choice(len(dests), 1 + i % 3, replace=False):
            batch[(f, dests[d])] = ("add", 0, None)
    for k in range(300):
        for d in rng.choice(len(dests), 1 + k % 2, replace=False):
            batch[(f"a{k % 50}/b{k % 40}/c{k % 7}".encode(), dests[d])] = ("add", 0, None)
    assert r.do_batch(batch) == {}
    return r


def _regroup(per_message):
    """match_routes_batch's lists -> ({class: [(message index, Route)]}, {index: exception})"""
    by, errs = {}, {}
    for i, routes in enumerate(per_message):
        if isinstance(routes, Exception):
            errs[i] = routes
            continue
        for r in routes:
            by.setdefault(dest_class(r.dest), []).append((i, r))
    return by, errs


def test_router_in_place_equals_the_regrouped_lists(router):
    ix = router._mirror._index
    for n in (1500, 6000):   # one launch; more entries than it takes (the retry on TM_ECAP included)
        topics = _topics(n, seed=n)
        one0, grid0 = ix.debug_get(ONE), ix.debug_get(GRID)
        exp, errs = _regroup(router.match_routes_batch(topics, errors="return"))
        got = router.match_routes_by_dest(topics, errors="return")
        assert set(got) == set(exp) == set(NODES) | set(GROUPS)
        for cls in exp:
            assert got[cls] == exp[cls], f"destination {cls!r}: lists differ"
        assert set(got.errors) == set(errs) and all(type(got.errors[i]) is type(errs[i]) for i in errs)
        assert ix.debug_get(ONE) + ix.debug_get(GRID) > one0 + grid0, "tm_route_batch32 served the call"
    with pytest.raises(ti.BadArg):
        router.match_routes_by_dest(_topics(200))


def test_publish_batch_by_dest_delivers_the_same_multiset(router):
    msgs = [Message(t, i) for i, t in enumerate(_topics(1200, seed=3))]
    log = Counter()

    def broker():
        return Broker(router, dispatch=lambda to, m: log.update([("n1", to, m.payload)]) or 1,
                      forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1)
    res = broker().publish_batch(msgs)
    exp, log = log, Counter()
    plans, errors = broker().publish_batch_by_dest(msgs)
    assert log == exp and sum(exp.values()) > 2000
    assert set(errors) == {i for i, r in enumerate(res) if isinstance(r, Exception)}


# ---- 10. the NIF core on the real library

@pytest.fixture(scope="module")
def nif(tmp_path_factory, gpu):
    out = tmp_path_factory.mktemp("nifreal") / "libnifreal.so"
    libdir = ROOT / "emqx_amd"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out),
                    str(ROOT / "c_src" / "tmatch_nif_core.c"), str(ROOT / "c_src" / "tmatch_nif_route.c"),
                    str(ROOT / "tests" / "native" / "nif_route_shim.c"),
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
    lib.tmn_route.argtypes = [vp, vp, u32, u32]
    lib.tmn_match.argtypes = [vp, vp, u32, u32]
    lib.tmn_route_dest.argtypes = [vp, u32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.tmn_row.argtypes = [vp, u32, u32, u32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for f in (lib.shim_vals, lib.shim_route_topics):
        f.argtypes, f.restype = [vp], C.POINTER(u32)
    lib.shim_err.argtypes, lib.shim_err.restype = [vp], C.POINTER(C.c_uint8)
    lib.shim_reruns.argtypes, lib.shim_reruns.restype = [vp], C.c_uint64
    return lib


def _nif_pack(lib, s, h, topics):
    arr = (C.c_char_p * len(topics))(*topics)
    lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
    return lib.tmn_pack(s, h, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))


@pytest.mark.parametrize("in_flags", [0, _native.TM_ALLOC_VRAM], ids=["pinned", "vram"])
def test_nif_core_routes_on_the_real_library(routed, nif, in_flags):
    """tmn_pack -> tmn_route -> tmn_route_dest == route_batch, with a forced TM_ECAP rerun
    (more than TMN_IDS_PER_TOPIC entries per topic); tmn_match / tmn_row == match_batch"""
    # 300 values on '#': 20 topics hold 6,000 entries, beyond the set's first guess
    # (TMN_IDS_PER_TOPIC per topic + 1024, and the half tmn_get allocates on top)
    fat = _native.Index()
    _insert(fat, [b"#"] * 300, np.arange(300), [v % 7 for v in range(300)])
    for ix, topics, rerun in ((routed, _topics(700, seed=12), 0), (fat, [b"t/%d" % i for i in range(20)], 1)):
        h = ix._h
        pool = nif.shim_pool_new(h, in_flags)   # (vram: the core falls back to pinned memory without a large BAR)
        s = nif.tmn_take(pool)
        n = len(topics)
        ref = _reference(ix, topics, N_DESTS)
        one0 = ix.debug_get(ONE)
        assert _nif_pack(nif, s, h, topics) == 0
        assert nif.tmn_route(s, h, n, N_DESTS) == 0
        assert nif.shim_reruns(s) == rerun
        assert ix.debug_get(ONE) - one0 == 1 + rerun, "in place, the rerun too"
        tv, tt, te = nif.shim_vals(s), nif.shim_route_topics(s), nif.shim_err(s)
        for d in range(N_DESTS + 1):
            b, e = C.c_uint64(), C.c_uint64()
            assert nif.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
            assert (b.value, e.value) == (int(ref[0][d]), int(ref[0][d + 1]))
            assert tt[b.value:e.value] == ref[1][b.value:e.value].tolist()
            assert tv[b.value:e.value] == ref[2][b.value:e.value].tolist()
        assert te[:n] == ref[3].tolist()
        nif.tmn_give(pool, s)
        nif.shim_pool_free(pool)
    fat.close()
    # the same C file's match half, on the device library for the first time
    h = routed._h
    pool = nif.shim_pool_new(h, in_flags)
    s = nif.tmn_take(pool)
    topics = _topics(300, seed=13)
    blob, offs = _native.pack_strings(topics)
    hit, vals, err = routed.match_batch(blob, offs)
    assert _nif_pack(nif, s, h, topics) == 0
    rc = nif.tmn_match(s, h, len(topics), 0)
    assert rc == 0
    tv = nif.shim_vals(s)
    for i in range(len(topics)):
        b, e = C.c_uint64(), C.c_uint64()
        flag = nif.tmn_row(s, len(topics), 0, i, C.byref(b), C.byref(e))
        assert flag == int(err[i])
        assert tv[b.value:e.value] == vals[int(hit[i]):int(hit[i + 1])].tolist()
    nif.tmn_give(pool, s)
    nif.shim_pool_free(pool)


# ---- 11. refusals: the six entry points of the route family, one table

R_N, R_DESTS, R_CAP, R_STATE = 1, 2, 8, 5
R_COUNTERS = (ONE, GRID, _native.TM_DEBUG_DISPATCH_ONE, _native.TM_DEBUG_DISPATCH_GRID,
              _native.TM_DEBUG_PUBLISH_ONE, _native.TM_DEBUG_PUBLISH_GRID)
R_ENTRIES = ("tm_route_batch_ex", "tm_route_batch32_ex", "tm_dispatch_batch", "tm_dispatch_batch32",
             "tm_publish_batch", "tm_publish_batch32")
ALL, WIDE32, DISPATCHING = R_ENTRIES, R_ENTRIES[1::2], R_ENTRIES[2:]
# row -> (the argument it spoils, its value, the entry points that have it)
R_ROWS = {
    "unknown-flag": ("flags", 0x80 | _native.TM_ROUTE_AGGRE, ALL),
    "n_dests-0": ("n_dests", 0, ALL),
    "n_dests-65537": ("n_dests", 65537, ALL),
    "local_dest-n_dests": ("local", R_DESTS, DISPATCHING),
    "null-dest_offsets": ("doff", None, ALL),
    "null-err": ("err", None, WIDE32),
    "null-topic": ("topic", None, ALL),
    "null-head": ("head", None, DISPATCHING),
    "null-dtopic": ("dt", None, DISPATCHING),
    "null-dvalue": ("dv", None, DISPATCHING),
    "null-dsub": ("ds", None, DISPATCHING),
    "misaligned-head": ("head", "+4", WIDE32[1:]),
    "no-aggre": ("flags", 0, R_ENTRIES[4:]),
    "null-member": ("member", None, R_ENTRIES[4:]),
}
R_CASES = [(entry, row) for entry in R_ENTRIES for row in R_ROWS if entry in R_ROWS[row][2]]
HEAD_CANARY = 0xABCDEF0123456789


@pytest.fixture(scope="module")
def refusing(gpu):
    """one filter, routed, with a subscriber and a shared slot whose state word is R_STATE; every
    buffer of every call pinned (an eligible in-place batch, were it not refused)"""
    ix = _native.Index()
    ix.set_route_filters([0], [0])
    ix.set_subscribers([0], [[7, 8]])
    ix.set_share_members([0], [[3, 4]], [0], [_native.TM_SHARE_ROUND_ROBIN])
    ix.share_state_set([0], [R_STATE])
    ix.set_share_slots([0], [0])
    _insert(ix, [b"a/b"], [0], [0])
    u32, u64 = np.uint32, np.uint64
    a = {"blob": ix.host_array(64, np.uint8), "offs32": ix.host_array(R_N + 1, u32), "offs64": ix.host_array(R_N + 1, u64),
         "doff32": ix.host_array(R_DESTS + 2 + TAIL, u32), "doff64": ix.host_array(R_DESTS + 2 + TAIL, u64),
         "err": ix.host_array(R_N + TAIL, np.uint8), "head": ix.host_array(3, u64),
         "kc": ix.host_array(R_N, u32), "kt": ix.host_array(R_N, u32)}
    for name in ("topic", "vals", "member", "dt", "dv", "ds"):
        a[name] = ix.host_array(R_CAP + TAIL, u32)
    a["blob"][:3] = np.frombuffer(b"a/b", np.uint8)
    a["offs32"][:], a["offs64"][:] = (0, 3), (0, 3)
    yield ix, a
    ix.close()


@pytest.mark.parametrize("entry,row", R_CASES, ids=[f"{e}-{r}" for e, r in R_CASES])
def test_refusals(refusing, entry, row):
    """a refused call returns TM_EINVAL, writes no output, counts on no leg, moves no state word,
    and says in tm_last_error which entry point was called"""
    ix, a = refusing
    w = "32" if "32" in entry else "64"
    outs = [a["doff" + w], a["err"], a["head"]] + [a[k] for k in ("topic", "vals", "member", "dt", "dv", "ds")]
    for o in outs:
        o[:] = HEAD_CANARY if o.dtype == np.uint64 else ERRC if o.dtype == np.uint8 else CANARY
    arg = {k: P(a[k]) for k in ("blob", "err", "head", "topic", "vals", "member", "dt", "dv", "ds", "kc", "kt")}
    arg.update(offs=P(a["offs" + w]), doff=P(a["doff" + w]), n_dests=R_DESTS, local=0, flags=_native.TM_ROUTE_AGGRE)
    what, value, _ = R_ROWS[row]
    arg[what] = C.c_void_p(a["head"].ctypes.data + 4) if value == "+4" else value
    head = [arg["n_dests"]]
    tail = [arg["doff"], arg["topic"], arg["vals"], R_CAP]
    if "route" in entry:
        args = head + tail + [arg["err"], arg["flags"]]
    else:
        args = head + [arg["local"], arg["flags"]] + tail + [arg["head"], arg["dt"], arg["dv"], arg["ds"], R_CAP]
        if "publish" in entry:
            args += [arg["kc"], arg["kt"], 1, arg["member"]]
        args.append(arg["err"])
    before = [ix.debug_get(k) for k in R_COUNTERS]
    rc = getattr(ix._lib, entry)(ix._h, R_N, arg["blob"], arg["offs"], *args)
    said = ix._lib.tm_last_error(ix._h)
    assert rc == _native.TM_EINVAL
    for o in outs:
        assert (o == (HEAD_CANARY if o.dtype == np.uint64 else ERRC if o.dtype == np.uint8 else CANARY)).all(), \
            "a refused call wrote an output"
    assert [ix.debug_get(k) for k in R_COUNTERS] == before, "a refused call counted on a leg"
    if "publish" in entry:
        assert ix.share_state_get([0]).tolist() == [R_STATE], "a refused call moved the state word"
    assert entry.encode() in said, f"tm_last_error names another function: {said!r}"
