"""tm_dispatch_batch32: the 32-bit, in-place route + local dispatch call for a
NIF's micro-batches.

The reference everywhere is the unchanged tm_dispatch_batch on the same index,
topics, n_dests, local_dest, flags, cap and dcap: the return code, the bucket
offsets, the head and every output array -- each filled with a canary first and
compared WHOLE, tail included, so a word written past min(total, cap), past
min(T, dcap) or past out_dest_offsets[n_dests + 1] fails the comparison.  On the
synthetic index the deliveries are also compared with include/tmatch.h's
definition worked out on the host.  The inputs are compared after every run,
and TM_DEBUG_DISPATCH_ONE / TM_DEBUG_DISPATCH_GRID say which leg finished the
call: the one-launch kernel (k_dp_one), or the grid kernels / the staged path.

k_dp_one gives each of its 16 waves a chunk of ceil(M / 16) entries rounded up
to 64 for the counts, and of ceil(W / 16) output positions rounded up to 64 for
the expansion: M = 1024 fills every wave's first step exactly, 1025 takes a
second; a list of 5,000 spans the chunks of all 16 waves.
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
from emqx_amd.subscribers import LocalSubs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FO1_TOPICS, FO1_ENTRIES, DP1_DELIVERIES = 8192, 16384, 32768   # emqx_amd/csrc/tm_dev.h
CANARY, OFFC, ERRC, HEADC, TAIL = 0xC0FFEE11, 0xDEADBEEF, 0xEE, 0xABCDEF0123456789, 64
ONE, GRID, DP1_MAX = _native.TM_DEBUG_DISPATCH_ONE, _native.TM_DEBUG_DISPATCH_GRID, _native.TM_DEBUG_DP1_MAX
AGGRE = _native.TM_ROUTE_AGGRE
OK, ECAP, EINVAL = _native.TM_OK, _native.TM_ECAP, _native.TM_EINVAL
P = _native._ptr


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _insert(ix, filters, values, dests, filter_ids=None):
    values = np.asarray(values, np.uint32)
    keep = [i for i, d in enumerate(dests) if d is not None]
    ix.set_dests(values[keep], np.array([dests[i] for i in keep], np.uint32))
    if filter_ids is not None:
        ix.set_route_filters(values, np.asarray(filter_ids, np.uint32))
    blob, offs = _native.pack_strings(filters)
    ix.apply(np.ones(len(filters), np.uint8), blob, offs, values)


# ---- the reference and the call under test, both on canary-filled outputs

def _reference(ix, topics, n_dests, local, flags, cap, dcap):
    """tm_dispatch_batch -> (rc, doff u64, topic, values, head, dtopic, dvalue, dsub, err), the arrays whole"""
    blob, offs = _native.pack_strings(topics)
    n = len(topics)
    doff, head = np.zeros(n_dests + 2, np.uint64), np.full(2, HEADC, np.uint64)
    t, v = (np.full(cap + TAIL, CANARY, np.uint32) for _ in range(2))
    dt, dv, ds = (np.full(dcap + TAIL, CANARY, np.uint32) for _ in range(3))
    err = np.zeros(max(n, 1), np.uint8)
    rc = ix._lib.tm_dispatch_batch(ix._h, n, P(blob), P(offs), n_dests, local, flags, P(doff), P(t), P(v), cap, P(head),
                                   P(dt), P(dv), P(ds), dcap, P(err))
    assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
    return rc, doff, t, v, head, dt, dv, ds, err[:n]


class Bufs:
    """one caller's batch buffers: host_array (pinned; the inputs optionally TM_ALLOC_VRAM) or plain numpy"""

    def __init__(self, ix, nmax, bytes_max, dmax, cap_max, dcap_max, pinned=True, vram_inputs=False, plain=()):
        def alloc(name, k, dt, vram=False):
            if not pinned or name in plain:
                return np.zeros(max(k, 1), dt)
            a = ix.host_array(k, dt, vram=vram)
            self.owned.append(a)
            return a
        self.ix, self.cap_max, self.dcap_max, self.owned = ix, cap_max, dcap_max, []
        self.blob = alloc("blob", bytes_max + 48, np.uint8, vram_inputs)
        self.offs = alloc("offs", nmax + 1, np.uint32, vram_inputs)
        self.doff, self.err = alloc("doff", dmax + 2 + TAIL, np.uint32), alloc("err", nmax + TAIL, np.uint8)
        self.topic, self.vals = alloc("topic", cap_max + TAIL, np.uint32), alloc("vals", cap_max + TAIL, np.uint32)
        self.head = alloc("head", 2, np.uint64)
        self.dt, self.dv, self.ds = (alloc(k, dcap_max + TAIL, np.uint32) for k in ("dt", "dv", "ds"))
        self.vram_inputs = vram_inputs

    def free(self):
        for a in self.owned:
            self.ix.host_free(a)

    def call(self, topics, n_dests, local, flags=0, cap=None, dcap=None, shift=0):
        """tm_dispatch_batch32 -> what _reference returns (doff as u32), arrays whole up to cap / dcap + TAIL"""
        blob, offs = _native.pack_strings(topics)
        n, nb = len(topics), int(offs[-1])
        cap = self.cap_max if cap is None else cap
        dcap = self.dcap_max if dcap is None else dcap
        assert cap <= self.cap_max and dcap <= self.dcap_max and n + 1 <= len(self.offs)
        assert nb + shift <= len(self.blob)
        self.blob[shift:shift + nb] = blob[:nb]
        self.offs[:n + 1] = offs
        self.doff[:], self.topic[:], self.vals[:], self.err[:] = OFFC, CANARY, CANARY, ERRC
        self.dt[:], self.dv[:], self.ds[:], self.head[:] = CANARY, CANARY, CANARY, HEADC
        ix = self.ix
        rc = ix._lib.tm_dispatch_batch32(ix._h, n, P(self.blob[shift:]), P(self.offs), n_dests, local, flags,
                                         P(self.doff), P(self.topic), P(self.vals), cap, P(self.head), P(self.dt),
                                         P(self.dv), P(self.ds), dcap, P(self.err))
        assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
        if not self.vram_inputs:   # (device memory is never read back by the host)
            assert np.array_equal(self.blob[shift:shift + nb], blob[:nb]) and np.array_equal(self.offs[:n + 1], offs), \
                "the inputs changed"
        assert (self.doff[n_dests + 2:] == OFFC).all(), "offsets: canary"
        assert (self.err[n:] == ERRC).all(), "err: canary"
        for a, c in ((self.topic, cap), (self.vals, cap), (self.dt, dcap), (self.dv, dcap), (self.ds, dcap)):
            assert (a[c:] == CANARY).all(), "written past the capacity"
        return rc, self.doff[:n_dests + 2].copy(), self.topic[:cap + TAIL].copy(), self.vals[:cap + TAIL].copy(), \
            self.head.copy(), self.dt[:dcap + TAIL].copy(), self.dv[:dcap + TAIL].copy(), self.ds[:dcap + TAIL].copy(), \
            self.err[:n].copy()


def _same(got, ref):
    names = ("rc", "bucket offsets", "topic", "values", "head", "dtopic", "dvalue", "dsub", "err")
    for name, g, r in zip(names, got, ref):
        if name == "rc":
            assert g == r, f"return code {g}, tm_dispatch_batch's {r}"
        else:
            assert np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(r).astype(np.uint64)), name


def _check(ix, bufs, topics, n_dests, local, leg, flags=0, cap=None, dcap=None, shift=0, ref=None):
    """one call against tm_dispatch_batch; leg: ONE or GRID must rise by one, the other stay put.
    -> (rc, total, M, T)"""
    cap = bufs.cap_max if cap is None else cap
    dcap = bufs.dcap_max if dcap is None else dcap
    ref = ref or _reference(ix, topics, n_dests, local, flags, cap, dcap)
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
    got = bufs.call(topics, n_dests, local, flags, cap, dcap, shift)
    c1 = (ix.debug_get(ONE), ix.debug_get(GRID))
    _same(got, ref)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if leg == ONE else (0, 1)), "which leg finished the call"
    rc, doff, t, v, head = got[:5]
    total, T = int(doff[-1]), int(head[1])
    assert (t[min(total, cap):] == CANARY).all() and (got[5][min(T, dcap):] == CANARY).all()
    return rc, total, int(head[0]), T


# ---- a routed index: 2,000 filters over 4 destinations, aggre drops something

N_DESTS, LOCAL = 4, 1


def _routed_index(copies=1):
    fs = ([f"a{x}/+/c{z}" for x in range(60) for z in range(9)] + [f"a{x}/#" for x in range(60)] +
          [f"+/b{y}/#" for y in range(45)] + [f"a{x}/b{y}/+" for y in range(45) for x in range(60)])[:2000]
    fs = [f.encode() for f in fs]
    nf = len(fs)
    assert len(set(fs)) == nf == 2000
    dests = [None if v % 11 == 0 else (v // 4) % N_DESTS for v in range(nf)]
    # every fourth filter has a second route with the same destination: aggre/1 keeps one of the two
    twins = list(range(0, nf, 4))
    ix = _native.Index(copies=copies)
    _insert(ix, fs + [fs[v] for v in twins], list(range(nf)) + [nf + k for k in range(len(twins))],
            dests + [dests[v] for v in twins], list(range(nf)) + twins)
    # subscribers: 0 to 4 each, values never set, one broadcast filter
    vals = [v for v in range(nf + len(twins)) if v % 7]
    ix.set_subscribers(vals, [[v * 8 + r for r in range(v % 5)] for v in vals])
    return ix


@pytest.fixture(scope="module")
def routed(gpu):
    return _routed_index()


@pytest.fixture(scope="module")
def bufs(routed):
    b = Bufs(routed, 4200, 4200 * 24, 256, 40_000, 70_000)
    yield b
    b.free()


def _topics(n, seed=1):
    rng = np.random.default_rng(seed)
    out = [f"a{rng.integers(0, 80)}/b{rng.integers(0, 45)}/c{rng.integers(0, 9)}".encode() for _ in range(n)]
    for i in range(0, n, 97):
        out[i] = (b"a1/+/c1", b"#", b"a/#/b")[i % 3]          # badarg
    for i in range(5, n, 89):
        out[i] = f"zzz{i}".encode()                          # no route at all
    return out


# ---- 1. shapes

@pytest.mark.parametrize("topics,deliveries", [([], 0), ([b"zzz"], 0), ([b"a1/b2/c3"], None), ([b"a1/+/c1"], 0)],
                         ids=["n0", "n1-nohit", "n1-local", "n1-badarg"])
def test_tiny_batches(gpu, topics, deliveries):
    ix = _native.Index()
    _insert(ix, [b"a1/#", b"a1/+/c3", b"+/b2/#"], [0, 1, 2], [LOCAL, 0, None])
    ix.set_subscribers([0, 1], [[70, 71], [72]])
    b = Bufs(ix, 4, 64, 16, 64, 64)
    rc, total, M, T = _check(ix, b, topics, N_DESTS, LOCAL, ONE)
    assert rc == OK and T == (2 if deliveries is None else deliveries)
    if deliveries is None:
        assert (total, M) == (3, 1) and b.ds[:2].tolist() == [70, 71] and b.dv[:2].tolist() == [0, 0]
    b.free()
    ix.close()


@pytest.mark.parametrize("flags", [0, AGGRE], ids=["plain", "aggre"])
@pytest.mark.parametrize("n", [63, 64, 65, 1000, 4096])
def test_shapes_equal_dispatch_batch(routed, bufs, n, flags):
    topics = _topics(n, seed=n)
    rc, total, M, T = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, flags)
    assert rc == OK and total > n // 2 and total <= FO1_ENTRIES and M > n // 8 and T > M
    if flags:
        plain = _reference(routed, topics, N_DESTS, LOCAL, 0, 40_000, 70_000)
        assert int(plain[1][-1]) > total, "aggre/1 dropped something"
        assert n < 1000 or int(plain[4][1]) > T, "local entries with subscribers too"


# ---- 2. a synthetic index: every entry's list is known

S_DESTS = 3
S_LISTS = {0: 1000, 1: 1, 2: 5000, 3: 0, 4: 3, 5: 2, 6: None, 7: 8, 8: 9, 9: 1}   # value -> list length (None: never set)
S_DEST = {4: 1, 5: S_DESTS - 1}                                                  # (every other value: destination 0)


def _subs(v):
    return [] if S_LISTS[v] is None else [(v << 20) + r for r in range(S_LISTS[v])]


@pytest.fixture(scope="module")
def synth(gpu):
    """'$s<v>/+' carries value v: topic '$s<v>/x' has exactly that one entry ('#' does not match a '$'
    topic), so bucket 0 holds the listed values' entries in topic order.  '#' x 3 (values 100-102) and
    '$e/x' (103), destination 0 and one subscriber each, make exact entry counts as in the route tests:
    a plain topics and s x '$e/x' have E = 3 a + s entries, every one local with one delivery"""
    ix = _native.Index()
    vs = sorted(S_LISTS)
    _insert(ix, [b"$s%d/+" % v for v in vs] + [b"#", b"#", b"#", b"$e/x"], vs + [100, 101, 102, 103],
            [S_DEST.get(v, 0) for v in vs] + [0, 0, 0, 0])
    ix.set_subscribers([v for v in vs if S_LISTS[v] is not None] + [100, 101, 102, 103],
                       [_subs(v) for v in vs if S_LISTS[v] is not None] + [[5000], [5001], [5002], [5003]])
    b = Bufs(ix, 8200, 8200 * 8, 16, 17_000, 70_000)
    yield ix, b
    b.free()


def _model(values, local):
    """include/tmatch.h's definition for topics '$s<v>/x': [(topic index, value, subscriber)] of bucket `local`"""
    return [(i, v, s) for i, v in enumerate(values) if S_DEST.get(v, 0) == local for s in _subs(v)]


def _check_synth(synth, values, local=0, leg=ONE, dcap=None):
    ix, b = synth
    rc, total, M, T = _check(ix, b, [b"$s%d/x" % v for v in values], S_DESTS, local, leg, dcap=dcap)
    exp = _model(values, local)
    assert total == len(values) and M == sum(S_DEST.get(v, 0) == local for v in values) and T == len(exp)
    assert list(zip(b.dt[:T].tolist(), b.dv[:T].tolist(), b.ds[:T].tolist())) == exp, "differs from the definition"
    return rc, total, M, T


SHAPES = {
    "one-list-of-1000-among-single-ones": [1] * 50 + [0] + [1] * 50,
    "a-list-of-5000-with-M-3": [1, 2, 1],
    "200-empty-entries-in-a-row": [1] + [3] * 200 + [1],
    "empty-first-and-last": [3, 1, 1, 3],
    "the-same-value-twice": [7, 7, 1, 1],
    "a-value-never-set": [1, 6, 6, 7, 6],
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_list_shapes(synth, shape):
    values = SHAPES[shape]
    rc, total, M, T = _check_synth(synth, values)
    assert rc == OK and M == len(values) and T == sum(S_LISTS[v] or 0 for v in values)


def test_entries_without_a_delivery_and_an_empty_local_bucket(gpu):
    ix = _native.Index()
    _insert(ix, [b"s3/+", b"s4/+", b"s1/+"], [3, 4, 1], [0, 1, 0])
    ix.set_subscribers([3, 4, 1], [[], [40, 41, 42], [10]])
    b = Bufs(ix, 64, 64 * 8, 16, 256, 256)
    rc, total, M, T = _check(ix, b, [b"s3/x"] * 10, S_DESTS, 0, ONE)             # M > 0 with T = 0
    assert (rc, total, M, T) == (OK, 10, 10, 0)
    rc, total, M, T = _check(ix, b, [b"s4/x"] * 20, S_DESTS, 0, ONE)             # the local bucket empty, another full
    assert (rc, total, M, T) == (OK, 20, 0, 0)
    rc, total, M, T = _check(ix, b, [b"s4/x"] * 20 + [b"s1/y"], S_DESTS, 1, ONE)
    assert (rc, total, M, T) == (OK, 21, 20, 60) and b.ds[:3].tolist() == [40, 41, 42]
    b.free()
    ix.close()


@pytest.mark.parametrize("local", [0, S_DESTS - 1])
def test_first_and_last_destination(synth, local):
    values = [1, 5, 4, 5, 7, 5]
    rc, total, M, T = _check_synth(synth, values, local=local)
    assert rc == OK and (M, T) == ((2, 9) if local == 0 else (3, 6))


def _exact_topics(a=0, s=0, z=0):
    t = [b"p/%d" % i for i in range(a)] + [b"$e/x"] * s + [b"$none"] * z
    rng = np.random.default_rng(len(t))
    return [t[i] for i in rng.permutation(len(t))], 3 * a + s


@pytest.mark.parametrize("E", [1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, FO1_ENTRIES - 1, FO1_ENTRIES,
                               FO1_ENTRIES + 1])
def test_local_bucket_sizes(synth, E):
    """every hit local, one subscriber each: M = T = E; FO1_ENTRIES + 1 is finished by the grid kernels"""
    ix, b = synth
    a = min(E // 3, 5000)
    topics, e = _exact_topics(a=a, s=E - 3 * a, z=37)
    assert e == E and len(topics) <= FO1_TOPICS
    rc, total, M, T = _check(ix, b, topics, S_DESTS, 0, ONE if E <= FO1_ENTRIES else GRID)
    assert (rc, total, M, T) == (OK, E, E, E)


# ---- 3. the bound on T

def test_delivery_bound_lowered(synth):
    ix, b = synth
    assert ix.debug_get(DP1_MAX) == DP1_DELIVERIES
    ix.debug_set(DP1_MAX, 1 << 40)
    assert ix.debug_get(DP1_MAX) == DP1_DELIVERIES, "clamped to the compiled bound"
    ix.debug_set(DP1_MAX, 256)
    try:
        assert ix.debug_get(DP1_MAX) == 256
        for T, leg in ((255, ONE), (256, ONE), (257, GRID)):
            topics, e = _exact_topics(s=T)
            rc, total, M, t = _check(ix, b, topics, S_DESTS, 0, leg)
            assert (rc, total, M, t) == (OK, T, T, T)
        # and cut by dcap on the grid leg: the head is exact, nothing past dcap
        topics, e = _exact_topics(s=300)
        rc, total, M, t = _check(ix, b, topics, S_DESTS, 0, GRID, dcap=100)
        assert (rc, M, t) == (ECAP, 300, 300)
    finally:
        ix.debug_set(DP1_MAX, DP1_DELIVERIES)


@pytest.mark.parametrize("over", [0, 1])
def test_delivery_bound_as_compiled(synth, over):
    """4,096 entries of 8 subscribers: T = DP1_DELIVERIES in one launch; one list of 9 among them: the grid"""
    ix, b = synth
    last, n = 8 if over else 7, DP1_DELIVERIES // 8
    topics = [b"$s7/x"] * (n - 1) + [b"$s%d/x" % last]
    rc, total, M, T = _check(ix, b, topics, S_DESTS, 0, GRID if over else ONE)
    assert (rc, total, M, T) == (OK, n, n, DP1_DELIVERIES + over)
    assert b.ds[T - 1] == (last << 20) + last and b.dt[T - 1] == n - 1


# ---- 4. capacity

def test_capacity(routed, bufs):
    topics = _topics(1000, seed=77)
    full = _reference(routed, topics, N_DESTS, LOCAL, 0, 40_000, 70_000)
    total, T = int(full[1][-1]), int(full[4][1])
    assert total > 500 and T > 300
    for dcap in (0, 1, T - 1, T, T + 1):
        rc, tot, M, t = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=total, dcap=dcap)
        assert (tot, t) == (total, T) and rc == (ECAP if T > dcap else OK)
    rc, tot, M, t = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=total - 1, dcap=T)
    assert rc == ECAP and (tot, t) == (total, T), "full offsets and the exact head"
    rc, tot, M, t = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=total // 2, dcap=T // 2)   # both too small
    assert rc == ECAP and (tot, t) == (total, T)
    rc, tot, M, t = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=0, dcap=0)
    assert rc == ECAP and (tot, t) == (total, T)


def test_capacity_under_aggre(routed, bufs):
    """the un-aggregated total above cap: TM_ECAP with the un-aggregated sizes and no entry, as
    tm_route_batch_ex; the head and the deliveries are the aggregated bucket's all the same"""
    topics = _topics(1000, seed=78)
    plain = _reference(routed, topics, N_DESTS, LOCAL, 0, 40_000, 70_000)
    ag = _reference(routed, topics, N_DESTS, LOCAL, AGGRE, 40_000, 70_000)
    total, K, T = int(plain[1][-1]), int(ag[1][-1]), int(ag[4][1])
    assert K < total and T < int(plain[4][1])
    for cap in (total, total - 1, K, K - 1, 1):
        rc, tot, M, t = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, AGGRE, cap=cap, dcap=T)
        assert rc == (ECAP if total > cap else OK) and tot == (total if total > cap else K) and t == T
        if total > cap:
            assert (bufs.topic == CANARY).all(), "no entry is written"
    rc, tot, M, t = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, AGGRE, cap=K, dcap=T - 1)
    assert rc == ECAP and t == T


# ---- 5. destinations

@pytest.mark.parametrize("n_dests,local,leg", [(1, 0, ONE), (255, LOCAL, ONE), (256, LOCAL, GRID)])
def test_destination_counts(routed, n_dests, local, leg):
    b = Bufs(routed, 1100, 1100 * 24, n_dests, 8000, 8000)
    try:
        rc, total, M, T = _check(routed, b, _topics(1000, seed=n_dests), n_dests, local, leg)
        assert rc == OK and total > 500 and M > 100 and T > 100
    finally:
        b.free()


# ---- 6. eligibility

def test_a_plain_delivery_array_takes_the_staged_path(routed):
    b = Bufs(routed, 600, 600 * 24, 16, 8000, 8000, plain=("dv",))
    try:
        rc, total, M, T = _check(routed, b, _topics(500, seed=3), N_DESTS, LOCAL, GRID)
        assert rc == OK and T > 100
    finally:
        b.free()


def test_a_misaligned_blob_takes_the_staged_path(routed, bufs):
    _check(routed, bufs, _topics(500, seed=4), N_DESTS, LOCAL, GRID, shift=4)
    _check(routed, bufs, _topics(500, seed=4), N_DESTS, LOCAL, ONE, shift=16)


def test_an_index_the_one_launch_walk_refuses(gpu):
    """two copies and a 33-level filter: deeper than the one-launch kernels' fallback store"""
    ix = _native.Index(copies=2)
    deep = b"/".join(b"l%d" % i for i in range(33))
    _insert(ix, [deep, b"l0/#", b"+/l1/#"], [0, 1, 2], [0, 1, None])
    ix.set_subscribers([0, 1, 2], [[1, 2, 3], [4], [5, 6]])
    b = Bufs(ix, 64, 64 * 200, 16, 1000, 1000)
    topics = [deep, b"l0/l1", b"x/l1/y", b"none", b"l0/+"] * 8
    rc, total, M, T = _check(ix, b, topics, 2, 0, GRID)
    assert (rc, total, M, T) == (OK, 8 * (3 + 2 + 1), 8, 24)
    b.free()
    ix.close()


def test_vram_inputs_run_in_place(routed):
    b = Bufs(routed, 600, 600 * 24, 16, 8000, 8000, vram_inputs=True)
    try:
        rc, total, M, T = _check(routed, b, _topics(500, seed=5), N_DESTS, LOCAL, ONE)
        assert rc == OK and T > 100
    finally:
        b.free()


def test_bad_arguments(routed, bufs):
    ix, b = routed, bufs
    offs = np.array([0, 3], np.uint32)
    blob = np.frombuffer(b"a/b" + b"\0" * 13, np.uint8)

    def call(n_dests=N_DESTS, local=LOCAL, flags=0, head=b.head, dt=b.dt, dcap=8, err=b.err, doff=b.doff):
        return ix._lib.tm_dispatch_batch32(ix._h, 1, P(blob), P(offs), n_dests, local, flags, P(doff), P(b.topic),
                                           P(b.vals), 8, None if head is None else head.ctypes.data, P(dt), P(b.dv),
                                           P(b.ds), dcap, P(err))
    assert call() == OK
    assert call(local=N_DESTS) == EINVAL and call(n_dests=0, local=0) == EINVAL and call(flags=2) == EINVAL
    assert call(head=None) == EINVAL and call(dt=None) == EINVAL and call(err=None) == EINVAL
    assert call(doff=None) == EINVAL
    assert call(dt=None, dcap=0) == OK        # (no room asked for: the buffers may be absent; nothing matches)
    odd = np.zeros(5, np.uint64).view(np.uint32)[1:]
    assert ix._lib.tm_dispatch_batch32(ix._h, 1, P(blob), P(offs), N_DESTS, LOCAL, 0, P(b.doff), P(b.topic), P(b.vals), 8,
                                       odd.ctypes.data, P(b.dt), P(b.dv), P(b.ds), 8, P(b.err)) == EINVAL


# ---- 7. read-your-writes

@pytest.mark.parametrize("copies", [1, 2])
def test_read_your_writes(gpu, copies):
    ix = _routed_index(copies)
    b = Bufs(ix, 300, 300 * 24, 16, 8000, 8000)
    topics = _topics(200, seed=5) + [b"fresh/x/y"]
    rc, total, M, T0 = _check(ix, b, topics, N_DESTS, LOCAL, ONE)
    v = int(b.dv[0])                                        # a value with deliveries in this batch
    hits = int((b.dv[:T0] == v).sum())
    entries = int((b.vals[:total] == v).sum())
    for lst in ([9, 8, 7, 6, 5, 4, 3], [9], []):            # a longer list, a shorter one, an empty one
        ix.set_subscribers([v], [lst])
        rc, total, M, T = _check(ix, b, topics, N_DESTS, LOCAL, ONE)
        assert int((b.dv[:T] == v).sum()) == entries * len(lst)
        assert T == T0 - hits + entries * len(lst)
    kid = 50_000
    ix.set_dests([kid], [LOCAL])
    ix.set_subscribers([kid], [[1, 2, 3]])
    blob, offs = _native.pack_strings([b"fresh/+/y"])
    ix.apply(np.ones(1, np.uint8), blob, offs, np.array([kid], np.uint32), commit=True)
    rc, total, M, T = _check(ix, b, topics, N_DESTS, LOCAL, ONE)
    assert b.dv[T - 3:T].tolist() == [kid] * 3 and b.ds[T - 3:T].tolist() == [1, 2, 3] and b.dt[T - 1] == 200
    ix.apply(np.zeros(1, np.uint8), blob, offs, np.array([kid], np.uint32), commit=True)   # the key deleted
    rc, total, M, T2 = _check(ix, b, topics, N_DESTS, LOCAL, ONE)
    assert T2 == T - 3 and not (b.dv[:T2] == kid).any()
    b.free()
    ix.close()


# ---- 8. concurrent callers

def test_eight_concurrent_callers(routed):
    failed0 = routed.debug_get(_native.TM_DEBUG_FAILED_BATCHES)
    batches = [_topics(512, seed=100 + k) for k in range(8)]
    refs = [_reference(routed, tp, N_DESTS, LOCAL, AGGRE if k % 2 else 0, 8000, 8000) for k, tp in enumerate(batches)]
    sets = [Bufs(routed, 512, 512 * 24, 16, 8000, 8000) for _ in range(8)]
    start, bad = threading.Barrier(8), []

    def caller(k):
        try:
            start.wait()
            for _ in range(50):
                _same(sets[k].call(batches[k], N_DESTS, LOCAL, AGGRE if k % 2 else 0), refs[k])
        except BaseException as e:   # noqa: BLE001
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

NODES = ("n1", "n2")
GROUPS = (b"g1", b"g2")


def _router(in_place):
    rng = np.random.default_rng(77)
    subs = LocalSubs()
    r = Router(node="n1", local_subs=subs, route_in_place=in_place)
    dests = list(NODES) + [(g, n) for g in GROUPS for n in ("n1", "n2", "n3")]
    filters = ([f"a{x}/+/c{z}" for x in range(60) for z in range(9)] + [f"a{x}/#" for x in range(60)] +
               [f"+/b{y}/#" for y in range(45)] + [f"a{x}/b{y}/+" for y in range(45) for x in range(60)])[:2000]
    filters = sorted(f.encode() for f in filters)
    pid = 0
    for k, f in enumerate(filters[::2]):              # subscribed before the route exists
        for _ in range(k % 4):
            subs.subscribe(f, ("pid", pid))
            pid += 1
    batch = {}
    for i, f in enumerate(filters):
        batch[(f, "n1" if i % 3 else "n2")] = ("add", 0, None)
        for d in rng.choice(len(dests), 1 + i % 3, replace=False):
            batch[(f, dests[d])] = ("add", 0, None)
    for k in range(300):                              # exact topics: the bag, some rows local
        t = f"a{k % 50}/b{k % 40}/c{k % 7}".encode()
        batch[(t, "n1" if k % 2 else "n2")] = ("add", 0, None)
        if k % 4 == 1:
            subs.subscribe(t, ("pid", k))
            subs.subscribe(t, ("exact", k))
    assert r.do_batch(batch) == {}
    for k, f in enumerate(filters[1::2]):             # and after it
        for _ in range((k + 1) % 4):
            subs.subscribe(f, ("pid", pid))
            pid += 1
    r.add_route(b"a7/#", "n1")
    for k in range(1500):                             # the broadcast filter: past 1,024, shard rows
        subs.subscribe(b"a7/#", ("all", k))
    assert any(isinstance(s, tuple) and s[0] == "shard" for s in subs.subscribers(b"a7/#"))
    return r


@pytest.fixture(scope="module")
def routers(gpu):
    return _router(False), _router(True)


def test_router_in_place_equals_the_default_router(routers):
    plain, inplace = routers
    ix = inplace._mirror._index
    topics = _topics(1500, seed=8)
    for aggre in (False, True):
        e_by, e_del = plain.match_routes_dispatch(topics, errors="return", aggre=aggre)
        c0 = ix.debug_get(ONE) + ix.debug_get(GRID)
        by, got = inplace.match_routes_dispatch(topics, errors="return", aggre=aggre)
        assert ix.debug_get(ONE) + ix.debug_get(GRID) > c0, "tm_dispatch_batch32 served the call"
        assert dict(by) == dict(e_by) and set(by.errors) == set(e_by.errors)
        assert got == e_del and len(got) > 10_000
        assert any(p[0] == "exact" for _, _, p in got) and any(p[0] == "all" for _, _, p in got)   # bag rows; shard rows


def test_broker_over_the_in_place_router_delivers_the_host_walks_multiset(routers):
    _, r = routers
    subs = r.local_subs
    msgs = [Message(t, i) for i, t in enumerate(_topics(1200, seed=9))]
    log, sent, got = Counter(), [], []

    def walk(to, m):
        pids = subs.dispatch_order(to)
        sent.extend((p, to, m.payload) for p in pids)
        return len(pids)

    def broker(**kw):
        return Broker(r, dispatch=walk, forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1, **kw)
    broker().publish_batch(msgs)
    exp_log, exp_sent, log, sent = log, sent, Counter(), []
    ix = r._mirror._index
    c0 = ix.debug_get(ONE) + ix.debug_get(GRID)
    broker(dispatch_on_device=True, deliver=lambda p, to, m: got.append((p, to, m.payload))).publish_batch_by_dest(msgs)
    assert ix.debug_get(ONE) + ix.debug_get(GRID) > c0
    assert sent == [] and log == exp_log and Counter(got) == Counter(exp_sent) and len(got) > 5_000


# ---- 10. the NIF half on the real library

@pytest.fixture(scope="module")
def nif(tmp_path_factory, gpu):
    out = tmp_path_factory.mktemp("nifdispatch") / "libnifdispatch.so"
    libdir = ROOT / "emqx_amd"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out),
                    str(ROOT / "c_src" / "tmatch_nif_core.c"), str(ROOT / "c_src" / "tmatch_nif_route.c"),
                    str(ROOT / "c_src" / "tmatch_nif_dispatch.c"), str(ROOT / "tests" / "native" / "nif_route_shim.c"),
                    f"-L{libdir}", "-l:libtmatch.so", f"-Wl,-rpath,{libdir}"], check=True)
    _native.load_library()
    lib = C.CDLL(str(out))
    vp, u32 = C.c_void_p, C.c_uint32
    p32, p64 = C.POINTER(u32), C.POINTER(C.c_uint64)
    lib.shim_pool_new.restype = vp
    lib.shim_pool_new.argtypes = [vp, u32]
    lib.shim_pool_free.argtypes = [vp]
    lib.tmn_take.restype = vp
    lib.tmn_take.argtypes = [vp]
    lib.tmn_give.argtypes = [vp, vp]
    lib.tmn_pack.argtypes = [vp, vp, u32, vp, vp]
    lib.tmn_dispatch.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_route_dest.argtypes = [vp, u32, p64, p64]
    lib.tmn_deliveries.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), C.POINTER(p32), p64]
    for f in (lib.shim_vals, lib.shim_route_topics):
        f.argtypes, f.restype = [vp], p32
    lib.shim_err.argtypes, lib.shim_err.restype = [vp], C.POINTER(C.c_uint8)
    lib.shim_reruns.argtypes, lib.shim_reruns.restype = [vp], C.c_uint64
    return lib


@pytest.mark.parametrize("in_flags", [0, _native.TM_ALLOC_VRAM], ids=["pinned", "vram"])
def test_nif_half_dispatches_on_the_real_library(routed, nif, in_flags):
    """tmn_pack -> tmn_dispatch -> tmn_route_dest / tmn_deliveries == Index.dispatch_batch, with a forced
    TM_ECAP rerun (more deliveries than TMN_IDS_PER_TOPIC per topic)"""
    fat = _native.Index()
    _insert(fat, [b"#"] * 30, np.arange(30), [v % 3 for v in range(30)])
    fat.set_subscribers(np.arange(30), [[v * 1000 + r for r in range(100)] for v in range(30)])
    for ix, topics, n_dests, local, aggre, rerun in ((routed, _topics(700, seed=12), N_DESTS, LOCAL, True, 0),
                                                     (fat, [b"t/%d" % i for i in range(20)], 3, 0, False, 1)):
        h = ix._h
        pool = nif.shim_pool_new(h, in_flags)   # (vram: the core falls back to pinned memory without a large BAR)
        s = nif.tmn_take(pool)
        n = len(topics)
        blob, offs = _native.pack_strings(topics)
        (doff, rt, rv, err), (dt, dv, ds) = ix.dispatch_batch(blob, offs, n_dests, local, cap=1 << 16, dcap=1 << 17,
                                                              aggre=aggre)
        one0 = ix.debug_get(ONE)
        arr = (C.c_char_p * n)(*topics)
        lens = (C.c_uint64 * n)(*[len(t) for t in topics])
        assert nif.tmn_pack(s, h, n, C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p)) == 0
        assert nif.tmn_dispatch(s, h, n, n_dests, local, AGGRE if aggre else 0) == 0
        assert nif.shim_reruns(s) == rerun
        assert ix.debug_get(ONE) - one0 == 1 + rerun, "in place, the rerun too"
        tv, tt, te = nif.shim_vals(s), nif.shim_route_topics(s), nif.shim_err(s)
        for d in range(n_dests + 1):
            b, e = C.c_uint64(), C.c_uint64()
            assert nif.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
            assert (b.value, e.value) == (int(doff[d]), int(doff[d + 1]))
            assert tt[b.value:e.value] == rt[b.value:e.value].tolist()
            assert tv[b.value:e.value] == rv[b.value:e.value].tolist()
        assert te[:n] == err.tolist()
        pt, pv, ps = (C.POINTER(C.c_uint32)() for _ in range(3))
        cnt = C.c_uint64()
        assert nif.tmn_deliveries(s, C.byref(pt), C.byref(pv), C.byref(ps), C.byref(cnt)) == 0
        T = cnt.value
        assert T == len(dt) and T > (3000 if rerun else 300)
        assert pt[:T] == dt.tolist() and pv[:T] == dv.tolist() and ps[:T] == ds.tolist()
        nif.tmn_give(pool, s)
        nif.shim_pool_free(pool)
    fat.close()
