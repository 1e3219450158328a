"""tm_deliver_batch32: the 32-bit, in-place route + local dispatch + grouping by
subscriber for a NIF's micro-batches.

The reference everywhere is the unchanged tm_deliver_batch on the same index,
topics, n_dests, local_dest, flags, cap, dcap and gcap: the return code, the
bucket offsets, both heads and every output array -- each filled with a canary
first and compared WHOLE, tail included, so a word written past min(total,
cap), min(T, dcap), min(G, gcap) or out_goff[min(G, gcap)] fails the
comparison; out_goff and the bucket offsets are compared after narrowing.
tests/group_ref.py's numpy definition applied to tm_dispatch_batch32's output
of the same batch is a second, independent check.  The inputs are compared
after every run, and TM_DEBUG_DELIVER_ONE / TM_DEBUG_DELIVER_GRID say which leg
finished the call: the one-workgroup grouping (k_gs_one), or the grid kernels /
the staged path.

k_gs_one gives each of its 16 waves ceil(W / 16) positions rounded up to 64: W =
1,024 fills every wave's first step exactly, 1,025 takes a second; 16,384 is
the compiled bound.  Large W comes from few topics and long subscriber lists.
"""
import threading

import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.broker import Broker, Message
from emqx_amd.router import Router
from emqx_amd.subscribers import LocalSubs
from group_ref import group_ref

pytestmark = pytest.mark.gpu

FO1_TOPICS, FO1_ENTRIES, GS1_DELIVERIES = 8192, 16384, 16384   # emqx_amd/csrc/tm_dev.h
CANARY, OFFC, ERRC, HEADC, TAIL = 0xC0FFEE11, 0xDEADBEEF, 0xEE, 0xABCDEF0123456789, 64
ONE, GRID = _native.TM_DEBUG_DELIVER_ONE, _native.TM_DEBUG_DELIVER_GRID
GS1_MAX, DP1_MAX = _native.TM_DEBUG_GS1_MAX, _native.TM_DEBUG_DP1_MAX
RUN, SKIPPED = _native.TM_DEBUG_GROUP_PASSES_RUN, _native.TM_DEBUG_GROUP_PASSES_SKIPPED
AGGRE = _native.TM_ROUTE_AGGRE
OK, ECAP, EINVAL = _native.TM_OK, _native.TM_ECAP, _native.TM_EINVAL
P = _native._ptr
NAMES = ("rc", "bucket offsets", "topic", "values", "head", "dtopic", "dvalue", "dsub", "ghead", "gsub", "goff", "err")


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

def _reference(ix, topics, n_dests, local, flags, cap, dcap, gcap):
    """tm_deliver_batch -> NAMES' tuple, the arrays whole (goff u64)"""
    blob, offs = _native.pack_strings(topics)
    n = len(topics)
    doff, head, ghead = np.zeros(n_dests + 2, np.uint64), np.full(2, HEADC, np.uint64), np.full(2, HEADC, np.uint64)
    t, v = (np.full(cap + TAIL, CANARY, np.uint32) for _ in range(2))
    dt, dv, ds = (np.full(dcap + TAIL, CANARY, np.uint32) for _ in range(3))
    gsub, goff = np.full(gcap + TAIL, CANARY, np.uint32), np.full(gcap + 1 + TAIL, OFFC, np.uint64)
    err = np.zeros(max(n, 1), np.uint8)
    rc = ix._lib.tm_deliver_batch(ix._h, n, P(blob), P(offs), n_dests, local, flags, P(doff), P(t), P(v), cap, P(head),
                                  P(dt), P(dv), P(ds), dcap, P(ghead), P(gsub), P(goff), gcap, P(err))
    assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
    return rc, doff, t, v, head, dt, dv, ds, ghead, gsub, goff, err[:n]


class Bufs:
    """one caller's batch buffers: host_array (pinned; the inputs optionally TM_ALLOC_VRAM) or plain numpy;
    x*: a second set of delivery arrays for the tm_dispatch_batch32 call the numpy definition is applied to"""

    def __init__(self, ix, nmax, bytes_max, dmax, cap_max, dcap_max, gcap_max=None, vram_inputs=False, plain=()):
        def alloc(name, k, dt, vram=False):
            if name in plain:
                return np.zeros(max(k, 1), dt)
            a = ix.host_array(k, dt, vram=vram)
            self.owned.append(a)
            return a
        gcap_max = dcap_max if gcap_max is None else gcap_max
        self.ix, self.cap_max, self.dcap_max, self.gcap_max, self.owned = ix, cap_max, dcap_max, gcap_max, []
        self.blob = alloc("blob", bytes_max + 48, np.uint8, vram_inputs)
        self.offs = alloc("offs", nmax + 1, np.uint32, vram_inputs)
        self.doff, self.err = alloc("doff", dmax + 2 + TAIL, np.uint32), alloc("err", nmax + TAIL, np.uint8)
        self.topic, self.vals = alloc("topic", cap_max + TAIL, np.uint32), alloc("vals", cap_max + TAIL, np.uint32)
        self.head, self.ghead, self.xhead = (alloc(k, 2, np.uint64) for k in ("head", "ghead", "xhead"))
        self.dt, self.dv, self.ds = (alloc(k, dcap_max + TAIL, np.uint32) for k in ("dt", "dv", "ds"))
        self.xdt, self.xdv, self.xds = (alloc(k, dcap_max + TAIL, np.uint32) for k in ("xdt", "xdv", "xds"))
        self.gsub, self.goff = alloc("gsub", gcap_max + TAIL, np.uint32), alloc("goff", gcap_max + 1 + TAIL, np.uint32)
        self.vram_inputs = vram_inputs

    def free(self):
        for a in self.owned:
            self.ix.host_free(a)

    def _load(self, topics, shift=0):
        blob, offs = _native.pack_strings(topics)
        n, nb = len(topics), int(offs[-1])
        assert n + 1 <= len(self.offs) and nb + shift <= len(self.blob)
        self.blob[shift:shift + nb] = blob[:nb]
        self.offs[:n + 1] = offs
        self.doff[:], self.topic[:], self.vals[:], self.err[:] = OFFC, CANARY, CANARY, ERRC
        return blob, offs, n, nb

    def dispatch32(self, topics, n_dests, local, flags, cap, dcap):
        """tm_dispatch_batch32 of the same batch -> (head, dtopic, dvalue, dsub), its first min(T, dcap) deliveries"""
        _, _, n, _ = self._load(topics)
        ix = self.ix
        rc = ix._lib.tm_dispatch_batch32(ix._h, n, P(self.blob), P(self.offs), n_dests, local, flags, P(self.doff),
                                         P(self.topic), P(self.vals), cap, P(self.xhead), P(self.xdt), P(self.xdv),
                                         P(self.xds), dcap, P(self.err))
        assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
        w = min(int(self.xhead[1]), dcap)
        return self.xhead.copy(), self.xdt[:w].copy(), self.xdv[:w].copy(), self.xds[:w].copy()

    def call(self, topics, n_dests, local, flags=0, cap=None, dcap=None, gcap=None, shift=0):
        """tm_deliver_batch32 -> what _reference returns (doff and goff as u32), arrays whole up to the cap + TAIL"""
        cap = self.cap_max if cap is None else cap
        dcap = self.dcap_max if dcap is None else dcap
        gcap = self.gcap_max if gcap is None else gcap
        assert cap <= self.cap_max and dcap <= self.dcap_max and gcap <= self.gcap_max
        blob, offs, n, nb = self._load(topics, shift)
        self.dt[:], self.dv[:], self.ds[:], self.head[:], self.ghead[:] = CANARY, CANARY, CANARY, HEADC, HEADC
        self.gsub[:], self.goff[:] = CANARY, OFFC
        ix = self.ix
        rc = ix._lib.tm_deliver_batch32(ix._h, n, P(self.blob[shift:]), P(self.offs), n_dests, local, flags, P(self.doff),
                                        P(self.topic), P(self.vals), cap, P(self.head), P(self.dt), P(self.dv), P(self.ds),
                                        dcap, P(self.ghead), P(self.gsub), P(self.goff), gcap, P(self.err))
        assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
        if not self.vram_inputs:   # (device memory is never read back by the host)
            assert np.array_equal(self.blob[shift:shift + nb], blob[:nb]) and np.array_equal(self.offs[:n + 1], offs), \
                "the inputs changed"
        assert (self.doff[n_dests + 2:] == OFFC).all(), "offsets: canary"
        assert (self.err[n:] == ERRC).all(), "err: canary"
        for a, c in ((self.topic, cap), (self.vals, cap), (self.dt, dcap), (self.dv, dcap), (self.ds, dcap),
                     (self.gsub, gcap)):
            assert (a[c:] == CANARY).all(), "written past the capacity"
        assert (self.goff[gcap + 1:] == OFFC).all(), "written past out_goff[gcap]"
        return rc, self.doff[:n_dests + 2].copy(), self.topic[:cap + TAIL].copy(), self.vals[:cap + TAIL].copy(), \
            self.head.copy(), self.dt[:dcap + TAIL].copy(), self.dv[:dcap + TAIL].copy(), self.ds[:dcap + TAIL].copy(), \
            self.ghead.copy(), self.gsub[:gcap + TAIL].copy(), self.goff[:gcap + 1 + TAIL].copy(), self.err[:n].copy()


def _same(got, ref):
    for name, g, r in zip(NAMES, got, ref):
        if name == "rc":
            assert g == r, f"return code {g}, tm_deliver_batch's {r}"
        elif name == "goff":   # narrowed: the written part equal, the canary tails each whole
            k = min(int(ref[8][0]), len(r) - 1 - TAIL) + 1
            assert np.array_equal(g[:k].astype(np.uint64), r[:k]) and (r[:k] < 1 << 32).all(), name
            assert (g[k:] == OFFC).all() and (r[k:] == OFFC).all() and len(g) == len(r), "past out_goff[min(G, gcap)]"
        else:
            assert np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(r).astype(np.uint64)), name


def _check(ix, bufs, topics, n_dests, local, leg, flags=0, cap=None, dcap=None, gcap=None, shift=0, ref=None,
           definition=True):
    """one call against tm_deliver_batch and against the numpy definition over tm_dispatch_batch32's
    output; leg: ONE or GRID must rise by one, the other stay put.  -> (rc, total, T, G, W)"""
    cap = bufs.cap_max if cap is None else cap
    dcap = bufs.dcap_max if dcap is None else dcap
    gcap = bufs.gcap_max if gcap is None else gcap
    ref = ref or _reference(ix, topics, n_dests, local, flags, cap, dcap, gcap)
    exp = group_ref(*bufs.dispatch32(topics, n_dests, local, flags, cap, dcap), dcap, gcap) if definition else None
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
    got = bufs.call(topics, n_dests, local, flags, cap, dcap, gcap, shift)
    c1 = (ix.debug_get(ONE), ix.debug_get(GRID))
    _same(got, ref)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if leg == ONE else (0, 1)), "which leg finished the call"
    rc, doff, t, v, head, dt, dv, ds, ghead, gsub, goff = got[:11]
    total, T, G, W = int(doff[-1]), int(head[1]), int(ghead[0]), int(ghead[1])
    assert W == min(T, dcap) and G <= W
    assert (t[min(total, cap):] == CANARY).all() and (dt[W:] == CANARY).all() and (gsub[min(G, gcap):] == CANARY).all()
    assert rc == (ECAP if total > cap or T > dcap or G > gcap else OK)
    if exp is not None:
        (eG, eW), et, ev, es, _, egs, ego = exp
        assert (G, W) == (eG, eW), "the definition's [G, W]"
        assert np.array_equal(dt[:W], et) and np.array_equal(dv[:W], ev) and np.array_equal(ds[:W], es), "the definition"
        assert np.array_equal(gsub[:len(egs)], egs) and np.array_equal(goff[:len(ego)].astype(np.uint64), ego)
    return rc, total, T, G, W


# ---- 1. a synthetic index: the delivered subscriber ids are chosen word by word

S_DESTS = 3


class Synth:
    """'$p/+', '$q/+' and '$s/+' (values 0, 1, 3), all local: topics '$p/x', '$q/x', '$s/x' deliver list 0,
    list 1, list 3 ('#' does not match a '$' topic); '$r/+' (value 2) goes to destination 1"""

    def __init__(self):
        self.ix = _native.Index()
        _insert(self.ix, [b"$p/+", b"$q/+", b"$r/+", b"$s/+"], [0, 1, 2, 3], [0, 0, 1, 0])
        self.ix.set_subscribers([2], [[9, 8, 7]])
        self.b = Bufs(self.ix, FO1_TOPICS + 8, (FO1_TOPICS + 8) * 8, 256, 17_000, 17_000)

    def lists(self, ids):
        """the deliveries' subscriber ids are `ids`: three lists, the middle one the longest  -> the topics"""
        ids = np.asarray(ids, np.uint32)
        a = len(ids) // 5
        self.ix.set_subscribers([0, 1, 3], [ids[:a], ids[a:len(ids) - a], ids[len(ids) - a:]])
        return [b"$p/x", b"$q/x", b"$r/x", b"none", b"$s/x"]


@pytest.fixture(scope="module")
def synth(gpu):
    s = Synth()
    yield s
    s.b.free()
    s.ix.close()


def _random_ids(W, bound, seed):
    return np.random.default_rng(seed).integers(0, bound, W, dtype=np.uint64).astype(np.uint32)


def _digits_that_differ(ids):
    return sum(len(np.unique((ids >> (8 * p)) & 255)) > 1 for p in range(4)) if len(ids) else 0


def _check_ids(synth, ids, leg=ONE, **kw):
    """the deliveries' subscribers are ids: against both references, and the pass counters' deltas against
    the rule (a digit on which all W ids agree is skipped)"""
    ix, b = synth.ix, synth.b
    topics = synth.lists(ids)
    ref = _reference(ix, topics, S_DESTS, 0, 0, b.cap_max, kw.get("dcap", b.dcap_max), kw.get("gcap", b.gcap_max))
    p0 = (ix.debug_get(RUN), ix.debug_get(SKIPPED))
    rc, total, T, G, W = _check(ix, b, topics, S_DESTS, 0, leg, ref=ref, **kw)
    p1 = (ix.debug_get(RUN), ix.debug_get(SKIPPED))
    assert (total, T) == (4, len(ids))   # ('$r/x' routes elsewhere, 'none' nowhere)
    ids = np.asarray(ids, np.uint32)[:W]
    run = _digits_that_differ(ids)
    assert (p1[0] - p0[0], p1[1] - p0[1]) == (run, 4 - run), "digit passes run / skipped"
    assert G == len(np.unique(ids))
    return rc, G, W, run


@pytest.mark.parametrize("W", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, GS1_DELIVERIES - 1, GS1_DELIVERIES])
def test_sizes_in_place(synth, W):
    rc, G, w, run = _check_ids(synth, _random_ids(W, 1 << 16, W), ONE)
    assert rc == OK and w == W and (run == 2 or W < 65)


def test_one_more_than_the_compiled_bound_goes_to_the_grid(synth):
    rc, G, w, run = _check_ids(synth, _random_ids(GS1_DELIVERIES + 1, 1 << 16, 5), GRID)
    assert rc == OK and w == GS1_DELIVERIES + 1


def test_the_bound_lowered(synth):
    ix = synth.ix
    assert ix.debug_get(GS1_MAX) == GS1_DELIVERIES
    ix.debug_set(GS1_MAX, 1 << 40)
    assert ix.debug_get(GS1_MAX) == GS1_DELIVERIES, "clamped to the compiled bound"
    ix.debug_set(GS1_MAX, 64)
    try:
        assert ix.debug_get(GS1_MAX) == 64
        for W, leg in ((64, ONE), (65, GRID)):
            rc, G, w, run = _check_ids(synth, _random_ids(W, 1 << 32, W), leg)
            assert rc == OK and w == W
        # cut by dcap and gcap on the grid leg: both heads exact, nothing past either
        rc, G, w, run = _check_ids(synth, _random_ids(300, 1 << 32, 1), GRID, dcap=100, gcap=7)
        assert rc == ECAP and w == 100 and G > 7
    finally:
        ix.debug_set(GS1_MAX, GS1_DELIVERIES)


def test_the_smaller_of_the_two_bounds_wins(synth):
    ix = synth.ix
    ix.debug_set(DP1_MAX, 100)
    try:
        for W, leg in ((100, ONE), (101, GRID)):
            _check_ids(synth, _random_ids(W, 1 << 16, W), leg)
        ix.debug_set(GS1_MAX, 50)
        for W, leg in ((50, ONE), (51, GRID)):
            _check_ids(synth, _random_ids(W, 1 << 16, W), leg)
    finally:
        ix.debug_set(DP1_MAX, _native.DP1_DELIVERIES)
        ix.debug_set(GS1_MAX, GS1_DELIVERIES)


N_PAT = 3000   # three 64-position steps a wave


def _patterns():
    rng = np.random.default_rng(11)
    asc = np.arange(N_PAT, dtype=np.uint64)
    pats = {
        "all-equal": (np.full(N_PAT, 0x01020304), 0),
        "ascending": (asc * 3 + 70_000, None),       # (None: whatever the rule gives, checked in _check_ids)
        "descending": (asc[::-1] * 40_000, None),
        "two-alternating": (np.tile([0xAABBCCDD, 0x11223344], N_PAT // 2), 4),
        "zero-and-all-ones": (np.where(asc % 3 == 0, 0, 0xFFFFFFFF), 4),
        "one-id-holds-90-percent": (np.where(rng.random(N_PAT) < 0.9, 777_777,
                                             rng.integers(0, 1 << 32, N_PAT, dtype=np.uint64)), 4),
        "random-below-2^8": (_random_ids(N_PAT, 1 << 8, 1), 1),
        "random-below-2^16": (_random_ids(N_PAT, 1 << 16, 2), 2),
        "random-below-2^32": (_random_ids(N_PAT, 1 << 32, 3), 4),
    }
    for byte in range(4):   # ids that differ in one byte only
        base = 0x5A6B7C8D & ~(0xFF << (8 * byte))
        pats[f"byte-{byte}-only"] = (base | (rng.integers(0, 256, N_PAT) << (8 * byte)), 1)
    return pats


PATTERNS = _patterns()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_subscriber_id_patterns(synth, name):
    ids, passes = PATTERNS[name]
    rc, G, W, run = _check_ids(synth, ids, ONE)
    assert rc == OK and W == N_PAT
    if passes is not None:
        assert run == passes, "the table's passes for this pattern"
    if name == "all-equal":
        assert G == 1
    if name == "two-alternating":
        assert G == 2 and synth.b.goff[:3].tolist() == [0, N_PAT // 2, N_PAT]


def test_the_same_patterns_on_the_grid_leg(synth):
    """the grid ending with a few dozen deliveries: the same results and the same pass rule"""
    synth.ix.debug_set(GS1_MAX, 16)
    try:
        for seed, bound in ((1, 1 << 8), (2, 1 << 32)):
            rc, G, W, run = _check_ids(synth, _random_ids(90, bound, seed), GRID)
            assert rc == OK and W == 90
    finally:
        synth.ix.debug_set(GS1_MAX, GS1_DELIVERIES)


# ---- 2. stability: one subscriber on several filters

def test_a_subscriber_on_several_filters_keeps_the_dispatch_order(gpu):
    ix = _native.Index()
    _insert(ix, [b"a/#", b"a/+", b"+/b", b"x/#"], [0, 1, 2, 3], [0, 0, 0, 0])
    ix.set_subscribers([0, 1, 2, 3], [[9, 7, 3], [7, 1], [5, 7, 7], [2]])
    b = Bufs(ix, 16, 256, 16, 256, 256)
    topics = [b"a/b", b"a/c", b"x/b", b"a/b", b"none", b"a/b/c"]
    rc, total, T, G, W = _check(ix, b, topics, S_DESTS, 0, ONE)
    assert rc == OK and T == W
    h, xt, xv, xs = b.dispatch32(topics, S_DESTS, 0, 0, 256, 256)
    g = b.gsub[:G].tolist().index(7)
    lo, hi = int(b.goff[g]), int(b.goff[g + 1])
    mine = [(int(t), int(v)) for t, v, s in zip(xt, xv, xs) if s == 7]
    assert list(zip(b.dt[lo:hi].tolist(), b.dv[lo:hi].tolist())) == mine, "tm_dispatch_batch32's order inside the group"
    assert len(mine) >= 8 and len({t for t, _ in mine}) >= 4 and max(mine.count(x) for x in mine) == 2
    assert b.gsub[:G].tolist() == sorted(set(xs.tolist()))
    b.free()
    ix.close()


# ---- 3. a routed index: 300 keys over 4 destinations, aggre drops something, subscribers shared by filters

N_DESTS, LOCAL = 4, 1


def _routed_index():
    fs = ([f"a{x}/+/c{z}" for x in range(12) for z in range(5)] + [f"a{x}/#" for x in range(12)] +
          [f"+/b{y}/#" for y in range(9)] + [f"a{x}/b{y}/+" for y in range(9) for x in range(12)])[:240]
    fs = [f.encode() for f in fs]
    nf = len(fs)
    assert len(set(fs)) == nf
    dests = [None if v % 11 == 0 else (v // 4) % N_DESTS for v in range(nf)]
    twins = list(range(0, nf, 4))   # a second route with the same destination: aggre/1 keeps one of the two
    ix = _native.Index()
    _insert(ix, fs + [fs[v] for v in twins], list(range(nf)) + [nf + k for k in range(len(twins))],
            dests + [dests[v] for v in twins], list(range(nf)) + twins)
    assert nf + len(twins) <= 300
    vals = [v for v in range(nf + len(twins)) if v % 7]
    ix.set_subscribers(vals, [[(v * 5 + r * 3) % 61 + (r << 20) * (v % 2) for r in range(v % 5)] for v in vals])
    return ix


@pytest.fixture(scope="module")
def routed(gpu):
    ix = _routed_index()
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def bufs(routed):
    b = Bufs(routed, 1100, 1100 * 24, 256, 12_000, 12_000)
    yield b
    b.free()


def _topics(n, seed=1):
    rng = np.random.default_rng(seed)
    out = [f"a{rng.integers(0, 16)}/b{rng.integers(0, 9)}/c{rng.integers(0, 5)}".encode() for _ in range(n)]
    for i in range(0, n, 97):
        out[i] = (b"a1/+/c1", b"#", b"a/#/b")[i % 3]          # badarg
    for i in range(5, n, 89):
        out[i] = f"zzz{i}".encode()                          # no route at all
    return out


@pytest.mark.parametrize("flags", [0, AGGRE], ids=["plain", "aggre"])
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_routed_batches_equal_deliver_batch(routed, bufs, n, flags):
    rc, total, T, G, W = _check(routed, bufs, _topics(n, seed=n), N_DESTS, LOCAL, ONE, flags)
    assert rc == OK and (n < 65 or (total > n // 2 and T > n // 8 and 1 < G < T))


def test_capacities(routed, bufs):
    topics = _topics(600, seed=77)
    full = _reference(routed, topics, N_DESTS, LOCAL, 0, 12_000, 12_000, 12_000)
    total, T, G = int(full[1][-1]), int(full[4][1]), int(full[8][0])
    assert total > 300 and T > 200 and 10 < G < T
    for gcap in (0, G - 1, G, G + 1):
        rc, tot, t, g, w = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=total, dcap=T, gcap=gcap)
        assert (tot, t, g, w) == (total, T, G, T) and rc == (ECAP if G > gcap else OK)
        if rc == ECAP:   # the retry sized from the outputs is exact
            rc, tot, t, g2, w = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=total, dcap=T, gcap=g)
            assert rc == OK and g2 == g
    for dcap in (0, T - 1):   # the groups are those of the first dcap deliveries
        rc, tot, t, g, w = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=total, dcap=dcap, gcap=G)
        assert rc == ECAP and (tot, t, w) == (total, T, dcap) and g <= G and int(bufs.ghead[1]) == dcap
        rc, tot, t, g, w = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=total, dcap=t, gcap=G)
        assert rc == OK and (g, w) == (G, T)
    for flags in (0, AGGRE):
        ref = _reference(routed, topics, N_DESTS, LOCAL, flags, 12_000, 12_000, 12_000)
        need = int(_reference(routed, topics, N_DESTS, LOCAL, 0, 12_000, 12_000, 12_000)[1][-1])
        rc, tot, t, g, w = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, flags, cap=need - 1)
        assert rc == ECAP and tot == need, "the un-aggregated total sizes the retry"
        rc, tot, t, g, w = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, flags, cap=tot)
        assert rc == OK and tot == int(ref[1][-1])
    rc, tot, t, g, w = _check(routed, bufs, topics, N_DESTS, LOCAL, ONE, cap=0, dcap=0, gcap=0)
    assert rc == ECAP and (tot, t, g, w) == (total, T, 0, 0) and bufs.goff[0] == 0, "entry 0 whatever gcap is"


# ---- 4. eligibility

@pytest.mark.parametrize("which", ["ghead", "gsub", "goff"])
def test_a_plain_group_array_takes_the_staged_path(routed, which):
    b = Bufs(routed, 600, 600 * 24, 16, 8000, 8000, plain=(which,))
    try:
        rc, total, T, G, W = _check(routed, b, _topics(500, seed=3), N_DESTS, LOCAL, GRID)
        assert rc == OK and G > 10
        rc, total, T, G2, W = _check(routed, b, _topics(500, seed=3), N_DESTS, LOCAL, GRID, gcap=G - 1)
        assert rc == ECAP and G2 == G
    finally:
        b.free()


def test_too_many_topics_take_the_staged_path(synth):
    ix, b = synth.ix, synth.b
    synth.lists(_random_ids(30, 1 << 16, 9))
    topics = [b"$p/x", b"$q/x"] + [b"none"] * (FO1_TOPICS - 2)
    _check(ix, b, topics, S_DESTS, 0, ONE)
    rc, total, T, G, W = _check(ix, b, topics + [b"$s/x"], S_DESTS, 0, GRID)
    assert (rc, total, T) == (OK, 3, 30)


@pytest.mark.parametrize("n_dests,leg", [(255, ONE), (256, GRID)])
def test_destination_counts(routed, n_dests, leg):
    b = Bufs(routed, 600, 600 * 24, n_dests, 8000, 8000)
    try:
        rc, total, T, G, W = _check(routed, b, _topics(500, seed=n_dests), n_dests, LOCAL, leg)
        assert rc == OK and T > 100
    finally:
        b.free()


def test_more_entries_than_the_fan_out_workgroup_takes(gpu):
    """60 '#' keys under 300 topics: 18,000 entries, the FO1_TOO_LARGE ending and the grid grouping behind it"""
    ix = _native.Index()
    _insert(ix, [b"#"] * 60, np.arange(60), [v % 3 for v in range(60)])
    ix.set_subscribers(np.arange(0, 60, 6), [[v + 100, 7, v + 100] for v in range(0, 60, 6)])
    b = Bufs(ix, 320, 320 * 8, 16, 20_000, 10_000)
    rc, total, T, G, W = _check(ix, b, [b"t/%d" % i for i in range(300)], S_DESTS, 0, GRID)
    assert (rc, total, T, G) == (OK, 18_000, 300 * 10 * 3, 11)
    rc, total, T, G, W = _check(ix, b, [b"t/%d" % i for i in range(300)], S_DESTS, 0, GRID, dcap=1000, gcap=5)
    assert rc == ECAP and W == 1000
    b.free()
    ix.close()


def test_vram_inputs_run_in_place(routed):
    b = Bufs(routed, 600, 600 * 24, 16, 8000, 8000, vram_inputs=True)
    try:
        rc, total, T, G, W = _check(routed, b, _topics(500, seed=5), N_DESTS, LOCAL, ONE)
        assert rc == OK and T > 100
    finally:
        b.free()


def test_bad_arguments(routed, bufs):
    ix, b = routed, bufs
    offs = np.array([0, 3], np.uint32)
    blob = np.frombuffer(b"a/b" + b"\0" * 13, np.uint8)

    def call(n_dests=N_DESTS, local=LOCAL, flags=0, head=b.head, dt=b.dt, dcap=8, err=b.err, ghead=b.ghead, gsub=b.gsub,
             goff=b.goff, gcap=8):
        return ix._lib.tm_deliver_batch32(ix._h, 1, P(blob), P(offs), n_dests, local, flags, P(b.doff), P(b.topic),
                                          P(b.vals), 8, P(head), P(dt), P(b.dv), P(b.ds), dcap,
                                          None if ghead is None else ghead.ctypes.data, P(gsub), P(goff), gcap, P(err))
    assert call() == OK
    assert call(local=N_DESTS) == EINVAL and call(n_dests=0, local=0) == EINVAL and call(flags=2) == EINVAL
    assert call(head=None) == EINVAL and call(dt=None) == EINVAL and call(err=None) == EINVAL
    assert call(ghead=None) == EINVAL and call(goff=None) == EINVAL and call(gsub=None) == EINVAL
    assert call(gsub=None, gcap=0) == OK
    odd = np.zeros(5, np.uint64).view(np.uint32)[1:]
    assert call(ghead=odd) == EINVAL, "out_ghead must be 8-byte aligned"


# ---- 5. reruns

@pytest.mark.parametrize("routed_values", [280, 9], ids=["every-value-routed", "nine-values-routed"])
def test_a_value_scratch_that_grows_runs_the_batch_twice(gpu, routed_values):
    """a fresh index: its lane's first value scratch (65,536 words) is too small for 240 topics under 280
    '#' keys, so the first call's run is queued twice (two one-launch walks) and k_gs_one with it; the
    results are the reference's all the same.  A run that is queued again never groups in place: the first
    value scratch is at least 65,536 words, a total above it is more than FO1_ENTRIES entries -- a value
    without a destination is an entry too, of the unrouted bucket: the second case -- so both runs end in
    FO1_TOO_LARGE, k_gs_one writes GS1_SKIPPED twice, and the grid kernels finish the call."""
    ix = _native.Index()
    _insert(ix, [b"#"] * 280, np.arange(280), [v % 3 if v < routed_values else None for v in range(280)])
    ix.set_subscribers([0, 3, 6], [[5, 1], [1], [9, 5, 1]])
    b = Bufs(ix, 256, 256 * 8, 16, 70_000, 4000)
    topics = [b"t/%d" % i for i in range(240)]
    small = _native.TM_DEBUG_PATH_SMALL
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID), ix.debug_get(small))
    got = b.call(topics, S_DESTS, 0)                                  # the index's very first batch
    c1 = (ix.debug_get(ONE), ix.debug_get(GRID), ix.debug_get(small))
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, 1), "the grid kernels finished the call"
    assert c1[2] - c0[2] == 2, "grown and run again, once"
    assert int(got[1][-1]) == 240 * 280 > 65_536 and int(got[1][-1]) - int(got[1][-2]) == 240 * (280 - routed_values)
    _same(got, _reference(ix, topics, S_DESTS, 0, 0, 70_000, 4000, 4000))
    assert int(got[4][1]) == 240 * 6 and got[9][:3].tolist() == [1, 5, 9]
    c2 = (ix.debug_get(ONE), ix.debug_get(GRID), ix.debug_get(small))
    got = b.call(topics, S_DESTS, 0)                                  # the scratch is kept: one walk now
    assert (ix.debug_get(ONE), ix.debug_get(GRID), ix.debug_get(small)) == (c2[0], c2[1] + 1, c2[2] + 1)
    _same(got, _reference(ix, topics, S_DESTS, 0, 0, 70_000, 4000, 4000))
    b.free()
    ix.close()


def test_lookback_retry_gives_the_same_outputs(routed):
    """the look-back lives in the CSR walk of the staged leg (the in-place leg's pairs walk has none): a plain
    array takes the call there, the forced failure runs the batch again, once"""
    ix = routed
    topics = _topics(600, seed=21)
    b = Bufs(ix, 700, 700 * 24, 16, 8000, 8000, plain=("gsub",))
    try:
        ref = _reference(ix, topics, N_DESTS, LOCAL, 0, 8000, 8000, 8000)
        r0 = ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES)
        ix.debug_set(_native.TM_DEBUG_LB_FAIL_BLOCK, 3)
        ix.debug_set(_native.TM_DEBUG_LB_LAUNCHES, 1)            # the first launch fails, the retry succeeds
        g0 = ix.debug_get(GRID)
        got = b.call(topics, N_DESTS, LOCAL, 0, 8000, 8000, 8000)
        assert ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES) == r0 + 1, "the look-back hook made no batch retry"
        assert ix.debug_get(GRID) == g0 + 1
        _same(got, ref)
    finally:
        b.free()


# ---- 6. concurrent callers

def test_four_concurrent_callers(routed):
    failed0 = routed.debug_get(_native.TM_DEBUG_FAILED_BATCHES)
    batches = [_topics(400, seed=100 + k) for k in range(4)]
    refs = [_reference(routed, tp, N_DESTS, LOCAL, AGGRE if k % 2 else 0, 8000, 8000, 8000) for k, tp in enumerate(batches)]
    sets = [Bufs(routed, 400, 400 * 24, 16, 8000, 8000) for _ in range(4)]
    start, bad = threading.Barrier(4), []

    def caller(k):
        try:
            start.wait()
            for _ in range(50):
                _same(sets[k].call(batches[k], N_DESTS, LOCAL, AGGRE if k % 2 else 0), refs[k])
        except BaseException as e:   # noqa: BLE001
            bad.append((k, repr(e)))

    one0 = routed.debug_get(ONE)
    th = [threading.Thread(target=caller, args=(k,)) for k in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not bad
    assert routed.debug_get(ONE) - one0 == 200
    assert routed.debug_get(_native.TM_DEBUG_FAILED_BATCHES) == failed0
    for s in sets:
        s.free()


# ---- 7. the Python layers

def test_index_deliver_batch32_returns_views(routed, bufs):
    b, topics = bufs, _topics(300, seed=31)
    blob, offs = _native.pack_strings(topics)
    n, nb = len(topics), int(offs[-1])
    b.blob[:nb], b.offs[:n + 1] = blob[:nb], offs
    out = (b.doff, b.topic, b.vals, b.err, b.head, b.dt, b.dv, b.ds, b.ghead, b.gsub, b.goff)
    (edoff, et, ev, eerr), (edt, edv, eds), (egs, ego) = routed.deliver_batch(blob, offs, N_DESTS, LOCAL, aggre=True)
    one0 = routed.debug_get(ONE)
    (doff, t, v, err), (dt, dv, ds), (gs, go) = routed.deliver_batch32(b.blob, b.offs[:n + 1], N_DESTS, LOCAL, out, aggre=True)
    assert routed.debug_get(ONE) == one0 + 1
    assert np.array_equal(doff, edoff) and np.array_equal(t, et) and np.array_equal(v, ev) and np.array_equal(err, eerr)
    assert np.array_equal(dt, edt) and np.array_equal(dv, edv) and np.array_equal(ds, eds) and len(ds) > 50
    assert np.array_equal(gs, egs) and np.array_equal(go, ego) and go.dtype == np.uint32
    assert np.shares_memory(ds, b.ds) and np.shares_memory(go, b.goff)
    with pytest.raises(_native.TmError) as e:
        routed.deliver_batch32(b.blob, b.offs[:n + 1], N_DESTS, LOCAL, out, gcap=len(gs) - 1, aggre=True)
    assert e.value.code == ECAP and int(b.ghead[0]) == len(gs)


NODES = ("n1", "n2")


def _router(in_place):
    rng = np.random.default_rng(77)
    subs = LocalSubs()
    r = Router(node="n1", local_subs=subs, route_in_place=in_place)
    dests = list(NODES) + [(g, n) for g in (b"g1", b"g2") for n in ("n1", "n2", "n3")]
    filters = ([f"a{x}/+/c{z}" for x in range(12) for z in range(5)] + [f"a{x}/#" for x in range(12)] +
               [f"+/b{y}/#" for y in range(9)] + [f"a{x}/b{y}/+" for y in range(9) for x in range(12)])[:180]
    filters = sorted(f.encode() for f in filters)
    for k, f in enumerate(filters[::2]):              # one pid on several filters
        for j in range(k % 4):
            subs.subscribe(f, ("pid", (k * 7 + j) % 40))
    batch = {}
    for i, f in enumerate(filters):
        batch[(f, "n1" if i % 3 else "n2")] = ("add", 0, None)
        for d in rng.choice(len(dests), 1 + i % 3, replace=False):
            batch[(f, dests[d])] = ("add", 0, None)
    for k in range(60):                               # exact topics: the bag, some rows local
        t = f"a{k % 16}/b{k % 9}/c{k % 5}".encode()
        batch[(t, "n1" if k % 2 else "n2")] = ("add", 0, None)
        if k % 4 == 1:
            subs.subscribe(t, ("exact", k))
    assert r.do_batch(batch) == {}
    return r


@pytest.fixture(scope="module")
def routers(gpu):
    return _router(False), _router(True)


def test_router_in_place_equals_the_default_router(routers):
    plain, inplace = routers
    ix = inplace._mirror._index
    topics = _topics(700, seed=8)
    for aggre in (False, True):
        e_by, e_del, e_groups = plain.match_routes_deliver(topics, errors="return", aggre=aggre)
        c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
        by, got, groups = inplace.match_routes_deliver(topics, errors="return", aggre=aggre)
        # (a TM_ECAP rerun on the pooled buffers is one more call on the same leg)
        assert ix.debug_get(ONE) > c0[0] and ix.debug_get(GRID) == c0[1], "tm_deliver_batch32 served the call, in place"
        assert dict(by) == dict(e_by) and set(by.errors) == set(e_by.errors)
        assert got == e_del and len(got) > 500
        assert groups == e_groups and list(groups) == list(e_groups) and len(groups) > 10
        assert any(p[0] == "exact" for p in groups), "a bag row's subscriber"
        assert any(len({to for _, to in items}) > 1 for items in groups.values()), "one pid on several filters"


def test_broker_over_the_in_place_router_delivers_once_per_subscriber(routers):
    plain, r = routers
    msgs = [Message(t, i) for i, t in enumerate(_topics(500, seed=9))]

    def run(router):
        calls = []
        Broker(router, forward=lambda n, to, m: "ok", share_dispatch=lambda g, to, m: 1, deliver_grouped=True,
               deliver_batch=lambda p, items: calls.append((p, [(to, m.payload) for to, m in items]))
               ).publish_batch_by_dest(msgs)
        return calls
    exp = run(plain)
    ix = r._mirror._index
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
    got = run(r)
    assert ix.debug_get(ONE) > c0[0] and ix.debug_get(GRID) == c0[1], "the in-place leg served the broker"
    assert len({p for p, _ in got}) == len(got) > 10, "deliver_batch once per subscriber"
    assert got == exp
