"""tm_publish_batch32: the 32-bit, in-place route + local dispatch + shared-
subscription pick call for a NIF's micro-batches.

The reference everywhere is the unchanged tm_publish_batch on the same index:
before each of the two calls the start state of every slot the case uses is
written with tm_share_state_set, after each it is read back with
tm_share_state_get.  The return code, the bucket offsets, the head, every
output array -- filled with a canary first and compared WHOLE, tail included
-- and the state words afterwards must be identical; the reference's own
picks and state are checked against the numpy definition
(shared_sub.pick_batch_ref) on its route outputs.  The inputs are compared
after the run, and TM_DEBUG_PUBLISH_ONE / TM_DEBUG_PUBLISH_GRID say which leg
picked: the one-launch kernel (k_sh_one), or the grid pick / the staged path.

The index: '$a<i>/+' and '$a<i>/#' (two entries for the topic '$a<i>/x'),
'$b<i>/+' (one entry) and three filters for '$c/y', every filter its own
value and its own filter id (aggre/1 keeps everything), so a batch of distinct
topics has K = 2 a + b + 3 c kept entries with K distinct values: each case
reads the entry order off a route call and gives every ENTRY the slot its
layout wants (tm_set_share_slots per value).  A slot's record (strategy byte,
sticky's init strategy, count, n_local) and start state follow from its rank
among the case's slots, cycling through every combination.

k_sh_one gives each of its 16 waves ceil(K / 16) entries rounded up to 64: K =
1024 fills every wave's first step exactly, 1025 takes a second.  Its sort
runs one 8-bit digit pass per byte of the largest ranked slot present: slots
below 200, 60,000 and 2^20 + 1 need one, two and three.

Not reachable through this call: a record whose span lies outside the pool
(tm_set_share_members only writes spans inside it; tm_share_pick_dev's tests
cover the rule on raw tables, and k_sh_one reads records through the same
sh_record).  The pairs walk of the in-place leg has no look-back, so the
forced look-back failure is driven through the staged leg of the call.
"""
import threading
from collections import Counter

import numpy as np
import pytest

from emqx_amd import _native, shared_sub
from emqx_amd.shared_sub import NONE, UNDEF, pick_batch_ref

pytestmark = pytest.mark.gpu

FO1_TOPICS, FO1_ENTRIES = 8192, 16384   # emqx_amd/csrc/tm_dev.h
CANARY, OFFC, ERRC, HEADC, TAIL = 0xC0FFEE22, 0xDEADBEEF, 0xEE, 0xABCDEF0123456789, 64
ONE, GRID = _native.TM_DEBUG_PUBLISH_ONE, _native.TM_DEBUG_PUBLISH_GRID
D_ONE, D_GRID = _native.TM_DEBUG_DISPATCH_ONE, _native.TM_DEBUG_DISPATCH_GRID
AGGRE = _native.TM_ROUTE_AGGRE
OK, ECAP, EINVAL = _native.TM_OK, _native.TM_ECAP, _native.TM_EINVAL
P = _native._ptr
V = 8192
NV = 3 * V + 3
N_DESTS, LOCAL, SEED = 3, 0, 0x5EED
CAP, DCAP = 17_000, 40_000
RR, PG, STICKY = shared_sub.ROUND_ROBIN, shared_sub.ROUND_ROBIN_PER_GROUP, shared_sub.STICKY
# every strategy byte, two unknown ones, sticky with each init strategy (and an unknown one: as random)
METAS = (0, 1, 2, 3, 3 | 4 << 8, 3 | 5 << 8, 3 | 6 << 8, 3 | 9 << 8, 4, 5, 6, 7, 200)
CNTS = (2, 3, 1, 0, 1000)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


class World:
    def __init__(self):
        self.ix = ix = _native.Index()
        fs = [b"$a%d/+" % i for i in range(V)] + [b"$a%d/#" % i for i in range(V)] + [b"$b%d/+" % i for i in range(V)]
        fs += [b"$c/+", b"$c/#", b"$c/y"]
        vals = np.arange(NV, dtype=np.uint32)
        dest = np.where(vals % 13 == 5, 1, 0).astype(np.uint32)
        routed = vals % 17 != 3                                   # the others land in the unrouted bucket
        ix.set_dests(vals[routed], dest[routed])
        ix.set_route_filters(vals, vals)
        blob, offs = _native.pack_strings(fs)
        ix.apply(np.ones(NV, np.uint8), blob, offs, vals)
        subs = [int(v) for v in vals if v % 5 == 0 or v % 7 == 0]
        ix.set_subscribers(subs, [[v * 4 + r for r in range(1 + v % 3)] for v in subs])

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.ix.close()


@pytest.fixture(scope="module")
def world(gpu):
    w = World()
    yield w
    w.close()


def _topics(K, z=0, seed=0):
    """distinct topics with exactly K entries (and z topics nothing matches), shuffled"""
    c = 1 if K > FO1_ENTRIES else 0
    a = min((K - 3 * c) // 2, V - c)
    b = K - 3 * c - 2 * a
    assert 0 <= b <= V
    t = [b"$a%d/x" % i for i in range(a)] + [b"$b%d/x" % i for i in range(b)] + [b"$c/y"] * c
    t += [b"$none%d/z" % i for i in range(z)]
    rng = np.random.default_rng(K + seed)
    return [t[i] for i in rng.permutation(len(t))]


# ---- layouts: entry q of K -> slot (NONE: no slot), slots below n_slots with the highest one present

def lay_one(q, n_slots):
    return np.full(len(q), n_slots - 1)


def lay_own(q, n_slots):
    return n_slots - 1 - q


def lay_alt2(q, n_slots):
    return (q % 2) * (n_slots - 1)


def lay_runs7(q, n_slots):
    i = (q // 5) % 7
    return np.where(i == 6, n_slots - 1, i * ((n_slots - 1) // 6))


def lay_gaps(q, n_slots):
    return np.where(q % 3 == 1, NONE, lay_runs7(q, n_slots))


def lay_spread(q, n_slots):
    s = np.random.default_rng(n_slots).integers(0, n_slots, len(q))
    s[:64] = n_slots - 1                                        # the highest slot, ranked 0 .. 63
    s[100:4000:3] = n_slots - 2
    return s


LAYOUTS = {"one": lay_one, "own": lay_own, "alt2": lay_alt2, "runs7": lay_runs7, "gaps": lay_gaps, "spread": lay_spread}


class Tables:
    """the records and start states of the slots a case uses, on the device and as the definition's arrays"""

    def __init__(self, ix, used, jbase=0, top_ranked=True, big=True):
        self.ix, self.used = ix, np.asarray(used, np.uint32)
        n = len(used)
        j = np.arange(n) + jbase
        meta = np.asarray(METAS, np.int64)[j % len(METAS)]
        cnt = np.asarray(CNTS, np.int64)[(j // len(METAS)) % len(CNTS)]
        cnt = np.where((cnt == 1000) & ((j % 7 != 0) | (not big)), 5, cnt)
        if top_ranked and n:                                     # the sort's passes follow the highest RANKED slot
            meta[-1], cnt[-1] = RR, 3
        nl = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 2), cnt + 1])[(j // 3) % 4, np.arange(n)]
        starts = np.stack([np.full(n, UNDEF), np.zeros(n, np.int64), np.maximum(cnt - 1, 0), cnt, cnt + 5,
                           np.full(n, 0xFFFFFFFE)])
        self.start = starts[(j // (len(METAS) * len(CNTS))) % 6, np.arange(n)].astype(np.uint32)
        self.set(self.used, [((int(s) * 2048 + np.arange(c)) & 0x7FFFFFFF).astype(np.uint32) for s, c in zip(used, cnt)],
                 nl, meta, fresh=True)

    def set(self, slots, lists, nl, meta, fresh=False):
        slots = np.asarray(slots, np.uint32)
        if len(slots):
            self.ix.set_share_members(slots, lists, np.asarray(nl, np.uint32), np.asarray(meta, np.uint32))
        if fresh:
            self.lists, self.nl, self.meta = {}, {}, {}
        for s, x, k, m in zip(slots.tolist(), lists, nl, meta):
            self.lists[s], self.nl[s], self.meta[s] = np.asarray(x, np.uint32), int(k), int(m)

    def arrays(self, state):
        """-> (rec, pool, state) dense up to the highest used slot, for pick_batch_ref"""
        n = int(self.used.max()) + 1 if len(self.used) else 0
        rec, pool, pos = np.zeros((n, 4), np.uint32), [], 0
        for s in self.used.tolist():
            rec[s] = (pos, len(self.lists[s]), self.nl[s], self.meta[s])
            pool.append(self.lists[s])
            pos += len(self.lists[s])
        st = np.full(n, UNDEF, np.uint32)
        st[self.used] = state
        return rec.reshape(-1), np.concatenate(pool) if pool else np.zeros(0, np.uint32), st

    def reset(self, state=None):
        if len(self.used):
            self.ix.share_state_set(self.used, self.start if state is None else state)

    def state(self):
        return self.ix.share_state_get(self.used)


def _place(w, topics, layout, n_slots, **kw):
    """gives every entry of the batch its slot -> (Tables, K); the entry order is read off a route call"""
    blob, offs = _native.pack_strings(topics)
    doff, t, v, err = w.ix.route_batch(blob, offs, N_DESTS, cap=1 << 17, aggre=True)
    K = int(doff[-1])
    assert len(np.unique(v)) == K, "the case wants every entry its own value"
    slots = np.asarray(LAYOUTS[layout](np.arange(K), n_slots), np.int64)
    slot_of = np.full(NV, NONE, np.uint32)
    slot_of[v] = slots.astype(np.uint32)
    w.ix.set_share_slots(np.arange(NV, dtype=np.uint32), slot_of)
    w.slot_of = slot_of
    used = np.unique(slots[slots != NONE])
    assert not len(used) or (used[-1] <= n_slots - 1 and used[0] >= 0)
    return Tables(w.ix, used, **kw), K


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, max(n, 1), dtype=np.uint32), rng.integers(0, 1 << 32, max(n, 1), dtype=np.uint32)


def _reference(ix, topics, n_dests, local, cap, dcap, kc, kt, seed=SEED):
    """tm_publish_batch -> (rc, doff u64, topic, values, member, head, dtopic, dvalue, dsub, err), the arrays whole"""
    blob, offs = _native.pack_strings(topics)
    n = len(topics)
    doff, head = np.zeros(n_dests + 2, np.uint64), np.full(2, HEADC, np.uint64)
    t, v, m = (np.full(cap + TAIL, CANARY, np.uint32) for _ in range(3))
    dt, dv, ds = (np.full(dcap + TAIL, CANARY, np.uint32) for _ in range(3))
    err = np.zeros(max(n, 1), np.uint8)
    rc = ix._lib.tm_publish_batch(ix._h, n, P(blob), P(offs), n_dests, local, AGGRE, P(doff), P(t), P(v), cap, P(head),
                                  P(dt), P(dv), P(ds), dcap, P(kc), P(kt), seed, P(m), P(err))
    assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
    return rc, doff, t, v, m, head, dt, dv, ds, err[:n]


class Bufs:
    """one caller's batch buffers: host_array (pinned; the keys optionally TM_ALLOC_VRAM), those in `plain` numpy"""

    def __init__(self, ix, nmax, bytes_max, dmax, cap_max, dcap_max, plain=(), vram_keys=False):
        def alloc(name, k, dt, vram=False):
            if name in plain:
                return np.zeros(max(k, 1), dt)
            a = ix.host_array(k, dt, vram=vram)
            self.owned.append(a)
            return a
        self.ix, self.cap_max, self.dcap_max, self.owned, self.vram_keys = ix, cap_max, dcap_max, [], vram_keys
        self.blob, self.offs = alloc("blob", bytes_max + 48, np.uint8), alloc("offs", nmax + 1, np.uint32)
        self.doff, self.err = alloc("doff", dmax + 2 + TAIL, np.uint32), alloc("err", nmax + TAIL, np.uint8)
        self.topic, self.vals, self.member = (alloc(k, cap_max + TAIL, np.uint32) for k in ("topic", "vals", "member"))
        self.head = alloc("head", 2, np.uint64)
        self.dt, self.dv, self.ds = (alloc(k, dcap_max + TAIL, np.uint32) for k in ("dt", "dv", "ds"))
        self.kc, self.kt = (alloc(k, nmax + 1, np.uint32, vram_keys) for k in ("kc", "kt"))

    def free(self):
        for a in self.owned:
            self.ix.host_free(a)

    def call(self, topics, n_dests, local, cap, dcap, kc, kt, seed=SEED, shift=0, flags=AGGRE, ok=(OK, ECAP)):
        """tm_publish_batch32 -> what _reference returns (doff as u32), arrays whole up to cap / dcap + TAIL"""
        blob, offs = _native.pack_strings(topics)
        n, nb = len(topics), int(offs[-1])
        assert cap <= self.cap_max and dcap <= self.dcap_max and n + 1 <= len(self.offs) and nb + shift <= len(self.blob)
        self.blob[shift:shift + nb] = blob[:nb]
        self.offs[:n + 1] = offs
        self.doff[:], self.topic[:], self.vals[:], self.member[:], self.err[:] = OFFC, CANARY, CANARY, CANARY, ERRC
        self.dt[:], self.dv[:], self.ds[:], self.head[:] = CANARY, CANARY, CANARY, HEADC
        keys = []
        for mine, k in ((self.kc, kc), (self.kt, kt)):
            if k is not None:
                mine[:n] = k[:n]
            keys.append(None if k is None else mine)
        ix = self.ix
        rc = ix._lib.tm_publish_batch32(ix._h, n, P(self.blob[shift:]), P(self.offs), n_dests, local, flags, P(self.doff),
                                        P(self.topic), P(self.vals), cap, P(self.head), P(self.dt), P(self.dv), P(self.ds),
                                        dcap, P(keys[0]), P(keys[1]), seed, P(self.member), P(self.err))
        assert rc in ok, ix._lib.tm_last_error(ix._h)
        assert np.array_equal(self.blob[shift:shift + nb], blob[:nb]) and np.array_equal(self.offs[:n + 1], offs), \
            "the inputs changed"
        if not self.vram_keys:   # (device memory is never read back by the host)
            assert all(k is None or np.array_equal(mine[:n], k[:n]) for mine, k in ((self.kc, kc), (self.kt, kt)))
        if rc in (OK, ECAP):
            assert (self.doff[n_dests + 2:] == OFFC).all(), "offsets: canary"
            assert (self.err[n:] == ERRC).all(), "err: canary"
        c = lambda a, k: a[:k + TAIL].copy()
        return rc, self.doff[:n_dests + 2].copy(), c(self.topic, cap), c(self.vals, cap), c(self.member, cap), \
            self.head.copy(), c(self.dt, dcap), c(self.dv, dcap), c(self.ds, dcap), self.err[:n].copy()


NAMES = ("rc", "bucket offsets", "topic", "values", "member", "head", "dtopic", "dvalue", "dsub", "err")


def _same(got, ref):
    for name, g, r in zip(NAMES, got, ref):
        if name == "rc":
            assert g == r, f"return code {g}, tm_publish_batch's {r}"
        else:
            assert np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(r).astype(np.uint64)), name


@pytest.fixture(scope="module")
def bufs(world):
    b = Bufs(world.ix, FO1_TOPICS + 8, (FO1_TOPICS + 8) * 12, 256, CAP, DCAP)
    yield b
    b.free()


def _check(w, b, topics, tab, leg, cap=CAP, dcap=DCAP, keys="both", seed=SEED, shift=0, n_dests=N_DESTS, start=None):
    """the reference from the start state, then the call under test from the same start state; every output,
    the state afterwards and the leg's counter.  leg: ONE, GRID or None (no pick at all).
    -> (rc, K, member, state after)"""
    ix, n = w.ix, len(topics)
    kc, kt = _keys(n, seed)
    kc, kt = (kc if keys in ("both", "clientid") else None), (kt if keys in ("both", "topic") else None)
    tab.reset(start)
    ref = _reference(ix, topics, n_dests, LOCAL, cap, dcap, kc, kt, seed)
    ref_state = tab.state()
    rc, doff, t, v, m = ref[:5]
    total = int(doff[-1])
    K = total if total <= cap else 0
    # the reference against the definition
    rec, pool, st0 = tab.arrays(tab.start if start is None else start)
    if total <= cap:
        want, head, after = pick_batch_ref(n_dests, doff, t[:K], v[:K], K, w.slot_of, rec, pool, st0, kc, kt, n, seed)
        assert np.array_equal(m[:K], want), "tm_publish_batch differs from the definition"
        assert np.array_equal(ref_state, after[tab.used]) if len(tab.used) else True
    assert (m[K:] == CANARY).all()
    tab.reset(start)
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
    got = b.call(topics, n_dests, LOCAL, cap, dcap, kc, kt, seed, shift)
    c1 = (ix.debug_get(ONE), ix.debug_get(GRID))
    _same(got, ref)
    assert np.array_equal(tab.state(), ref_state), "the state words afterwards"
    assert (c1[0] - c0[0], c1[1] - c0[1]) == {ONE: (1, 0), GRID: (0, 1), None: (0, 0)}[leg], "which leg picked"
    return rc, K, got[4][:K], ref_state


# ---- 1. sizes

@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 1023, 1024, 1025, FO1_ENTRIES, FO1_ENTRIES + 1])
def test_entry_counts(world, bufs, K):
    """one step of the 16 waves and one more; FO1_ENTRIES + 1: the grid fan-out, dispatch and pick"""
    topics = _topics(K, z=5 if K < 1000 else 0)
    tab, k = _place(world, topics, "gaps", 60_000)
    assert k == K and len(topics) <= FO1_TOPICS
    rc, k, member, _ = _check(world, bufs, topics, tab, ONE if K <= FO1_ENTRIES else GRID)
    assert rc == OK and k == K
    if K >= 63:
        assert (member == NONE).sum() >= K // 3 and (member != NONE).sum() > K // 4


@pytest.mark.parametrize("n,leg", [(0, ONE), (1, ONE), (64, ONE), (FO1_TOPICS, ONE), (FO1_TOPICS + 1, GRID)])
def test_topic_counts(world, bufs, n, leg):
    """FO1_TOPICS + 1 topics are staged: widened, tm_publish_batch, narrowed"""
    topics = [b"$b%d/x" % i for i in range(min(n, V))] + [b"$a%d/x" % i for i in range(n - min(n, V))]
    tab, K = _place(world, topics, "runs7", 200)
    assert K == n + max(n - V, 0)
    rc, k, member, _ = _check(world, bufs, topics, tab, leg)
    assert rc == OK and k == K


# ---- 2. slot layouts and the sort's passes

@pytest.mark.parametrize("jbase", [1, 2, 3, 0], ids=["round_robin", "per_group", "sticky", "random"])
@pytest.mark.parametrize("K", [1025, FO1_ENTRIES])
def test_every_entry_in_one_slot(world, bufs, K, jbase):
    topics = _topics(K)
    tab, _ = _place(world, topics, "one", 200, jbase=jbase, top_ranked=False)
    for start in (None, np.array([1], np.uint32)):
        rc, k, member, after = _check(world, bufs, topics, tab, ONE, start=start)
        assert rc == OK and k == K and (member != NONE).all()
        if jbase in (1, 2):                                      # cnt = 2: the members alternate in entry order
            assert (member[::2] == member[0]).all() and (member[1::2] == member[1]).all() and member[0] != member[1]
        if jbase == 3:
            assert (member == member[0]).all()


@pytest.mark.parametrize("layout,K,n_slots", [("own", 1025, 1025), ("own", FO1_ENTRIES, FO1_ENTRIES), ("alt2", 1025, 200),
                                              ("alt2", FO1_ENTRIES, 70_000), ("runs7", 1024, 200),
                                              ("runs7", FO1_ENTRIES, 60_000), ("gaps", 1025, 7), ("gaps", 4097, 200)])
def test_slot_layouts(world, bufs, layout, K, n_slots):
    topics = _topics(K)
    tab, _ = _place(world, topics, layout, n_slots)
    rc, k, member, _ = _check(world, bufs, topics, tab, ONE)
    assert rc == OK and k == K


@pytest.mark.parametrize("n_slots", [200, 60_000, (1 << 20) + 1])
@pytest.mark.parametrize("K", [1025, 9000])
def test_slot_ids_needing_one_two_and_three_digit_passes(world, bufs, K, n_slots):
    topics = _topics(K)
    tab, _ = _place(world, topics, "spread", n_slots, big=False)
    assert tab.meta[n_slots - 1] == RR and tab.meta[n_slots - 2] in METAS
    rc, k, member, _ = _check(world, bufs, topics, tab, ONE)
    assert rc == OK and k == K


# ---- 3. strategies, records, start states, keys

@pytest.fixture(scope="module")
def records(world):
    """every meta x count x start state (n_local rotating), five entries a slot"""
    n_slots = len(METAS) * len(CNTS) * 6
    topics = _topics(5 * n_slots)
    w = world
    blob, offs = _native.pack_strings(topics)
    v = w.ix.route_batch(blob, offs, N_DESTS, cap=1 << 17, aggre=True)[2]
    return topics, v, n_slots


def _place_records(w, records):
    topics, v, n_slots = records
    slot_of = np.full(NV, NONE, np.uint32)
    slot_of[v] = np.random.default_rng(4).permutation(np.arange(len(v)) % n_slots)
    w.ix.set_share_slots(np.arange(NV, dtype=np.uint32), slot_of)
    w.slot_of = slot_of
    tab = Tables(w.ix, np.arange(n_slots), top_ranked=False)
    cnts = Counter(len(x) for x in tab.lists.values())
    assert set(cnts) == {0, 1, 2, 3, 5, 1000} and set(tab.meta.values()) == set(METAS)
    assert {UNDEF, 0, 1, 2, 3, 7, 8, 0xFFFFFFFE} <= set(tab.start.tolist())
    assert any(tab.nl[s] > len(tab.lists[s]) for s in tab.lists) and {0, 1, 2} <= set(tab.nl.values())
    return topics, tab


@pytest.mark.parametrize("keys", ["both", "none", "clientid", "topic"])
def test_strategies_counts_start_states_and_null_keys(world, bufs, records, keys):
    topics, tab = _place_records(world, records)
    rc, K, member, after = _check(world, bufs, topics, tab, ONE, keys=keys)
    assert rc == OK and K == len(records[1]) == 5 * len(tab.used)
    moved = after != tab.start
    assert moved.sum() > 100 and (~moved).sum() > 100


def test_key_arrays_in_vram(world, records):
    topics, tab = _place_records(world, records)
    b = Bufs(world.ix, len(topics) + 8, len(topics) * 12, 16, CAP, DCAP, vram_keys=True)
    try:
        rc, K, _, _ = _check(world, b, topics, tab, ONE)
        assert rc == OK
    finally:
        b.free()


# ---- 4. the gate

def test_ecap_from_cap_picks_nothing_and_the_resubmitted_call_equals_the_reference(world, bufs):
    topics = _topics(3000)
    tab, K = _place(world, topics, "runs7", 200)
    rc, k, _, after = _check(world, bufs, topics, tab, None, cap=K // 2)
    assert rc == ECAP and k == 0 and np.array_equal(after, tab.start)
    assert (bufs.member == CANARY).all() and int(bufs.doff[N_DESTS + 1]) == K
    rc, k, _, after = _check(world, bufs, topics, tab, ONE, cap=K)
    assert rc == OK and k == K and not np.array_equal(after, tab.start)


def test_ecap_from_dcap_alone_the_picks_and_the_state_stand(world, bufs):
    topics = _topics(3000)
    tab, K = _place(world, topics, "runs7", 200)
    T = int(_reference(world.ix, topics, N_DESTS, LOCAL, CAP, DCAP, None, None)[5][1])
    assert T > 100
    rc, k, member, after = _check(world, bufs, topics, tab, ONE, dcap=T // 2)
    assert rc == ECAP and k == K and int(bufs.head[1]) == T
    assert (member != NONE).any() and not np.array_equal(after, tab.start)


def test_lookback_retry_moves_the_state_once(world):
    """the look-back lives in the CSR walk of the staged leg (the in-place leg's pairs walk has none): plain
    buffers take it there, the forced failure runs the batch again, and the state still moves once"""
    ix = world.ix
    topics = _topics(600)
    tab, K = _place(world, topics, "runs7", 200)
    b = Bufs(ix, 700, 700 * 12, 16, CAP, DCAP, plain=("member",))
    try:
        r0 = ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES)
        kc, kt = _keys(len(topics), 7)
        tab.reset()
        ref = _reference(ix, topics, N_DESTS, LOCAL, CAP, DCAP, kc, kt)
        ref_state = tab.state()
        tab.reset()
        ix.debug_set(_native.TM_DEBUG_LB_FAIL_BLOCK, 3)
        ix.debug_set(_native.TM_DEBUG_LB_LAUNCHES, 1)            # the first launch fails, the retry succeeds
        g0 = ix.debug_get(GRID)
        got = b.call(topics, N_DESTS, LOCAL, CAP, DCAP, kc, kt)
        assert ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES) == r0 + 1, "the look-back hook made no batch retry"
        assert ix.debug_get(GRID) == g0 + 1
        _same(got, ref)
        assert np.array_equal(tab.state(), ref_state) and not np.array_equal(ref_state, tab.start)
    finally:
        b.free()


def test_a_value_scratch_that_grows_moves_the_state_once(gpu):
    """a fresh index: its lane's first value scratch (65536 words) is too small for 7,000 topics under ten
    '#' filters, so the batch runs twice; both runs have too many entries for the one-launch kernels, the
    gate keeps k_sh_one out of both, and the grid pick runs once"""
    ix = _native.Index()
    try:
        vals = np.arange(10, dtype=np.uint32)
        ix.set_dests(vals, vals % 2)
        ix.set_route_filters(vals, vals)
        blob, offs = _native.pack_strings([b"#"] * 10)
        ix.apply(np.ones(10, np.uint8), blob, offs, vals)
        ix.set_subscribers([0, 3], [[1, 2], [3]])
        ix.set_share_slots(vals, vals % 4)
        ix.set_share_members([0, 1, 2, 3], [[10, 11, 12], [20, 21], [30, 31, 32, 33, 34], [40]], [0, 0, 0, 0],
                             [RR, PG, STICKY | 5 << 8, RR])
        n, cap, dcap = 7000, 80_000, 40_000
        topics = [b"t/%d" % i for i in range(n)]
        kc, kt = _keys(n, 9)
        b = Bufs(ix, n + 8, n * 8, 16, cap, dcap)
        keys = (_native.TM_DEBUG_PATH_PHASES, _native.TM_DEBUG_PATH_SMALL)
        p0, g0, o0 = sum(ix.debug_get(k) for k in keys), ix.debug_get(GRID), ix.debug_get(ONE)
        got = b.call(topics, 2, 0, cap, dcap, kc, kt)           # FIRST on this index: the scratch is still small
        assert sum(ix.debug_get(k) for k in keys) == p0 + 2, "the batch did not run twice"
        assert (ix.debug_get(GRID), ix.debug_get(ONE)) == (g0 + 1, o0)
        state = ix.share_state_get([0, 1, 2, 3])
        ix.share_state_set([0, 1, 2, 3], [UNDEF] * 4)
        ref = _reference(ix, topics, 2, 0, cap, dcap, kc, kt)
        _same(got, ref)
        assert got[0] == OK and int(got[1][-1]) == 10 * n
        assert np.array_equal(ix.share_state_get([0, 1, 2, 3]), state) and state[1] != UNDEF
        b.free()
    finally:
        import torch
        torch.cuda.synchronize()
        ix.close()


def test_dp1_too_large_picks_from_the_one_launch_kernel_deliveries_from_the_grid(world, bufs):
    ix = world.ix
    topics = _topics(2000)
    tab, K = _place(world, topics, "runs7", 200)
    ix.debug_set(_native.TM_DEBUG_DP1_MAX, 10)
    try:
        d0 = (ix.debug_get(D_ONE), ix.debug_get(D_GRID))
        rc, k, member, _ = _check(world, bufs, topics, tab, ONE)
        assert rc == OK and k == K and int(bufs.head[1]) > 10
        assert (ix.debug_get(D_ONE), ix.debug_get(D_GRID)) == (d0[0], d0[1] + 1), "the grid kernels wrote the deliveries"
    finally:
        ix.debug_set(_native.TM_DEBUG_DP1_MAX, _native.DP1_DELIVERIES)


# ---- 5. fallbacks: the staged path, identical results

@pytest.mark.parametrize("plain", ["member", "kc", "kt"])
def test_a_plain_numpy_buffer_takes_the_staged_path(world, plain):
    topics = _topics(1025)
    tab, K = _place(world, topics, "runs7", 200)
    b = Bufs(world.ix, 1100, 1100 * 12, 16, CAP, DCAP, plain=(plain,))
    try:
        rc, k, _, _ = _check(world, b, topics, tab, GRID)
        assert rc == OK and k == K
    finally:
        b.free()


def test_misaligned_topic_bytes_take_the_staged_path(world, bufs):
    topics = _topics(1025)
    tab, K = _place(world, topics, "runs7", 200)
    rc, k, _, _ = _check(world, bufs, topics, tab, GRID, shift=4)
    assert rc == OK and k == K


def test_256_destinations_take_the_staged_path(world, bufs):
    topics = _topics(1025)
    tab, K = _place(world, topics, "runs7", 200)
    rc, k, _, _ = _check(world, bufs, topics, tab, GRID, n_dests=256)
    assert rc == OK and k == K


def test_einval_with_a_handle(world, bufs):
    topics = _topics(10)
    tab, K = _place(world, topics, "runs7", 200)
    tab.reset()
    kc, kt = _keys(10, 1)
    assert bufs.call(topics, N_DESTS, LOCAL, CAP, DCAP, kc, kt, flags=0, ok=(EINVAL,))[0] == EINVAL
    assert bufs.call(topics, N_DESTS, LOCAL, CAP, DCAP, kc, kt, flags=AGGRE | 2, ok=(EINVAL,))[0] == EINVAL
    assert bufs.call(topics, N_DESTS, N_DESTS, CAP, DCAP, kc, kt, ok=(EINVAL,))[0] == EINVAL
    assert bufs.call(topics, 0, 0, CAP, DCAP, kc, kt, ok=(EINVAL,))[0] == EINVAL
    ix = world.ix
    args = lambda member, head: (ix._h, 10, P(bufs.blob), P(bufs.offs), N_DESTS, LOCAL, AGGRE, P(bufs.doff), P(bufs.topic),
                                 P(bufs.vals), 16, head, P(bufs.dt), P(bufs.dv), P(bufs.ds), 16, None, None, 0, member,
                                 P(bufs.err))
    assert ix._lib.tm_publish_batch32(*args(None, P(bufs.head))) == EINVAL         # a null out_member with cap > 0
    assert ix._lib.tm_publish_batch32(*args(P(bufs.member), None)) == EINVAL
    assert np.array_equal(tab.state(), tab.start), "a refused call moved a state"


# ---- 6. state across calls

def test_five_consecutive_batches_with_members_and_words_changed_in_between(world, bufs):
    """the reference's five from the start state, then the call's five: every batch's outputs and the words
    after it are equal"""
    w, ix = world, world.ix
    topics = _topics(2049)
    tab, K = _place(w, topics, "runs7", 200)
    rng = np.random.default_rng(12)
    changes = []
    for b_ in range(5):
        slots = rng.choice(tab.used, 3, replace=False).tolist()
        lists = [rng.integers(0, 1 << 31, int(rng.integers(0, 9))).astype(np.uint32) for _ in slots]
        changes.append((slots, lists, [0, 1, 2], [int(rng.integers(0, 7)) | 5 << 8 for _ in slots],
                        ([int(slots[0])], [int(rng.integers(0, 6))]) if b_ % 2 else None))

    first = [tab.used.tolist(), [tab.lists[s] for s in tab.used.tolist()], [tab.nl[s] for s in tab.used.tolist()],
             [tab.meta[s] for s in tab.used.tolist()]]

    def run(call):
        tab.set(*first)                                          # both runs start from the same tables and words
        tab.reset()
        outs = []
        for b_ in range(5):
            kc, kt = _keys(len(topics), 300 + b_)
            outs.append((call(kc, kt, 40 + b_), tab.state()))
            slots, lists, nl, meta, word = changes[b_]
            tab.set(slots, lists, nl, meta)
            if word:
                ix.share_state_set(*word)
        return outs
    ref = run(lambda kc, kt, seed: _reference(ix, topics, N_DESTS, LOCAL, CAP, DCAP, kc, kt, seed))
    o0 = ix.debug_get(ONE)
    got = run(lambda kc, kt, seed: bufs.call(topics, N_DESTS, LOCAL, CAP, DCAP, kc, kt, seed))
    assert ix.debug_get(ONE) == o0 + 5
    for (g, gs), (r, rs) in zip(got, ref):
        _same(g, r)
        assert np.array_equal(gs, rs)
    assert len({tuple(s.tolist()) for _, s in ref}) == 5, "the words never moved"


# ---- 7. concurrency

def test_four_threads_share_one_round_robin_per_group_slot(world):
    """4 x 50 calls of one entry each on one slot of cnt = 5: each call's transition is one compare-and-swap
    loop on the device-resident word, so the 200 picks are those of 200 sequential calls, as a multiset"""
    w, ix = world, world.ix
    topic = [b"$b7/x"]
    tab, K = _place(w, topic, "one", 1, top_ranked=False)
    assert K == 1
    members = np.array([100, 101, 102, 103, 104], np.uint32)
    tab.set([0], [members], [0], [PG])
    c0 = 3
    ix.share_state_set([0], [c0])
    o0 = ix.debug_get(ONE)
    bs = [Bufs(ix, 4, 64, 16, 64, 64) for _ in range(4)]
    picks, errors = [[] for _ in bs], []

    def work(i):
        try:
            for _ in range(50):
                rc, doff, t, v, m = bs[i].call(topic, N_DESTS, LOCAL, 64, 64, None, None)[:5]
                assert rc == OK and int(doff[-1]) == 1
                picks[i].append(int(m[0]))
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for b in bs:
        b.free()
    assert not errors, errors
    assert ix.debug_get(ONE) == o0 + 200
    want = Counter(int(members[(c0 + i) % 5]) for i in range(200))
    assert Counter(p for ps in picks for p in ps) == want
    assert ix.share_state_get([0]).tolist() == [(c0 + 199) % 5 + 1]


# ---- 8. the layers: Router(route_in_place=True, shared_subs=...) and Broker(share_on_device=True)

def test_router_and_broker_in_place_pick_what_shared_subs_pick_picks_per_message(gpu):
    from test_gpu_publish_batch import _both, _expected
    from test_gpu_publish_batch import _keys as keys_of
    from test_gpu_publish_batch import _topics as topics_of
    from emqx_amd.broker import Broker, Message
    from emqx_amd.router import Router
    from emqx_amd.shared_sub import SharedSubs
    from emqx_amd.subscribers import LocalSubs
    ss, ref = SharedSubs(node="n1"), SharedSubs(node="n1")
    r = Router(node="n1", local_subs=LocalSubs(), shared_subs=ss, route_in_place=True)
    for s in (ss, ref):
        s.set_strategy(b"rr", "round_robin")
        s.set_strategy(b"pg", "round_robin_per_group")
        s.set_strategy(b"hc", "hash_clientid")
        s.set_strategy(b"st", "sticky", "hash_topic")
        s.set_strategy(b"one", "round_robin")
        s.set_strategy(b"rnd", "random")
    try:
        groups = (b"rr", b"pg", b"hc", b"st", b"rnd")
        filters = (b"a1/#", b"+/b2/+", b"a1/b2/+", b"#")
        exact = b"a1/b2/c3"
        pid = 0
        for g in groups:
            for f in filters + (exact,):
                for k in range(2 + (len(f) + len(g)) % 3):
                    _both(ss, ref, "subscribe", g, f, ("n1" if k % 3 != 2 else "n2", pid))
                    pid += 1
                r.add_route(f, (g, "n2"))
                r.add_route(f, (g, "n3"))
        _both(ss, ref, "subscribe", b"one", b"a1/#", ("n1", "solo"))
        r.add_route(b"a1/#", (b"one", "n2"))
        for f in filters:
            r.add_route(f, "n2")
            r.add_route(f, "n1")
            r.local_subs.subscribe(f, ("local", f))
        topics = [t for t in topics_of(400, seed=71) if b"+" not in t and b"#" not in t]
        topics[5] = exact
        n = len(topics)
        ix = r._mirror._index
        for batch in range(3):
            kc, kt = keys_of(n, 80 + batch)
            o0 = ix.debug_get(ONE)
            by, deliveries, picks = r.match_routes_publish(topics, kc, kt, seed=batch)
            assert ix.debug_get(ONE) == o0 + 1, "the router did not go through tm_publish_batch32 in place"
            plain, plain_del = r.match_routes_dispatch(topics, aggre=True)
            assert dict(by) == dict(plain) and deliveries == plain_del and len(deliveries) > n
            assert set(picks) == set(groups) | {b"one"}
            assert picks == _expected(ref, picks, kc, kt, batch), f"batch {batch}"
            if batch == 0:
                gone = ss.subscribers(b"rr", b"a1/#")[0]
                _both(ss, ref, "unsubscribe", b"rr", b"a1/#", gone)
                _both(ss, ref, "subscribe", b"pg", b"#", ("n1", "late"))
        kc, kt = keys_of(n, 99)
        msgs = [Message(t, i) for i, t in enumerate(topics)]
        br = Broker(r, share_on_device=True, share_send=lambda p, to, m: "ok", share_seed=9,
                    share_keys=lambda m: (int(kc[m.payload]), int(kt[m.payload])),
                    share_dispatch=lambda g, to, m: 1 / 0)
        o0 = ix.debug_get(ONE)
        plans, errors = br.publish_batch_by_dest(msgs)
        assert errors == {} and ix.debug_get(ONE) == o0 + 1
        ref.seed = 9
        for g in plans:
            if g in ("n1", "n2"):
                continue
            want = []
            for i, to, _ in plans[g]:
                res = ref.pick(g, to, int(kc[i]), int(kt[i]), None, i)
                want.append((i, to, res[1] if res else ("error", "no_subscribers")))
            assert [tuple(x) for x in plans[g]] == want, g
    finally:
        import torch
        torch.cuda.synchronize()
        r._mirror._index.close()
