"""The shared-subscription pick through the product path: tm_publish_batch.

A route table of 76 wildcard filters, each routed to two nodes and to two
shared groups with members on three nodes (so aggre/1 really drops entries),
this node's subscribers in a LocalSubs.  One slot per {Group, Filter}; the
three keys {Filter, {Group, Node_i}} share it; member lists of 0 to 6 ids and
every strategy.  The references are tm_dispatch_batch for the route outputs,
the head and the deliveries (identical), and the numpy definition
(shared_sub.pick_batch_ref) on those route outputs for the picks, with a host
model of the tables and of the state words that is carried from batch to batch
and compared with tm_share_state_get.
"""
import numpy as np
import pytest

from emqx_amd import _native, shared_sub
from emqx_amd import topic_index as ti
from emqx_amd.router import Router
from emqx_amd.shared_sub import NONE, UNDEF, pick_batch_ref
from emqx_amd.subscribers import LocalSubs

pytestmark = pytest.mark.gpu

GROUPS = (b"g1", b"g2")
CANARY = 0xC0FFEE33
SEED = 0xABCD


def _filters():
    r4 = range(4)
    fs = [f"a{x}/#" for x in r4] + [f"+/b{y}/#" for y in r4] + [f"+/+/c{z}" for z in r4]
    fs += [f"a{x}/b{y}/+" for x in r4 for y in r4] + [f"a{x}/+/c{z}" for x in r4 for z in r4]
    fs += [f"+/b{y}/c{z}" for y in r4 for z in r4] + ["#", "+/#", "+/+/+", "+/+/#"]
    fs += [f"a{x}/+/+" for x in r4] + [f"a{x}/+/#" for x in r4] + [f"+/b{y}/+" for y in r4]
    return sorted(set(f.encode() for f in fs))


class World:
    """a router with its device mirror, and the host model of the share tables"""

    def __init__(self):
        self.subs = LocalSubs()
        self.r = Router(node="n1", local_subs=self.subs)
        self.filters = _filters()
        assert len(self.filters) < 200
        batch = {}
        for i, f in enumerate(self.filters):
            for d in ["n1", "n2"] + [(g, n) for g in GROUPS for n in ("n1", "n2", "n3")]:
                batch[(f, d)] = ("add", 0, None)
            for k in range(i % 3):
                self.subs.subscribe(f, ("pid", i, k))
        assert self.r.do_batch(batch) == {}
        self.tab = self.r._mirror
        self.tab.flush()
        self.ix = self.tab._index
        self.n_dests, self.local = len(self.r._dest_classes), self.r.dest_id("n1")
        assert self.n_dests == 4
        # one slot per {Group, Filter}
        self.slot = {(g, f): s for s, (g, f) in enumerate((g, f) for g in GROUPS for f in self.filters)}
        self.n_slots = len(self.slot)
        self.slot_of = np.full(len(self.tab._keys), NONE, np.uint32)
        for kid, key in enumerate(self.tab._keys):
            if key is None:
                continue
            dest = ti.get_id(key)
            if isinstance(dest, tuple) and dest[0] in GROUPS:
                self.slot_of[kid] = self.slot[(dest[0], ti.get_topic(key))]
        kids = np.nonzero(self.slot_of != NONE)[0].astype(np.uint32)
        assert len(kids) == 3 * self.n_slots
        self.ix.set_share_slots(kids, self.slot_of[kids])
        self.lists, self.meta, self.n_local = {}, {}, {}
        self.state = np.full(self.n_slots, UNDEF, np.uint32)
        rng = np.random.default_rng(3)
        slots = list(range(self.n_slots))
        self.set_members(slots, [rng.integers(0, 1 << 31, s % 7).tolist() for s in slots],
                         [s % 7 | (shared_sub.HASH_TOPIC, shared_sub.RANDOM, shared_sub.LOCAL)[s % 3] << 8 for s in slots])

    def set_members(self, slots, lists, metas):
        nl = [min(len(x), (s % 3)) for s, x in zip(slots, lists)]
        self.ix.set_share_members(slots, lists, nl, metas)
        for s, x, m, k in zip(slots, lists, metas, nl):
            self.lists[s], self.meta[s], self.n_local[s] = list(x), m, k

    def tables(self):
        rec, pool = np.zeros((self.n_slots, 4), np.uint32), []
        for s in range(self.n_slots):
            rec[s] = (len(pool), len(self.lists[s]), self.n_local[s], self.meta[s])
            pool.extend(self.lists[s])
        return rec.reshape(-1), np.array(pool, np.uint32)

    def expect(self, doff, t, v, kc, kt, n, advance=True):
        rec, pool = self.tables()
        member, head, after = pick_batch_ref(self.n_dests, doff, t, v, len(t), self.slot_of, rec, pool, self.state, kc, kt,
                                             n, SEED)
        if advance:
            self.state = after
        return member

    def device_state(self):
        return self.ix.share_state_get(np.arange(self.n_slots, dtype=np.uint32))

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.ix.close()


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    w = World()
    yield w
    w.close()


def _topics(n, seed=1):
    lv = np.random.default_rng(seed).integers(0, 5, (n, 3)).tolist()
    out = [f"a{x}/b{y}/c{z}".encode() for x, y, z in lv]
    for i in range(3, n, 97):
        out[i] = (b"a1/+/c1", b"#", b"a/#/b")[i % 3]          # badarg
    return out


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, n, dtype=np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint32)


def _raw(ix, blob, offs, n_dests, local, cap, dcap, kc, kt, flags=_native.TM_ROUTE_AGGRE):
    n = len(offs) - 1
    doff, head = np.zeros(n_dests + 2, np.uint64), np.zeros(2, np.uint64)
    t, v, m = (np.full(cap + 16, CANARY, np.uint32) for _ in range(3))
    dt, dv, ds = (np.full(dcap + 16, CANARY, np.uint32) for _ in range(3))
    err = np.zeros(max(n, 1), np.uint8)
    P = _native._ptr
    rc = ix._lib.tm_publish_batch(ix._h, n, P(blob), P(offs), n_dests, local, flags, P(doff), P(t), P(v), cap, P(head),
                                  P(dt), P(dv), P(ds), dcap, P(kc), P(kt), SEED, P(m), P(err))
    return rc, doff, t, v, m, head, dt, dv, ds, err[:n]


def _check(w, topics, seed, cap=None, dcap=None):
    """one publish_batch against dispatch_batch and the definition; the model's state moves"""
    blob, offs = _native.pack_strings(topics)
    n = len(topics)
    kc, kt = _keys(n, seed)
    (e_doff, e_t, e_v, e_err), (e_dt, e_dv, e_ds) = w.ix.dispatch_batch(blob, offs, w.n_dests, w.local, cap=cap,
                                                                        dcap=dcap, aggre=True)
    (doff, t, v, err), (dt, dv, ds), member = w.ix.publish_batch(blob, offs, w.n_dests, w.local, cap=cap, dcap=dcap,
                                                                 key_clientid=kc, key_topic=kt, seed=SEED)
    assert np.array_equal(doff, e_doff) and np.array_equal(t, e_t) and np.array_equal(v, e_v) and np.array_equal(err, e_err)
    assert np.array_equal(dt, e_dt) and np.array_equal(dv, e_dv) and np.array_equal(ds, e_ds)
    want = w.expect(doff, t, v, kc, kt, n)
    assert len(member) == int(doff[-1]) and np.array_equal(member, want)
    assert np.array_equal(w.device_state(), w.state)
    return doff, member


@pytest.mark.parametrize("n", [1, 64, 70_000])
def test_equals_dispatch_batch_and_the_definition(world, n):
    big = n > 1000
    topics = _topics(n, seed=n)
    doff, member = _check(world, topics, n, cap=1 << 23 if big else None, dcap=1 << 22 if big else None)
    plain = world.ix.route_batch(*_native.pack_strings(topics), world.n_dests, cap=1 << 23 if big else None)[0]
    if n > 1:
        assert int(plain[-1]) > int(doff[-1]), "aggre/1 dropped nothing"
        assert (member != NONE).sum() > n and (member == NONE).sum() > n   # groups' entries; nodes' entries


def test_state_across_five_batches_with_subscriptions_changing(world):
    w = world
    rng = np.random.default_rng(12)
    for b in range(5):
        _check(w, _topics(300, seed=100 + b), 200 + b)
        slots = rng.choice(w.n_slots, 12, replace=False).tolist()
        lists = [rng.integers(0, 1 << 31, int(rng.integers(0, 9))).tolist() for _ in slots]
        before = w.device_state()
        w.set_members(slots, lists, [int(rng.integers(0, 7)) | shared_sub.HASH_CLIENTID << 8 for _ in slots])
        assert np.array_equal(w.device_state(), before), "set_share_members touched a state"
        if b == 2:                                               # a subscribe's counter reset, a reused slot
            w.ix.share_state_set(slots[:3], [0, UNDEF, 5])
            w.state[slots[:3]] = [0, UNDEF, 5]


def test_ecap_from_cap_moves_no_state_and_the_resubmitted_call_stands(world):
    w = world
    topics = _topics(400, seed=31)
    blob, offs = _native.pack_strings(topics)
    kc, kt = _keys(400, 32)
    plain = w.ix.route_batch(blob, offs, w.n_dests)[0]
    total = int(plain[-1])
    before = w.device_state()
    rc, doff, t, v, m, head, dt, dv, ds, err = _raw(w.ix, blob, offs, w.n_dests, w.local, total // 2, 1 << 20, kc, kt)
    assert rc == _native.TM_ECAP and int(doff[-1]) == total
    assert (m == CANARY).all(), "a pick was written under TM_ECAP from cap"
    assert np.array_equal(w.device_state(), before)
    rc, doff, t, v, m, head, dt, dv, ds, err = _raw(w.ix, blob, offs, w.n_dests, w.local, total, 1 << 20, kc, kt)
    assert rc == _native.TM_OK
    K = int(doff[-1])
    want = w.expect(doff, t[:K], v[:K], kc, kt, 400)
    assert np.array_equal(m[:K], want) and (m[K:] == CANARY).all()
    assert np.array_equal(w.device_state(), w.state)


def test_ecap_from_dcap_alone_the_picks_stand(world):
    w = world
    topics = _topics(400, seed=41)
    blob, offs = _native.pack_strings(topics)
    kc, kt = _keys(400, 42)
    (f_doff, f_t, f_v, _), (f_dt, f_dv, f_ds) = w.ix.dispatch_batch(blob, offs, w.n_dests, w.local, aggre=True)
    T = len(f_dt)
    assert T > 100
    rc, doff, t, v, m, head, dt, dv, ds, err = _raw(w.ix, blob, offs, w.n_dests, w.local, 1 << 20, T // 2, kc, kt)
    assert rc == _native.TM_ECAP and int(head[1]) == T
    K = int(doff[-1])
    assert np.array_equal(doff, f_doff) and np.array_equal(t[:K], f_t) and np.array_equal(v[:K], f_v)
    assert np.array_equal(ds[:T // 2], f_ds[:T // 2]) and (ds[T // 2:] == CANARY).all()
    want = w.expect(doff, t[:K], v[:K], kc, kt, 400)
    assert np.array_equal(m[:K], want) and (m[K:] == CANARY).all()
    assert np.array_equal(w.device_state(), w.state)
    # bad arguments, with a handle
    E = _native.TM_EINVAL
    assert _raw(w.ix, blob, offs, w.n_dests, w.local, 16, 16, kc, kt, flags=0)[0] == E      # without TM_ROUTE_AGGRE
    assert _raw(w.ix, blob, offs, w.n_dests, w.n_dests, 16, 16, kc, kt)[0] == E             # local_dest >= n_dests
    assert np.array_equal(w.device_state(), w.state)


def test_lookback_retry_moves_the_state_once(world):
    w = world
    ix = w.ix
    topics = [t for t in _topics(256, seed=51) if b"+" not in t and b"#" not in t]
    r0 = ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES)
    ix.debug_set(_native.TM_DEBUG_LB_FAIL_BLOCK, 3)
    ix.debug_set(_native.TM_DEBUG_LB_LAUNCHES, 1)                # the first launch fails, the retry succeeds
    blob, offs = _native.pack_strings(topics)
    kc, kt = _keys(len(topics), 52)
    (doff, t, v, err), _, member = ix.publish_batch(blob, offs, w.n_dests, w.local, key_clientid=kc, key_topic=kt,
                                                    seed=SEED, cap=1 << 16, dcap=1 << 16)
    assert ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES) == r0 + 1, "the look-back hook made no batch retry"
    assert not err.any()
    want = w.expect(doff, t, v, kc, kt, len(topics))
    assert np.array_equal(member, want) and np.array_equal(w.device_state(), w.state)


def test_a_value_scratch_that_grows_moves_the_state_once():
    """a fresh index: its lane's first value scratch (65536 words) is too small
    for 3,000 topics' hits, so the batch runs twice"""
    w = World()
    try:
        ix = w.ix
        topics = [t for t in _topics(3000, seed=61) if b"+" not in t and b"#" not in t]
        n = len(topics)
        blob, offs = _native.pack_strings(topics)
        kc, kt = _keys(n, 62)
        keys = (_native.TM_DEBUG_PATH_PHASES, _native.TM_DEBUG_PATH_SMALL)
        p0 = sum(ix.debug_get(k) for k in keys)
        (doff, t, v, err), (dt, dv, ds), member = ix.publish_batch(blob, offs, w.n_dests, w.local, cap=1 << 20,
                                                                   dcap=1 << 20, key_clientid=kc, key_topic=kt, seed=SEED)
        assert sum(ix.debug_get(k) for k in keys) == p0 + 2, "the batch did not run twice"
        assert int(ix.route_batch(blob, offs, w.n_dests)[0][-1]) > 65536
        want = w.expect(doff, t, v, kc, kt, n)
        assert np.array_equal(member, want) and np.array_equal(w.device_state(), w.state)
        (e_doff, e_t, e_v, _), (e_dt, e_dv, e_ds) = ix.dispatch_batch(blob, offs, w.n_dests, w.local, cap=1 << 20,
                                                                      dcap=1 << 20, aggre=True)
        assert np.array_equal(doff, e_doff) and np.array_equal(t, e_t) and np.array_equal(v, e_v)
        assert np.array_equal(ds, e_ds)
    finally:
        w.close()


# ---- the layers: Router(shared_subs=...) and Broker(share_on_device=True)

def _layer_world():
    """-> (router, its SharedSubs, an independent reference SharedSubs fed the same calls)"""
    from emqx_amd.shared_sub import SharedSubs
    ss, ref = SharedSubs(node="n1"), SharedSubs(node="n1")
    r = Router(node="n1", local_subs=LocalSubs(), shared_subs=ss)
    for s in (ss, ref):
        s.set_strategy(b"rr", "round_robin")
        s.set_strategy(b"pg", "round_robin_per_group")
        s.set_strategy(b"hc", "hash_clientid")
        s.set_strategy(b"st", "sticky", "hash_topic")
        s.set_strategy(b"one", "round_robin")
        s.set_strategy(b"rnd", "random")
    return r, ss, ref


def _both(ss, ref, call, *a):
    getattr(ss, call)(*a)
    getattr(ref, call)(*a)


def _expected(ref, picks, kc, kt, seed):
    """SharedSubs.pick per message, pair by pair in message order"""
    ref.seed = seed
    want = {}
    for g, rows in picks.items():
        for i, to, _ in rows:
            res = ref.pick(g, to, int(kc[i]), int(kt[i]), None, i)
            want.setdefault(g, []).append((i, to, res[1] if res else None))
    return want


def test_router_and_broker_pick_what_shared_subs_pick_picks_per_message():
    import torch
    from emqx_amd.broker import Broker, Message
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    r, ss, ref = _layer_world()
    try:
        groups = (b"rr", b"pg", b"hc", b"st", b"rnd")
        filters = (b"a1/#", b"+/b2/+", b"a1/b2/+", b"#")
        exact = b"a1/b2/c3"                                      # an exact-topic $share route: the host bag's
        pid = 0
        for g in groups:
            for f in filters + (exact,):
                for k in range(2 + (len(f) + len(g)) % 3):
                    _both(ss, ref, "subscribe", g, f, ("n1" if k % 3 != 2 else "n2", pid))
                    pid += 1
                r.add_route(f, (g, "n2"))                        # the pair's routes on two more nodes: aggre/1 drops them
                r.add_route(f, (g, "n3"))
        _both(ss, ref, "subscribe", b"one", b"a1/#", ("n1", "solo"))          # a group with one member
        r.add_route(b"a1/#", (b"one", "n2"))
        for k in range(3):                                                    # a group whose name is a str
            _both(ss, ref, "subscribe", "sg", b"#", ("n1", "s%d" % k))
        r.add_route(b"#", ("sg", "n3"))
        for f in filters:
            r.add_route(f, "n2")
            r.add_route(f, "n1")
            r.local_subs.subscribe(f, ("local", f))
        assert exact in r._bag and len(r._filters) > 40
        topics = [t for t in _topics(400, seed=71) if b"+" not in t and b"#" not in t]
        topics[5] = exact
        n = len(topics)
        for batch in range(4):
            kc, kt = _keys(n, 80 + batch)
            by, deliveries, picks = r.match_routes_publish(topics, kc, kt, seed=batch)
            plain, plain_del = r.match_routes_dispatch(topics, aggre=True)
            assert dict(by) == dict(plain) and deliveries == plain_del and len(deliveries) > n
            assert set(picks) == set(groups) | {b"one", "sg"} and len(picks["sg"]) == n
            assert picks == _expected(ref, picks, kc, kt, batch), f"batch {batch}"
            assert len(picks[b"one"]) > 10 and (batch >= 2 or all(p == ("n1", "solo") for _, _, p in picks[b"one"]))
            assert sum(to == exact for _, to, _ in picks[b"rr"]) == topics.count(exact) > 0
            # every message's (To, Group) entries appear once: aggre/1 ran before the pick
            assert all(len(rows) == len({(i, to) for i, to, _ in rows}) for rows in picks.values())
            if batch == 0:                                       # subscriptions change between batches
                gone = ss.subscribers(b"rr", b"a1/#")[0]
                _both(ss, ref, "unsubscribe", b"rr", b"a1/#", gone)
                _both(ss, ref, "subscribe", b"pg", b"#", ("n1", "late"))      # a local subscribe: the counter resets
                _both(ss, ref, "subscribe", b"st", b"#", ("n2", "late2"))
            if batch == 1:                                       # the group's last member leaves
                _both(ss, ref, "unsubscribe", b"one", b"a1/#", ("n1", "solo"))
            if batch >= 2:                                       # ... its n2 route still matches: no_subscribers
                assert all(p is None for _, _, p in picks[b"one"])
        # the Broker: the groups' plans are the picks; a refused send falls back on the host and excludes the pid
        refused = ss.subscribers(b"rr", b"#")[0]
        kc, kt = _keys(n, 99)
        msgs = [Message(t, i) for i, t in enumerate(topics)]
        sent = []

        def share_send(p, to, m):
            sent.append((p, to, m.payload))
            return "nack" if p == refused else "ok"

        br = Broker(r, share_on_device=True, share_send=share_send, share_seed=9,
                    share_keys=lambda m: (int(kc[m.payload]), int(kt[m.payload])),
                    share_dispatch=lambda g, to, m: 1 / 0)
        plans, errors = br.publish_batch_by_dest(msgs)
        assert errors == {} and len(plans["n1"]) == len(deliveries)
        ref.seed = 9
        want, again = {}, []
        for g in plans:
            if g in ("n1", "n2"):
                continue
            for i, to, _ in plans[g]:                            # the batch's picks first ...
                res = ref.pick(g, to, int(kc[i]), int(kt[i]), None, i)
                want.setdefault(g, []).append([i, to, res[1] if res else ("error", "no_subscribers")])
                if res and res[1] == refused:
                    again.append((g, len(want[g]) - 1))
        for g in plans:                                          # ... then dispatch/4 again for the refused ones,
            for gg, at in again:                                 # in the order the Broker walks its plans
                if gg == g:
                    i, to, _ = want[g][at]
                    want[g][at][2] = ref.pick(g, to, int(kc[i]), int(kt[i]), {refused: "nack"}, i)[1]
        assert again and {g: [tuple(x) for x in rows] for g, rows in want.items()} == \
            {g: rows for g, rows in plans.items() if g not in ("n1", "n2")}
        assert all(p != refused for _, _, p in plans[b"rr"]) and sum(p == refused for p, _, _ in sent) == len(again)
        # the words the fallback wrote back are what the next batch starts from
        kc, kt = _keys(n, 100)
        _, _, picks = r.match_routes_publish(topics, kc, kt, seed=11)
        assert picks == _expected(ref, picks, kc, kt, 11)
    finally:
        torch.cuda.synchronize()
        r._mirror._index.close()
