"""The picks grouped with the deliveries through the product path:
tm_publish_deliver_batch.

test_gpu_publish_batch.py's route table (76 wildcard filters, each routed to
two nodes and to two shared groups with members on three nodes, this node's
subscribers in a LocalSubs) with member ids below 400, about half of them
connections of this node (tm_set_member_subs) -- onto the very subscriber ids
the direct deliveries go to, so that a subscriber gets both kinds in one batch.
The references: tm_publish_batch from the same start state for every output it
has and for the state words afterwards, and the numpy definition
(tests/group_picks_ref.py) applied to tm_publish_batch's deliveries, entries
and picks for the merged and grouped arrays.
"""
import numpy as np
import pytest

from emqx_amd import _native, shared_sub
from emqx_amd.shared_sub import NONE, UNDEF
from group_picks_ref import group_picks_ref
from test_gpu_publish_batch import SEED, World, _keys, _topics

pytestmark = pytest.mark.gpu

CANARY = 0xC0FFEE44
N_MEMBERS = 400


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    w = World()
    rng = np.random.default_rng(77)
    slots = list(range(w.n_slots))
    strategies = (shared_sub.ROUND_ROBIN, shared_sub.HASH_CLIENTID, shared_sub.ROUND_ROBIN_PER_GROUP, shared_sub.STICKY,
                  shared_sub.HASH_TOPIC)
    w.set_members(slots, [rng.permutation(N_MEMBERS)[:s % 6].tolist() for s in slots],
                  [strategies[s % 5] | shared_sub.HASH_TOPIC << 8 for s in slots])
    n_sub_ids = len(w.subs._pids)
    assert n_sub_ids > 20
    w.sub_of = np.where(rng.random(N_MEMBERS) < 0.5, rng.integers(0, n_sub_ids, N_MEMBERS), NONE).astype(np.uint32)
    w.ix.set_member_subs(np.arange(N_MEMBERS, dtype=np.uint32), w.sub_of)
    yield w
    w.close()


def _reset(w):
    w.ix.share_state_set(np.arange(w.n_slots, dtype=np.uint32), np.full(w.n_slots, UNDEF, np.uint32))


def _raw(w, blob, offs, cap, dcap, gcap, kc, kt):
    ix, n = w.ix, len(offs) - 1
    doff, head, ghead = np.zeros(w.n_dests + 2, np.uint64), np.zeros(2, np.uint64), np.full(2, 99, np.uint64)
    t, v, m = (np.full(cap + 16, CANARY, np.uint32) for _ in range(3))
    dt, dv, ds = (np.full(dcap + 16, CANARY, np.uint32) for _ in range(3))
    gsub, goff = np.full(gcap + 16, CANARY, np.uint32), np.full(gcap + 1 + 16, 7777, np.uint64)
    err = np.zeros(max(n, 1), np.uint8)
    P = _native._ptr
    rc = ix._lib.tm_publish_deliver_batch(ix._h, n, P(blob), P(offs), w.n_dests, w.local, _native.TM_ROUTE_AGGRE, P(doff),
                                          P(t), P(v), cap, P(head), P(dt), P(dv), P(ds), dcap, P(kc), P(kt), SEED, P(m),
                                          P(ghead), P(gsub), P(goff), gcap, P(err))
    return rc, doff, t, v, m, head, dt, dv, ds, ghead, gsub, goff, err[:n]


def _baseline(w, n):
    """tm_publish_batch from the all-UNDEF start state -> its outputs, the state afterwards, the definition's arrays"""
    topics = _topics(n, seed=n + 5)
    blob, offs = _native.pack_strings(topics)
    kc, kt = _keys(n, n + 6)
    _reset(w)
    (doff, t, v, err), (dt, dv, ds), member = w.ix.publish_batch(blob, offs, w.n_dests, w.local, key_clientid=kc,
                                                                 key_topic=kt, seed=SEED)
    after = w.device_state().copy()
    T, K = len(dt), int(doff[-1])
    exp = group_picks_ref([0, T], dt, dv, ds, T, w.n_dests, doff, t, v, member, K, w.sub_of, T + K, T + K)
    return (blob, offs, kc, kt), (doff, t, v, err, dt, dv, ds, member), after, exp


@pytest.mark.parametrize("n", [64, 1000])
def test_equals_publish_batch_and_the_definition(world, n):
    w = world
    (blob, offs, kc, kt), (doff, t, v, err, dt, dv, ds, member), after, exp = _baseline(w, n)
    (G, N), x_t, x_v, x_s, _, x_gsub, x_goff, W, P = exp
    T, K = len(dt), int(doff[-1])
    # the fixture is not degenerate: a subscriber with both kinds, a remote pick, a "no pick"
    local = member < N_MEMBERS
    local[local] = w.sub_of[member[local]] != NONE
    assert P == local.sum() > 0 and T > 0
    assert len(set(ds.tolist()) & set(w.sub_of[member[local]].tolist())) > 0, "no subscriber with both kinds"
    assert ((member != NONE) & ~local).sum() > 0, "no remote pick"
    assert (member == NONE).sum() > 0, "no entry without a pick"
    print(f"n={n}: K={K} T={T} P={P} N={N} G={G}")
    _reset(w)
    (g_doff, g_t, g_v, g_err), (g_dt, g_dv, g_ds), g_member, (gsub, goff), g_T = w.ix.publish_deliver_batch(
        blob, offs, w.n_dests, w.local, key_clientid=kc, key_topic=kt, seed=SEED, gcap=T + K)
    assert np.array_equal(g_doff, doff) and np.array_equal(g_t, t) and np.array_equal(g_v, v) and np.array_equal(g_err, err)
    assert np.array_equal(g_member, member) and g_T == T
    assert np.array_equal(w.device_state(), after)
    assert np.array_equal(g_dt, x_t) and np.array_equal(g_dv, x_v) and np.array_equal(g_ds, x_s)
    assert np.array_equal(gsub, x_gsub) and np.array_equal(goff, x_goff)


def test_dcap_one_short_moves_no_state_and_the_retry_succeeds(world):
    w = world
    (blob, offs, kc, kt), (doff, t, v, err, dt, dv, ds, member), after, exp = _baseline(w, 300)
    (G, N), x_t, x_v, x_s, _, x_gsub, x_goff, W, P = exp
    T, K = len(dt), int(doff[-1])
    cap = int(w.ix.route_batch(blob, offs, w.n_dests)[0][-1])       # the un-aggregated total: what cap must hold
    _reset(w)
    before = w.device_state().copy()
    r = _raw(w, blob, offs, cap, T + K - 1, T + K, kc, kt)
    assert r[0] == _native.TM_ECAP and r[5].tolist() == [int(r[5][0]), T] and int(r[1][-1]) == K
    assert np.array_equal(w.device_state(), before), "the state moved under TM_ECAP from dcap"
    assert (r[4] == CANARY).all() and (r[6] == CANARY).all() and (r[8] == CANARY).all()
    r = _raw(w, blob, offs, cap, T + K, T + K, kc, kt)
    rc, g_doff, g_t, g_v, g_m, head, g_dt, g_dv, g_ds, ghead, gsub, goff, g_err = r
    assert rc == _native.TM_OK and head[1] == T and ghead.tolist() == [G, N]
    assert np.array_equal(g_m[:K], member) and (g_m[K:] == CANARY).all()
    assert np.array_equal(g_dt[:N], x_t) and np.array_equal(g_dv[:N], x_v) and np.array_equal(g_ds[:N], x_s)
    for a in (g_dt, g_dv, g_ds):
        assert (a[N:] == CANARY).all()
    assert np.array_equal(gsub[:G], x_gsub) and (gsub[G:] == CANARY).all()
    assert np.array_equal(goff[:G + 1], x_goff) and (goff[G + 1:] == 7777).all()
    assert np.array_equal(w.device_state(), after)
    # total > cap: no pick, no state either
    before = w.device_state().copy()
    r = _raw(w, blob, offs, cap // 2, T + K, T + K, kc, kt)
    assert r[0] == _native.TM_ECAP and (r[4] == CANARY).all() and np.array_equal(w.device_state(), before)


def test_gcap_one_short_the_picks_stand(world):
    w = world
    (blob, offs, kc, kt), (doff, t, v, err, dt, dv, ds, member), after, exp = _baseline(w, 300)
    (G, N), x_t, x_v, x_s, _, x_gsub, x_goff, W, P = exp
    T, K = len(dt), int(doff[-1])
    cap = int(w.ix.route_batch(blob, offs, w.n_dests)[0][-1])       # the un-aggregated total: what cap must hold
    _reset(w)
    rc, g_doff, g_t, g_v, g_m, head, g_dt, g_dv, g_ds, ghead, gsub, goff, g_err = _raw(w, blob, offs, cap, T + K, G - 1, kc, kt)
    assert rc == _native.TM_ECAP and ghead.tolist() == [G, N]
    assert np.array_equal(w.device_state(), after), "the state moved other than once"
    assert np.array_equal(g_m[:K], member)
    assert np.array_equal(g_dt[:N], x_t) and np.array_equal(g_dv[:N], x_v) and np.array_equal(g_ds[:N], x_s)
    assert np.array_equal(gsub[:G - 1], x_gsub[:G - 1]) and (gsub[G - 1:] == CANARY).all()
    assert np.array_equal(goff[:G], x_goff[:G]) and (goff[G:] == 7777).all()
    # the wrapper derives the groups and does not call again
    _reset(w)
    out = w.ix.publish_deliver_batch(blob, offs, w.n_dests, w.local, key_clientid=kc, key_topic=kt, seed=SEED, gcap=G - 1)
    assert np.array_equal(out[3][0], x_gsub) and np.array_equal(out[3][1], x_goff)
    assert np.array_equal(w.device_state(), after)
    E = _native.TM_EINVAL
    ix, P_ = w.ix, _native._ptr
    doff8, h2 = np.zeros(w.n_dests + 2, np.uint64), np.zeros(2, np.uint64)
    a = np.zeros(16, np.uint32)
    g8 = np.zeros(17, np.uint64)
    e8 = np.zeros(300, np.uint8)

    def call(flags=_native.TM_ROUTE_AGGRE, ghead=h2, gsub=a, goff=g8, gcap=16):
        return ix._lib.tm_publish_deliver_batch(ix._h, 300, P_(blob), P_(offs), w.n_dests, w.local, flags, P_(doff8), P_(a),
                                                P_(a), 16, P_(h2), P_(a), P_(a), P_(a), 16, None, None, 0, P_(a),
                                                P_(ghead), P_(gsub), P_(goff), gcap, P_(e8))
    assert call(flags=0) == E and call(ghead=None) == E and call(goff=None) == E and call(gsub=None) == E
    assert call(gsub=None, gcap=0) == _native.TM_ECAP                 # (allowed; 16 entries are too few)
    assert np.array_equal(w.device_state(), after)


# ---- the layers: Router.match_routes_publish_deliver and Broker(share_grouped=True) on the device

def _layers():
    """a router over a real device mirror: four wildcard filters routed to n1 and n2, four groups with members on n1
    (some of which also subscribe directly) and n2, an exact-topic $share route in the host bag"""
    from emqx_amd.router import Router
    from emqx_amd.shared_sub import SharedSubs
    from emqx_amd.subscribers import LocalSubs
    ss = SharedSubs(node="n1")
    r = Router(node="n1", local_subs=LocalSubs(), shared_subs=ss)
    ss.set_strategy(b"rr", "round_robin")
    ss.set_strategy(b"pg", "round_robin_per_group")
    ss.set_strategy(b"hc", "hash_clientid")
    ss.set_strategy(b"st", "sticky", "hash_topic")
    filters = (b"a1/#", b"+/b2/+", b"a1/b2/+", b"#")
    pid = 0
    for g in (b"rr", b"pg", b"hc", b"st"):
        for f in filters + (b"a1/b2/c3",):
            for k in range(2 + (len(f) + len(g)) % 3):
                p = ("n1" if k % 3 != 2 else "n2", pid)
                ss.subscribe(g, f, p)
                if k == 0 and f != b"a1/b2/c3":
                    r.local_subs.subscribe(f, p)                 # a member that subscribes directly as well
                pid += 1
            r.add_route(f, (g, "n2"))
    r.add_route(b"#", (b"empty", "n3"))                          # a pair without members: no pick
    for f in filters:
        r.add_route(f, "n2")
        r.add_route(f, "n1")
        r.local_subs.subscribe(f, ("local", f))
    return r


def test_router_and_broker_on_the_device():
    import torch
    from collections import Counter
    from emqx_amd.broker import Broker, Message
    from test_publish_deliver_cpu import _host_grouping
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    r1, r2, r3, r4 = _layers(), _layers(), _layers(), _layers()
    try:
        topics = [t for t in _topics(300, seed=71) if b"+" not in t and b"#" not in t]
        topics[5] = b"a1/b2/c3"
        n = len(topics)
        for batch in range(3):
            kc, kt = _keys(n, 80 + batch)
            by, deliveries, picks = r1.match_routes_publish(topics, kc, kt, seed=batch)
            by2, deliveries2, picks2, by_sub = r2.match_routes_publish_deliver(topics, kc, kt, seed=batch)
            assert dict(by2) == dict(by) and deliveries2 == deliveries and picks2 == picks and len(deliveries) > n
            assert by_sub == _host_grouping(r1, deliveries, picks)
            direct = {p for _, _, p in deliveries}
            local = {p for rows in picks.values() for _, _, p in rows if p is not None and r1.member_is_local(p)}
            assert direct & local, "no subscriber with both kinds"
            assert any(p is not None and not r1.member_is_local(p) for rows in picks.values() for _, _, p in rows)
            assert all(p is None for _, _, p in picks[b"empty"]) and len(picks[b"empty"]) == n
        kc, kt = _keys(n, 99)
        msgs = [Message(t, i) for i, t in enumerate(topics)]
        one, two = [], []

        def broker(r, log, **kw):
            return Broker(r, share_on_device=True, share_seed=9, share_keys=lambda m: (int(kc[m.payload]), int(kt[m.payload])),
                          share_send=lambda p, to, m: log.append((p, to, m.payload)) or "ok",
                          deliver=lambda p, to, m: log.append((p, to, m.payload)),
                          deliver_batch=lambda p, items: log.append(("batch", p, [(to, m.payload) for to, m in items])),
                          share_dispatch=lambda g, to, m: 1 / 0, **kw)
        plans, errors = broker(r3, one).publish_batch_by_dest(msgs)
        plans2, errors2 = broker(r4, two, share_grouped=True).publish_batch_by_dest(msgs)
        assert plans2 == plans and errors2 == errors == {}
        batches = [e for e in two if e[0] == "batch"]
        assert len(batches) == len({e[1] for e in batches}) > 4
        flat = Counter((p, to, i) for _, p, items in batches for to, i in items) + Counter(e for e in two if e[0] != "batch")
        assert flat == Counter(one)
        assert all(not r4.member_is_local(e[0]) for e in two if e[0] != "batch")
    finally:
        torch.cuda.synchronize()
        for r in (r1, r2, r3, r4):
            r._mirror._index.close()
