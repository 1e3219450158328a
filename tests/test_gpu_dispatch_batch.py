"""Local dispatch through the product path: tm_dispatch_batch under
Router.match_routes_dispatch and Broker(dispatch_on_device=True).

A 2,000-filter route table over 4 destinations (two nodes and two shared
groups with members on three), this node's
subscribers in a LocalSubs -- lists of 0 to 3 pids, one broadcast filter with
2,000 (past the 1024 threshold: shard rows) -- some subscribed before their
route exists (the list goes up with the insert), some after (set_subscribers).
The references are tm_route_batch_ex for the route outputs, the numpy
definition of include/tmatch.h on those outputs for the deliveries, and
publish_batch with a dispatch callback that walks LocalSubs for the Broker.
"""
from collections import Counter

import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.broker import Broker, Message
from emqx_amd.router import Router
from emqx_amd.subscribers import LocalSubs

pytestmark = pytest.mark.gpu

NODES = ("n1", "n2")
GROUPS = (b"g1", b"g2")
CANARY = 0xC0FFEE11


@pytest.fixture(scope="module")
def routed():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    rng = np.random.default_rng(77)
    subs = LocalSubs()
    r = Router(node="n1", local_subs=subs)
    dests = list(NODES) + [(g, n) for g in GROUPS for n in ("n1", "n2", "n3")]
    filters = ([f"a{x}/+/c{z}" for x in range(60) for z in range(9)] + [f"a{x}/#" for x in range(60)] +
               [f"+/b{y}/#" for y in range(45)] + [f"a{x}/b{y}/+" for y in range(45) for x in range(60)])[:2000]
    filters = sorted(f.encode() for f in filters)
    assert len(set(filters)) == 2000
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
    for k in range(2000):                             # the broadcast filter
        subs.subscribe(b"a7/#", ("all", k))
    for k in range(0, 2000, 7):                       # and some of them gone again
        subs.unsubscribe(b"a7/#", ("all", k))
    assert any(isinstance(s, tuple) and s[0] == "shard" for s in subs.subscribers(b"a7/#"))
    assert len(r._filters) > 1500 and len(r._bag) > 100 and len(r._dest_classes) == 4
    return r


def _topics(n, seed=1):
    rng = np.random.default_rng(seed)
    out = [f"a{rng.integers(0, 60)}/b{rng.integers(0, 45)}/c{rng.integers(0, 9)}".encode() for _ in range(n)]
    for i in range(0, n, 97):
        out[i] = (b"a1/+/c1", b"#", b"a/#/b")[i % 3]          # badarg
    for i in range(5, n, 89):
        out[i] = f"zzz/{i}".encode()                         # no route at all
    return out


def _table(router):
    """the mirror's lists as the definition's (span, pool), from the host's side"""
    tab = router._mirror
    span = np.zeros(2 * len(tab._keys), np.int64)
    pool = []
    for kid, key in enumerate(tab._keys):
        ids = list(router._key_subs(key)) if key is not None else []
        span[2 * kid], span[2 * kid + 1] = len(pool), len(ids)
        pool.extend(ids)
    return span, np.asarray(pool, np.uint32)


def _model(doff, t, v, bucket, span, pool):
    """include/tmatch.h's numpy definition on a route call's outputs -> (M, T, topic, value, sub)"""
    q0, q1 = int(doff[bucket]), int(doff[bucket + 1])
    t, v = t[q0:q1], v[q0:q1].astype(np.int64)
    ok = v < len(span) // 2
    pos, cnt = np.zeros(len(v), np.int64), np.zeros(len(v), np.int64)
    pos[ok], cnt[ok] = span[2 * v[ok]], span[2 * v[ok] + 1]
    cnt[pos + cnt > len(pool)] = 0
    off = np.concatenate([[0], np.cumsum(cnt)])
    src = np.repeat(np.arange(len(v)), cnt)
    r = np.arange(int(off[-1])) - off[src]
    return len(v), int(off[-1]), t[src], v[src].astype(np.uint32), pool[pos[src] + r]


def _raw(ix, blob, offs, n_dests, local, flags, cap, dcap):
    n = len(offs) - 1
    doff, head = np.zeros(n_dests + 2, np.uint64), np.zeros(2, np.uint64)
    t, v = (np.full(cap + 16, CANARY, np.uint32) for _ in range(2))
    dt, dv, ds = (np.full(dcap + 16, CANARY, np.uint32) for _ in range(3))
    err = np.zeros(max(n, 1), np.uint8)
    P = _native._ptr
    rc = ix._lib.tm_dispatch_batch(ix._h, n, P(blob), P(offs), n_dests, local, flags, P(doff), P(t), P(v), cap, P(head),
                                   P(dt), P(dv), P(ds), dcap, P(err))
    return rc, doff, t, v, head, dt, dv, ds, err[:n]


@pytest.mark.parametrize("aggre", [False, True])
def test_route_outputs_and_deliveries(routed, aggre):
    tab = routed._mirror
    tab.flush()
    ix = tab._index
    topics = _topics(3000, seed=2)
    blob, offs = _native.pack_strings(topics)
    n_dests, local = len(routed._dest_classes), routed.dest_id("n1")
    e_doff, e_t, e_v, e_err = ix.route_batch(blob, offs, n_dests, aggre=aggre)
    (doff, t, v, err), (dt, dv, ds) = ix.dispatch_batch(blob, offs, n_dests, local, aggre=aggre)
    assert np.array_equal(doff, e_doff) and np.array_equal(t, e_t) and np.array_equal(v, e_v)
    assert np.array_equal(err, e_err) and (err == 1).sum() > 20          # a bad topic's flag, as tm_route_batch's
    span, pool = _table(routed)
    M, T, m_t, m_v, m_s = _model(doff, t, v, local, span, pool)
    print(f"aggre={aggre}: entries {int(doff[-1])}, local bucket M={M}, deliveries T={T}")
    assert M > 500 and T > 65536, "the lane's first delivery scratch must prove too small"
    assert len(dt) == T and np.array_equal(dt, m_t) and np.array_equal(dv, m_v) and np.array_equal(ds, m_s)
    if aggre:
        plain = ix.route_batch(blob, offs, n_dests)[0]
        assert int(plain[-1]) > int(doff[-1])                              # aggre/1 dropped something


def test_dcap_too_small_then_one_retry(routed):
    tab = routed._mirror
    tab.flush()
    ix = tab._index
    topics = _topics(1000, seed=4)
    blob, offs = _native.pack_strings(topics)
    n_dests, local = len(routed._dest_classes), routed.dest_id("n1")
    (f_doff, f_t, f_v, f_err), (f_dt, f_dv, f_ds) = ix.dispatch_batch(blob, offs, n_dests, local)
    total, T = int(f_doff[-1]), len(f_dt)
    assert T > 3000
    dcap = T // 3
    rc, doff, t, v, head, dt, dv, ds, err = _raw(ix, blob, offs, n_dests, local, 0, total, dcap)
    assert rc == _native.TM_ECAP and head.tolist() == [int(f_doff[local + 1] - f_doff[local]), T]
    assert np.array_equal(doff, f_doff) and np.array_equal(t[:total], f_t) and np.array_equal(v[:total], f_v)
    for got, full in ((dt, f_dt), (dv, f_dv), (ds, f_ds)):
        assert np.array_equal(got[:dcap], full[:dcap]) and (got[dcap:] == CANARY).all()
    rc, doff, t, v, head2, dt, dv, ds, err = _raw(ix, blob, offs, n_dests, local, 0, total, int(head[1]))
    assert rc == _native.TM_OK and head2.tolist() == head.tolist()
    for got, full in ((dt, f_dt), (dv, f_dv), (ds, f_ds)):
        assert np.array_equal(got[:T], full) and (got[T:] == CANARY).all()
    # the route's own TM_ECAP rule stands beside it: cap too small, the deliveries still whole
    rc, doff, t, v, head3, dt, dv, ds, err = _raw(ix, blob, offs, n_dests, local, 0, total // 2, T)
    assert rc == _native.TM_ECAP and np.array_equal(doff, f_doff) and head3.tolist() == head.tolist()
    assert np.array_equal(t[:total // 2], f_t[:total // 2]) and (t[total // 2:] == CANARY).all()
    assert np.array_equal(ds[:T], f_ds)
    # bad arguments, with a handle
    E = _native.TM_EINVAL
    assert _raw(ix, blob, offs, n_dests, n_dests, 0, 16, 16)[0] == E        # local_dest >= n_dests
    assert _raw(ix, blob, offs, n_dests, local, 2, 16, 16)[0] == E          # an unknown flag


def test_a_batch_above_the_zero_copy_limit(routed):
    """70,000 topics: the head words come back with the staged results"""
    tab = routed._mirror
    tab.flush()
    ix = tab._index
    topics = _topics(70_000, seed=6)
    blob, offs = _native.pack_strings(topics)
    n_dests, local = len(routed._dest_classes), routed.dest_id("n1")
    (doff, t, v, err), (dt, dv, ds) = ix.dispatch_batch(blob, offs, n_dests, local, cap=1 << 19, dcap=1 << 22)
    M, T, m_t, m_v, m_s = _model(doff, t, v, local, *_table(routed))
    assert T > 1 << 20 and len(dt) == T
    assert np.array_equal(dt, m_t) and np.array_equal(dv, m_v) and np.array_equal(ds, m_s)


def _expected_deliveries(router, per_message):
    subs, out = router.local_subs, []
    for i, routes in enumerate(per_message):
        if isinstance(routes, Exception):
            continue
        for r in routes:
            if r.dest == router.node:
                out.extend((i, r.topic, p) for p in subs.dispatch_order(r.topic))
    return out


def test_router_and_broker_deliver_what_the_host_walk_delivers(routed):
    subs = routed.local_subs
    topics = _topics(1500, seed=8)
    per = routed.match_routes_batch(topics, errors="return")
    exp = _expected_deliveries(routed, per)
    for aggre in (False, True):
        by, got = routed.match_routes_dispatch(topics, errors="return", aggre=aggre)
        plain = routed.match_routes_by_dest(topics, errors="return", aggre=aggre)
        assert dict(by) == dict(plain) and set(by.errors) == set(plain.errors)
        assert got == exp, "deliveries differ (message order, then the routes' order, then dispatch_order)"
    assert len(exp) > 10_000
    assert any(p[0] == "exact" for _, _, p in exp) and any(p[0] == "all" for _, _, p in exp)   # bag rows; shard rows
    # a later change reaches the device before the next batch
    f = next(to for _, to, p in exp if p[0] == "pid" and b"+" in to)
    subs.subscribe(f, ("late", 1))
    gone = subs.dispatch_order(f)[0]
    subs.unsubscribe(f, gone)
    exp2 = _expected_deliveries(routed, per)
    assert exp2 != exp and routed.match_routes_dispatch(topics, errors="return")[1] == exp2
    # the Broker: the local node's plan is the deliveries
    msgs = [Message(t, i) for i, t in enumerate(topics)]
    log, sent, got = Counter(), [], []

    def walk(to, m):
        pids = subs.dispatch_order(to)
        sent.extend((p, to, m.payload) for p in pids)
        return len(pids)

    def broker(**kw):
        return Broker(routed, dispatch=walk, forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1, **kw)
    broker().publish_batch(msgs)
    exp_log, exp_sent, log, sent = log, sent, Counter(), []
    plans, errors = broker(dispatch_on_device=True,
                           deliver=lambda p, to, m: got.append((p, to, m.payload))).publish_batch_by_dest(msgs)
    assert sent == [] and log == exp_log and Counter(got) == Counter(exp_sent) and len(got) > 10_000
    assert plans["n1"] == exp2 and len(errors) > 10
    per_pair = {}
    for p, to, m in got:
        per_pair.setdefault((m, to), []).append(p)
    assert all(pids == subs.dispatch_order(to) for (m, to), pids in per_pair.items())
    # route deleted: its list goes with the key
    routed.delete_route(f, "n1")
    exp3 = _expected_deliveries(routed, routed.match_routes_batch(topics, errors="return"))
    assert len(exp3) < len(exp2) and routed.match_routes_dispatch(topics, errors="return")[1] == exp3
    routed.add_route(f, "n1")
    assert routed.match_routes_dispatch(topics, errors="return")[1] == exp2
