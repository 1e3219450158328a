"""Deliveries grouped by subscriber through the product path: tm_deliver_batch
under Router.match_routes_deliver and Broker(deliver_grouped=True).

A 300-filter route table over 4 destinations (two nodes, two shared groups),
this node's subscribers in a LocalSubs from a pool of 40 pids, so one pid takes
several messages of a batch and several Tos of one message; one fan-in pid
subscribes to most filters, one filter has 300 subscribers; some exact topics
have a local bag row.  The references are tm_dispatch_batch for the route
outputs, out_head and the deliveries, and the numpy definition of
include/tmatch.h (tests/group_ref.py) applied to those deliveries.
"""
import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.broker import Broker, Message
from emqx_amd.router import Router
from emqx_amd.subscribers import LocalSubs
from group_ref import group_ref

pytestmark = pytest.mark.gpu

CANARY = 0xC0FFEE11
OFFS_CANARY = 0xFFFFFFFFFFFFFF77


@pytest.fixture(scope="module")
def routed():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    rng = np.random.default_rng(31)
    subs = LocalSubs()
    r = Router(node="n1", local_subs=subs)
    dests = ["n1", "n2", (b"g1", "n1"), (b"g1", "n2"), (b"g2", "n3")]
    filters = ([f"a{x}/+/c{z}" for x in range(12) for z in range(5)] + [f"a{x}/#" for x in range(12)] +
               [f"+/b{y}/#" for y in range(9)] + [f"a{x}/b{y}/+" for y in range(9) for x in range(12)])
    filters = sorted(set(f.encode() for f in filters))[:300]
    assert len(filters) > 180
    batch = {}
    for i, f in enumerate(filters):
        batch[(f, "n1" if i % 4 else "n2")] = ("add", 0, None)
        for d in rng.choice(len(dests), 1 + i % 2, replace=False):
            batch[(f, dests[d])] = ("add", 0, None)
    for k in range(40):                               # exact topics: the bag, some rows local with subscribers
        t = f"a{k % 12}/b{k % 9}/c{k % 5}".encode()
        batch[(t, "n1" if k % 2 else "n2")] = ("add", 0, None)
        if k % 4 == 1:
            subs.subscribe(t, ("pid", k % 40))
            subs.subscribe(t, ("exact", k))
    assert r.do_batch(batch) == {}
    for i, f in enumerate(filters):
        for p in rng.choice(40, i % 4, replace=False):
            subs.subscribe(f, ("pid", int(p)))
        if i % 5:
            subs.subscribe(f, ("fan-in", 0))          # the backend consumer: most of every batch
    for k in range(300):
        subs.subscribe(b"a7/#", ("all", k))
    assert len(r._filters) > 180 and len(r._dest_classes) == 4
    return r


def _topics(n, seed=1):
    rng = np.random.default_rng(seed)
    out = [f"a{rng.integers(0, 12)}/b{rng.integers(0, 9)}/c{rng.integers(0, 5)}".encode() for _ in range(n)]
    for i in range(0, n, 31):
        out[i] = (b"a1/+/c1", b"#", b"a/#/b")[i % 3]          # badarg
    for i in range(5, n, 29):
        out[i] = f"zzz/{i}".encode()                         # no route at all
    return out


def _raw(ix, blob, offs, n_dests, local, flags, cap, dcap, gcap):
    n = len(offs) - 1
    doff, head, ghead = np.zeros(n_dests + 2, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    t, v = (np.full(cap + 16, CANARY, np.uint32) for _ in range(2))
    dt, dv, ds = (np.full(dcap + 16, CANARY, np.uint32) for _ in range(3))
    gsub, goff = np.full(gcap + 16, CANARY, np.uint32), np.full(gcap + 1 + 16, OFFS_CANARY, np.uint64)
    err = np.zeros(max(n, 1), np.uint8)
    P = _native._ptr
    rc = ix._lib.tm_deliver_batch(ix._h, n, P(blob), P(offs), n_dests, local, flags, P(doff), P(t), P(v), cap, P(head),
                                  P(dt), P(dv), P(ds), dcap, P(ghead), P(gsub), P(goff), gcap, P(err))
    return rc, (doff, t, v, err[:n]), head, (dt, dv, ds), ghead, gsub, goff


def _setup(routed, n, seed):
    tab = routed._mirror
    tab.flush()
    blob, offs = _native.pack_strings(_topics(n, seed=seed))
    return tab._index, blob, offs, len(routed._dest_classes), routed.dest_id("n1")


@pytest.mark.parametrize("n", [64, 1000])
@pytest.mark.parametrize("aggre", [False, True])
def test_route_outputs_head_and_grouped_deliveries(routed, n, aggre):
    ix, blob, offs, n_dests, local = _setup(routed, n, seed=2 + n)
    (e_doff, e_t, e_v, e_err), (e_dt, e_dv, e_ds) = ix.dispatch_batch(blob, offs, n_dests, local, aggre=aggre)
    (doff, t, v, err), (dt, dv, ds), (gsub, goff) = ix.deliver_batch(blob, offs, n_dests, local, aggre=aggre)
    assert np.array_equal(doff, e_doff) and np.array_equal(t, e_t) and np.array_equal(v, e_v)
    assert np.array_equal(err, e_err) and (err == 1).sum() >= 2          # bad topics: flagged, nothing delivered
    T = len(e_ds)
    (G, W), x_t, x_v, x_s, _, x_gsub, x_goff = group_ref([0, T], e_dt, e_dv, e_ds, T, T)
    print(f"n={n} aggre={aggre}: deliveries T={T}, subscribers G={G}, the largest group {int(np.diff(x_goff.astype(np.int64)).max())}")
    assert T > 2 * n and 20 < G < T // 2, "pids must take several messages and several Tos of one message"
    assert len(dt) == T and np.array_equal(dt, x_t) and np.array_equal(dv, x_v) and np.array_equal(ds, x_s)
    assert np.array_equal(gsub, x_gsub) and np.array_equal(goff, x_goff)
    bad = set(np.nonzero(err)[0].tolist())
    assert bad and not bad & set(dt.tolist())
    # the raw call: heads, and nothing written past what it returns
    total = int(doff[-1])
    room = int(ix.route_batch(blob, offs, n_dests)[0][-1])    # (under aggre cap bounds the entries BEFORE aggregation)
    rc, route, head, (rt, rv, rs), ghead, rgsub, rgoff = _raw(ix, blob, offs, n_dests, local,
                                                               _native.TM_ROUTE_AGGRE if aggre else 0, room, T, G)
    assert rc == _native.TM_OK and ghead.tolist() == [G, T]
    assert head.tolist() == [int(doff[local + 1] - doff[local]), T]
    for got, want in ((rt, x_t), (rv, x_v), (rs, x_s)):
        assert np.array_equal(got[:T], want) and (got[T:] == CANARY).all()
    assert np.array_equal(rgsub[:G], x_gsub) and (rgsub[G:] == CANARY).all()
    assert np.array_equal(rgoff[:G + 1], x_goff) and (rgoff[G + 1:] == OFFS_CANARY).all()
    assert np.array_equal(route[1][:total], e_t) and (route[1][room:] == CANARY).all()


def test_ecap_for_dcap_and_for_gcap_then_a_retry_sized_from_the_heads(routed):
    ix, blob, offs, n_dests, local = _setup(routed, 1000, seed=9)
    (f_doff, f_t, f_v, f_err), (f_dt, f_dv, f_ds) = ix.dispatch_batch(blob, offs, n_dests, local)
    total, T = int(f_doff[-1]), len(f_ds)
    (G, _), x_t, x_v, x_s, _, x_gsub, x_goff = group_ref([0, T], f_dt, f_dv, f_ds, T, T)
    assert T > 3000 and G > 40
    # dcap too small: the first dcap deliveries grouped, the heads exact; then the retry
    dcap = T // 3
    (g3, w3), y_t, y_v, y_s, _, y_gsub, y_goff = group_ref([0, T], f_dt, f_dv, f_ds, dcap, G)
    rc, route, head, (dt, dv, ds), ghead, gsub, goff = _raw(ix, blob, offs, n_dests, local, 0, total, dcap, G)
    assert rc == _native.TM_ECAP and head.tolist()[1] == T and ghead.tolist() == [g3, dcap]
    assert np.array_equal(route[0], f_doff) and np.array_equal(route[1][:total], f_t)
    for got, want in ((dt, y_t), (dv, y_v), (ds, y_s)):
        assert np.array_equal(got[:dcap], want) and (got[dcap:] == CANARY).all()
    assert np.array_equal(gsub[:g3], y_gsub) and np.array_equal(goff[:g3 + 1], y_goff)
    rc, route, head, (dt, dv, ds), ghead, gsub, goff = _raw(ix, blob, offs, n_dests, local, 0, total, int(head[1]), G)
    assert rc == _native.TM_OK and ghead.tolist() == [G, T]
    assert np.array_equal(ds[:T], x_s) and np.array_equal(gsub[:G], x_gsub) and np.array_equal(goff[:G + 1], x_goff)
    # gcap too small: the grouped deliveries still whole, ghead[0] sizes the retry
    for gcap in (G // 2, 0):
        rc, route, head, (dt, dv, ds), ghead, gsub, goff = _raw(ix, blob, offs, n_dests, local, 0, total, T, gcap)
        assert rc == _native.TM_ECAP and ghead.tolist() == [G, T] and head.tolist()[1] == T
        for got, want in ((dt, x_t), (dv, x_v), (ds, x_s)):
            assert np.array_equal(got[:T], want) and (got[T:] == CANARY).all()
        assert np.array_equal(gsub[:gcap], x_gsub[:gcap]) and (gsub[gcap:] == CANARY).all()
        assert np.array_equal(goff[:gcap + 1], x_goff[:gcap + 1]) and (goff[gcap + 1:] == OFFS_CANARY).all()
    rc, route, head, (dt, dv, ds), ghead, gsub, goff = _raw(ix, blob, offs, n_dests, local, 0, total, T, int(ghead[0]))
    assert rc == _native.TM_OK and np.array_equal(gsub[:G], x_gsub) and np.array_equal(goff[:G + 1], x_goff)
    # the route's own TM_ECAP rule stands beside it
    rc, route, head, (dt, dv, ds), ghead, gsub, goff = _raw(ix, blob, offs, n_dests, local, 0, total // 2, T, G)
    assert rc == _native.TM_ECAP and np.array_equal(route[0], f_doff) and ghead.tolist() == [G, T]
    assert np.array_equal(ds[:T], x_s) and (route[1][total // 2:] == CANARY).all()
    # the binding's loop finds all three sizes by itself
    (doff, t, v, err), (dt, dv, ds), (gsub, goff) = ix.deliver_batch(blob, offs, n_dests, local, cap=8, dcap=8, gcap=2)
    assert np.array_equal(t, f_t) and np.array_equal(ds, x_s) and np.array_equal(gsub, x_gsub) and np.array_equal(goff, x_goff)
    # bad arguments, with a handle: each message names the entry point
    E = _native.TM_EINVAL
    P = _native._ptr
    a = [np.zeros(64, np.uint32) for _ in range(6)]
    d8 = [np.zeros(64, np.uint64) for _ in range(4)]
    err = np.zeros(1000, np.uint8)

    def call(local_=local, flags=0, ghead_=d8[2], gsub_=a[5], goff_=d8[3], gcap=8):
        return ix._lib.tm_deliver_batch(ix._h, 1000, P(blob), P(offs), n_dests, local_, flags, P(d8[0]), P(a[0]), P(a[1]), 8,
                                        P(d8[1]), P(a[2]), P(a[3]), P(a[4]), 8, P(ghead_), P(gsub_), P(goff_), gcap, P(err))
    for kw in ({"local_": n_dests}, {"flags": 2}, {"ghead_": None}, {"goff_": None}, {"gsub_": None}):
        assert call(**kw) == E, kw
        assert b"tm_deliver_batch" in ix._lib.tm_last_error(ix._h), kw
    assert call(gsub_=None, gcap=0) == _native.TM_ECAP      # (allowed: no subscriber array with gcap == 0)


def test_router_and_broker_group_what_dispatch_delivers(routed):
    topics = _topics(1000, seed=12)
    for aggre in (False, True):
        by, deliveries = routed.match_routes_dispatch(topics, errors="return", aggre=aggre)
        by2, deliveries2, by_sub = routed.match_routes_deliver(topics, errors="return", aggre=aggre)
        assert dict(by2) == dict(by) and set(by2.errors) == set(by.errors) and by2.host_rows == by.host_rows
        assert deliveries2 == deliveries and len(deliveries) > 5000
        want = {}
        for i, to, p in deliveries:
            want.setdefault(p, []).append((i, to))
        assert by_sub == want
    assert any(p[0] == "exact" for p in by_sub) and ("fan-in", 0) in by_sub     # a bag row present; the fan-in pid
    assert len(by_sub[("fan-in", 0)]) > len(deliveries) // 10
    bagged = next(p for p in by_sub if p[0] == "pid" and any(b"+" not in to and b"#" not in to for _, to in by_sub[p]))
    assert any(b"+" in to or b"#" in to for _, to in by_sub[bagged])           # bag rows and device rows in one list
    # the Broker: deliver_batch once per pid, the per-delivery sends grouped
    msgs = [Message(t, i) for i, t in enumerate(topics)]
    one, calls = [], []
    plans, errors = Broker(routed, dispatch_on_device=True,
                           deliver=lambda p, to, m: one.append((p, to, m.payload))).publish_batch_by_dest(msgs)
    plans2, errors2 = Broker(routed, deliver_grouped=True, deliver=lambda *x: calls.append("per delivery"),
                             deliver_batch=lambda p, items: calls.append((p, [(to, m.payload) for to, m in items]))
                             ).publish_batch_by_dest(msgs)
    assert plans2 == plans and set(errors2) == set(errors) and len(errors) > 10
    assert "per delivery" not in calls and len(calls) == len({p for p, _ in calls}) == len(by_sub)
    want = {}
    for p, to, i in one:
        want.setdefault(p, []).append((to, i))
    assert dict(calls) == want
