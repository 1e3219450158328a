"""Route fan-out through the product path: tm_route_batch under
Router.match_routes_by_dest and Broker.publish_batch_by_dest.

The reference is the existing path: match_routes_batch's per-message route
lists (lookup_route_tab ++ the filter matches), regrouped on the host by
destination class -- exactly and in order -- and publish_batch's deliveries.
"""
from collections import Counter

import numpy as np
import pytest

from emqx_amd import _native, topic_index as ti
from emqx_amd.broker import Broker, Message
from emqx_amd.router import Route, Router, dest_class

pytestmark = pytest.mark.gpu

NODES = ("n1", "n2", "n3")
GROUPS = (b"g1", b"g2")


@pytest.fixture(scope="module")
def routed():
    """3 nodes and 2 shared groups on ~2,000 wildcard filters, exact topics in the bag"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    rng = np.random.default_rng(2024)
    r = Router(node="n1")
    dests = list(NODES) + [(g, n) for g in GROUPS for n in NODES]
    batch = {}
    for i in range(2000):
        shape = i % 4
        f = (f"a{i % 50}/+/c{i % 7}", f"a{i % 50}/#", f"+/b{i % 40}/#", f"a{i % 50}/b{i % 40}/+")[shape].encode()
        for d in rng.choice(len(dests), 1 + i % 3, replace=False):
            batch[(f, dests[d])] = ("add", 0, None)
    for k in range(300):   # exact topics: the bag
        for d in rng.choice(len(dests), 1 + k % 2, replace=False):
            batch[(f"a{k % 50}/b{k % 40}/c{k % 7}".encode(), dests[d])] = ("add", 0, None)
    assert r.do_batch(batch) == {}
    assert len(r._filters) > 1500 and len(r._bag) > 100
    return r


def _topics(n, seed=1):
    rng = np.random.default_rng(seed)
    out = [f"a{rng.integers(0, 60)}/b{rng.integers(0, 45)}/c{rng.integers(0, 9)}".encode() for _ in range(n)]
    for i in range(0, n, 97):
        out[i] = (b"a1/+/c1", b"#", b"a/#/b")[i % 3]          # badarg
    for i in range(5, n, 89):
        out[i] = f"zzz/{i}".encode()                         # no route at all
    return out


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


def _assert_same(router, topics):
    exp, errs = _regroup(router.match_routes_batch(topics, errors="return"))
    got = router.match_routes_by_dest(topics, errors="return")
    assert set(got) == set(exp)
    for cls in exp:
        assert got[cls] == exp[cls], f"destination {cls!r}: lists differ"
    assert set(got.errors) == set(errs) and all(type(got.errors[i]) is type(errs[i]) for i in errs)
    return got


def test_by_dest_equals_the_regrouped_per_message_lists(routed):
    topics = _topics(5000)
    got = _assert_same(routed, topics)
    assert set(got) == set(NODES) | set(GROUPS)
    assert len(got.errors) > 40 and sum(len(v) for v in got.values()) > 10000
    with pytest.raises(ti.BadArg):
        routed.match_routes_by_dest(topics)   # errors="raise": the first bad topic


def test_publish_batch_by_dest_delivers_the_same_multiset(routed):
    msgs = [Message(t, i) for i, t in enumerate(_topics(3000, seed=3))]
    log = Counter()

    def broker():
        return Broker(routed, dispatch=lambda to, m: log.update([("n1", to, m.payload)]) or 1,
                      forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1)
    res = broker().publish_batch(msgs)
    exp, log = log, Counter()
    plans, errors = broker().publish_batch_by_dest(msgs)
    assert log == exp and sum(exp.values()) > 5000
    assert set(errors) == {i for i, r in enumerate(res) if isinstance(r, Exception)}
    assert set(plans) <= set(NODES) | set(GROUPS)
    for dest, plan in plans.items():   # one plan per destination, in message order
        assert [i for i, _, _ in plan] == sorted(i for i, _, _ in plan)
        assert sum(exp[k] for k in exp if k[0] == dest) == len(plan)
    # the per-message results, regrouped, are the plans
    per = {}
    for i, r in enumerate(res):
        if not isinstance(r, Exception):
            for (to, dest), (tag, to2, out) in zip(*r):
                per.setdefault(dest, Counter()).update([(i, to, out)])
    assert {d: Counter(p) for d, p in plans.items()} == per


def test_read_your_writes_and_cleanup(routed):
    topics = _topics(400, seed=5) + [b"fresh/x/y"]
    routed.add_route(b"fresh/+/y", "n9")   # a new filter on a new destination class
    got = _assert_same(routed, topics)
    assert got["n9"] == [(400, Route(b"fresh/+/y", "n9"))]
    routed.delete_route(b"fresh/+/y", "n9")
    assert "n9" not in _assert_same(routed, topics)
    before = _assert_same(routed, topics)
    assert "n3" in before
    routed.cleanup_routes("n3")
    routed.drain_events()
    after = _assert_same(routed, topics)
    assert "n3" not in after
    assert all(r.dest[1] != "n3" for g in GROUPS for _, r in after.get(g, []))
    # (put the node back for the tests that follow)
    routed.do_batch({(f"a{i}/#".encode(), "n3"): ("add", 0, None) for i in range(50)})


def test_route_batch_cap_too_small_then_one_retry(routed):
    """TM_ECAP with the full bucket sizes; one retry sized from them is exact"""
    tab = routed._mirror
    tab.flush()
    ix = tab._index
    topics = _topics(2000, seed=7)
    blob, offs = _native.pack_strings(topics)
    n, n_dests = len(topics), len(routed._dest_classes)
    full_off, full_t, full_v, full_err = ix.route_batch(blob, offs, n_dests, cap=1 << 20)
    total = int(full_off[-1])
    assert total > 4000 and (np.diff(full_off.astype(np.int64)) > 0).sum() >= 5
    cap = total // 3
    doff = np.zeros(n_dests + 2, np.uint64)
    t = np.full(cap + 16, 0xC0FFEE11, np.uint32)
    v = np.full(cap + 16, 0xC0FFEE11, np.uint32)
    err = np.zeros(n, np.uint8)
    P = _native._ptr
    rc = ix._lib.tm_route_batch(ix._h, n, P(blob), P(offs), n_dests, P(doff), P(t), P(v), cap, P(err))
    assert rc == _native.TM_ECAP
    assert np.array_equal(doff, full_off), "the bucket sizes must be the full ones"
    assert np.array_equal(t[:cap], full_t[:cap]) and np.array_equal(v[:cap], full_v[:cap])
    assert (t[cap:] == 0xC0FFEE11).all() and (v[cap:] == 0xC0FFEE11).all() and np.array_equal(err, full_err)
    cap = int(doff[-1])
    t, v = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    rc = ix._lib.tm_route_batch(ix._h, n, P(blob), P(offs), n_dests, P(doff), P(t), P(v), cap, P(err))
    assert rc == _native.TM_OK
    assert np.array_equal(doff, full_off) and np.array_equal(t, full_t) and np.array_equal(v, full_v)


def test_host_batch_above_the_one_launch_limit(routed):
    """70,000 topics (more than one launch takes, and than the zero-copy
    staging): tm_route_batch == the stable partition of tm_match_batch's CSR"""
    tab = routed._mirror
    topics = _topics(70_000, seed=11)
    n_dests = len(routed._dest_classes)
    ticket = tab.read_begin()
    try:
        tab.flush()
        blob, offs = _native.pack_strings(topics)
        hit, vals, err = tab._index.match_batch(blob, offs)
        doff, t, v, err2 = tab.route_kids(topics, n_dests)
        dest_of = np.full(len(tab._keys), 0xFFFFFFFF, np.uint32)
        for kid, key in enumerate(tab._keys):
            if key is not None:
                dest_of[kid] = routed.dest_id(ti.get_id(key))
    finally:
        tab.read_end(ticket)
    assert np.array_equal(err, err2) and int(hit[-1]) > 150_000
    topic = np.repeat(np.arange(len(topics), dtype=np.uint32), np.diff(hit.astype(np.int64)))
    b = dest_of[vals].astype(np.int64)
    b[b >= n_dests] = n_dests
    order = np.argsort(b, kind="stable")
    assert np.array_equal(t, topic[order]) and np.array_equal(v, vals[order])
    exp = np.zeros(n_dests + 2, np.uint64)
    exp[1:] = np.cumsum(np.bincount(b, minlength=n_dests + 1))
    assert np.array_equal(doff, exp)
