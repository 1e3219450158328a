"""CPU-side checks of the local dispatch on the device: the new calls are
exported and refuse bad arguments without touching a device; a pure-Python model
of the definition in include/tmatch.h (spans into a pool, expanded entry by
entry) equals a transcription of do_dispatch2/2's fold over the ?SUBSCRIBER bag
(emqx_broker.erl:726-760) on seeded subscribe / unsubscribe histories that
cross the 1024 threshold; LocalSubs interns pids and keeps a stub mirror's list
of {Filter, node()} current, set before the insert; and a Broker over a stub
router delivers, with dispatch_on_device, what publish_batch delivers with a
dispatch callback that walks LocalSubs."""
import random
from collections import Counter

from emqx_amd import _native, build
from emqx_amd.broker import Broker, Message
from emqx_amd.router import ByDest, Route, Router, dest_class
from emqx_amd.subscribers import LocalSubs
from emqx_amd.trie_search import filter as tfilter, get_id, get_topic, make_key


def test_new_calls_are_exported_and_refuse_bad_arguments():
    build.build_tmatch()
    lib = _native.load_library()
    for name in ("tm_set_subscribers", "tm_dispatch_dev", "tm_dispatch_batch"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    E = _native.TM_EINVAL
    assert lib.tm_set_subscribers(None, 0, None, None, None) == E
    assert lib.tm_set_subscribers(None, 1, None, None, None) == E
    for n_dests, bucket in ((1, 0), (0, 0), (65537, 0), (4, 5)):   # a null handle; n_dests and bucket out of range
        assert lib.tm_dispatch_dev(None, n_dests, None, bucket, None, None, 0, None, 0, None, 0, None, None, None, None,
                                   None, 0, None) == E
    for n_dests, local, flags in ((1, 0, 0), (1, 0, _native.TM_ROUTE_AGGRE), (4, 4, 0), (0, 0, 0), (1, 0, 2)):
        assert lib.tm_dispatch_batch(None, 0, None, None, n_dests, local, flags, None, None, None, 0, None, None, None,
                                     None, 0, None) == E
    assert _native.TM_DEBUG_SUB_COMPACTIONS == 31


def test_abi_minor_version_covers_dispatch():
    v = _native.load_library().tm_abi_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 16


# ---- the definition equals do_dispatch2/2

class Ets:
    """?SUBSCRIBER written as emqx_broker's pool workers write it (:637-705), with
    emqx_broker_helper's sequence and shard rule -- a transcription kept apart from LocalSubs"""

    def __init__(self, shards, after=1024):
        self.rows = []          # the bag: (Key, Object) in insertion order
        self.seq = {}
        self.subopt = {}
        self.shards, self.after = shards, after

    def member(self, key):
        return any(k == key for k, _ in self.rows)

    def lookup(self, key):
        return [o for k, o in self.rows if k == key]

    def subscribe(self, topic, pid, phash):
        if (topic, pid) in self.subopt:
            return
        self.seq[topic] = self.seq.get(topic, 0) + 1
        i = 0 if self.seq[topic] <= self.after else phash(pid, self.shards) + 1
        self.subopt[(topic, pid)] = i
        if i == 0:
            self.rows.append((topic, pid))
            return
        if not self.member(("shard", topic, i)):
            self.rows.append((topic, ("shard", i)))
        self.rows.append((("shard", topic, i), pid))

    def unsubscribe(self, topic, pid):
        if (topic, pid) not in self.subopt:
            return
        i = self.subopt.pop((topic, pid))
        self.seq[topic] -= 1
        if i == 0:
            self.rows.remove((topic, pid))
            return
        self.rows.remove((("shard", topic, i), pid))
        if not self.member(("shard", topic, i)):
            self.rows.remove((topic, ("shard", i)))

    def do_dispatch2(self, topic, msg, sent):
        """the fold of do_dispatch2/2: -> DispN, every send appended to `sent`"""
        def one(sub):
            if isinstance(sub, tuple) and sub[0] == "shard":
                return sum(one(p) for p in self.lookup(("shard", topic, sub[1])))
            sent.append((sub, topic, msg))
            return 1
        return sum(one(s) for s in self.lookup(topic))


def _device_model(entries, span, pool):
    """the header's definition, entry by entry: [(topic, value)] -> [(topic, value, sub)]"""
    out = []
    for t, v in entries:
        pos, cnt = (span[2 * v], span[2 * v + 1]) if 2 * v + 1 < len(span) else (0, 0)
        if pos + cnt > len(pool):
            cnt = 0
        out.extend((t, v, pool[pos + r]) for r in range(cnt))
    return out


def test_the_definition_equals_do_dispatch2():
    from emqx_amd.subscribers import phash
    rng = random.Random(11)
    filters = [b"a/+", b"a/#", b"big/#", b"dead/+", b"+/x"]
    for shards, after in ((8, 1024), (3, 20)):
        ets, subs = Ets(shards, after), LocalSubs(shards=shards, shard_after=after)
        pids = [("pid", i) for i in range(1400)]
        for p in pids[:1300]:                          # big/# crosses the threshold: shard rows exist
            ets.subscribe(b"big/#", p, phash)
            subs.subscribe(b"big/#", p)
        for step in range(3000):
            f, p = rng.choice(filters[:3] + filters[4:]), rng.choice(pids)   # one pid on several filters
            if rng.random() < 0.6:
                ets.subscribe(f, p, phash)
                subs.subscribe(f, p)
            else:
                ets.unsubscribe(f, p)
                subs.unsubscribe(f, p)
        assert any(isinstance(o, tuple) and o[0] == "shard" for k, o in ets.rows if k == b"big/#")
        assert after > 100 or any(isinstance(o, tuple) and o[0] == "shard" for k, o in ets.rows if k == b"a/+")
        on = {}
        for (f, p) in ets.subopt:
            on.setdefault(p, set()).add(f)
        assert max(len(fs) for fs in on.values()) >= 3     # one pid on several filters
        # the device's table, as the Router would ship it: value = the filter's index
        span, pool = [], []
        for f in filters:
            ids = subs.dispatch_ids(f)
            span += [len(pool), len(ids)]
            pool += ids
        assert span[2 * 3 + 1] == 0                    # dead/+: no subscriber
        for f in filters:                              # LocalSubs is the same bag
            assert subs.subscribers(f) == ets.lookup(f)
        # a bucket of (message, value) entries, some filters twice, the dead one too
        entries = [(m, rng.randrange(len(filters) + 1)) for m in range(40) for _ in range(rng.randrange(4))]
        sent, n_exp = [], 0
        for m, v in entries:
            if v < len(filters):
                n = ets.do_dispatch2(filters[v], m, sent)
                assert (n == 0) == (not ets.lookup(filters[v]))     # {error, no_subscribers}
                n_exp += n
        got = _device_model(entries, span, pool)
        assert len(got) == n_exp == len(sent)
        assert [(subs.pid_of(s), filters[v], m) for m, v, s in got] == sent


# ---- LocalSubs, interning and the Router's hook

class StubMirror:
    """the key set of a device mirror; logs what the Router's hooks make it ship"""

    def __init__(self):
        self.dest_fn = self.filter_fn = self.filter_release = self.sub_fn = None
        self.keys = {}
        self.lists = {}
        self.log = []

    def sync_keys(self, keys, present, commit=False):
        for k, here in zip(keys, present):
            if here and k not in self.keys:
                self.keys[k] = self.filter_fn(k)
                self.lists[k] = list(self.sub_fn(k))
                self.log.append(("set_subscribers", k, self.lists[k]))
                self.log.append(("insert", k))
            elif not here and k in self.keys:
                del self.keys[k]
                self.lists.pop(k, None)
                self.filter_release(k)
                self.log.append(("delete", k))

    def set_subscribers(self, key, ids):
        if key in self.keys:
            self.lists[key] = list(ids)
            self.log.append(("set_subscribers", key, list(ids)))


def test_local_subs_interning_and_the_router_hook():
    subs = LocalSubs(shards=4, shard_after=5)
    m = StubMirror()
    r = Router(node="n1", mirror=m, local_subs=subs)
    assert m.sub_fn is not None and subs.on_change is not None
    subs.subscribe(b"a/+", "p1")
    subs.subscribe(b"a/+", "p2")
    subs.subscribe(b"a/+", "p1")                       # again: nothing changes
    assert subs.sub_id("p1") == 0 and subs.sub_id("p2") == 1 and subs.pid_of(1) == "p2"
    assert m.log == []                                 # no key yet: nothing to set
    r.add_route(b"a/+", "n1")
    r.add_route(b"a/+", "n2")                          # another node's route: no local list
    k1, k2 = make_key(tfilter(b"a/+"), "n1"), make_key(tfilter(b"a/+"), "n2")
    assert m.lists[k1] == [0, 1] and m.lists[k2] == []
    for i, e in enumerate(m.log):                      # every insert is preceded by its list
        if e[0] == "insert":
            assert m.log[i - 1][:2] == ("set_subscribers", e[1])
    subs.subscribe(b"a/+", "p3")
    assert m.lists[k1] == [0, 1, 2] and m.lists[k2] == []
    subs.unsubscribe(b"a/+", "p1")
    assert m.lists[k1] == [1, 2]
    subs.subscribe(b"exact", "p1")                     # an exact topic: the bag stays on the host
    subs.subscribe(b"b/#", "p1")                       # a filter without a route key: a no-op for the mirror
    assert set(m.lists) == {k1, k2}
    for i in range(10):                                # past the threshold: shard rows, flattened where they stand
        subs.subscribe(b"a/+", "q%d" % i)
    order = subs.dispatch_order(b"a/+")
    assert any(isinstance(s, tuple) for s in subs.subscribers(b"a/+")) and len(order) == 12 == len(set(order))
    assert m.lists[k1] == [subs.sub_id(p) for p in order] and order[:2] == ["p2", "p3"]
    r.delete_route(b"a/+", "n1")
    assert k1 not in m.lists
    subs.subscribe(b"a/+", "late")                     # the key is gone: nothing is set
    assert m.log[-1] == ("delete", k1)
    r.add_route(b"a/+", "n1")                          # and back: the current list, before the insert
    assert m.lists[k1] == subs.dispatch_ids(b"a/+") and m.lists[k1][-1] == subs.sub_id("late")


def test_tab_ships_lists_before_the_insert_and_clears_them_on_delete():
    from emqx_amd.topic_index import Tab

    class Index:
        def __init__(self):
            self.log = []

        def set_subscribers(self, values, lists):
            self.log.append(("subs", list(values), [list(x) for x in lists]))

        def apply(self, ops, blob, offs, vals, flags, commit=False):
            self.log.append(("apply", ops.tolist(), vals.tolist()))
            return 1

        def epoch(self):
            return 1, 1

    ix = Index()
    tab = Tab(index=ix)
    lists = {}
    tab.sub_fn = lambda key: lists.get(key, ())
    ka, kb = make_key(tfilter(b"a/+"), "n1"), make_key(tfilter(b"b/#"), "n1")
    lists[ka] = [5, 6]
    tab.insert_key(ka, [])
    tab.insert_key(kb, [])                             # no subscribers: nothing to ship for it
    tab.flush()
    assert ix.log == [("subs", [0], [[5, 6]]), ("apply", [1, 1], [0, 1])]
    tab.set_subscribers(kb, [9])
    tab.set_subscribers(make_key(tfilter(b"c/+"), "n1"), [1])   # not in the table: a no-op
    tab.flush()
    assert ix.log[2:] == [("subs", [1], [[9]])]
    tab.delete_key(ka)
    tab.flush()
    assert ix.log[3:] == [("subs", [0], [[]]), ("apply", [0], [0])]


# ---- a Broker fed deliveries

class StubRouter:
    """per-message route lists (the bag's rows first); match_routes_dispatch as the Router
    returns it: the buckets, and the local node's routes expanded through LocalSubs"""
    node = "n1"

    def __init__(self, per_message, subs):
        self.per_message, self.subs = per_message, subs

    def match_routes_batch(self, topics, errors="raise"):
        return self.per_message

    def match_routes_dispatch(self, topics, errors="raise", aggre=False):
        by, deliveries = ByDest(), []
        for i, routes in enumerate(self.per_message):
            if isinstance(routes, Exception):
                by.errors[i] = routes
                continue
            for r in routes:
                by.setdefault(dest_class(r.dest), []).append((i, r))
                if r.dest == self.node:
                    deliveries.extend((i, r.topic, p) for p in self.subs.dispatch_order(r.topic))
        return by, deliveries


def test_broker_with_deliveries_delivers_the_same_multiset():
    from emqx_amd.trie_search import BadArg
    subs = LocalSubs(shards=3, shard_after=4)
    for i in range(9):
        subs.subscribe(b"a/+", "p%d" % i)              # shard rows
    subs.subscribe(b"t0", "p1")
    subs.subscribe(b"a/#", "p1")
    subs.subscribe(b"a/#", "p0")
    per = [[Route(b"t0", "n1"), Route(b"t0", "n2"), Route(b"a/+", "n1"), Route(b"a/+", (b"g", "n1")), Route(b"a/#", "n1")],
           BadArg(b"a/+"),
           [Route(b"dead/+", "n1")],                   # a local route without subscribers
           [Route(b"#", "n2"), Route(b"a/+", "n1"), Route(b"x/#", ("external", "c1"))],
           []]
    msgs = [Message(b"t%d" % i, i) for i in range(len(per))]
    log, sent = Counter(), []

    def walk(to, m):                                   # dispatch/2 on the host: the walk over LocalSubs
        pids = subs.dispatch_order(to)
        sent.extend((p, to, m.payload) for p in pids)
        return len(pids)

    def broker(**kw):
        return Broker(StubRouter(per, subs), dispatch=walk,
                      forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1, **kw)
    broker().publish_batch(msgs)
    exp_log, exp_sent, log, sent = log, sent, Counter(), []
    assert len(exp_sent) == 1 + 9 + 2 + 9
    got = []
    plans, errors = broker(dispatch_on_device=True,
                           deliver=lambda p, to, m: got.append((p, to, m.payload))).publish_batch_by_dest(msgs)
    assert sent == [] and log == exp_log and set(errors) == {1}
    assert Counter(got) == Counter(exp_sent)
    assert plans["n1"] == [(m, to, p) for p, to, m in got]
    per_pair = {}
    for p, to, m in got:
        per_pair.setdefault((m, to), []).append(p)
    assert all(pids == subs.dispatch_order(to) for (m, to), pids in per_pair.items())
    assert (2, b"dead/+") not in per_pair and "n2" in plans and "external" in plans
    # the default stays off: dispatch is called per (message, To), nothing is asked of match_routes_dispatch
    log, sent = Counter(), []

    class Plain(StubRouter):
        def match_routes_by_dest(self, topics, errors="raise", aggre=False):
            return StubRouter.match_routes_dispatch(self, topics)[0]

        def match_routes_dispatch(self, topics, errors="raise", aggre=False):
            raise AssertionError("not asked for by default")

    b = Broker(Plain(per, subs), dispatch=walk)
    b.publish_batch_by_dest(msgs)
    assert Counter(sent) == Counter(exp_sent) and b.dispatch_on_device is False
