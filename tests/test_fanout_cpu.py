"""CPU-side checks of the route fan-out's boundary: the three new calls are
exported and refuse a null handle without touching a device (their other
TM_EINVAL cases need a handle, so they are in tests/test_gpu_fanout.py), the
ABI minor version moved, and the Router interns destination classes to the
u32 ids the device buckets by (a stub mirror stands in for the device)."""
from emqx_amd import _native, build
from emqx_amd.router import MAX_DEST_CLASSES, UNROUTED, Router, dest_class
from emqx_amd.trie_search import filter as tfilter, get_id, make_key


def test_new_calls_are_exported_and_refuse_a_null_handle():
    build.build_tmatch()
    lib = _native.load_library()
    for name in ("tm_set_dests", "tm_fanout_dev", "tm_route_batch"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    assert lib.tm_set_dests(None, 0, None, None) == _native.TM_EINVAL
    assert lib.tm_fanout_dev(None, 0, None, None, 0, None, 0, 1, None, None, None, None) == _native.TM_EINVAL
    assert lib.tm_route_batch(None, 0, None, None, 1, None, None, None, 0, None) == _native.TM_EINVAL


def test_abi_minor_version_covers_the_fanout():
    v = _native.load_library().tm_abi_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 11


class StubMirror:
    """records what a destination-shipping mirror (topic_index.Tab) would send:
    the class id of every key it inserts, before the insert"""

    def __init__(self):
        self.dest_fn = None
        self.keys = {}
        self.log = []

    def sync_keys(self, keys, present, commit=False):
        for k, here in zip(keys, present):
            if here and k not in self.keys:
                self.keys[k] = self.dest_fn(k)
                self.log.append(("set_dest", k, self.keys[k]))
                self.log.append(("insert", k))
            elif not here:
                self.keys.pop(k, None)


def test_dest_class():
    assert dest_class("n1") == "n1"
    assert dest_class((b"g", "n1")) == b"g" and dest_class((b"g", "n2")) == b"g"
    assert dest_class(("external", "x")) == ("external", "x") != dest_class(("external", "y"))


def test_router_interns_node_group_and_external_classes():
    m = StubMirror()
    r = Router(node="n1", mirror=m)
    assert m.dest_fn is not None
    r.add_route(b"a/+", "n1")
    r.add_route(b"a/#", "n2")
    r.add_route(b"a/+", (b"g", "n1"))
    r.add_route(b"b/+", (b"g", "n2"))        # the same group on another node: the same class
    r.add_route(b"c/+", ("external", "x"))
    r.add_route(b"c/#", ("external", "y"))
    r.add_route(b"d/+", "n1")
    r.add_route(b"exact/topic", "n7")        # a bag row: no key, no class interned
    ids = {get_id(k): i for k, i in m.keys.items()}
    assert ids == {"n1": 0, "n2": 1, (b"g", "n1"): 2, (b"g", "n2"): 2, ("external", "x"): 3, ("external", "y"): 4}
    assert r._dest_classes == ["n1", "n2", b"g", ("external", "x"), ("external", "y")]
    # every insert is preceded by its destination
    for i, e in enumerate(m.log):
        if e[0] == "insert":
            assert m.log[i - 1][:2] == ("set_dest", e[1])
    assert r.dest_id("n2") == 1 and r.dest_id((b"g", "n9")) == 2


def test_class_65537_stays_unrouted():
    r = Router(node="n1", mirror=StubMirror())
    for i in range(MAX_DEST_CLASSES):
        assert r.dest_id(f"node{i}") == i
    assert r.dest_id("one-too-many") == UNROUTED and r.dest_id((b"late-group", "node0")) == UNROUTED
    assert r.dest_id("node65535") == 65535 and len(r._dest_classes) == MAX_DEST_CLASSES
    r.add_route(b"x/+", "one-too-many")      # not an error: the route exists, its key ships as unrouted
    key = make_key(tfilter(b"x/+"), "one-too-many")
    assert r._mirror.keys[key] == UNROUTED and r.has_route(b"x/+", "one-too-many")


class StubRouter:
    """per-message route lists, and their regrouping by destination class"""
    node = "n1"

    def __init__(self, per_message):
        self.per_message = per_message

    def match_routes_batch(self, topics, errors="raise"):
        return self.per_message

    def match_routes_by_dest(self, topics, errors="raise"):
        from emqx_amd.router import ByDest
        by = ByDest()
        for i, routes in enumerate(self.per_message):
            if isinstance(routes, Exception):
                by.errors[i] = routes
                continue
            for r in routes:
                by.setdefault(dest_class(r.dest), []).append((i, r))
        return by


def test_publish_batch_by_dest_dedupes_groups_like_aggre():
    from collections import Counter
    from emqx_amd.broker import Broker, Message
    from emqx_amd.router import Route
    from emqx_amd.trie_search import BadArg
    per = [[Route(b"a/+", "n1"), Route(b"a/+", (b"g", "n1")), Route(b"a/+", (b"g", "n2")), Route(b"a/#", (b"g", "n2")),
            Route(b"a/#", "n2")],
           BadArg(b"a/+"),
           [Route(b"a/x", (b"g", "n3"))],                      # aggre/1's one-route clause
           [Route(b"#", "n2"), Route(b"a/+", "n1"), Route(b"x/#", ("external", "c1"))],
           [Route(b"x/#", ("external", "c2")), Route(b"x/+", (b"h", "n1"))],
           [],
           [Route(b"z/#", ("external", "c1")), Route(b"z/#", ("external", "c2"))]]   # aggre/1: one (z/#, external)
    msgs = [Message(b"t%d" % i, i) for i in range(len(per))]
    log = Counter()

    def broker():
        return Broker(StubRouter(per), dispatch=lambda to, m: log.update([("n1", to, m.payload)]) or 1,
                      forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1)
    res = broker().publish_batch(msgs)
    exp, log = log, Counter()
    plans, errors = broker().publish_batch_by_dest(msgs)
    assert log == exp and set(errors) == {1} and isinstance(res[1], BadArg)
    assert exp[(b"g", b"a/+", 0)] == 1 and exp[(b"g", b"a/#", 0)] == 1     # (g, n1) and (g, n2): one delivery
    assert sorted(plans, key=repr) == sorted(["n1", "n2", b"g", b"h", "external"], key=repr)
    assert [(i, to) for i, to, _ in plans[b"g"]] == [(0, b"a/+"), (0, b"a/#"), (2, b"a/x")]
    assert [(i, to) for i, to, _ in plans["n1"]] == [(0, b"a/+"), (3, b"a/+")]
    # two external classes share the plan "external": message order, not class order
    assert [(i, to) for i, to, _ in plans["external"]] == [(3, b"x/#"), (4, b"x/#"), (6, b"z/#")]
