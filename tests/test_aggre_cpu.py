"""CPU-side checks of aggre/1 on the device's output order: the new calls are
exported and refuse bad arguments without touching a device, the consecutive
rule of include/tmatch.h equals emqx_broker:aggre/1 on a pure-Python model of
the device (key order, stable partition by destination class), the Router
interns filters to the u32 ids the device compares (a stub mirror stands in for
the device), and a Broker fed aggregated buckets delivers what publish_batch
delivers."""
import random
from collections import Counter

from emqx_amd import _native, build
from emqx_amd.broker import Broker, Message, aggre
from emqx_amd.router import NO_FILTER, ByDest, Route, Router, dest_class
from emqx_amd.trie_search import filter as tfilter, get_id, get_topic, key_order, make_key


def test_new_calls_are_exported_and_refuse_bad_arguments():
    build.build_tmatch()
    lib = _native.load_library()
    for name in ("tm_set_route_filters", "tm_aggre_dev", "tm_route_batch_ex", "tm_route_batch32_ex"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    E = _native.TM_EINVAL
    assert lib.tm_set_route_filters(None, 0, None, None) == E
    assert lib.tm_aggre_dev(None, 1, None, None, None, 0, None, 0, None, None, None, None) == E
    for flags in (0, _native.TM_ROUTE_AGGRE, 2, 0x80000001):   # a null handle, an unknown flag bit
        assert lib.tm_route_batch_ex(None, 0, None, None, 1, None, None, None, 0, None, flags) == E
        assert lib.tm_route_batch32_ex(None, 0, None, None, 1, None, None, None, 0, None, flags) == E
    assert _native.TM_ROUTE_AGGRE == 1 and _native.NO_FILTER == NO_FILTER == 0xFFFFFFFF


def test_abi_minor_version_covers_aggre():
    v = _native.load_library().tm_abi_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 14


# ---- the definition equals aggre/1

NODES = ("n1", "n2", "n3")
GROUPS = (b"g1", b"g2")
EXTERNAL = ("external", "c1")


def _device_model(keys, kid):
    """one topic's matching keys -> the aggregated buckets: device order (ascending term order
    of the filters, one filter's keys by their u32 values), stable partition by class, then the
    consecutive rule inside each bucket.  -> ([(To, class)], dropped)"""
    order = sorted(keys, key=lambda k: (key_order(k)[0], kid[k]))
    buckets: dict = {}
    for k in order:
        buckets.setdefault(dest_class(get_id(k)), []).append(k)
    out, dropped = [], 0
    for cls, ks in buckets.items():
        for q, k in enumerate(ks):
            if q and ks[q - 1][0] == k[0]:
                dropped += 1
                continue
            out.append((get_topic(k), cls[0] if isinstance(cls, tuple) else cls))
    return out, dropped


def test_the_consecutive_rule_equals_aggre():
    rng = random.Random(20240)
    filters = [tfilter(f) for f in (b"a/+", b"a/#", b"+/b", b"#", b"a/+/c", b"+/+", b"a/b/#", b"+/b/#")]
    dests = list(NODES) + [(g, n) for g in GROUPS for n in NODES] + [EXTERNAL]
    total = dropped = 0
    shapes = Counter()
    for trial in range(300):
        keys = set()
        for f in rng.sample(filters, rng.randint(1, len(filters))):
            for d in rng.sample(dests, rng.randint(1, 6)):
                keys.add(make_key(f, d))
        keys = list(keys)
        rng.shuffle(keys)
        kid = {k: i for i, k in enumerate(keys)}   # insertion order: any
        routes = [Route(get_topic(k), get_id(k)) for k in keys]
        got, d = _device_model(keys, kid)
        assert Counter(got) == Counter(aggre(routes)), f"trial {trial}"
        total, dropped = total + len(keys), dropped + d
        by_f = {}
        for k in keys:
            by_f.setdefault(k[0], []).append(get_id(k))
        for ds in by_f.values():
            gs = {x[0] for x in ds if isinstance(x, tuple) and x[0] != "external"}
            shapes["several groups on one filter"] += len(gs) > 1
            shapes["node and group routes on one filter"] += bool(gs) and any(isinstance(x, str) for x in ds)
            shapes["a group on several nodes"] += any(sum(1 for x in ds if isinstance(x, tuple) and x[0] == g) > 1 for g in gs)
    assert dropped > 300 and dropped < total
    assert all(shapes[s] > 50 for s in ("several groups on one filter", "node and group routes on one filter",
                                       "a group on several nodes")), shapes
    # one route, and node routes only: aggre/1's other clauses drop nothing either
    for keys in ([make_key(filters[0], (b"g1", "n1"))], [make_key(f, "n1") for f in filters[:3]]):
        got, d = _device_model(keys, {k: i for i, k in enumerate(keys)})
        assert d == 0 and Counter(got) == Counter(aggre([Route(get_topic(k), get_id(k)) for k in keys]))


# ---- the Router's filter interning

class StubMirror:
    """records what a filter-shipping mirror (topic_index.Tab) would send: the filter id of
    every key it inserts, before the insert, and the release of every key it deletes"""

    def __init__(self):
        self.dest_fn = self.filter_fn = self.filter_release = None
        self.keys = {}
        self.log = []

    def sync_keys(self, keys, present, commit=False):
        for k, here in zip(keys, present):
            if here and k not in self.keys:
                self.keys[k] = self.filter_fn(k)
                self.log.append(("set_filter", k, self.keys[k]))
                self.log.append(("insert", k))
            elif not here and k in self.keys:
                del self.keys[k]
                self.filter_release(k)
                self.log.append(("delete", k))


def test_router_interns_filters():
    m = StubMirror()
    r = Router(node="n1", mirror=m)
    assert m.filter_fn is not None and m.filter_release is not None
    r.add_route(b"a/+", "n1")
    r.add_route(b"a/+", (b"g", "n1"))
    r.add_route(b"a/+", (b"g", "n2"))
    r.add_route(b"a/#", "n2")
    r.add_route(b"exact/topic", "n7")        # a bag row: no key, no filter interned
    ids = {(get_topic(k), get_id(k)): i for k, i in m.keys.items()}
    assert ids[(b"a/+", "n1")] == ids[(b"a/+", (b"g", "n1"))] == ids[(b"a/+", (b"g", "n2"))] != ids[(b"a/#", "n2")]
    assert len(r._filter_ids) == 2 and NO_FILTER not in ids.values()
    for i, e in enumerate(m.log):            # every insert is preceded by its filter
        if e[0] == "insert":
            assert m.log[i - 1][:2] == ("set_filter", e[1])
    # the id lives as long as one key of the filter
    a_plus = ids[(b"a/+", "n1")]
    r.delete_route(b"a/+", "n1")
    r.delete_route(b"a/+", (b"g", "n1"))
    assert a_plus in r._filter_live
    r.add_route(b"a/+", "n3")
    assert m.keys[make_key(tfilter(b"a/+"), "n3")] == a_plus
    r.delete_route(b"a/+", "n3")
    r.delete_route(b"a/+", (b"g", "n2"))
    assert a_plus not in r._filter_live and tuple(tfilter(b"a/+")) not in r._filter_ids
    r.delete_route(b"a/+", (b"g", "n2"))     # deleting a missing key releases nothing
    assert len(r._filter_ids) == 1


def test_no_live_id_is_handed_out_twice():
    m = StubMirror()
    r = Router(node="n1", mirror=m)
    r._filter_next = NO_FILTER - 2           # the counter wraps here: NO_FILTER and live ids are skipped
    for i in range(3):
        r.add_route(b"w%d/+" % i, "n1")
    got = [m.keys[make_key(tfilter(b"w%d/+" % i), "n1")] for i in range(3)]
    assert got == [NO_FILTER - 2, NO_FILTER - 1, 0]
    r._filter_next = NO_FILTER - 2           # and again over ids that are still live
    r.delete_route(b"w1/+", "n1")
    for i in range(3, 6):
        r.add_route(b"w%d/+" % i, "n1")
    got = [m.keys[make_key(tfilter(b"w%d/+" % i), "n1")] for i in range(3, 6)]
    assert got == [NO_FILTER - 1, 1, 2]
    live = [i for _, i in m.keys.items()]
    assert len(set(live)) == len(live) == 5 and NO_FILTER not in live
    rng = random.Random(7)
    names = [b"r%d/#" % i for i in range(40)]
    for _ in range(2000):                    # churn: at every moment distinct live filters, distinct ids
        f = rng.choice(names)
        d = rng.choice(NODES)
        (r.add_route if rng.random() < 0.55 else r.delete_route)(f, d)
        by_filter = {}
        for k, i in m.keys.items():
            by_filter.setdefault(k[0], set()).add(i)
        assert all(len(s) == 1 for s in by_filter.values())
        ids = [next(iter(s)) for s in by_filter.values()]
        assert len(set(ids)) == len(ids) and set(ids) == r._filter_live


# ---- a Broker fed aggregated buckets

class StubRouter:
    """per-message route lists (the bag's rows first), regrouped by destination class; aggre:
    as the device returns them -- inside a class and a message, a filter match whose
    predecessor has the same filter is gone; the bag's rows are left alone"""
    node = "n1"

    def __init__(self, per_message):
        self.per_message = per_message
        self.asked = []

    def match_routes_batch(self, topics, errors="raise"):
        return self.per_message

    def match_routes_by_dest(self, topics, errors="raise", aggre=False):
        self.asked.append(aggre)
        by = ByDest()
        for i, routes in enumerate(self.per_message):
            if isinstance(routes, Exception):
                by.errors[i] = routes
                continue
            for r in routes:
                rows = by.setdefault(dest_class(r.dest), [])
                wild = tfilter(r.topic) is not False
                if aggre and wild and rows and rows[-1][0] == i and rows[-1][1].topic == r.topic:
                    continue
                if aggre and not wild:
                    by.host_rows.setdefault(dest_class(r.dest), set()).add(len(rows))
                rows.append((i, r))
        return by


def test_broker_with_aggregated_buckets_delivers_the_same_multiset():
    from emqx_amd.trie_search import BadArg
    per = [[Route(b"t0", (b"g", "n1")), Route(b"t0", (b"g", "n2")), Route(b"t0", "n2"),     # bag rows: host dedupe
            Route(b"a/+", "n1"), Route(b"a/+", (b"g", "n1")), Route(b"a/+", (b"g", "n2")), Route(b"a/#", (b"g", "n2")),
            Route(b"a/#", "n2")],
           BadArg(b"a/+"),
           [Route(b"a/x", (b"g", "n3"))],
           [Route(b"#", "n2"), Route(b"a/+", "n1"), Route(b"x/#", ("external", "c1"))],
           [Route(b"x/#", ("external", "c2")), Route(b"x/+", (b"h", "n1")), Route(b"x/+", (b"h", "n3"))],
           [],
           [Route(b"z/#", ("external", "c1")), Route(b"z/#", ("external", "c2"))]]   # aggre/1: one (z/#, external)
    msgs = [Message(b"t%d" % i, i) for i in range(len(per))]
    log = Counter()

    def broker(router, **kw):
        return Broker(router, dispatch=lambda to, m: log.update([("n1", to, m.payload)]) or 1,
                      forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                      share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1, **kw)
    broker(StubRouter(per)).publish_batch(msgs)
    exp, log = log, Counter()
    host = StubRouter(per)
    broker(host).publish_batch_by_dest(msgs)
    assert log == exp and host.asked == [False]          # the default: today's call
    log = Counter()
    dev = StubRouter(per)
    plans, errors = broker(dev, aggre_on_device=True).publish_batch_by_dest(msgs)
    assert log == exp and dev.asked == [True] and set(errors) == {1}
    assert exp[(b"g", b"t0", 0)] == 1 and exp[(b"g", b"a/+", 0)] == 1 and exp[(b"h", b"x/+", 4)] == 1
    assert [(i, to) for i, to, _ in plans[b"g"]] == [(0, b"t0"), (0, b"a/+"), (0, b"a/#"), (2, b"a/x")]
    assert [(i, to) for i, to, _ in plans["external"]] == [(3, b"x/#"), (4, b"x/#"), (6, b"z/#")]


# ---- groups the device leaves in the unrouted bucket

class UnroutedMirror(StubMirror):
    """a mirror whose device returns every key for every topic, in device order, bucketed by the
    class ids the Router shipped -- but the classes in `hidden` come back in the unrouted bucket
    (a class interned past MAX_DEST_CLASSES, or after the batch's snapshot of the classes), which
    TM_ROUTE_AGGRE copies whole"""

    def __init__(self, hidden=()):
        super().__init__()
        self.hidden = set(hidden)
        self.dests = {}
        self.order = []

    def sync_keys(self, keys, present, commit=False):
        for k, here in zip(keys, present):
            if here and k not in self.keys:
                self.dests[k] = self.dest_fn(k)
                self.order.append(k)
        super().sync_keys(keys, present, commit)

    def read_begin(self):
        return 1

    def read_end(self, ticket):
        pass

    def decode(self, kids):
        return [self.order[i] for i in kids.tolist()]

    def route_kids(self, topics, n_dests, aggre=False):
        import numpy as np
        live = sorted((k for k in self.order if k in self.keys), key=lambda k: (key_order(k)[0], self.order.index(k)))
        buckets = [[] for _ in range(n_dests + 1)]
        for i in range(len(topics)):
            for k in live:
                d = self.dests[k]
                b = n_dests if d >= n_dests or dest_class(get_id(k)) in self.hidden else d
                rows = buckets[b]
                if aggre and b < n_dests and rows and rows[-1][0] == i and self.order[rows[-1][1]][0] == k[0]:
                    continue
                rows.append((i, self.order.index(k)))
        doff = np.cumsum([0] + [len(b) for b in buckets]).astype(np.uint64)
        flat = [e for b in buckets for e in b]
        return (doff, np.array([e[0] for e in flat], np.uint32), np.array([e[1] for e in flat], np.uint32),
                np.zeros(len(topics), np.uint8))


class MirrorRouter(Router):
    """match_routes_batch from the same stub (it has no matcher): the bag's rows, then every key"""

    def match_routes_batch(self, topics, errors="raise"):
        m = self._mirror
        keys = sorted((k for k in m.order if k in m.keys), key=key_order)[::-1]
        return [self.lookup_route_tab(bytes(t)) + [Route(get_topic(k), get_id(k)) for k in keys] for t in topics]


def test_a_group_in_the_unrouted_bucket_is_delivered_once():
    msgs = [Message(b"exact/t", 0), Message(b"other", 1)]
    for hidden in ((), (b"g",), (b"g", b"h", "n2")):
        log = Counter()
        r = MirrorRouter(node="n1", mirror=UnroutedMirror(hidden))
        for f, d in ((b"a/+", "n1"), (b"a/+", (b"g", "n1")), (b"a/+", (b"g", "n2")), (b"a/+", (b"g", "n3")),
                     (b"a/#", (b"g", "n2")), (b"a/#", "n2"), (b"a/#", (b"h", "n1")), (b"a/#", (b"h", "n2")),
                     (b"b/#", ("external", "c1")), (b"b/#", ("external", "c2")),
                     (b"exact/t", (b"g", "n1")), (b"exact/t", (b"g", "n2"))):
            r.add_route(f, d)

        def broker(**kw):
            return Broker(r, dispatch=lambda to, m: log.update([("n1", to, m.payload)]) or 1,
                          forward=lambda n, to, m: log.update([(n, to, m.payload)]) or "ok",
                          share_dispatch=lambda g, to, m: log.update([(g, to, m.payload)]) or 1, **kw)
        broker().publish_batch(msgs)
        exp, log = log, Counter()
        assert max(exp.values()) == 1 and exp[(b"g", b"a/+", 1)] == 1 and exp[(b"g", b"exact/t", 0)] == 1
        broker().publish_batch_by_dest(msgs)
        assert log == exp, f"host aggre, hidden {hidden}"
        log = Counter()
        broker(aggre_on_device=True).publish_batch_by_dest(msgs)
        assert log == exp, f"device aggre, hidden {hidden}"
        by = r.match_routes_by_dest([m.topic for m in msgs], aggre=True)
        assert [(i, x.topic) for i, x in by[b"g"]] == [(0, b"exact/t"), (0, b"exact/t"), (0, b"a/+"), (0, b"a/#"),
                                                       (1, b"a/+"), (1, b"a/#")]
        assert by.host_rows[b"g"] == {0, 1}


# ---- the NIF core's tmn_route_aggre against the stand-in library

import ctypes as C   # noqa: E402
import subprocess   # noqa: E402
from pathlib import Path   # noqa: E402

import pytest   # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
H = C.c_void_p(1)


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """tmatch_nif_aggre.c on top of tmatch_nif_route.c, and -- first -- tmatch_nif_route.c alone
    against the stand-in that predates tm_route_batch32_ex: it must still link"""
    native, c_src = ROOT / "tests" / "native", ROOT / "c_src"
    cc = ["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread", "-Wl,--no-undefined",
          f"-I{ROOT / 'include'}", f"-I{c_src}"]
    base = [str(c_src / "tmatch_nif_core.c"), str(c_src / "tmatch_nif_route.c"), str(native / "fake_tmatch.c"),
            str(native / "fake_tmatch_route.c")]
    tmp = tmp_path_factory.mktemp("nifaggre")
    subprocess.run(cc + ["-o", str(tmp / "libnifroute.so")] + base, check=True)
    out = tmp / "libnifaggre.so"
    subprocess.run(cc + ["-o", str(out)] + base + [str(c_src / "tmatch_nif_aggre.c"),
                                                  str(native / "fake_tmatch_aggre.c")], check=True)
    lib = C.CDLL(str(out))
    vp = C.c_void_p
    lib.fake_pool_new.restype = vp
    lib.fake_pool_free.argtypes = [vp]
    lib.tmn_take.restype = vp
    lib.tmn_take.argtypes = [vp]
    lib.tmn_give.argtypes = [vp, vp]
    lib.tmn_pack.argtypes = [vp, vp, C.c_uint32, vp, vp]
    lib.tmn_route.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    lib.tmn_route_aggre.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    lib.tmn_route_dest.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for f in (lib.fake_set_vals, lib.fake_set_route_topics):
        f.argtypes, f.restype = [vp], C.POINTER(C.c_uint32)
    lib.fake_set_reruns.argtypes, lib.fake_set_reruns.restype = [vp], C.c_uint64
    lib.fake_aggre_count.restype = C.c_long
    lib.fake_aggre_cap.argtypes, lib.fake_aggre_cap.restype = [C.c_long], C.c_uint64
    return lib


def _pack(lib, s, topics):
    arr = (C.c_char_p * len(topics))(*topics)
    lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
    return lib.tmn_pack(s, H, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))


def _slices(lib, s, n_dests):
    vals, tops = lib.fake_set_vals(s), lib.fake_set_route_topics(s)
    out = []
    for d in range(n_dests + 1):
        b, e = C.c_uint64(), C.c_uint64()
        assert lib.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
        out.append([(tops[k], vals[k]) for k in range(b.value, e.value)])
    return out


def _expected(topics, n_dests, aggregated):
    """the stand-in's buckets (topic i: the values 1000 i + k, bucket v % (n_dests + 1)); aggregated:
    without the entries whose predecessor has the same topic and the same k / (2 (n_dests + 1))"""
    D = n_dests + 1
    out = [[] for _ in range(D)]
    for i, t in enumerate(topics):
        if t[:1] == b"+":
            continue
        for k in range(len(t)):
            row = out[(1000 * i + k) % D]
            if aggregated and (1000 * i + k) % D < n_dests and row and row[-1][0] == i and \
                    (row[-1][1] % 1000) // (2 * D) == k // (2 * D):
                continue
            row.append((i, 1000 * i + k))
    return out


def test_nif_core_aggregated_slices_and_the_capacity_rerun(core):
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    topics = [b"abcdefghijklmnopqrstuvwxyz", b"+x", b"", b"xyz" * 9]
    assert _pack(core, s, topics) == _native.TM_OK
    assert core.tmn_route_aggre(s, H, len(topics), 3) == _native.TM_OK
    got = _slices(core, s, 3)
    plain = _expected(topics, 3, False)
    assert got == _expected(topics, 3, True)
    assert sum(map(len, got)) < sum(map(len, plain)) == 26 + 27 and got[3] == plain[3]   # the unrouted bucket: whole
    assert core.tmn_route(s, H, len(topics), 3) == _native.TM_OK and _slices(core, s, 3) == plain
    assert core.tmn_route_aggre(s, H, len(topics), 0) == _native.TM_EINVAL
    # more entries before aggregation than the first guess: one rerun, sized from the un-aggregated offsets
    topics = [b"x" * 900, b"y" * 900, b"z" * 900, b"w" * 500]
    total = 3200
    assert _pack(core, s, topics) == _native.TM_OK
    c0, r0 = core.fake_aggre_count(), core.fake_set_reruns(s)
    assert core.tmn_route_aggre(s, H, 4, 4) == _native.TM_OK
    assert core.fake_aggre_count() - c0 == 2 and core.fake_set_reruns(s) - r0 == 1
    assert core.fake_aggre_cap(c0) < total <= core.fake_aggre_cap(c0 + 1)
    got = _slices(core, s, 4)
    assert got == _expected(topics, 4, True) and sum(map(len, got)) < total
    for bad in ([b"ab", b"!x", b"cd"], [b"ab", b"~x"]):   # a device failure is a device error
        assert _pack(core, s, bad) == _native.TM_OK
        assert core.tmn_route_aggre(s, H, len(bad), 2) == _native.TM_EDEVICE
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
