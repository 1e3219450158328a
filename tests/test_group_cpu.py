"""CPU-side checks of the grouping by subscriber: the new calls are exported,
ABI minor 20, the debug keys, the ctypes signatures against the header; the
numpy definition the GPU tests use as their yardstick (tests/group_ref.py)
against a plain dict-of-lists grouping on random inputs; and the Router's and
the Broker's grouping logic over the stub mirror of tests/test_aggre_cpu.py,
given a deliver_kids that applies the same definition."""
import ctypes as C
import random
import re

import numpy as np

from emqx_amd import _native, build
from emqx_amd.broker import Broker, Message
from emqx_amd.router import Router
from emqx_amd.subscribers import LocalSubs
from group_ref import group_by_dict, group_ref
from test_aggre_cpu import MirrorRouter, UnroutedMirror


def test_new_calls_are_exported_and_refuse_a_null_handle():
    build.build_tmatch()
    lib = _native.load_library()
    for name in ("tm_group_subs_dev", "tm_deliver_batch"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    E = _native.TM_EINVAL
    assert lib.tm_group_subs_dev(None, None, None, None, None, 0, None, None, None, 0, None, None, None, None, None) == E
    assert b"tm_group_subs_dev" in lib.tm_last_error(None)
    for flags in (0, _native.TM_ROUTE_AGGRE, 2):
        assert lib.tm_deliver_batch(None, 0, None, None, 1, 0, flags, None, None, None, 0, None, None, None, None, 0,
                                    None, None, None, 0, None) == E
        assert b"tm_deliver_batch" in lib.tm_last_error(None)
    for m in ("group_subs_dev", "deliver_batch"):
        assert callable(getattr(_native.Index, m))


def test_abi_minor_version_and_debug_keys():
    v = _native.load_library().tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 20
    header = (build.ROOT / "include" / "tmatch.h").read_text()
    for name, val in (("TM_DEBUG_GROUP_TILE", 37), ("TM_DEBUG_GROUP_PASSES_RUN", 38), ("TM_DEBUG_GROUP_PASSES_SKIPPED", 39),
                      ("TM_DEBUG_GROUP_GRID", 40)):
        assert getattr(_native, name) == val and f"{name} = {val}" in header


def test_ctypes_signatures_match_the_header():
    header = (build.ROOT / "include" / "tmatch.h").read_text()
    lib = _native.load_library()
    kinds = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    for name in ("tm_group_subs_dev", "tm_deliver_batch"):
        m = re.search(r"^int %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(C.c_void_p if "*" in arg else kinds[arg.replace("const ", "").split()[0]])
        f = getattr(lib, name)
        assert f.restype is C.c_int and list(f.argtypes) == want, name


# ---- the yardstick itself

def test_the_numpy_definition_equals_a_dict_of_lists():
    rng = random.Random(20)
    for case in range(60):
        T = rng.choice([0, 1, 2, 5, 64, 300, 2000])
        space = rng.choice([1, 2, 7, 300, 1 << 32])
        sub = np.array([rng.choice([0, 0xFFFFFFFF, rng.randrange(space)]) if rng.random() < 0.1 else rng.randrange(space)
                        for _ in range(T)], dtype=np.uint32)
        topic = np.array([rng.randrange(1 << 32) for _ in range(T)], dtype=np.uint32)
        value = np.array([rng.randrange(1 << 32) for _ in range(T)], dtype=np.uint32)
        cap = rng.choice([T, T + 9, T // 2, 0])
        W = min(T, cap)
        d = group_by_dict(topic[:W], value[:W], sub[:W])
        G = len(d)
        gcap = rng.choice([G, G + 3, G // 2, 0])
        (g, w), o_t, o_v, o_s, o_p, gsub, goff = group_ref([7, T], topic, value, sub, cap, gcap)
        assert (g, w) == (G, W) and len(o_t) == len(o_v) == len(o_s) == len(o_p) == W
        ids = sorted(d)                                   # ascending subscriber id, unsigned
        flat = [(s,) + e for s in ids for e in d[s]]      # input order inside a group
        assert o_s.tolist() == [e[0] for e in flat] and o_p.tolist() == [e[1] for e in flat]
        assert o_t.tolist() == [e[2] for e in flat] and o_v.tolist() == [e[3] for e in flat]
        Gw = min(G, gcap)
        assert gsub.tolist() == ids[:Gw] and len(goff) == Gw + 1
        ends = np.cumsum([0] + [len(d[s]) for s in ids]).tolist()
        assert goff.tolist() == ends[:Gw + 1]
        assert gsub.dtype == np.uint32 and goff.dtype == np.uint64 and o_p.dtype == np.uint32


# ---- the Router's and the Broker's grouping

class DeliverMirror(UnroutedMirror):
    """test_aggre_cpu's stub with the local dispatch (every entry of bucket `local`
    expanded through sub_fn, as the device does through set_subscribers' lists) and
    deliver_kids: the header's definition applied to those deliveries"""

    def __init__(self, hidden=()):
        super().__init__(hidden)
        self.sub_fn = None
        self.calls = []

    def dispatch_kids(self, topics, n_dests, local, aggre=False):
        self.calls.append("dispatch")
        doff, tidx, kids, err = self.route_kids(topics, n_dests, aggre)
        t, k, s = [], [], []
        for q in range(int(doff[local]), int(doff[local + 1])):
            for sub in self.sub_fn(self.order[int(kids[q])]):
                t.append(int(tidx[q])), k.append(int(kids[q])), s.append(sub)
        return (doff, tidx, kids, err), tuple(np.array(a, dtype=np.uint32) for a in (t, k, s))

    def deliver_kids(self, topics, n_dests, local, aggre=False):
        route, (t, k, s) = self.dispatch_kids(topics, n_dests, local, aggre)
        self.calls[-1] = "deliver"
        _, g_t, g_k, g_s, _, gsub, goff = group_ref([0, len(s)], t, k, s, len(s), len(s))
        return route, (g_t, g_k, g_s), (gsub, goff)


def _world(hidden=()):
    subs = LocalSubs(shards=3, shard_after=4)
    m = DeliverMirror(hidden)
    r = MirrorRouter(node="n1", mirror=m, local_subs=subs)
    # p1 takes several messages and several Tos of one message; a/+ has shard rows; the exact topic a bag row
    for i in range(7):
        subs.subscribe(b"a/+", "p%d" % i)
    for p in ("p1", "p9", "p0"):
        subs.subscribe(b"a/#", p)
    subs.subscribe(b"#", "p1")
    subs.subscribe(b"exact/t", "p1")
    subs.subscribe(b"exact/t", "p8")
    for f, d in ((b"a/+", "n1"), (b"a/+", "n2"), (b"a/#", "n1"), (b"#", "n1"), (b"a/+", (b"g", "n1")), (b"dead/+", "n1"),
                 (b"exact/t", "n1"), (b"exact/t", "n2")):
        r.add_route(f, d)
    return r, m, subs


def test_match_routes_deliver_equals_dispatch_grouped_in_python():
    for aggre in (False, True):
        for hidden in ((), (b"g",)):
            r, m, subs = _world(hidden)
            topics = [b"exact/t", b"other", b"exact/t", b"third"]
            by, deliveries = r.match_routes_dispatch(topics, aggre=aggre)
            by2, deliveries2, by_sub = r.match_routes_deliver(topics, aggre=aggre)
            assert m.calls == ["dispatch", "deliver"]
            assert dict(by2) == dict(by) and by2.errors == by.errors and by2.host_rows == by.host_rows
            assert deliveries2 == deliveries and len(deliveries) > 20
            want = {}
            for i, to, p in deliveries:
                want.setdefault(p, []).append((i, to))
            assert by_sub == want == Router.group_deliveries(deliveries)
            assert len(by_sub["p1"]) > len(topics)            # several messages, several Tos of one message
            assert by_sub["p1"][0] == (0, b"exact/t")         # the bag's row first inside its message
            assert by_sub["p8"] == [(0, b"exact/t"), (2, b"exact/t")]   # a pid the device never saw


def test_broker_deliver_grouped_calls_deliver_batch_once_per_pid():
    r, m, subs = _world()
    msgs = [Message(t, n) for n, t in enumerate([b"exact/t", b"other", b"exact/t"])]
    one = []
    plans, errors = Broker(r, dispatch_on_device=True,
                           deliver=lambda p, to, msg: one.append((p, to, msg.payload))).publish_batch_by_dest(msgs)
    calls = []
    plans2, errors2 = Broker(r, deliver_grouped=True, deliver=lambda *a: calls.append("per delivery"),
                             deliver_batch=lambda p, items: calls.append((p, [(to, msg.payload) for to, msg in items]))
                             ).publish_batch_by_dest(msgs)
    assert plans2 == plans and errors2 == errors              # what the call returns is unchanged
    assert "per delivery" not in calls and len(calls) == len({p for p, _ in calls})   # once per pid
    want = {}
    for p, to, n in one:                                      # the per-delivery sends, grouped stably by pid
        want.setdefault(p, []).append((to, n))
    assert dict(calls) == want
    # the defaults stay off
    b = Broker(r)
    assert b.deliver_grouped is False and m.calls[-1] == "deliver"
    m.calls.clear()
    b.publish_batch_by_dest(msgs)
    assert m.calls == []
