"""The picks grouped with the deliveries, without a device: the three exports
(tm_set_member_subs, tm_group_picks_dev, tm_publish_deliver_batch), the ABI
minor, each ctypes signature against the header's prototype, the null handle;
the numpy definition (tests/group_picks_ref.py) against a plain dict-of-lists
construction; and Router.match_routes_publish_deliver and
Broker(share_on_device=True, share_grouped=True) over a stub mirror (the stub of
test_group_cpu.py with the share tables and both publish calls: the header's
definitions applied on the host).
"""
import ctypes as C
import re
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.broker import Broker, Message
from emqx_amd.shared_sub import UNDEF, SharedSubs, pick_batch_ref
from emqx_amd.subscribers import LocalSubs
from group_picks_ref import NONE, group_picks_by_dict, group_picks_ref
from group_ref import group_ref
from test_aggre_cpu import MirrorRouter
from test_group_cpu import DeliverMirror

ROOT = Path(__file__).resolve().parent.parent
TM_EINVAL = -1
NEW = ("tm_set_member_subs", "tm_group_picks_dev", "tm_publish_deliver_batch")


def test_exports_and_abi_minor():
    lib = _native.load_library()
    for name in NEW:
        assert name in _native.EXPORTS and hasattr(lib, name)
    v = lib.tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 22
    for attr in ("set_member_subs", "group_picks_dev", "publish_deliver_batch"):
        assert hasattr(_native.Index, attr)
    from emqx_amd.topic_index import Tab
    assert hasattr(Tab, "publish_deliver_kids") and hasattr(Tab, "set_member_sub")


@pytest.mark.parametrize("name,count", [("tm_set_member_subs", 4), ("tm_group_picks_dev", 24),
                                        ("tm_publish_deliver_batch", 25)])
def test_the_ctypes_signature_is_the_headers_prototype(name, count):
    header = (ROOT / "include" / "tmatch.h").read_text()
    m = re.search(r"int %s\((.*?)\);" % name, header, re.S)
    assert m, "the prototype is in the header"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    kinds = {"tm_index *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}

    def ctype(p):
        return C.c_void_p if "*" in p else kinds[p.replace("const ", "").rsplit(" ", 1)[0]]
    lib = _native.load_library()
    f = getattr(lib, name)
    assert f.restype == C.c_int32
    assert list(f.argtypes) == [ctype(p) for p in params] and len(params) == count
    names = [p.rsplit(" ", 1)[1].lstrip("*") for p in params]
    if name == "tm_group_picks_dev":
        assert names[5:14] == ["cap", "n_dests", "d_dest_offsets", "d_etopic", "d_evalue", "d_member", "ecap", "d_sub_of",
                               "sub_of_len"]
        assert names[-3:] == ["d_out_src", "out_cap", "stream"]
    if name == "tm_publish_deliver_batch":
        assert names[15:24] == ["dcap", "key_clientid", "key_topic", "seed", "out_member", "out_ghead", "out_gsub",
                                "out_goff", "gcap"] and names[24] == "out_err"


def test_the_header_defines_the_calls_in_numpy():
    header = (ROOT / "include" / "tmatch.h").read_text()
    for line in ("p = lexsort((t, s))", "ls = where(m < sub_of_len, sub_of[m], NONE)", "ghead = [G, N]", "ABI minor 22",
                 "T + K > dcap"):
        assert line in header, line


def test_null_handle_is_einval():
    lib = _native.load_library()
    a = (C.c_uint32 * 4)()
    o = (C.c_uint64 * 4)()
    assert lib.tm_set_member_subs(None, 1, a, a) == TM_EINVAL
    assert b"tm_set_member_subs" in lib.tm_last_error(None)
    assert lib.tm_group_picks_dev(None, o, a, a, a, 1, 1, o, a, a, a, 1, a, 1, o, a, o, 1, a, a, a, a, 1, None) == TM_EINVAL
    assert b"tm_group_picks_dev" in lib.tm_last_error(None)
    err = (C.c_uint8 * 1)()
    assert lib.tm_publish_deliver_batch(None, 1, b"a" * 16, o, 1, 0, _native.TM_ROUTE_AGGRE, o, a, a, 1, o, a, a, a, 1,
                                        None, None, 0, a, o, a, o, 1, err) == TM_EINVAL
    assert b"tm_publish_deliver_batch" in lib.tm_last_error(None)


# ---- the yardstick against a construction with no sort over the whole

def _random_case(rng, W, E, n_msgs, n_subs, n_dests=3):
    topic = np.sort(rng.integers(0, n_msgs, W)).astype(np.uint32)
    value = rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)
    sub = rng.integers(0, n_subs, W).astype(np.uint32)
    doff = np.concatenate([[0], np.sort(rng.integers(0, E + 1, n_dests)), [E]]).astype(np.uint64)
    etopic = np.concatenate([np.sort(rng.integers(0, n_msgs, int(doff[b + 1] - doff[b]))) for b in range(n_dests + 1)]
                            + [np.zeros(0, np.int64)]).astype(np.uint32)
    evalue = rng.integers(0, 1 << 32, E, dtype=np.uint64).astype(np.uint32)
    sub_of = np.where(rng.random(2 * n_subs) < 0.5, rng.integers(0, n_subs, 2 * n_subs), NONE).astype(np.uint32)
    member = np.where(rng.random(E) < 0.8, rng.integers(0, 2 * n_subs + 3, E), NONE).astype(np.uint32)
    return topic, value, sub, doff, etopic, evalue, member, sub_of, n_dests


def test_the_reference_equals_a_dict_of_lists():
    rng = np.random.default_rng(4)
    for W, E, n_msgs, n_subs in ((0, 0, 5, 3), (40, 0, 5, 3), (0, 40, 5, 3), (200, 150, 12, 9), (300, 300, 300, 5),
                                 (500, 400, 3, 40)):
        topic, value, sub, doff, etopic, evalue, member, sub_of, n_dests = _random_case(rng, W, E, n_msgs, n_subs)
        (G, N), o_t, o_v, o_s, o_p, gsub, goff, w, P = group_picks_ref([0, W], topic, value, sub, W, n_dests, doff, etopic,
                                                                      evalue, member, E, sub_of, W + E, W + E)
        ls = np.array([sub_of[m] if m < len(sub_of) else NONE for m in member.tolist()], np.uint32)
        d = group_picks_by_dict(topic, value, sub, etopic, evalue, ls)
        assert w == W and P == int((ls != NONE).sum()) and N == W + P and G == len(d)
        assert gsub.tolist() == sorted(d) and goff[-1] == N
        for g, s in enumerate(gsub.tolist()):
            lo, hi = int(goff[g]), int(goff[g + 1])
            assert list(zip(o_p[lo:hi].tolist(), o_t[lo:hi].tolist(), o_v[lo:hi].tolist())) == d[s]
            assert (o_s[lo:hi] == s).all()


def test_the_tie_rule_and_the_caps():
    # subscriber 7: a direct delivery and a pick in message 3 -- the direct first; its pick of message 1 before both
    topic, value, sub = np.array([0, 3, 3, 5], np.uint32), np.array([10, 11, 12, 13], np.uint32), np.array([7, 7, 2, 7], np.uint32)
    doff = np.array([0, 2, 4, 4], np.uint64)
    etopic, evalue = np.array([3, 4, 1, 3], np.uint32), np.array([20, 21, 22, 23], np.uint32)
    member, sub_of = np.array([0, 1, 0, 2], np.uint32), np.array([7, NONE, 7], np.uint32)
    (G, N), o_t, o_v, o_s, o_p, gsub, goff, W, P = group_picks_ref([9, 4], topic, value, sub, 4, 2, doff, etopic, evalue,
                                                                  member, 4, sub_of, 99, 99)
    assert (G, N, W, P) == (2, 7, 4, 3) and gsub.tolist() == [2, 7] and goff.tolist() == [0, 1, 7]
    assert o_v.tolist() == [12, 10, 22, 11, 20, 23, 13]
    assert o_p.tolist() == [2, 0, 4 + 1, 1, 4 + 0, 4 + 2, 3]
    # out_cap and gcap cut the outputs, never ghead; cap and ecap cut the inputs
    r = group_picks_ref([9, 4], topic, value, sub, 4, 2, doff, etopic, evalue, member, 4, sub_of, 3, 1)
    assert r[0] == [2, 7] and r[2].tolist() == [12, 10, 22] and r[5].tolist() == [2] and r[6].tolist() == [0, 1]
    r = group_picks_ref([9, 4], topic, value, sub, 2, 2, doff, etopic, evalue, member, 1, sub_of, 99, 99)
    assert r[0] == [1, 3] and r[2].tolist() == [10, 11, 20]
    # no local pick: tm_group_subs_dev's definition
    for seed in range(3):
        rng = np.random.default_rng(seed)
        topic, value, sub, doff, etopic, evalue, member, sub_of, n_dests = _random_case(rng, 300, 100, 20, 11)
        sub_of[:] = NONE
        a = group_picks_ref([0, 300], topic, value, sub, 280, n_dests, doff, etopic, evalue, member, 100, sub_of, 999, 7)
        b = group_ref([0, 300], topic, value, sub, 280, 7)
        assert a[0] == b[0] and a[8] == 0
        for x, y in zip(a[1:7], b[1:7]):
            assert np.array_equal(x, y) and x.dtype == y.dtype


# ---- the mirror's hook over a stub index

def test_the_tab_ships_the_member_table_ahead_of_the_members():
    from emqx_amd.topic_index import Tab

    class Index:
        def __init__(self):
            self.log = []

        def set_member_subs(self, members, subs):
            self.log.append(("member_subs", members.tolist(), subs.tolist()))

        def set_share_members(self, slots, lists, n_local, meta):
            self.log.append(("members", list(slots), [list(x) for x in lists]))

    t = Tab(index=Index())
    assert t.member_subs_fn is None
    local = {3: 30, 5: 50}
    t.member_subs_fn = local.get
    t.set_share_members(0, [3, 4, 5], 0, 1)
    t.set_share_members(1, [5, 3], 0, 1)                 # known already: not shipped twice
    t.flush()
    assert t._index.log == [("member_subs", [3, 5], [30, 50]), ("members", [0, 1], [[3, 4, 5], [5, 3]])]
    local[4] = 40
    del local[3]
    t.set_share_members(0, [3, 4, 5], 0, 1)              # what changed goes up again
    t.set_member_sub(9, 90)
    t.flush()
    assert t._index.log[2] == ("member_subs", [3, 4, 9], [NONE, 40, 90])


# ---- the Router's and the Broker's merged grouping

class PublishMirror(DeliverMirror):
    """test_group_cpu's stub with the share tables (share_fn, set_share_members, set_share_state,
    member_subs_fn) and the two publish calls: pick_batch_ref over the aggregated entries with the
    tables as shipped, and group_picks_ref over the deliveries and those picks"""

    def __init__(self):
        super().__init__()
        self.share_fn = self.share_release = self.member_subs_fn = None
        self.slot_of, self.members, self.state, self.member_sub = {}, {}, {}, {}

    @property
    def _keys(self):
        return self.order

    def sync_keys(self, keys, present, commit=False):
        gone = []
        for k, here in zip(keys, present):
            if here and k not in self.keys:
                s = self.share_fn(k) if self.share_fn else None
                if s is not None:
                    self.slot_of[k] = s
            elif not here and k in self.keys and k in self.slot_of:
                del self.slot_of[k]
                gone.append(k)
        super().sync_keys(keys, present, commit)
        for k in gone:
            self.share_release(k)

    def set_share_members(self, slot, ids, n_local, meta):
        self.members[slot] = (list(ids), n_local, meta)
        for m in ids:
            self.member_sub[m] = self.member_subs_fn(m) if self.member_subs_fn else None

    def set_share_state(self, slot, word):
        self.state[slot] = word

    def share_state(self, slots, dev=0):
        return [self.state.get(s, UNDEF) for s in slots]

    def publish_kids(self, topics, n_dests, local, kc=None, kt=None, seed=0):
        route, (t, k, s) = self.dispatch_kids(topics, n_dests, local, True)
        self.calls[-1] = "publish"
        doff, tidx, kids, err = route
        n_slots = max(list(self.members) + list(self.slot_of.values()) + [-1]) + 1
        slot_of = np.array([self.slot_of.get(key, NONE) if key in self.keys else NONE for key in self.order], np.uint32)
        rec, pool = np.zeros((n_slots, 4), np.uint32), []
        for sl in range(n_slots):
            ids, n_local, meta = self.members.get(sl, ([], 0, 0))
            rec[sl] = (len(pool), len(ids), n_local, meta)
            pool.extend(ids)
        state = np.array([self.state.get(sl, UNDEF) for sl in range(n_slots)], np.uint32)
        member, _, after = pick_batch_ref(n_dests, doff, tidx, kids, len(kids), slot_of, rec, np.array(pool, np.uint32),
                                          state, kc, kt, len(topics), seed)
        for sl in range(n_slots):
            self.state[sl] = int(after[sl])
        return route, (t, k, s), member

    def publish_deliver_kids(self, topics, n_dests, local, kc=None, kt=None, seed=0):
        route, (t, k, s), member = self.publish_kids(topics, n_dests, local, kc, kt, seed)
        self.calls[-1] = "publish_deliver"
        sub_of = np.full(max(list(self.member_sub) + [-1]) + 1, NONE, np.uint32)
        for m, sub in self.member_sub.items():
            if sub is not None:
                sub_of[m] = sub
        E, W = len(route[2]), len(s)
        (G, N), o_t, o_k, o_s, _, gsub, goff, _, _ = group_picks_ref([0, W], t, k, s, W, n_dests, route[0], route[1],
                                                                    route[2], member, E, sub_of, W + E, W + E)
        return route, (o_t, o_k, o_s), member, (gsub, goff), W


A, B, C3, X, Y = ("n1", "a"), ("n1", "b"), ("n1", "c"), ("n2", "x"), ("n3", "y")


def _world(in_place=False):
    subs, ss = LocalSubs(shards=3, shard_after=4), SharedSubs(node="n1", default_strategy="round_robin")
    m = PublishMirror()
    r = MirrorRouter(node="n1", mirror=m, local_subs=subs, shared_subs=ss, route_in_place=in_place)
    assert m.member_subs_fn is not None
    for p in (A, B, "p1", "p2"):                       # A and B also subscribe directly
        subs.subscribe(b"a/+", p)
    subs.subscribe(b"#", A)
    subs.subscribe(b"exact/t", A)
    subs.subscribe(b"exact/t", "p8")
    for f, d in ((b"a/+", "n1"), (b"a/+", "n2"), (b"#", "n1"), (b"exact/t", "n1"), (b"exact/t", "n2")):
        r.add_route(f, d)
    ss.set_strategy(b"hc", "hash_clientid")
    for g, f, pids in ((b"g", b"a/+", (A, X, B, C3)), (b"g", b"a/#", (X, Y)), (b"hc", b"#", (B, A, Y)),
                       (b"g", b"exact/t", (A, X)), (b"solo", b"a/#", (C3,))):
        for p in pids:
            ss.subscribe(g, f, p)
    for f, g in ((b"a/+", b"g"), (b"a/#", b"g"), (b"#", b"hc"), (b"none/#", b"gone")):
        r.add_route(f, (g, "n2"))                      # the pairs' routes on another node: aggre/1 drops them
    return r, m, subs, ss


TOPICS = [b"exact/t", b"other", b"exact/t", b"third", b"fifth"]
KC, KT = [5, 6, 7, 8, 9], [11, 12, 13, 14, 15]


def _host_grouping(r, deliveries, picks):
    """{pid: [(message index, To)]}: the deliveries grouped stably by pid, a pid's local picks behind
    the direct deliveries of their message, in the order `picks` lists them"""
    rows = {}
    for n, (i, to, p) in enumerate(deliveries):
        rows.setdefault(p, []).append((i, 0, n, to))
    n = 0
    for g, lst in picks.items():
        for i, to, p in lst:
            if p is not None and r.member_is_local(p):
                rows.setdefault(p, []).append((i, 1, n, to))
            n += 1
    return {p: [(i, to) for i, _, _, to in sorted(v, key=lambda e: e[:3])] for p, v in rows.items()}


def test_match_routes_publish_deliver_equals_publish_grouped_in_python():
    for in_place in (False, True):
        (r1, m1, _, _), (r2, m2, _, _) = _world(), _world(in_place)
        for batch in range(3):                             # the state carries from batch to batch
            by, deliveries, picks = r1.match_routes_publish(TOPICS, KC, KT, seed=batch)
            by2, deliveries2, picks2, by_sub = r2.match_routes_publish_deliver(TOPICS, KC, KT, seed=batch)
            assert m1.calls[-1] == "publish" and m2.calls[-1] == "publish_deliver"
            assert dict(by2) == dict(by) and by2.errors == by.errors and by2.host_rows == by.host_rows
            assert deliveries2 == deliveries and picks2 == picks and len(deliveries) > 20
            assert by_sub == _host_grouping(r1, deliveries, picks)
            assert m1.state == m2.state and r1._share_host_state == r2._share_host_state
            both = [p for p in by_sub if len(by_sub[p]) > len(Router_group(deliveries).get(p, ()))]
            assert A in both or B in both, "a subscriber with both kinds"
            assert any(p is not None and not r1.member_is_local(p) for rows in picks.values() for _, _, p in rows)
            assert any(p is None for rows in picks.values() for _, _, p in rows), "a pair without members"
            assert any(to == b"exact/t" for _, to, _ in picks[b"g"]), "the bag's host picks"
        assert X not in by_sub and Y not in by_sub and "p8" in by_sub
    with pytest.raises(ValueError):
        MirrorRouter(node="n1", mirror=PublishMirror(), local_subs=LocalSubs()).match_routes_publish_deliver(TOPICS)


def Router_group(deliveries):
    from emqx_amd.router import Router
    return Router.group_deliveries(deliveries)


def _broker(r, log, fail=(), **kw):
    def deliver_batch(p, items):
        log.append(("batch", p, [(to, m.payload) for to, m in items]))
        return "noproc" if p in fail else None

    def share_send(p, to, m):
        log.append(("send", p, to, m.payload))
        return "ok"
    return Broker(r, share_on_device=True, share_send=share_send, share_seed=3,
                  share_keys=lambda m: (KC[m.payload], KT[m.payload]), share_dispatch=lambda g, to, m: 1 / 0,
                  deliver=lambda p, to, m: log.append(("deliver", p, to, m.payload)), deliver_batch=deliver_batch, **kw)


def test_broker_share_grouped_one_list_per_subscriber_and_the_same_multiset():
    msgs = [Message(t, n) for n, t in enumerate(TOPICS)]
    (r1, _, _, _), (r2, _, _, _) = _world(), _world()
    one, two = [], []
    plans, errors = _broker(r1, one).publish_batch_by_dest(msgs)
    plans2, errors2 = _broker(r2, two, share_grouped=True).publish_batch_by_dest(msgs)
    assert plans2 == plans and errors2 == errors           # what share_on_device alone returns
    batches = [e for e in two if e[0] == "batch"]
    assert not any(e[0] == "deliver" for e in two) and len(batches) == len({e[1] for e in batches}) > 3
    flat = Counter((p, to, n) for _, p, items in batches for to, n in items) + \
        Counter((p, to, n) for k, p, to, n in [e for e in two if e[0] == "send"])
    assert flat == Counter(e[1:] for e in one) and len(one) > 30
    # share_send only for picks whose member is not local; every local pick inside its pid's list, in publish order
    assert all(not r2.member_is_local(e[1]) for e in two if e[0] == "send") and any(e[0] == "send" for e in two)
    by_pid = {p: items for _, p, items in batches}
    assert all([n for _, n in items] == sorted(n for _, n in items) for items in by_pid.values())
    local_picks = [(p, to, i) for g, rows in plans.items() if g not in ("n1", "n2") for i, to, p in rows
                   if isinstance(p, tuple) and p[0] == "n1"]
    assert local_picks and all((to, i) in by_pid[p] for p, to, i in local_picks)
    # the flag alone is refused; deliver_grouped beside share_on_device stays without effect
    with pytest.raises(ValueError):
        Broker(r1, share_grouped=True)
    assert Broker(r1).share_grouped is False
    three = []
    _broker(_world()[0], three, deliver_grouped=True).publish_batch_by_dest(msgs)
    assert three == one


def test_a_failed_deliver_batch_reaches_the_host_fallback():
    msgs = [Message(t, n) for n, t in enumerate(TOPICS)]
    (r1, _, _, _), (r2, _, _, ss2) = _world(), _world()
    base, log = [], []
    plans, _ = _broker(r1, base, share_grouped=True).publish_batch_by_dest(msgs)
    lost = [(g, i, to) for g, rows in plans.items() if g not in ("n1", "n2") for i, to, p in rows if p == A]
    assert len(lost) > 1
    plans2, _ = _broker(r2, log, fail={A}, share_grouped=True).publish_batch_by_dest(msgs)
    assert plans2["n1"] == plans["n1"]                      # the direct items are dropped, the plan is the same
    for g, rows in plans2.items():
        if g in ("n1", "n2"):
            continue
        for (i, to, p), (_, _, p0) in zip(rows, plans[g]):
            if p0 == A:                                      # dispatch/4 again with A in FailedSubs
                others = [q for q in ss2.subscribers(g, to) if q != A]
                assert p != A and (p in others if others else p == ("error", "no_subscribers"))
            else:
                assert p == p0
    # one more share_send per lost pick that has another member (to whichever member dispatch/4 picks then)
    resent = Counter((e[2], e[3]) for e in log if e[0] == "send") - Counter((e[2], e[3]) for e in base if e[0] == "send")
    assert sorted(resent.elements()) == sorted((to, i) for g, i, to in lost if [q for q in ss2.subscribers(g, to) if q != A])
    assert sum(1 for e in log if e[0] == "batch" and e[1] == A) == 1
