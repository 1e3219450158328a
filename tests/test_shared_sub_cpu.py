"""SharedSubs on the CPU: its two tables against a scripted sequence of
subscribe, unsubscribe and down events (the ?SHARED_SUBSCRIPTION bag is keyed
by group: subscribers/2 is the group's insertion order filtered by topic), the
route add / delete calls, slot interning with reuse (a reused slot gets its
state set), what the on_change hook is told, and the host fallback pick with
FailedSubs (the failed pid excluded, {retry, _} when every member failed)."""
from emqx_amd import shared_sub
from emqx_amd.shared_sub import SUBSCRIBER_DOWN, UNDEF, SharedSubs


class StubRouter:
    def __init__(self):
        self.calls = []

    def add_route(self, topic, dest):
        self.calls.append(("add", topic, dest))

    def delete_route(self, topic, dest):
        self.calls.append(("delete", topic, dest))


def _subs(**kw):
    log, router = [], StubRouter()
    s = SharedSubs(node="n1", router=router, on_change=lambda *a: log.append(a), **kw)
    return s, log, router


def test_tables_follow_a_scripted_sequence():
    s, log, router = _subs()
    a, b, c, r = ("n1", "a"), ("n1", "b"), ("n1", "c"), ("n2", "r")
    s.subscribe(b"g", b"t/1", a)
    s.subscribe(b"g", b"t/2", b)
    s.subscribe(b"g", b"t/1", r)
    s.subscribe(b"g", b"t/1", c)
    s.subscribe(b"h", b"t/1", b)
    s.subscribe(b"g", b"t/1", a)                                  # an identical record: the bag keeps one
    assert s.bag[b"g"] == [(b"t/1", a), (b"t/2", b), (b"t/1", r), (b"t/1", c)]
    assert s.subscribers(b"g", b"t/1") == [a, r, c] and s.subscribers(b"g", b"t/2") == [b]
    assert s.local == {(b"g", b"t/1"): [a, c], (b"g", b"t/2"): [b], (b"h", b"t/1"): [b]}
    # one route per {Group, Topic} with a local member, added with the first
    assert router.calls == [("add", b"t/1", (b"g", "n1")), ("add", b"t/2", (b"g", "n1")), ("add", b"t/1", (b"h", "n1"))]
    s.unsubscribe(b"g", b"t/1", a)
    assert len(router.calls) == 3 and s.subscribers(b"g", b"t/1") == [r, c]
    s.unsubscribe(b"g", b"t/1", c)                                # the last local one: delete_route_if_needed
    assert router.calls[-1] == ("delete", b"t/1", (b"g", "n1")) and s.subscribers(b"g", b"t/1") == [r]
    assert (b"g", b"t/1") not in s.local
    s.down(b)                                                     # cleanup_down/1: every record of the pid
    assert s.subscribers(b"g", b"t/2") == [] and s.subscribers(b"h", b"t/1") == [] and b"h" not in s.bag
    assert router.calls[-2:] == [("delete", b"t/2", (b"g", "n1")), ("delete", b"t/1", (b"h", "n1"))]
    assert b not in s.monitored and s.bag == {b"g": [(b"t/1", r)]}


def test_slots_are_dense_reused_and_a_reused_slot_gets_its_state():
    s, log, _ = _subs()
    a, b = ("n1", "a"), ("n1", "b")
    s.subscribe(b"g", b"x", a)
    s.subscribe(b"g", b"y", a)
    s.subscribe(b"g", b"x", b)
    assert (s.slot(b"g", b"x"), s.slot(b"g", b"y"), s.n_slots) == (0, 1, 2)
    ida, idb = s.pid_id(a), s.pid_id(b)
    meta = shared_sub.ROUND_ROBIN | shared_sub.RANDOM << 8
    # (slot, member ids, n_local, meta, state): a fresh slot's state is set, a later change leaves it alone
    assert log == [(0, [ida], 1, meta, UNDEF), (1, [ida], 1, meta, UNDEF), (0, [ida, idb], 2, meta, None)]
    s.unsubscribe(b"g", b"y", a)                                  # its last member: the slot is retired, emptied
    assert log[-1] == (1, [], 0, meta, UNDEF) and s.slot(b"g", b"y") is None and s.slot_key[1] is None
    s.rr[(b"g", b"z")] = 4                                        # (what a host pick left for the pair)
    s.subscribe(b"g", b"z", b)
    assert s.slot(b"g", b"z") == 1 and s.n_slots == 2             # reused, and its state set
    assert log[-1] == (1, [idb], 1, meta, 4)
    assert s.pid_id(a) == ida and s.pids[idb] == b                # interned once


def test_strategy_configuration_and_member_order():
    s, log, _ = _subs()
    loc1, rem, loc2 = ("n1", 1), ("n2", 2), ("n1", 3)
    for p in (rem, loc1, loc2):
        s.subscribe(b"g", b"t", p)
    assert s.members(b"g", b"t") == ([rem, loc1, loc2], 0)        # subscribers/2's order: round robin's parity
    s.set_strategy(b"g", "local")
    assert s.members(b"g", b"t") == ([loc1, loc2, rem], 2)        # the members on this node first
    assert log[-1] == (0, [s.pid_id(p) for p in (loc1, loc2, rem)], 2, shared_sub.LOCAL | shared_sub.RANDOM << 8, None)
    s.set_strategy(b"g", "sticky", "hash_topic")
    assert s.meta(b"g") == shared_sub.STICKY | shared_sub.HASH_TOPIC << 8
    assert s.strategy(b"other") == "round_robin" and s.initial_sticky_pick(b"other") == "random"


def test_the_host_fallback_excludes_failed_pids():
    s, _, _ = _subs()
    a, b, c = ("n1", "a"), ("n1", "b"), ("n2", "c")
    for p in (a, b, c):
        s.subscribe(b"g", b"t", p)
    s.rr[(b"g", b"t")] = 0
    assert s.pick(b"g", b"t") == ("fresh", b)                     # Rem 1 of [a, b, c]
    # the send to b failed: dispatch/4 recurses with b in FailedSubs -- Rem 2 of the remaining [a, c] wraps to a
    assert s.pick(b"g", b"t", failed={b: "nack"}) == ("fresh", a)
    assert s.pick(b"g", b"t", failed={a: "x", b: "x", c: "x"})[0] == "retry"      # all offline? pick one anyway
    assert s.pick(b"g", b"t", failed={a: SUBSCRIBER_DOWN, b: SUBSCRIBER_DOWN}) == ("fresh", c)   # [Sub] -> Sub
    assert s.pick(b"g", b"t", failed={a: SUBSCRIBER_DOWN, b: SUBSCRIBER_DOWN, c: SUBSCRIBER_DOWN}) is False
    assert s.pick(b"nobody", b"t") is False


def test_sticky_keeps_its_member_while_it_is_one():
    s, log, _ = _subs(default_strategy="sticky", default_initial_sticky_pick="hash_clientid")
    a, b, c = ("n1", "a"), ("n1", "b"), ("n1", "c")
    for p in (a, b, c):
        s.subscribe(b"g", b"t", p)
    assert s.pick(b"g", b"t", clientid_hash=7) == ("fresh", b)    # 1 + 7 rem 3
    assert s.pick(b"g", b"t", clientid_hash=8) == ("fresh", b)    # remembered
    assert s.device_state(b"g", b"t") == 1
    s.unsubscribe(b"g", b"t", a)                                  # the idx follows its pid through the list
    assert log[-1][1] == [s.pid_id(b), s.pid_id(c)] and log[-1][4] == 0
    assert s.pick(b"g", b"t", failed={b: "nack"}) == ("fresh", c)  # not active: picked anew and remembered
    assert s.sticky[(b"g", b"t")] == c
    s.unsubscribe(b"g", b"t", c)
    assert log[-1][4] == UNDEF                                    # the remembered member left: no idx
    s.adopt_state(b"g", b"t", 0)
    assert s.sticky[(b"g", b"t")] == b


# ---- the layers above: Tab's shipping order, the Broker fed picks

def test_tab_ships_slot_and_members_before_the_key_and_clears_the_slot_with_it():
    from emqx_amd.topic_index import Tab
    from emqx_amd.trie_search import filter as tfilter, get_id, make_key

    class Index:
        def __init__(self):
            self.log = []

        def set_share_members(self, slots, lists, n_local, meta):
            self.log.append(("members", list(slots), [list(x) for x in lists], list(n_local), list(meta)))

        def share_state_set(self, slots, states):
            self.log.append(("state", list(slots), list(states)))

        def set_share_slots(self, values, slots):
            self.log.append(("slots", values.tolist(), slots.tolist()))

        def apply(self, ops, blob, offs, vals, flags, commit=False):
            self.log.append(("apply", ops.tolist(), vals.tolist()))
            return 1

        def epoch(self):
            return 1, 1

    ix = Index()
    tab = Tab(index=ix)
    tab.share_fn = lambda key: 7 if isinstance(get_id(key), tuple) else None
    kg1, kg2 = make_key(tfilter(b"a/+"), (b"g", "n1")), make_key(tfilter(b"a/+"), (b"g", "n2"))
    kn = make_key(tfilter(b"a/+"), "n1")
    tab.insert_key(kg1, [])                              # queued first ...
    tab.set_share_members(7, [4, 5], 1, shared_sub.ROUND_ROBIN)
    tab.set_share_state(7, UNDEF)
    tab.insert_key(kn, [])                               # a plain node route: no slot
    tab.insert_key(kg2, [])                              # the pair's second key shares the slot
    tab.flush()
    # ... and still shipped last: members, state, slots, then the inserts
    assert ix.log == [("members", [7], [[4, 5]], [1], [shared_sub.ROUND_ROBIN]), ("state", [7], [UNDEF]),
                      ("slots", [0, 2], [7, 7]), ("apply", [1, 1, 1], [0, 1, 2])]
    tab.delete_key(kg1)
    tab.delete_key(kn)
    tab.flush()
    assert ix.log[4:] == [("slots", [0], [UNDEF]), ("apply", [0, 0], [0, 1])]      # the slot is cleared with the key


def test_the_router_hooks_ship_members_before_the_route():
    """Router(shared_subs=...) over a stub mirror: a subscribe ships the slot's
    list, then the route's key with its slot; an exact-topic pair stays on the host"""
    from emqx_amd.router import Router
    from emqx_amd import topic_index as ti

    class Mirror:
        def __init__(self):
            self.dest_fn = self.filter_fn = self.filter_release = self.sub_fn = self.share_fn = None
            self.keys, self.log = {}, []

        def sync_keys(self, keys, present, commit=False):
            for k, here in zip(keys, present):
                if here and k not in self.keys:
                    self.keys[k] = self.share_fn(k)
                    self.log.append(("insert", ti.get_topic(k), ti.get_id(k), self.keys[k]))
                elif not here and k in self.keys:
                    del self.keys[k]
                    self.filter_release(k)
                    self.log.append(("delete", ti.get_topic(k), ti.get_id(k)))

        def set_share_members(self, slot, ids, n_local, meta):
            self.log.append(("members", slot, list(ids), n_local))

        def set_share_state(self, slot, state):
            self.log.append(("state", slot, state))

        def share_state(self, slots, dev=0):             # (read back before a stateful pair's members change)
            return [UNDEF for _ in slots]

    m = Mirror()
    ss = SharedSubs(node="n1")
    r = Router(node="n1", mirror=m, shared_subs=ss)
    a, b = ("n1", "a"), ("n2", "b")
    ss.subscribe(b"g", b"t/+", a)
    assert m.log == [("members", 0, [0], 1), ("state", 0, UNDEF), ("insert", b"t/+", (b"g", "n1"), 0)]
    r.add_route(b"t/+", (b"g", "n2"))                    # the other node's route of the pair: the same slot
    ss.subscribe(b"g", b"t/+", b)
    assert m.log[3:] == [("insert", b"t/+", (b"g", "n2"), 0), ("members", 0, [0, 1], 1)]
    r.add_route(b"t/+", "n2")
    assert m.log[-1] == ("insert", b"t/+", "n2", None)
    ss.subscribe(b"g", b"exact", a)                      # an exact topic: the bag's row, nothing on the device
    assert len(m.log) == 6 and (b"g", "n1") in r._bag[b"exact"]
    r.set_share_state(ss.slot(b"g", b"exact"), 3)
    assert r.share_state(ss.slot(b"g", b"exact")) == 3
    ss.unsubscribe(b"g", b"t/+", a)                      # the last local member: the route goes, then the list
    assert m.log[6:] == [("delete", b"t/+", (b"g", "n1")), ("members", 0, [1], 0)]


def test_broker_fed_picks_sends_them_and_falls_back_when_a_send_fails():
    from emqx_amd.broker import Broker, Message
    from emqx_amd.router import ByDest, Route

    ss = SharedSubs(node="n1", default_strategy="round_robin")
    a, b, c = ("n1", "a"), ("n1", "b"), ("n1", "c")
    for p in (a, b, c):
        ss.subscribe(b"g", b"t/+", p)
    ss.subscribe(b"solo", b"t/+", a)
    slot = ss.slot(b"g", b"t/+")

    class StubRouter:
        node, shared_subs = "n1", ss
        state = {slot: 1}                                # what the device left: the last pick was idx 1 (b)
        wrote = []

        def match_routes_publish(self, topics, kc, kt, seed=0, errors="raise"):
            by = ByDest()
            by[b"g"] = [(0, Route(b"t/+", (b"g", "n1"))), (1, Route(b"t/+", (b"g", "n1")))]
            by[b"solo"] = [(0, Route(b"t/+", (b"solo", "n1")))]
            by[b"none"] = [(1, Route(b"t/+", (b"none", "n2")))]
            by["n2"] = [(0, Route(b"t/+", "n2"))]
            picks = {b"g": [(0, b"t/+", a), (1, b"t/+", b)], b"solo": [(0, b"t/+", a)], b"none": [(1, b"t/+", None)]}
            return by, [], picks

        def share_state(self, s):
            return self.state.get(s, UNDEF)

        def set_share_state(self, s, w):
            self.state[s] = w
            self.wrote.append((s, w))

    sent, fwd = [], []

    def share_send(pid, to, msg):
        sent.append((pid, to, msg.payload))
        return "nack" if pid == b else "ok"

    br = Broker(StubRouter(), share_on_device=True, share_send=share_send,
                forward=lambda n, to, m: fwd.append((n, to, m.payload)) or "ok",
                share_dispatch=lambda g, to, m: 1 / 0)   # never called
    plans, errors = br.publish_batch_by_dest([Message(b"t/x", "m0"), Message(b"t/y", "m1")])
    # message 1's pick b refused: dispatch/4 again with b in FailedSubs -- Rem (1 + 1) rem 2 of [a, c] is a
    assert sent == [(a, b"t/+", "m0"), (b, b"t/+", "m1"), (a, b"t/+", "m1"), (a, b"t/+", "m0")]
    assert plans[b"g"] == [(0, b"t/+", a), (1, b"t/+", a)] and plans[b"solo"] == [(0, b"t/+", a)]
    assert plans[b"none"] == [(1, b"t/+", ("error", "no_subscribers"))]
    assert plans["n2"] == [(0, b"t/+", "ok")] and fwd == [("n2", b"t/+", "m0")] and errors == {}
    assert StubRouter.wrote == [(slot, 0)] and ss.rr[(b"g", b"t/+")] == 0     # the state read, advanced, written back


def test_the_last_member_of_a_wildcard_pair_leaves_through_a_real_tab():
    """Router + SharedSubs over a real Tab (a stub index under it): the pair's last
    member unsubscribes, its last key goes, the slot is given back and emptied --
    the slot cleared with the key first, then the list -- and nothing waits for
    the table's lock; the same when the pair's last REMOTE key goes later"""
    import threading
    from emqx_amd.router import Router
    from emqx_amd.topic_index import Tab

    class Index:
        def __init__(self):
            self.log = []

        def set_share_members(self, slots, lists, n_local, meta):
            self.log.append(("members", list(slots), [list(x) for x in lists]))

        def share_state_set(self, slots, states):
            self.log.append(("state", list(slots), list(states)))

        def share_state_get(self, slots, dev=0):
            return [UNDEF for _ in slots]

        def set_share_slots(self, values, slots):
            self.log.append(("slots", values.tolist(), slots.tolist()))

        def set_dests(self, values, dests):
            pass

        def set_route_filters(self, values, ids):
            pass

        def apply(self, ops, blob, offs, vals, flags, commit=False):
            self.log.append(("apply", ops.tolist(), vals.tolist()))
            return 1

        def epoch(self):
            return 1, 1

    ix = Index()
    tab = Tab(index=ix)
    ss = SharedSubs(node="n1")
    r = Router(node="n1", mirror=tab, shared_subs=ss)
    a = ("n1", "a")
    done = []

    def script():
        ss.subscribe(b"g", b"t/+", a)
        tab.flush()
        assert ix.log == [("members", [0], [[0]]), ("state", [0], [UNDEF]), ("slots", [0], [0]), ("apply", [1], [0])]
        del ix.log[:]
        ss.unsubscribe(b"g", b"t/+", a)                  # the last member, the last key
        tab.flush()
        assert ix.log == [("slots", [0], [UNDEF]), ("apply", [0], [0]), ("members", [0], [[]]), ("state", [0], [UNDEF])]
        assert ss.slot(b"g", b"t/+") is None and ss._holds == {}
        # a pair known only through another node's route: its key holds the slot, its delete gives it back
        del ix.log[:]
        r.add_route(b"u/#", (b"g", "n2"))
        assert ss.slot(b"g", b"u/#") == 0 and ss._holds == {0: 1}
        r.delete_route(b"u/#", (b"g", "n2"))
        tab.flush()
        assert ss.slot(b"g", b"u/#") is None and ss._holds == {}
        shipped = [e for e in ix.log if e[0] in ("slots", "members")]
        assert shipped == [("slots", [0], [0]), ("slots", [0], [UNDEF]), ("members", [0], [[]])]   # (the key's u32 is reused)
        done.append(True)

    t = threading.Thread(target=script, daemon=True)     # (a deadlock must fail the test, not hang the suite)
    t.start()
    t.join(timeout=20)
    assert done == [True], "the script did not finish: an assertion above failed, or it waits for the table's lock"
