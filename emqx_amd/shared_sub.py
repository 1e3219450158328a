"""Shared subscriptions: the host side of the device's pick (include/tmatch.h
"Shared-subscription pick on the device").

``SharedSubs`` mirrors emqx_shared_sub's two tables -- the ?SHARED_SUBSCRIPTION
bag (keyed by group: ``subscribers(Group, Topic)`` is the group's insertion
order filtered by topic) and the local node's ?SHARED_SUBSCRIBER bag -- with
``subscribe/3`` / ``unsubscribe/3`` / a pid going down, the
round_robin_per_group counter rules, per-group strategy configuration, pid
interning and dense slot interning (one slot per {Group, Topic} pair, reused),
and tells an ``on_change`` hook what the device tables need.

Two references live here as well:

- ``SharedSubs.pick`` is a straight transcription of pick/6, do_pick/7 and
  pick_subscriber/6 (apps/emqx/src/emqx_shared_sub.erl:335-406) with
  FailedSubs: the host fallback after a failed send.
- ``pick_batch_ref`` is the numpy definition of tm_share_pick_dev.

The state word of a slot, as the device keeps it: round_robin's last Rem,
round_robin_per_group's counter, sticky's idx into the slot's member list.
"""
from __future__ import annotations

import numpy as np

NONE = UNDEF = 0xFFFFFFFF
RANDOM, ROUND_ROBIN, ROUND_ROBIN_PER_GROUP, STICKY, LOCAL, HASH_CLIENTID, HASH_TOPIC = range(7)
STRATEGIES = {"random": RANDOM, "round_robin": ROUND_ROBIN, "round_robin_per_group": ROUND_ROBIN_PER_GROUP,
              "sticky": STICKY, "local": LOCAL, "hash_clientid": HASH_CLIENTID, "hash_topic": HASH_TOPIC}
INITIAL_STICKY = ("random", "local", "hash_topic", "hash_clientid")
SUBSCRIBER_DOWN = "noproc"

_M32 = 0xFFFFFFFF


def mix(seed: int, a: int, b: int) -> int:
    """R(a, b) of include/tmatch.h on Python ints"""
    x = (seed ^ (a * 0x9E3779B1) ^ (b * 0x85EBCA77)) & _M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def mix_np(seed: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """R(a, b) on u32 arrays (as u64 words below 2^32)"""
    a = a.astype(np.uint64) & _M32
    b = b.astype(np.uint64) & _M32
    x = (np.uint64(seed & _M32) ^ ((a * np.uint64(0x9E3779B1)) & _M32) ^ ((b * np.uint64(0x85EBCA77)) & _M32)) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    x ^= x >> np.uint64(16)
    return x


def pick_batch_ref(n_dests, doff, topic, value, cap, slot_of, rec, pool, state, key_clientid=None, key_topic=None,
                   n_topics=0, seed=0):
    """The definition of tm_share_pick_dev in numpy.  rec: u32[4 * n_slots] (pos,
    cnt, n_local, meta per slot); state: u32[n_slots], not modified.
    -> (member u32[E], head (entries with a slot, entries with a pick), the
    state after the call)."""
    doff = np.asarray(doff, dtype=np.uint64)
    E = int(min(int(doff[n_dests + 1]), cap, 0xFFFFFFFF))
    slot_of = np.asarray(slot_of, dtype=np.uint32).reshape(-1)
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 4)
    pool = np.asarray(pool, dtype=np.uint32).reshape(-1)
    state = np.array(state, dtype=np.uint32).reshape(-1)
    n_slots = min(len(rec), len(state)) if len(rec) else 0
    t = np.asarray(topic[:E], dtype=np.uint32).astype(np.uint64)
    v = np.asarray(value[:E], dtype=np.uint32).astype(np.int64)
    member = np.full(E, NONE, dtype=np.uint32)
    if E == 0:
        return member, (0, 0), state
    s = np.full(E, NONE, dtype=np.uint64)
    if len(slot_of):
        inside = v < len(slot_of)
        s[inside] = slot_of[v[inside]]
    s[s >= n_slots] = NONE
    has = s != NONE
    si = np.where(has, s, 0).astype(np.int64)
    if n_slots:
        pos, cnt, nl, meta = (rec[si, k].astype(np.uint64) for k in range(4))
    else:
        pos = cnt = nl = meta = np.zeros(E, dtype=np.uint64)
    cnt = np.where(has & (pos + cnt <= len(pool)), cnt, 0)
    nl = np.minimum(nl, cnt)
    strat = meta & np.uint64(0xFF)
    init = (meta >> np.uint64(8)) & np.uint64(0xFF)
    pick = has & (cnt > 0) & (strat < 7)
    single = pick & (cnt == 1)
    active = pick & (cnt >= 2)
    ranked = active & ((strat == ROUND_ROBIN) | (strat == ROUND_ROBIN_PER_GROUP) | (strat == STICKY))

    def keys(k):
        out = np.zeros(E, dtype=np.uint64)
        if k is not None:
            k = np.asarray(k, dtype=np.uint32)
            ok = t < min(n_topics, len(k))
            out[ok] = k[t[ok].astype(np.int64)]
        return out

    safe = np.maximum(cnt, 1)
    r = mix_np(seed, t, s)
    kc, kt = keys(key_clientid), keys(key_topic)

    def stateless(st):
        """the idx of every entry under strategy byte st (an array); unknown: as RANDOM"""
        out = r % safe
        out = np.where(st == HASH_CLIENTID, kc % safe, out)
        out = np.where(st == HASH_TOPIC, kt % safe, out)
        loc = np.where(nl == 0, r % safe, np.where(nl == 1, 0, r % np.maximum(nl, 1)))
        return np.where(st == LOCAL, loc, out)

    idx = np.where(active & ~ranked, stateless(strat), 0).astype(np.uint64)
    new_state = state.copy()
    new_state[si[single & (strat == STICKY)]] = 0
    qs = np.nonzero(ranked)[0]
    if len(qs):
        order = qs[np.argsort(s[qs], kind="stable")]
        ss = s[order].astype(np.int64)
        pos_in = np.arange(len(order), dtype=np.int64)
        first = np.r_[True, ss[1:] != ss[:-1]]
        last = np.r_[ss[1:] != ss[:-1], True]
        start = np.maximum.accumulate(np.where(first, pos_in, 0))
        k = (pos_in - start).astype(np.uint64)
        c0 = state[ss].astype(np.uint64)
        n, st_, undef = cnt[order], strat[order], c0 == UNDEF
        rr0 = np.where(undef, mix_np(seed, np.full(len(order), NONE, dtype=np.uint64), ss.astype(np.uint64)) % n,
                       (c0 + 1) % n)
        pg0 = np.minimum(np.where(undef, 0, c0), n) % n
        init0 = stateless(init)[order[start]]          # the rank-0 entry's initial pick
        sk0 = np.where(c0 < n, c0, init0)
        base = np.where(st_ == ROUND_ROBIN, rr0, np.where(st_ == ROUND_ROBIN_PER_GROUP, pg0, sk0))
        ridx = np.where(st_ == STICKY, base, (base + k) % n)
        idx[order] = ridx
        after = np.where(st_ == ROUND_ROBIN_PER_GROUP, ridx + 1, ridx)
        new_state[ss[last]] = after[last].astype(np.uint32)
    got = single | active
    at = (pos + idx)[got].astype(np.int64)
    member[got] = pool[at]
    return member, (int(has.sum()), int(pick.sum())), new_state


class SharedSubs:
    """emqx_shared_sub's tables and calls on one node.

    node: this node's name; node_of(pid) -> the node a pid lives on (default:
    pid[0] of a (node, x) tuple, else this node).  router (optional): gets
    ``add_route(topic, (group, node))`` / ``delete_route(...)`` as
    handle_call({subscribe, ..}) / delete_route_if_needed do.  on_change(slot,
    member ids, n_local, meta, state or None): a slot's device tables changed
    (state None: leave the device's word alone).  state_reader(slot): reads the
    device's word back before a stateful pair's members change, so that a
    sticky idx follows its pid and a counter is what the device left."""

    def __init__(self, node="emqx@local", node_of=None, router=None, default_strategy="round_robin",
                 default_initial_sticky_pick="random", on_change=None, seed=0, state_reader=None):
        self.node = node
        self.node_of = node_of or (lambda pid: pid[0] if isinstance(pid, tuple) and len(pid) == 2 else node)
        self.router = router
        self.default_strategy = default_strategy
        self.default_initial = default_initial_sticky_pick
        self.group_strategy: dict = {}
        self.group_initial: dict = {}
        self.on_change = on_change
        self.state_reader = state_reader      # slot -> the device's state word (None: the host's tables are current)
        self.seed = seed
        self.bag: dict = {}            # ?SHARED_SUBSCRIPTION: group -> [(topic, pid)] in insertion order
        self.local: dict = {}          # ?SHARED_SUBSCRIBER: (group, topic) -> [pid] (a bag: no duplicates)
        self.rr_counter: dict = {}     # ?SHARED_SUBS_ROUND_ROBIN_COUNTER
        self.rr: dict = {}             # the publishing process's {shared_sub_round_robin, Group, Topic}
        self.sticky: dict = {}         # ... and {shared_sub_sticky, Group, Topic}
        self.monitored: set = set()
        self._pid_id: dict = {}
        self.pids: list = []
        self._slot: dict = {}          # (group, topic) -> slot
        self.slot_key: list = []       # slot -> (group, topic) or None
        self._free: list = []
        self._holds: dict = {}         # slot -> route keys on the device that carry it

    # ---- configuration
    def set_strategy(self, group, strategy, initial_sticky_pick=None):
        if strategy not in STRATEGIES:
            raise ValueError(f"unknown strategy {strategy!r}")
        if initial_sticky_pick is not None and initial_sticky_pick not in INITIAL_STICKY:
            raise ValueError(f"unknown initial_sticky_pick {initial_sticky_pick!r}")
        self.group_strategy[group] = strategy
        if initial_sticky_pick is not None:
            self.group_initial[group] = initial_sticky_pick
        for (g, t) in list(self._slot):
            if g == group:
                self._changed(g, t, None)

    def strategy(self, group):
        return self.group_strategy.get(group, self.default_strategy)

    def initial_sticky_pick(self, group):
        return self.group_initial.get(group, self.default_initial)

    def meta(self, group) -> int:
        return STRATEGIES[self.strategy(group)] | STRATEGIES[self.initial_sticky_pick(group)] << 8

    # ---- interning
    def pid_id(self, pid) -> int:
        i = self._pid_id.get(pid)
        if i is None:
            i = self._pid_id[pid] = len(self.pids)
            if i >= NONE:
                raise OverflowError("more than 2^32 - 1 interned pids")
            self.pids.append(pid)
        return i

    def slot(self, group, topic, create=False):
        s = self._slot.get((group, topic))
        if s is None and create:
            if self._free:
                s = self._free.pop()
                self.slot_key[s] = (group, topic)
            else:
                s = len(self.slot_key)
                self.slot_key.append((group, topic))
            self._slot[(group, topic)] = s
        return s

    @property
    def n_slots(self) -> int:
        return len(self.slot_key)

    # ---- the tables
    def subscribers(self, group, topic):
        """subscribers/2: ets:select on the bag -- the group's insertion order, filtered by topic"""
        return [p for t, p in self.bag.get(group, ()) if t == topic]

    def members(self, group, topic):
        """-> (the device's member list, n_local): subscribers/2's order; under the
        `local` strategy (or sticky picking initially by it) the members on this
        node first, so that the local prefix is contiguous"""
        subs = self.subscribers(group, topic)
        loc = [p for p in subs if self.node_of(p) == self.node]
        if "local" in (self.strategy(group), self.initial_sticky_pick(group) if self.strategy(group) == "sticky" else ""):
            return loc + [p for p in subs if self.node_of(p) != self.node], len(loc)
        n = 0
        while n < len(subs) and self.node_of(subs[n]) == self.node:
            n += 1
        return subs, n

    def device_state(self, group, topic):
        """the slot's state word as the device keeps it, from the host's tables"""
        st = self.strategy(group)
        if st == "round_robin":
            return self.rr.get((group, topic), UNDEF)
        if st == "round_robin_per_group":
            return self.rr_counter.get((group, topic), UNDEF)
        if st == "sticky":
            mem, _ = self.members(group, topic)
            p = self.sticky.get((group, topic))
            return mem.index(p) if p in mem else UNDEF
        return UNDEF

    def adopt_state(self, group, topic, word):
        """the device's state word back into the host's tables (before a host pick)"""
        st, key = self.strategy(group), (group, topic)
        if st == "round_robin":
            if word == UNDEF:
                self.rr.pop(key, None)
            else:
                self.rr[key] = int(word)
        elif st == "round_robin_per_group":
            self.rr_counter[key] = 0 if word == UNDEF else int(word)
        elif st == "sticky":
            mem, _ = self.members(group, topic)
            if word < len(mem):
                self.sticky[key] = mem[int(word)]
            else:
                self.sticky.pop(key, None)

    def _changed(self, group, topic, state):
        if self.on_change is None:
            return
        s = self.slot(group, topic)
        if s is None:
            return
        mem, n_local = self.members(group, topic)
        self.on_change(s, [self.pid_id(p) for p in mem], n_local, self.meta(group), state)

    def hold(self, group, topic) -> int:
        """One more route key carries the pair's slot (interned if need be): the
        slot is not handed to another pair while a key on the device names it."""
        s = self.slot(group, topic, create=True)
        self._holds[s] = self._holds.get(s, 0) + 1
        return s

    def release(self, group, topic):
        """One such key is gone; with the last one a pair without members gives its slot back."""
        s = self._slot.get((group, topic))
        if s is None:
            return
        self._holds[s] = self._holds.get(s, 0) - 1
        if self._holds[s] <= 0:
            del self._holds[s]
            if not self.subscribers(group, topic):
                self._retire(group, topic)

    def _retire(self, group, topic):
        s = self._slot.get((group, topic))
        if s is None:
            return
        if self._holds.get(s, 0) > 0:   # keys still name the slot: it stays the pair's, emptied
            self.rr.pop((group, topic), None)
            self.sticky.pop((group, topic), None)
            self._changed(group, topic, UNDEF)
            return
        del self._slot[(group, topic)]
        if self.on_change is not None:
            self.on_change(s, [], 0, self.meta(group), UNDEF)
        self.slot_key[s] = None
        self._free.append(s)
        self.rr.pop((group, topic), None)
        self.sticky.pop((group, topic), None)

    # ---- the calls (handle_call({subscribe | unsubscribe, ..}), 'DOWN')
    STATEFUL = ("round_robin", "round_robin_per_group", "sticky")

    def _sync(self, group, topic):
        """the device's state word of the pair into the host's tables, before they change"""
        if self.state_reader is None or self.strategy(group) not in self.STATEFUL:
            return
        s = self.slot(group, topic)
        if s is not None:
            self.adopt_state(group, topic, int(self.state_reader(s)))

    def subscribe(self, group, topic, pid):
        key = (group, topic)
        self._sync(group, topic)
        rows = self.bag.setdefault(group, [])
        if (topic, pid) not in rows:                     # (mria:dirty_write of an identical record: a bag keeps one)
            rows.append((topic, pid))
        fresh = self.slot(group, topic) is None
        self.slot(group, topic, create=True)
        moved = fresh                                    # (a reused slot gets its state set)
        need_route = False
        if self.node_of(pid) == self.node:
            need_route = key not in self.local
            # maybe_insert_round_robin_count: ets:insert of {GT, 0} -- it RESETS the counter
            if self.strategy(group) == "round_robin_per_group":
                self.rr_counter[key] = 0
                moved = True
            loc = self.local.setdefault(key, [])
            if pid not in loc:
                loc.append(pid)
            self.monitored.add(pid)
        # (sticky's word is an idx: it follows its pid through a list that changed)
        moved = moved or (self.strategy(group) == "sticky" and key in self.sticky)
        # the slot's members go out before the route's key can: a key never points at a list not yet set
        self._changed(group, topic, self.device_state(group, topic) if moved else None)
        if need_route and self.router is not None:
            self.router.add_route(topic, (group, self.node))

    def unsubscribe(self, group, topic, pid):
        key = (group, topic)
        self._sync(group, topic)
        rows = self.bag.get(group, [])
        if (topic, pid) in rows:
            rows.remove((topic, pid))
            if not rows:
                del self.bag[group]
        loc = self.local.get(key)
        was_local = loc is not None and pid in loc
        if was_local:
            loc.remove(pid)
            if not loc:
                del self.local[key]
        moved = False
        # delete_route_if_needed / maybe_delete_round_robin_count: if_no_more_subscribers
        if was_local and key not in self.local:
            if self.router is not None:
                self.router.delete_route(topic, (group, self.node))
            if self.strategy(group) == "round_robin_per_group":
                self.rr_counter.pop(key, None)
                moved = True
        if self.slot(group, topic) is None:
            return
        if not self.subscribers(group, topic):
            self._retire(group, topic)
            return
        moved = moved or (self.strategy(group) == "sticky" and key in self.sticky)
        self._changed(group, topic, self.device_state(group, topic) if moved else None)

    def down(self, pid):
        """cleanup_down/1: every record of the pid goes, as by unsubscribe"""
        for group in list(self.bag):
            for topic, p in list(self.bag.get(group, ())):
                if p == pid:
                    self.unsubscribe(group, topic, pid)
        self.monitored.discard(pid)

    # ---- pick/6, do_pick/7, pick_subscriber/6
    def _uniform(self, count, a, b):
        """rand:uniform(Count), made reproducible: 1 + R(a, b) % Count"""
        return 1 + mix(self.seed, a & _M32, b & _M32) % count

    def pick(self, group, topic, clientid_hash=0, topic_hash=0, failed=None, msg=0):
        """-> ('fresh' | 'retry', pid) or False.  clientid_hash / topic_hash: the
        BEAM's phash2 words; failed: FailedSubs {pid: reason}; msg: the
        message's index in its batch (what the device's R(t, s) hashes)."""
        failed = failed or {}
        strategy = self.strategy(group)
        if strategy == "sticky":
            key = (group, topic)
            sub0 = self.sticky.get(key)
            all_ = self._subscribers_alive(group, topic, failed)
            if sub0 is not None and sub0 not in failed and sub0 in all_:      # is_active_sub/3
                return ("fresh", sub0)
            failed1 = dict(failed)
            failed1[sub0] = SUBSCRIBER_DOWN
            res = self._do_pick(all_, self.initial_sticky_pick(group), clientid_hash, topic_hash, group, topic, failed1,
                                msg)
            if res:
                self.sticky[key] = res[1]
            return res
        all_ = self._subscribers_alive(group, topic, failed)
        return self._do_pick(all_, strategy, clientid_hash, topic_hash, group, topic, failed, msg)

    def _subscribers_alive(self, group, topic, failed):
        """subscribers/3: the members (in the device's order) that are not down"""
        mem, _ = self.members(group, topic)
        return [p for p in mem if failed.get(p, False) != SUBSCRIBER_DOWN]

    def _do_pick(self, all_, strategy, ch, th, group, topic, failed, msg):
        if not all_:
            return False
        subs = [p for p in all_ if p not in failed]
        if not subs:
            return ("retry", self._pick_subscriber(group, topic, strategy, ch, th, all_, msg))
        return ("fresh", self._pick_subscriber(group, topic, strategy, ch, th, subs, msg))

    def _pick_subscriber(self, group, topic, strategy, ch, th, subs, msg):
        if len(subs) == 1:
            return subs[0]
        if strategy == "local":
            loc = [p for p in subs if self.node_of(p) == self.node]
            return self._pick_subscriber(group, topic, "random", ch, th, loc or subs, msg)
        return subs[self._do_pick_subscriber(group, topic, strategy, ch, th, len(subs), msg) - 1]

    def _do_pick_subscriber(self, group, topic, strategy, ch, th, count, msg):
        key = (group, topic)
        s = self._slot.get(key, NONE)
        if strategy == "random":
            return self._uniform(count, msg, s)
        if strategy == "hash_clientid":
            return 1 + ch % count
        if strategy == "hash_topic":
            return 1 + th % count
        if strategy == "round_robin":
            n = self.rr.get(key)
            rem = self._uniform(count, NONE, s) - 1 if n is None else (n + 1) % count
            self.rr[key] = rem
            return rem + 1
        if strategy == "round_robin_per_group":
            # ets:update_counter(.., {2, 1, Count, 1}, {.., 0})
            c = self.rr_counter.get(key, 0) + 1
            if c > count:
                c = 1
            self.rr_counter[key] = c
            return c
        raise ValueError(f"unknown strategy {strategy!r}")
