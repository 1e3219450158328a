"""The local subscriber tables of ``emqx_broker``, and their device lists.

apps/emqx/src/emqx_broker.erl keeps, per node, the bag ``?SUBSCRIBER``
(:182-193, :637-705): ``{Topic, SubPid}`` rows, and for a topic with many
subscribers ``{Topic, {shard, I}}`` rows that point at ``{{shard, Topic, I},
SubPid}`` rows.  Which of the two a subscribe writes is
``emqx_broker_helper:get_sub_shard/2`` (emqx_broker_helper.erl:87-92): the
topic's subscriber sequence (``create_seq/1``, given back by ``reclaim_seq/1``
on unsubscribe) up to 1024 -> shard 0, the plain row; beyond it -> shard
``phash2(SubPid, shards_num()) + 1``.  ``do_dispatch2/2`` (:726-760) folds over
``subscribers(Topic)`` in the bag's order and expands a shard row where it
stands.

``LocalSubs`` is that bag (``?SUBOPTION`` only as far as it remembers a
subscription's shard) plus what the device needs: every pid interned to a u32,
and ``dispatch_order(Topic)`` -- the flat pid list do_dispatch2/2 visits --
handed to ``on_change`` after every write, so the Router can keep the device
list of the route key ``{Filter, node()}`` current (tm_set_subscribers).
``is_process_alive/1`` is not mirrored: every subscribed pid counts as alive.
"""
from __future__ import annotations

import threading
import zlib

SHARD = 1024          # emqx_broker_helper.erl ?SHARD
SHARDS_NUM = 32       # shards_num(): schedulers x 32 in the reference; any positive number serves


def phash(pid, n: int) -> int:
    """stands in for erlang:phash2(SubPid, N): stable per pid, in [0, N)"""
    return zlib.crc32(repr(pid).encode()) % n


class LocalSubs:
    def __init__(self, shards: int = SHARDS_NUM, shard_after: int = SHARD):
        self.shards = shards
        self.shard_after = shard_after
        self._bag: dict = {}        # ?SUBSCRIBER: key -> {object: None}, a bag in insertion order
        self._seq: dict = {}        # emqx_broker_helper's sequence per topic
        self._shard: dict = {}      # ?SUBOPTION's shard of (Topic, SubPid)
        self._ids: dict = {}        # pid -> u32
        self._pids: list = []       # u32 -> pid
        self._lock = threading.RLock()
        self.on_change = None       # on_change(topic): the topic's rows changed

    # ---- pid <-> u32
    def sub_id(self, pid) -> int:
        with self._lock:
            i = self._ids.get(pid)
            if i is None:
                if len(self._pids) > 0xFFFFFFFF:
                    raise OverflowError("more than 2^32 subscriber ids")
                i = self._ids[pid] = len(self._pids)
                self._pids.append(pid)
            return i

    def pid_of(self, sub_id: int):
        return self._pids[sub_id]

    # ---- the bag
    def _insert(self, key, obj):
        self._bag.setdefault(key, {})[obj] = None

    def _delete_object(self, key, obj):
        rows = self._bag.get(key)
        if rows is not None and obj in rows:
            del rows[obj]
            if not rows:
                del self._bag[key]

    def subscribe(self, topic, pid):
        """do_subscribe/3 (:182-193) and the pool worker's {subscribe, ..} (:637-675)"""
        topic = bytes(topic)
        with self._lock:
            if (topic, pid) in self._shard:
                return "ok"            # subscribe/3: already in ?SUBOPTION
            seq = self._seq[topic] = self._seq.get(topic, 0) + 1          # create_seq/1
            i = 0 if seq <= self.shard_after else phash(pid, self.shards) + 1   # get_sub_shard/2
            self._shard[(topic, pid)] = i
            self.sub_id(pid)
            if i == 0:
                self._insert(topic, pid)
            else:
                if ("shard", topic, i) not in self._bag:
                    self._insert(topic, ("shard", i))
                self._insert(("shard", topic, i), pid)
        self._changed(topic)
        return "ok"

    def unsubscribe(self, topic, pid):
        """do_unsubscribe2/3 and the worker's {unsubscribed, ..} (:683-705)"""
        topic = bytes(topic)
        with self._lock:
            i = self._shard.pop((topic, pid), None)
            if i is None:
                return "ok"
            left = self._seq.get(topic, 0) - 1                            # reclaim_seq/1
            if left > 0:
                self._seq[topic] = left
            else:
                self._seq.pop(topic, None)
            if i == 0:
                self._delete_object(topic, pid)
            else:
                self._delete_object(("shard", topic, i), pid)
                if ("shard", topic, i) not in self._bag:
                    self._delete_object(topic, ("shard", i))
        self._changed(topic)
        return "ok"

    def subscribers(self, key):
        """subscribers/1: ets:lookup_element(?SUBSCRIBER, Key, 2), [] for no row;
        Key is a topic or ("shard", Topic, I)"""
        if not isinstance(key, tuple):
            key = bytes(key)
        with self._lock:
            return list(self._bag.get(key, ()))

    def dispatch_order(self, topic):
        """the pids do_dispatch2/2 sends {deliver, Topic, Msg} to, in its order"""
        topic = bytes(topic)
        out = []
        with self._lock:
            for sub in self._bag.get(topic, ()):
                if isinstance(sub, tuple) and len(sub) == 2 and sub[0] == "shard":
                    out.extend(self._bag.get(("shard", topic, sub[1]), ()))
                else:
                    out.append(sub)
        return out

    def dispatch_ids(self, topic):
        """dispatch_order as the u32s the device list holds"""
        with self._lock:
            return [self._ids[p] for p in self.dispatch_order(topic)]

    def topics(self):
        with self._lock:
            return [k for k in self._bag if not isinstance(k, tuple)]

    def _changed(self, topic):
        if self.on_change is not None:
            self.on_change(topic)
