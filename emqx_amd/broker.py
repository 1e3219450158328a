"""Broker publish micro-batching on the MI355X index.

The reference routes every PUBLISH on its own: ``emqx_broker:do_publish/1``
(apps/emqx/src/emqx_broker.erl:293-298) = ``route(aggre(match_routes(Topic)),
Delivery)``, called once per ``{incoming, Packet}`` by the connection process
(emqx_connection.erl:585-587, 802-807).  Here publishes are collected into a
micro-batch -- flushed when it holds ``max_batch`` messages or when the oldest
has waited ``max_wait_ms`` -- and the whole batch is matched with ONE
``Router.match_routes_batch`` (one device launch); ``aggre/1`` (:408-424) and
the per-route dispatch (do_route2, :400-406) then run per message exactly as
in the reference, so each message gets the same route list and the same
deliveries as an unbatched publish.

Delivery itself (sessions, cluster RPC) is out of scope: ``dispatch(To,
Msg)``, ``forward(Node, To, Msg)`` and ``share_dispatch(Group, To, Msg)`` are
caller-supplied callbacks.  With ``share_on_device`` the shared-subscription
pick of emqx_shared_sub:dispatch/3 has run on the device too, and the callback
is ``share_send(SubPid, To, Msg)``; a failed send falls back to the
reference's dispatch/4 recursion on the host (SharedSubs.pick with FailedSubs).  With
``dispatch_on_device`` the local node's ``dispatch/2`` -- the ?SUBSCRIBER
lookups of do_dispatch2/2 (:726-760) -- has run on the device as well, and the
callback is ``deliver(SubPid, To, Msg)``, the ``SubPid ! {deliver, To, Msg}``.
"""
from __future__ import annotations

import threading
import time
from collections import namedtuple
from concurrent.futures import Future

from .trie_search import term_key

Message = namedtuple("Message", "topic payload")


def aggre(routes):
    """aggre/1 (emqx_broker.erl:408-424): routes -> [{To, Node} | {To, Group}].
    Plain node routes come out in reverse order (accumulated by prepending);
    if any destination is a shared group, the result is lists:usort'ed."""
    if not routes:
        return []
    if len(routes) == 1:
        r = routes[0]
        if isinstance(r.dest, tuple):
            return [(r.topic, r.dest[0])]
        return [(r.topic, r.dest)]
    acc, dedup = [], False
    for r in routes:
        if isinstance(r.dest, tuple):
            dedup = True
            acc.insert(0, (r.topic, r.dest[0]))
        else:
            acc.insert(0, (r.topic, r.dest))
    if dedup:
        return sorted(set(acc), key=term_key)
    return acc


class Broker:
    def __init__(self, router, node=None, dispatch=None, forward=None, share_dispatch=None,
                 max_batch: int = 4096, max_wait_ms: float = 0.2, start: bool = False,
                 aggre_on_device: bool = False, dispatch_on_device: bool = False, deliver=None,
                 share_on_device: bool = False, share_send=None, share_keys=None, share_seed: int = 0,
                 deliver_grouped: bool = False, deliver_batch=None, share_grouped: bool = False):
        """aggre_on_device: publish_batch_by_dest asks the router for buckets
        the device has already applied aggre/1 to (TM_ROUTE_AGGRE).
        dispatch_on_device: publish_batch_by_dest asks the router for the local
        node's deliveries too (Router.match_routes_dispatch); the local node's
        plan is then [(message index, To, subscriber)], each handed to
        deliver(subscriber, To, message), and dispatch is not called.
        share_on_device: publish_batch_by_dest asks the router for the picks
        as well (Router.match_routes_publish: aggre/1, the local dispatch and
        the pick in one device call); a group's plan is then [(message index,
        To, pid)], each handed to share_send(pid, To, message) -> "ok" or an
        error reason, and share_dispatch is not called.  share_keys(message) ->
        (phash2(ClientId), phash2(Topic)) for the two hash strategies (default:
        zeros); share_seed: the seed of the batch's random picks.
        deliver_grouped: publish_batch_by_dest asks the router for the local
        node's deliveries grouped by subscriber as well
        (Router.match_routes_deliver) and calls deliver_batch(SubPid, [(To,
        message)]) once per subscriber per batch, the list in publish order --
        what the connection process gathers from its mailbox
        (emqx_connection.erl:611-612) -- in place of one deliver per delivery.
        What publish_batch_by_dest returns is unchanged.
        share_grouped (needs share_on_device; deliver_grouped beside
        share_on_device alone stays without effect): publish_batch_by_dest asks
        the router for the local picks grouped with the local deliveries
        (Router.match_routes_publish_deliver).  Each local subscriber then gets
        ONE deliver_batch(SubPid, [(To, message)]) per batch, direct and picked
        items together in publish order, and share_send is called only for picks
        whose member is not a connection of this node.  A deliver_batch that
        returns a reason other than None or "ok" (a dead pid): the subscriber's
        picked items re-enter the host's dispatch/4 recursion with the pid in
        FailedSubs, its direct items are dropped, as do_dispatch2 drops them.
        What publish_batch_by_dest returns is what share_on_device alone returns."""
        if share_grouped and not share_on_device:
            raise ValueError("share_grouped needs share_on_device")
        self.share_grouped = share_grouped
        self.deliver_grouped = deliver_grouped
        self.deliver_batch = deliver_batch or (lambda sub, items: None)
        self.share_on_device = share_on_device
        self.share_send = share_send or (lambda pid, to, msg: "ok")
        self.share_keys = share_keys or (lambda msg: (0, 0))
        self.share_seed = share_seed
        self.router = router
        self.aggre_on_device = aggre_on_device
        self.dispatch_on_device = dispatch_on_device
        self.deliver = deliver or (lambda sub, to, msg: None)
        self.node = router.node if node is None else node
        self.dispatch = dispatch or (lambda to, msg: 0)
        self.forward = forward or (lambda node, to, msg: "ok")
        self.share_dispatch = share_dispatch or (lambda group, to, msg: 0)
        self.max_batch = max_batch
        self.max_wait = max_wait_ms / 1000.0
        self.batches = 0
        self._q: list = []
        self._first_at = None
        self._cv = threading.Condition()
        self._stop = False
        self._thread = None
        if start:
            self._thread = threading.Thread(target=self._loop, daemon=True)
            self._thread.start()

    # do_route2/2 (emqx_broker.erl:400-406)
    def _route2(self, to_dest, msg):
        to, dest = to_dest
        if dest == self.node:
            return (dest, to, self.dispatch(to, msg))
        if isinstance(dest, str):
            return (dest, to, self.forward(dest, to, msg))
        return ("share", to, self.share_dispatch(dest, to, msg))

    def publish_batch(self, msgs):
        """do_publish/1 for every message of a batch, with one device match.
        -> per message: (routes after aggre, route results), or the exception
        of a message whose topic is invalid (badarg): it fails alone, the
        other messages of the batch are routed (emqx_trie_search.erl:374-375
        raises in the one publishing process)."""
        if not msgs:
            return []
        all_routes = self.router.match_routes_batch([m.topic for m in msgs], errors="return")
        self.batches += 1
        out = []
        for m, routes in zip(msgs, all_routes):
            if isinstance(routes, Exception):
                out.append(routes)
                continue
            agg = aggre(routes)
            out.append((agg, [self._route2(r, m) for r in agg]))
        return out

    def publish_batch_by_dest(self, msgs):
        """do_publish/1 for a micro-batch, destination-major: the routes come
        from Router.match_routes_by_dest (matched and bucketed on the device),
        so each destination gets ONE plan for the whole batch -- the
        (message, To) pairs do_route2/2 (emqx_broker.erl:401-406) would
        dispatch, forward (forward/4, :429) or hand to the shared group one
        hit at a time.  A group's plan is deduplicated per message on
        (To, Group), which is what aggre/1's usort does to a message's routes
        (:412-424; node routes are unique per message as they are).
        -> (plans, errors): plans = {destination: [(message index, To,
        result)]}, the destination being what aggre/1 names (a node, or the
        group); errors = {message index: exception} for invalid topics, which
        fail alone as in publish_batch.  Every plan is in message order.
        As in aggre/1, every ("external", X) destination goes into the one
        plan "external"; and, as in do_route2/2, a destination is told apart
        by its name only, so a node and a group must not share one (a class
        is taken for a group when its first route's dest is a pair).  The
        deliveries are the same
        (destination, To, message) multiset as publish_batch's.
        With aggre_on_device the filter matches of a group arrive deduplicated;
        the host check stays only for what the device cannot see: the bag's
        rows (by_dest.host_rows names them) and the plan "external", which
        merges several device classes."""
        if not msgs:
            return {}, {}
        on_dev = self.aggre_on_device
        deliveries = picks = keys = by_sub = None
        if self.share_on_device:
            keys = [self.share_keys(m) for m in msgs]
            if self.share_grouped:
                by_dest, deliveries, picks, by_sub = self.router.match_routes_publish_deliver(
                    [m.topic for m in msgs], [k[0] for k in keys], [k[1] for k in keys], seed=self.share_seed,
                    errors="return")
            else:
                by_dest, deliveries, picks = self.router.match_routes_publish(
                    [m.topic for m in msgs], [k[0] for k in keys], [k[1] for k in keys], seed=self.share_seed,
                    errors="return")
            on_dev = True
        elif self.deliver_grouped:
            by_dest, deliveries, by_sub = self.router.match_routes_deliver([m.topic for m in msgs], errors="return",
                                                                           aggre=on_dev)
        elif self.dispatch_on_device:
            by_dest, deliveries = self.router.match_routes_dispatch([m.topic for m in msgs], errors="return",
                                                                    aggre=on_dev)
        elif on_dev:
            by_dest = self.router.match_routes_by_dest([m.topic for m in msgs], errors="return", aggre=True)
        else:
            by_dest = self.router.match_routes_by_dest([m.topic for m in msgs], errors="return")
        self.batches += 1
        plans: dict = {}
        seen = set()
        for cls, rows in by_dest.items():
            if deliveries is not None and cls == self.node:
                continue   # the local node's routes are already expanded: its plan is the deliveries
            node = not isinstance(rows[0][1].dest, tuple)
            if picks is not None and not node and not isinstance(cls, tuple) and cls in picks:
                continue   # a group's routes are already picked: its plan is the picks (a group no pick
                           # came back for keeps the host path: share_dispatch)
            dest = cls[0] if isinstance(cls, tuple) else cls   # aggre/1: {Group, _Node} -> Group, whatever the pair
            plan = plans.setdefault(dest, [])
            # rows the device has aggregated need no check: all but the bag's, unless classes merge here
            check = None if not on_dev or isinstance(cls, tuple) else by_dest.host_rows.get(cls, ())
            for at, (i, r) in enumerate(rows):
                if not node and (check is None or at in check):
                    if (i, r.topic, dest) in seen:
                        continue
                    seen.add((i, r.topic, dest))
                plan.append((i, r.topic))
        out = {}
        for dest, plan in plans.items():
            plan.sort(key=lambda e: e[0])   # several classes in one plan (every ("external", X)): message order again
            out[dest] = [(i, to) + (self._route2((to, dest), msgs[i])[2],) for i, to in plan]
        failed: dict = {}   # share_grouped: SubPid -> the reason its deliver_batch gave
        if self.share_grouped:
            for sub, items in by_sub.items():
                reason = self.deliver_batch(sub, [(to, msgs[i]) for i, to in items])
                if reason is not None and reason != "ok":
                    failed[sub] = reason
            if deliveries:
                out[self.node] = list(deliveries)
        elif deliveries:
            if by_sub is not None:
                for sub, items in by_sub.items():
                    self.deliver_batch(sub, [(to, msgs[i]) for i, to in items])
            else:
                for i, to, sub in deliveries:
                    self.deliver(sub, to, msgs[i])
            out[self.node] = list(deliveries)
        for group, rows in (picks or {}).items():
            plan = out[group] = []
            for i, to, pid in rows:
                if self.share_grouped and pid is not None and self.router.member_is_local(pid):
                    # its deliver_batch carried the message; a dead pid: dispatch/4's recursion on the host
                    res = pid if pid not in failed else self._share_failed(group, to, i, pid, failed[pid], msgs[i], keys[i])
                else:
                    res = self._share_deliver(group, to, i, pid, msgs[i], keys[i])
                plan.append((i, to, res))
        return out, by_dest.errors

    def _share_deliver(self, group, to, i, pid, msg, hashes):
        """do_dispatch/5 to the device's pick; when the send fails, dispatch/4's
        recursion on the host: the slot's state word read back, SharedSubs.pick
        with the failed pids in FailedSubs until a send succeeds (or a {retry,
        _} pick, which is sent without an ack), and the word written back.
        -> the pid the message went to, or ("error", "no_subscribers")."""
        if pid is None:
            return ("error", "no_subscribers")
        reason = self.share_send(pid, to, msg)
        if reason == "ok":
            return pid
        return self._share_failed(group, to, i, pid, reason, msg, hashes)

    def _share_failed(self, group, to, i, pid, reason, msg, hashes):
        """dispatch/4's recursion after the send to `pid` failed with `reason`"""
        ss = self.router.shared_subs
        slot = ss.slot(group, to)
        if slot is not None:
            ss.adopt_state(group, to, self.router.share_state(slot))
        failed = {pid: reason}
        result = ("error", "no_subscribers")
        while True:
            res = ss.pick(group, to, hashes[0], hashes[1], failed, i)
            if not res:
                break
            kind, p = res
            reason = self.share_send(p, to, msg)
            if reason == "ok" or kind == "retry":
                result = p
                break
            failed[p] = reason
        if slot is not None:
            self.router.set_share_state(slot, ss.device_state(group, to))
        return result

    # ---- asynchronous micro-batching
    def publish(self, msg) -> Future:
        """Queue one message; the future resolves to (routes, results) once its
        micro-batch has been matched and dispatched."""
        fut: Future = Future()
        with self._cv:
            if not self._q:
                self._first_at = time.monotonic()
            self._q.append((msg, fut))
            if len(self._q) == 1 or len(self._q) >= self.max_batch:
                self._cv.notify()   # start the wait bound / flush a full batch
        if self._thread is None:
            self.flush_if_due()
        return fut

    def _take(self):
        batch, self._q = self._q[: self.max_batch], self._q[self.max_batch:]
        self._first_at = time.monotonic() if self._q else None
        return batch

    def _run(self, batch):
        try:
            res = self.publish_batch([m for m, _ in batch])
            for (_, fut), r in zip(batch, res):
                if isinstance(r, Exception):
                    fut.set_exception(r)        # this message only (badarg)
                else:
                    fut.set_result(r)
        except BaseException as e:   # a failure of the whole batch (device error): every caller sees it
            for _, fut in batch:
                if not fut.done():
                    fut.set_exception(e)

    def flush_if_due(self, force: bool = False):
        with self._cv:
            due = self._q and (force or len(self._q) >= self.max_batch or
                               time.monotonic() - self._first_at >= self.max_wait)
            batch = self._take() if due else []
        if batch:
            self._run(batch)
        return len(batch)

    def flush(self):
        n = 0
        while True:
            k = self.flush_if_due(force=True)
            if not k:
                return n
            n += k

    def _loop(self):
        while True:
            with self._cv:
                while not self._stop and (not self._q or (
                        len(self._q) < self.max_batch and time.monotonic() - self._first_at < self.max_wait)):
                    timeout = None if not self._q else max(0.0, self.max_wait - (time.monotonic() - self._first_at))
                    self._cv.wait(timeout)
                if self._stop and not self._q:
                    return
                batch = self._take()
            self._run(batch)

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify()
        if self._thread:
            self._thread.join(timeout=5)
        self.flush()
