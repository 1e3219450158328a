"""Drop-in mirror of ``emqx_topic_index`` backed by the MI355X index.

Same names, argument meaning and results as apps/emqx/src/emqx_topic_index.erl
(new/0,1 :40-48, insert/4 :53-56, delete/3 :60-62, match/2 :70-72,
matches/3 :76-78, get_id/1, get_topic/1, get_record/2 :86-106).

``Tab`` plays the part of the caller-owned ETS table: it keeps the records
(the source of truth, SURVEY.md 8b "Ownership") and interns every key
``{Filter, {ID}}`` to a dense u32 that the device index stores.  Inserts and
deletes are queued and shipped with one ``tm_apply_deltas`` call before the
next match (the router-syncer batch boundary, emqx_router_syncer.erl:297-356).
Matching always runs on the GPU through ``libtmatch``; there is no CPU path.

Concurrency (as on the reference's read_concurrency table,
emqx_topic_index.erl:41-48): any number of threads may match while one
thread writes.  A reader registers with the library's reader epochs
(include/tmatch.h) around its device batch AND the decoding of the returned
u32s; a deleted key's u32 sits in quarantine until every reader that began
before the delete has finished, so a value decodes to its own key or to
nothing (a key deleted meanwhile is dropped) -- never to a key inserted later.

Result order: the device returns keys in traversal order (ascending Erlang
term order).  ``matches/3`` returns them like the reference does -- reversed,
because match_add/2 prepends (emqx_trie_search.erl:350-356); ``[unique]``
keeps the last key per ID (maps:values): for up to 32 IDs that is the
reference's list element for element (a flatmap iterates in key term order);
beyond 32 the BEAM iterates a HAMT in the order of its internal term hash,
which this mirror does not restate, so the list is the same set of keys in
ID term order (the Erlang module, src/emqx_topic_index_gpu.erl, calls
maps:values itself and is exact); ``match/2`` is the first key in traversal
order.
"""
from __future__ import annotations

import threading
from collections import deque

import numpy as np

from . import _native
from .trie_search import (BadArg, HASH, PLUS, filter_words, get_id, get_topic, key_order,  # noqa: F401
                          make_key, term_key, topic_words)


ROUTE_POOL_SETS = 4   # pinned buffer sets route_kids32 keeps (concurrent callers beyond them allocate their own)


class Tab:
    """An index table: records + the device-resident mirror of its keys."""

    def __init__(self, device: int = -1, hint_keys: int = 0, index=None, copies: int = 1):
        """copies: copies of the tables on the device (tm_options.copies; new/1's
        {copies, N}): under churn a batch after a delta runs on a copy no batch
        is reading."""
        self._index = index if index is not None else _native.Index(device=device, hint_keys=hint_keys,
                                                                    copies=copies)
        self._records: dict = {}        # key -> record        (the ETS rows)
        self._kid: dict = {}            # key -> u32 value on the device
        self._keys: list = []           # u32 -> key (None: deleted)
        self._free: list[int] = []      # u32s no reader can still return
        self._released: list[int] = []  # freed by deletes not yet shipped
        self._quarantine = deque()      # (epoch of the delete, u32): reusable once the safe epoch reaches it
        self._ops: list = []            # pending (op, filter_bytes, kid, flags)
        self._lock = threading.Lock()   # pending deltas and u32 bookkeeping (writer side)
        self._sorted = None             # (keys, order keys) in term order, for matches_filter/3
        # route fan-out (include/tmatch.h): dest_fn(key) -> the u32 destination id of a
        # key's value, set by the owner (Router); shipped with tm_set_dests ahead of the
        # delta that inserts the key
        self.dest_fn = None
        self._dests: list = []          # pending (kid, destination id)
        # aggre/1 on the device: filter_fn(key) -> the owner's u32 id of the key's topic
        # filter (equal filters, equal ids), shipped with tm_set_route_filters in the same
        # flush as the destinations; filter_release(key) tells the owner a key is gone
        self.filter_fn = None
        self.filter_release = None
        self._filts: list = []          # pending (kid, filter id)
        # local dispatch on the device: sub_fn(key) -> the u32 subscriber ids of the key's
        # value in dispatch order, shipped with tm_set_subscribers in the same flush, ahead
        # of the insert; set_subscribers(key, ids) for later changes
        self.sub_fn = None
        self._subs: list = []           # pending (kid, [subscriber ids])
        self._with_subs: set = set()    # kids whose device list is not empty
        # shared-subscription pick on the device: share_fn(key) -> the owner's slot of the
        # key's {Group, To} pair (None: the key is no shared route), shipped with
        # tm_set_share_slots in the same flush, ahead of the insert, and cleared with the
        # key; set_share_members / set_share_state queue a slot's list and state word, which
        # go up in the same flush ahead of the slots
        self.share_fn = None
        # share_release(key): a key that carried a slot is gone.  Called AFTER the table's lock
        # is dropped: the owner may answer with set_share_members (a pair's last key gone, its
        # slot emptied), which takes the lock
        self.share_release = None
        self._share_gone: list = []     # keys whose release is still owed
        self._shares: list = []         # pending (kid, slot)
        self._with_share: set = set()   # kids whose device slot is not "none"
        self._share_members: list = []  # pending (slot, [member ids], n_local, meta)
        self._share_states: list = []   # pending (slot, state word)
        # picks grouped with the deliveries: member_subs_fn(member id) -> the local subscriber
        # id of a share member (None: not a connection of this node), asked for every member
        # id set_share_members queues whose answer differs from what was shipped, and shipped
        # with tm_set_member_subs in the same flush, ahead of the members
        self.member_subs_fn = None
        self._member_subs: list = []    # pending (member id, subscriber id)
        self._member_sub_of: dict = {}  # member id -> subscriber id as shipped or queued
        self._route_pool: list = []     # route_kids32: idle sets of pinned batch buffers (host_array)

    # -- key <-> device encoding
    @staticmethod
    def _encode(key):
        """-> (filter bytes, flags) for tm_apply_deltas (include/tmatch.h "Keys")."""
        f = key[0]
        if not isinstance(f, tuple):
            return bytes(f), _native.TM_KEY_BINARY
        if len(f) == 0:
            return b"", _native.TM_KEY_EMPTY_LIST
        return encode_words(f)

    def _queue(self, op, key, kid):
        enc = self._encode(key)
        self._ops.append((op, enc[0], kid, enc[1]))

    def flush(self, commit: bool = False):
        """Ship the queued deltas as ONE call (commit: tm_commit -- the route
        mirror's group commit, which no batch waits for on the GPU)."""
        with self._lock:
            self._flush_locked(commit)

    def sync_keys(self, keys, present, commit: bool = False):
        """Reconcile `keys` (present[i]: the key is in the table) and ship the
        delta in ONE call, the queueing and the shipping under one hold of the
        lock: a reader's flush (match_kids) cannot take these ops in between
        and ship them as a plain tm_apply_deltas, which a tm_commit running
        meanwhile would publish only with itself (include/tmatch.h) -- the
        writer's commit would then find nothing to ship and return before its
        keys were readable (the router's read-your-writes)."""
        with self._lock:
            for k, here in zip(keys, present):
                if here:
                    self._insert_locked(k, [])
                else:
                    self._delete_locked(k)
            self._flush_locked(commit)
            gone, self._share_gone = self._share_gone, []
        self._released_shares(gone)

    def _flush_locked(self, commit: bool):
        if self._dests:
            d = np.array(self._dests, dtype=np.uint32).reshape(-1, 2)
            self._dests = []
            self._index.set_dests(d[:, 0], d[:, 1])
        if self._filts:
            f = np.array(self._filts, dtype=np.uint32).reshape(-1, 2)
            self._filts = []
            self._index.set_route_filters(f[:, 0], f[:, 1])
        if self._subs:
            subs, self._subs = self._subs, []
            self._index.set_subscribers([k for k, _ in subs], [ids for _, ids in subs])
        if self._member_subs:
            ms = np.array(self._member_subs, dtype=np.uint32).reshape(-1, 2)
            self._member_subs = []
            self._index.set_member_subs(ms[:, 0], ms[:, 1])
        if self._share_members:
            mem, self._share_members = self._share_members, []
            self._index.set_share_members([m[0] for m in mem], [m[1] for m in mem], [m[2] for m in mem],
                                          [m[3] for m in mem])
        if self._share_states:
            st, self._share_states = self._share_states, []
            self._index.share_state_set([x[0] for x in st], [x[1] for x in st])
        if self._shares:
            sh = np.array(self._shares, dtype=np.uint32).reshape(-1, 2)
            self._shares = []
            self._index.set_share_slots(sh[:, 0], sh[:, 1])
        if not self._ops:
            return
        ops = np.array([o[0] for o in self._ops], dtype=np.uint8)
        blob, offs = _native.pack_strings([o[1] for o in self._ops])
        vals = np.array([o[2] for o in self._ops], dtype=np.uint32)
        flags = np.array([o[3] for o in self._ops], dtype=np.uint8)
        self._ops = []
        epoch = (self._index.apply(ops, blob, offs, vals, flags, commit=True) if commit
                 else self._index.apply(ops, blob, offs, vals, flags))
        # the deletes just shipped are visible from `epoch` on: their u32s
        # wait until no reader that began earlier is running
        for kid in self._released:
            self._quarantine.append((epoch, kid))
        self._released = []

    def _take_kid(self) -> int:
        if not self._free and self._quarantine:
            _, safe = self._index.epoch()
            while self._quarantine and self._quarantine[0][0] <= safe:
                self._free.append(self._quarantine.popleft()[1])
        if self._free:
            return self._free.pop()
        self._keys.append(None)
        return len(self._keys) - 1

    # -- table operations (one writer at a time, as the reference's callers)
    def insert_key(self, key, record):
        with self._lock:
            self._insert_locked(key, record)

    def delete_key(self, key):
        with self._lock:
            self._delete_locked(key)
            gone, self._share_gone = self._share_gone, []
        self._released_shares(gone)

    def _released_shares(self, keys):
        """the owner hears of the deleted keys that carried a slot -- without the lock"""
        for key in keys:
            self.share_release(key)

    def _insert_locked(self, key, record):
        if key not in self._records:
            self._sorted = None
            kid = self._take_kid()
            self._keys[kid] = key
            self._kid[key] = kid
            if self.dest_fn is not None:
                self._dests.append((kid, self.dest_fn(key)))
            if self.filter_fn is not None:
                self._filts.append((kid, self.filter_fn(key)))
            if self.sub_fn is not None:
                self._set_subs_locked(kid, self.sub_fn(key))
            if self.share_fn is not None:
                slot = self.share_fn(key)
                if slot is not None:
                    self._shares.append((kid, int(slot)))
                    self._with_share.add(kid)
            self._queue(_native.TM_OP_INSERT, key, kid)
        self._records[key] = record

    def _delete_locked(self, key):
        if key in self._records:
            self._sorted = None
            kid = self._kid.pop(key)
            del self._records[key]
            self._queue(_native.TM_OP_DELETE, key, kid)
            self._keys[kid] = None
            self._released.append(kid)
            self._set_subs_locked(kid, ())   # the key's list goes with it
            if kid in self._with_share:      # ... and its slot
                self._with_share.discard(kid)
                self._shares.append((kid, _native.TM_SHARE_NONE))
                if self.share_release is not None:
                    self._share_gone.append(key)
            if self.filter_release is not None:
                self.filter_release(key)

    def _set_subs_locked(self, kid, sub_ids):
        ids = [int(x) for x in sub_ids]
        if not ids and kid not in self._with_subs:
            return   # (empty is what the device holds for it)
        (self._with_subs.add if ids else self._with_subs.discard)(kid)
        self._subs.append((kid, ids))

    def set_subscribers(self, key, sub_ids):
        """The local subscriber list of `key`'s value becomes sub_ids (u32s, in
        dispatch order), shipped with tm_set_subscribers at the next flush.  A
        key not in the table: nothing to do (sub_fn is asked when it is inserted)."""
        with self._lock:
            kid = self._kid.get(key)
            if kid is not None:
                self._set_subs_locked(kid, sub_ids)

    def set_share_members(self, slot: int, member_ids, n_local: int, meta: int):
        """Slot `slot`'s member list (u32s in subscribers/2's order), its local
        prefix and meta = strategy | init_strategy << 8, shipped with
        tm_set_share_members at the next flush -- ahead of the slots and the
        inserts of that flush.  A slot queued twice ships its last list."""
        with self._lock:
            ids = [int(x) for x in member_ids]
            if self.member_subs_fn is not None:
                for m in ids:
                    sub = self.member_subs_fn(m)
                    sub = _native.TM_SHARE_NONE if sub is None else int(sub)
                    if self._member_sub_of.get(m, _native.TM_SHARE_NONE) != sub:
                        self._member_sub_of[m] = sub
                        self._member_subs.append((m, sub))
            self._share_members.append((int(slot), ids, int(n_local), int(meta)))

    def set_member_sub(self, member_id: int, sub_id):
        """Share member `member_id` is local subscriber `sub_id` (None: not a
        connection of this node), shipped with tm_set_member_subs at the next flush."""
        with self._lock:
            sub = _native.TM_SHARE_NONE if sub_id is None else int(sub_id)
            self._member_sub_of[int(member_id)] = sub
            self._member_subs.append((int(member_id), sub))

    def set_share_state(self, slot: int, state: int):
        """Slot `slot`'s state word becomes `state` on every device entry
        (tm_share_state_set), at the next flush, after the members queued before it."""
        with self._lock:
            self._share_states.append((int(slot), int(state)))

    def share_state(self, slots, dev: int = 0):
        """The slots' state words on device entry `dev` (tm_share_state_get), after
        everything queued here and every pick queued there so far."""
        self.flush()
        return self._index.share_state_get(slots, dev)

    def publish_kids(self, topics, n_dests: int, local_dest: int, key_clientid=None, key_topic=None, seed: int = 0):
        """tm_publish_batch -> (dispatch_kids' two tuples under aggre, member id
        u32[K]): the picked member of every kept entry (TM_SHARE_NONE: none),
        with the tables of share_fn / set_share_members."""
        self.flush()
        blob, offs = _native.pack_strings(topics)
        return self._index.publish_batch(blob, offs, n_dests, local_dest, key_clientid=key_clientid,
                                         key_topic=key_topic, seed=seed)

    def publish_deliver_kids(self, topics, n_dests: int, local_dest: int, key_clientid=None, key_topic=None,
                             seed: int = 0):
        """tm_publish_deliver_batch -> (route_kids' result, (topic index, kid,
        subscriber id) u32[N] -- the direct deliveries and the picks whose
        member is a local subscriber (member_subs_fn / set_member_sub), merged
        by message and GROUPED by subscriber id --, member id u32[K] as
        publish_kids, (subscriber id u32[G], offsets u64[G + 1]), T the number
        of direct deliveries among the N)."""
        self.flush()
        blob, offs = _native.pack_strings(topics)
        return self._index.publish_deliver_batch(blob, offs, n_dests, local_dest, key_clientid=key_clientid,
                                                 key_topic=key_topic, seed=seed)

    def attach(self, rows, batch_size: int = 1000) -> int:
        """Boot the device mirror from an existing table (emqx_topic_index_gpu:
        attach/2): rows are (Key, Record) in the table's key order, loaded in
        batches of at most batch_size keys, one tm_apply_deltas per batch (the
        Erlang module counts the batch as it fills: linear in the rows).
        Returns the device calls made."""
        calls, k = 0, 0
        for key, rec in rows:
            self.insert_key(key, rec)
            k += 1
            if k >= batch_size:
                self.flush()
                calls, k = calls + 1, 0
        if k:
            self.flush()
            calls += 1
        return calls

    def size(self) -> int:
        return len(self._records)

    def keys(self):
        return list(self._records)

    def sorted_keys(self):
        """every key of the table in Erlang term order (the ordered_set view)"""
        if self._sorted is None:
            keys = sorted(self._records, key=key_order)
            self._sorted = (keys, [key_order(k) for k in keys])
        return self._sorted

    def lookup(self, key):
        return [self._records[key]] if key in self._records else []

    # -- matching (batched: the unit the broker micro-batch hands over)
    def match_kids(self, topics):
        """-> (list of kid arrays in traversal order, badarg flags).  The
        caller decodes the kids inside a read_begin()/read_end() pair."""
        self.flush()
        blob, offs = _native.pack_strings(topics)
        hit, vals, err = self._index.match_batch(blob, offs)
        return [vals[hit[i]:hit[i + 1]] for i in range(len(topics))], err

    def route_kids(self, topics, n_dests: int, aggre: bool = False):
        """tm_route_batch -> (dest_offsets u64[n_dests + 2], topic index u32[],
        kid u32[], err u8[n]): destination b's (topic index, kid) pairs are
        [dest_offsets[b], dest_offsets[b + 1]), in topic order and traversal
        order inside a topic; bucket n_dests: kids without a destination
        below n_dests.  Decoded like match_kids' results.  aggre: the buckets
        after aggre/1 (TM_ROUTE_AGGRE; the filter ids of filter_fn)."""
        self.flush()
        blob, offs = _native.pack_strings(topics)
        return self._index.route_batch(blob, offs, n_dests, aggre=aggre)

    def dispatch_kids(self, topics, n_dests: int, local_dest: int, aggre: bool = False):
        """tm_dispatch_batch -> (route_kids' result, (topic index u32[T], kid u32[T],
        subscriber id u32[T])): the buckets, and bucket local_dest expanded to one
        delivery per subscriber of each entry's kid, in entry order and list
        order (the lists of sub_fn / set_subscribers)."""
        self.flush()
        blob, offs = _native.pack_strings(topics)
        return self._index.dispatch_batch(blob, offs, n_dests, local_dest, aggre=aggre)

    def deliver_kids(self, topics, n_dests: int, local_dest: int, aggre: bool = False):
        """tm_deliver_batch -> (route_kids' result, dispatch_kids' three delivery
        arrays GROUPED by subscriber id -- ascending ids, a subscriber's
        deliveries in dispatch_kids' order -- and (subscriber id u32[G], offsets
        u64[G + 1]): subscriber g owns the deliveries [offsets[g], offsets[g + 1]))."""
        self.flush()
        blob, offs = _native.pack_strings(topics)
        return self._index.deliver_batch(blob, offs, n_dests, local_dest, aggre=aggre)

    def _route_set(self, n: int, nbytes: int, n_dests: int, cap: int, dcap: int | None = None, pick: bool = False,
                   group: bool = False) -> dict:
        """A set of pinned buffers (host_array) large enough for the batch, from
        the pool or new -- what a NIF keeps per scheduler.  Arrays too small are
        replaced; the set goes back with _route_put.  dcap: the head and the
        three delivery arrays of dispatch_kids32 as well (a set that never
        dispatched has none); pick: publish_kids32's member array -- a pick per
        entry the set has room for -- and its two key arrays; group:
        deliver_kids32's group head, subscribers and offsets, with room for a
        group per delivery (G <= T: the groups never ask for a rerun of their
        own)."""
        with self._lock:
            s = self._route_pool.pop() if self._route_pool else {}
        want = {"blob": (nbytes + 16, np.uint8), "offs": (n + 1, np.uint32), "doff": (n_dests + 2, np.uint32),
                "topic": (cap, np.uint32), "vals": (cap, np.uint32), "err": (max(n, 1), np.uint8)}
        if dcap is not None:
            want.update({"head": (2, np.uint64), "dtopic": (dcap, np.uint32), "dvals": (dcap, np.uint32),
                         "dsubs": (dcap, np.uint32)})
        if group:
            room = max(dcap, len(s.get("dsubs", ())))
            want.update({"ghead": (2, np.uint64), "gsub": (room, np.uint32), "goff": (room + 1, np.uint32)})
        if pick:
            want.update({"member": (max(cap, len(s.get("topic", ()))), np.uint32), "kc": (max(n, 1), np.uint32),
                         "kt": (max(n, 1), np.uint32)})
        for name, (need, dt) in want.items():
            if name not in s or len(s[name]) < need:
                self._route_grow(s, name, need, dt)
        return s

    def _route_grow(self, s: dict, name: str, need: int, dt=np.uint32):
        """array `name` of the set replaced by one with room for `need` and a quarter"""
        if name in s:
            self._index.host_free(s.pop(name))
        s[name] = self._index.host_array(need + need // 4, dt)

    def _route_put(self, s: dict):
        with self._lock:
            if len(self._route_pool) < ROUTE_POOL_SETS:
                self._route_pool.append(s)
                return
        for a in s.values():
            self._index.host_free(a)

    def _kids32(self, topics, n_dests: int, local_dest: int | None = None, aggre: bool = False, pick=None,
                group: bool = False):
        """The pooled, in-place call behind route_kids32 (local_dest None),
        dispatch_kids32, publish_kids32 (pick: (key_clientid, key_topic,
        seed); always with aggre) and deliver_kids32 (group) -> (route outputs,
        deliveries or (), members or None -- under group the (subscribers,
        offsets) pair), copies: the buffers go back to the pool.  One retry on
        TM_ECAP."""
        self.flush()
        ix = self._index
        blob, offs = _native.pack_strings(topics)
        n, nbytes = len(offs) - 1, int(offs[-1])
        if nbytes >= 1 << 32:   # no 32-bit offsets for them: the staged calls
            if local_dest is None:
                return ix.route_batch(blob, offs, n_dests, aggre=aggre), (), None
            if group:
                return ix.deliver_batch(blob, offs, n_dests, local_dest, aggre=aggre)
            if pick is None:
                return ix.dispatch_batch(blob, offs, n_dests, local_dest, aggre=aggre) + (None,)
            return ix.publish_batch(blob, offs, n_dests, local_dest, key_clientid=pick[0], key_topic=pick[1], seed=pick[2])
        first = max(4 * n, 1024)
        s = self._route_set(n, nbytes, n_dests, first, None if local_dest is None else first, pick is not None, group)

        def copied(doff, tidx, kids, err):
            return doff.astype(np.uint64), tidx.copy(), kids.copy(), err.copy()
        try:
            s["blob"][:nbytes] = blob[:nbytes]
            s["offs"][: n + 1] = offs
            keys = []
            for name, k in (("kc", pick[0]), ("kt", pick[1])) if pick is not None else ():
                if k is None:
                    keys.append(None)
                    continue
                k = np.asarray(k, dtype=np.uint32)
                if len(k) < n:
                    raise ValueError("publish_kids32: one key word per topic")
                s[name][:n] = k[:n]
                keys.append(s[name][:max(n, 1)])
            entries = ("topic", "vals") if pick is None else ("topic", "vals", "member")
            kept = None   # a publish whose picks stand: its route outputs and members
            for attempt in (0, 1):
                b, o = s["blob"], s["offs"][: n + 1]
                out = (s["doff"], s["topic"], s["vals"], s["err"])
                if local_dest is not None:
                    out += (s["head"], s["dtopic"], s["dvals"], s["dsubs"])
                try:
                    if local_dest is None:
                        res = ix.route_batch32(b, o, n_dests, out, aggre=aggre), (), None
                    elif group:
                        res = ix.deliver_batch32(b, o, n_dests, local_dest, out + (s["ghead"], s["gsub"], s["goff"]),
                                                 aggre=aggre)
                    elif pick is None or kept is not None:
                        res = ix.dispatch_batch32(b, o, n_dests, local_dest, out, aggre=aggre) + (None,)
                    else:
                        res = ix.publish_batch32(b, o, n_dests, local_dest, out, s["member"], keys[0], keys[1], pick[2])
                    break
                except _native.TmError as e:
                    if e.code != _native.TM_ECAP or attempt:
                        raise
                total = int(s["doff"][n_dests + 1])
                if pick is not None and total <= min(len(s[name]) for name in entries):
                    # a publish whose deliveries alone were short made its picks (the state has moved): its
                    # route outputs and members are kept, and only the dispatch is fetched again
                    kept = copied(s["doff"][: n_dests + 2], s["topic"][:total], s["vals"][:total], s["err"][:n]), \
                        s["member"][:total].copy()
                # the entry arrays grow from the bucket offsets (the full sizes) ...
                short = [(entries, total)]
                if local_dest is not None:   # ... and the delivery arrays from the head
                    short.append((("dtopic", "dvals", "dsubs"), int(s["head"][1])))
                for names, need in short:
                    if need > len(s[names[0]]):
                        for name in names:
                            self._route_grow(s, name, need)
                if group and len(s["gsub"]) < len(s["dsubs"]):   # (a group per delivery, as _route_set sizes them)
                    self._route_grow(s, "gsub", len(s["dsubs"]))
                    self._route_grow(s, "goff", len(s["dsubs"]) + 1)
            route, deliveries, member = res
            deliveries = tuple(a.copy() for a in deliveries)
            if group:
                return copied(*route), deliveries, (member[0].copy(), member[1].astype(np.uint64))
            if kept is not None:
                return kept[0], deliveries, kept[1]
            return copied(*route), deliveries, None if member is None else member.copy()
        finally:
            self._route_put(s)

    def route_kids32(self, topics, n_dests: int, aggre: bool = False):
        """route_kids through tm_route_batch32 on pooled pinned buffers: a
        micro-batch is matched and fanned out in place (two launches, no
        staging copy).  One retry on TM_ECAP, sized from the bucket offsets.
        Returns what route_kids returns (copies: the buffers go back to the
        pool)."""
        return self._kids32(topics, n_dests, aggre=aggre)[0]

    def dispatch_kids32(self, topics, n_dests: int, local_dest: int, aggre: bool = False):
        """dispatch_kids through tm_dispatch_batch32 on pooled pinned buffers: a
        micro-batch is matched, fanned out and dispatched in place (one
        synchronisation, no staging copy).  One retry on TM_ECAP, sized from the
        bucket offsets and the head.  Returns what dispatch_kids returns
        (copies: the buffers go back to the pool)."""
        return self._kids32(topics, n_dests, local_dest, aggre)[:2]

    def deliver_kids32(self, topics, n_dests: int, local_dest: int, aggre: bool = False):
        """deliver_kids through tm_deliver_batch32 on pooled pinned buffers: a
        micro-batch is matched, fanned out, dispatched and grouped by subscriber
        in place (one synchronisation, no staging copy).  One retry on TM_ECAP,
        sized from the bucket offsets and the head; the group arrays have room
        for a group per delivery.  Returns what deliver_kids returns (copies:
        the buffers go back to the pool)."""
        return self._kids32(topics, n_dests, local_dest, aggre, group=True)

    def publish_kids32(self, topics, n_dests: int, local_dest: int, key_clientid=None, key_topic=None, seed: int = 0):
        """publish_kids through tm_publish_batch32 on pooled pinned buffers: a
        micro-batch is matched, fanned out, dispatched and picked for in place
        (one synchronisation, no staging copy).  TM_ECAP from the entries: no
        pick was made and no state moved, so the call is made once more with
        larger arrays.  TM_ECAP from the deliveries alone: the picks stand (the
        state has moved), so only the dispatch is fetched again, through
        tm_dispatch_batch32.  Returns what publish_kids returns (copies: the
        buffers go back to the pool)."""
        return self._kids32(topics, n_dests, local_dest, True, (key_clientid, key_topic, seed))

    def publish_deliver_kids32(self, topics, n_dests: int, local_dest: int, key_clientid=None, key_topic=None,
                               seed: int = 0):
        """publish_deliver_kids through tm_publish_deliver_batch32 on pooled pinned
        buffers: a micro-batch is matched, fanned out, dispatched, picked for,
        merged and grouped by subscriber in place (one synchronisation, no
        staging copy).  The member-subs table is shipped ahead by the flush, as
        in publish_deliver_kids.  The delivery arrays have room for T + K of the
        previous sizes and the group arrays for a group per delivery, so a short
        gcap cannot occur.  TM_ECAP from the entries or the deliveries: no pick
        was made and no state moved, so the call is made once more, sized from
        the bucket offsets and the head.  Returns what publish_deliver_kids
        returns (copies: the buffers go back to the pool)."""
        self.flush()
        ix = self._index
        blob, offs = _native.pack_strings(topics)
        n, nbytes = len(offs) - 1, int(offs[-1])
        if nbytes >= 1 << 32:   # no 32-bit offsets for them: the staged call
            return ix.publish_deliver_batch(blob, offs, n_dests, local_dest, key_clientid=key_clientid,
                                            key_topic=key_topic, seed=seed)
        first = max(4 * n, 1024)
        s = self._route_set(n, nbytes, n_dests, first, 2 * first, True, True)
        try:
            s["blob"][:nbytes] = blob[:nbytes]
            s["offs"][: n + 1] = offs
            keys = []
            for name, k in (("kc", key_clientid), ("kt", key_topic)):
                if k is None:
                    keys.append(None)
                    continue
                k = np.asarray(k, dtype=np.uint32)
                if len(k) < n:
                    raise ValueError("publish_deliver_kids32: one key word per topic")
                s[name][:n] = k[:n]
                keys.append(s[name][:max(n, 1)])
            for attempt in (0, 1):
                if len(s["gsub"]) < len(s["dsubs"]) or len(s["goff"]) < len(s["dsubs"]) + 1:   # a group per delivery
                    self._route_grow(s, "gsub", len(s["dsubs"]))
                    self._route_grow(s, "goff", len(s["dsubs"]) + 1)
                out = (s["doff"], s["topic"], s["vals"], s["err"], s["head"], s["dtopic"], s["dvals"], s["dsubs"], s["ghead"],
                       s["gsub"], s["goff"])
                try:
                    route, deliveries, member, groups, T = ix.publish_deliver_batch32(
                        s["blob"], s["offs"][: n + 1], n_dests, local_dest, out, s["member"], keys[0], keys[1], seed)
                    break
                except _native.TmError as e:
                    if e.code != _native.TM_ECAP or attempt:
                        raise
                # nothing moved: the entry arrays grow from the bucket offsets (under total > cap the
                # un-aggregated total, an upper bound of K), the delivery arrays to T + that
                total, T = int(s["doff"][n_dests + 1]), int(s["head"][1])
                for names, need in ((("topic", "vals", "member"), total), (("dtopic", "dvals", "dsubs"), T + total)):
                    if need > min(len(s[name]) for name in names):
                        for name in names:
                            self._route_grow(s, name, need)
            doff, tidx, kids, err = route
            return (doff.astype(np.uint64), tidx.copy(), kids.copy(), err.copy()), tuple(a.copy() for a in deliveries), \
                member.copy(), (groups[0].copy(), groups[1].astype(np.uint64)), T
        finally:
            self._route_put(s)

    def read_begin(self) -> int:
        return self._index.read_begin()

    def read_end(self, ticket: int):
        self._index.read_end(ticket)

    def decode(self, kids):
        """u32s -> keys; a key deleted since the batch began is dropped (its
        u32 is quarantined, so it cannot name a newer key yet)."""
        keys = self._keys
        return [k for k in (keys[i] for i in kids.tolist()) if k is not None]

    def stats(self) -> dict:
        self.flush()
        return self._index.stats()


def new(options=None, device: int = -1) -> Tab:
    """new/0,1: an empty index table (ETS options are accepted and ignored)."""
    return Tab(device=device)


def insert(filter_, ident, record, tab: Tab):
    """insert/4: associate Filter with ID (and Record)."""
    tab.insert_key(make_key(filter_, ident), record)
    return True


def delete(filter_, ident, tab: Tab):
    """delete/3: deleting a missing entry is not an error."""
    tab.delete_key(make_key(filter_, ident))
    return True


class TopicTooDeep(ValueError):
    """A topic of more than 65536 levels: longer than MQTT's 65535-byte
    maximum (emqx_mqtt.hrl:44), so no client can publish it; the device walk's
    scratch ends there (include/tmatch.h, err flag 2)."""


def matches_batch(topics, tab: Tab, opts=(), errors: str = "raise"):
    """matches/3 over a batch of topics (one device launch).

    A topic with a '+'/'#' level is badarg (emqx_trie_search.erl:374-375) and
    one of more than 65536 levels is TopicTooDeep; the device flags each topic
    on its own.  A batch the device failed (err flag 4: the library already
    ran it again once) raises DeviceError for the whole call -- never BadArg,
    which the reference reserves for the topic itself.  errors="raise" raises for the first such topic (one call, one
    topic: the reference's behaviour); errors="return" puts the exception in
    that topic's slot and still returns every other topic's matches -- a
    micro-batch of many publishers fails only the bad publish, as each
    publishing process does in the reference."""
    topics = [bytes(t) for t in topics]
    ticket = tab.read_begin()
    try:
        kids, err = tab.match_kids(topics)
        if len(err) and (err == 4).any():   # (the library returns TM_EDEVICE instead; never a client error)
            raise _native.DeviceError(_native.TM_EDEVICE, "batch failed on the device (err flag 4)")
        out = []
        for i, ks in enumerate(kids):
            if err[i]:
                e = TopicTooDeep(len(topics[i])) if err[i] == 2 else BadArg(topics[i])
                if errors == "raise":
                    raise e
                out.append(e)
                continue
            out.append(_finish(tab.decode(ks), opts))
    finally:
        tab.read_end(ticket)
    return out


def traversal_order(keys):
    """Device order -> the reference's traversal order.  The device emits keys
    in ascending Erlang term order of their filters, but the keys of ONE
    filter (several IDs on one filter: $share groups, many subscribers of a
    rule topic) come in the order of their u32 values, which Tab hands out by
    insertion (and reuses).  The reference orders them by {ID}
    (emqx_trie_search.erl:107-111: {Filter, {ID}} in an ordered_set), so each
    run of equal filters is sorted by the ID's term order."""
    out = []
    i, n = 0, len(keys)
    while i < n:
        j = i + 1
        f = keys[i][0]
        while j < n and keys[j][0] == f:
            j += 1
        if j - i > 1:
            out.extend(sorted(keys[i:j], key=lambda k: term_key(k[1][0])))
        else:
            out.append(keys[i])
        i = j
    return out


class FirstHit(Exception):
    """matches/3 with [return_first] found a key: the reference's search throws
    {first, Key} at the first hit (match_add/2, emqx_trie_search.erl:355-356)
    and the caller catches it (match/2 does, :172-178)."""

    def __init__(self, key):
        super().__init__(key)
        self.key = key


FIRST = "first"   # the atom matches/3 with [return_first] returns when nothing matches


def _finish(keys, opts):
    """Device keys (traversal order) -> the accumulator the reference's
    search/3 returns for `opts` (emqx_trie_search.erl:201-226): return_first
    before unique before a plain list.  With return_first: ("first", Key) for
    the first key in traversal order, or FIRST when nothing matched (its
    initial accumulator, returned as is)."""
    keys = traversal_order(keys)
    if "return_first" in opts:
        return (FIRST, keys[0]) if keys else FIRST
    if "unique" in opts:
        by_id = {}
        for k in keys:                             # traversal order; later keys win
            by_id[get_id(k)] = k
        return [by_id[i] for i in sorted(by_id, key=term_key)]
    return keys[::-1]          # matches/3 is the reverse of the traversal order (match_add/2 prepends)


def matches(topic, tab: Tab, opts=()):
    """matches/3.  With return_first it raises FirstHit(Key) at a match, as the
    reference's call throws {first, Key}, and returns FIRST otherwise."""
    r = matches_batch([topic], tab, opts)[0]
    if isinstance(r, tuple) and len(r) == 2 and r[0] == FIRST:
        raise FirstHit(r[1])
    return r


def match(topic, tab: Tab):
    """match/2: the first match in traversal order, or False."""
    keys = matches_batch([topic], tab, ())[0]
    return keys[-1] if keys else False


def matches_filter(filter_, tab: Tab, opts=()):
    """matches_filter/3 (emqx_topic_index.erl:82-84 -> emqx_trie_search.erl:186-189):
    the index keys a subscription to `filter_` covers, by the reference's
    ordered search (filter_words/1, base_init/1, compare/3 with the filter
    clauses :291-300, no match_topics phase -- binary keys never match).

    Its result depends on where the ordered walk stops (a stored key below the
    query at a query '+' ends the whole search), which the trie walk has no
    notion of, so the device runs the reference's walk itself over the keys in
    term order (tm_matches_filter_ex) -- every key of the table, those no topic
    can match included (binary words '+'/'#' or holding a '/': the escaped
    key form), and a query given as a word list in the same form.  Callers are
    control-plane (durable-storage stream discovery,
    emqx_ds_new_streams.erl:325)."""
    if isinstance(filter_, (bytes, bytearray)):
        q, qf = bytes(filter_), 0
    else:
        q, qf = encode_words(tuple(filter_words(filter_)))
    ticket = tab.read_begin()
    try:
        tab.flush()
        blob, offs = _native.pack_strings([q])
        _, vals, err = tab._index.matches_filter_batch(blob, offs, np.array([qf], np.uint8))
        if len(err) and err[0]:   # the device walk hit its step bound: no silent truncation
            raise RuntimeError(f"matches_filter: device walk exceeded its step bound for {filter_!r}")
        return _finish(tab.decode(vals), opts)
    finally:
        tab.read_end(ticket)


def encode_words(words):
    """A word list -> (bytes, flags) in the C ABI's key form: '/'-joined
    (TM_KEY_WORDS), or -- when a binary word holds a '/' or equals "+" / "#",
    which no topic level can equal -- the escaped form (TM_KEY_WORDS |
    TM_KEY_ESCAPED: "\\/" a '/', "\\\\" a '\\', "\\+" / "\\#" the binary
    words, bare "+" / "#" the wildcards).  The library keeps such a key for
    matches_filter/3 only; it never matches a topic."""
    plain, esc, escaped = [], [], False
    for w in words:
        if w == PLUS or w == HASH:
            plain.append(w.encode())
            esc.append(w.encode())
        elif isinstance(w, (bytes, bytearray)):
            w = bytes(w)
            if w in (b"+", b"#"):
                escaped = True
                esc.append(b"\\" + w)
            else:
                escaped |= b"/" in w
                esc.append(w.replace(b"\\", b"\\\\").replace(b"/", b"\\/"))
            plain.append(w)
        else:
            raise TypeError(f"bad filter word {w!r}")
    if escaped:
        return b"/".join(esc), _native.TM_KEY_WORDS | _native.TM_KEY_ESCAPED
    return b"/".join(plain), _native.TM_KEY_WORDS


def get_record(key, tab: Tab):
    """get_record/2: [Record] or [] if the entry was deleted meanwhile."""
    return tab.lookup(key)


DeviceError = _native.DeviceError

__all__ = ["new", "insert", "delete", "match", "matches", "matches_batch", "matches_filter", "make_key", "get_id",
           "get_topic", "get_record", "Tab", "BadArg", "TopicTooDeep", "DeviceError", "FirstHit", "FIRST"]
