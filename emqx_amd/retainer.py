"""A mirror of the ``emqx_retainer_mnesia`` backend callbacks over the device
store (:class:`emqx_amd._native.Retained`).

The store keeps topic names, a u32 value and an expiry per row and answers
``emqx_topic:match/2`` of a subscription filter over all of them on the GPU.
The messages themselves stay on the host, in a dict keyed by value slot: a
row's value is the slot of its message.

Callback by callback (emqx_retainer_mnesia.erl):

* ``store_retained``  :207-224 -- refused when the table is full and the topic
  is new (:210, :530-539);
* ``delete_message``  :271-283 -- a wildcard argument deletes every match,
  looked up with ``now = 0`` so that expired rows go too (:277);
* ``read_message``    :285-286, :502-514 -- exact, ``expiry == 0 or expiry >= now``;
* ``match_messages``  :288-304, :409-475 -- ``expiry == 0 or expiry > now``;
  with ``batch_read_number`` set, ``match_messages_cursor`` is ``match_messages/3``
  with its cursor (:288-304), ``delete_cursor`` ends one early, and ``dispatch``
  restates the dispatcher's loop over it (emqx_retainer_dispatcher.erl:248-301)
  without the limiter;
* ``clear_expired``   :226-269 -- ``(complete, n)``;
* ``page_read``       :309-332 -- sorted by timestamp as ``compare_message`` does;
* ``size``, ``clean`` :334-340.

Not built: ``msg_expiry_interval_override`` (:235-250); clear_expired is the
``disabled`` branch (:231-234); the dispatcher's limiter.

A cursor pins the store while it is open (rows then keep their places: no
compaction), so every cursor is either drained to the end or handed to
``delete_cursor``, as the dispatcher does.  Rows written while a cursor is open
are seen if they land at or after it and not otherwise; the reference's ets
stream is no stronger.
"""
from __future__ import annotations

import time


def words(topic: bytes):
    """emqx_topic:words/1: split on '/', the empty level an ordinary word"""
    return bytes(topic).split(b"/")


def is_wildcard(topic: bytes) -> bool:
    """emqx_topic:wildcard/1: some level is exactly '+' or '#'"""
    return any(w in (b"+", b"#") for w in words(topic))


def topic_match(name: bytes, flt: bytes) -> bool:
    """emqx_topic:match/2 for binaries (emqx_topic.erl:80-116)"""
    t, f = words(name), words(flt)
    if name[:1] == b"$" and f[0] in (b"+", b"#"):
        return False
    for i, w in enumerate(f):
        if w == b"#":
            return i == len(f) - 1
        if i >= len(t) or (w != b"+" and w != t[i]):
            return False
    return len(t) == len(f)


def _now_ms() -> int:
    return int(time.time() * 1000)


CURSOR_BEGIN, CURSOR_DONE, ERR_STALE = 0, 0xFFFFFFFFFFFFFFFF, 3   # tm_retained_match_page's (include/tmatch.h)


class StaleCursor(RuntimeError):
    """The store compacted after the cursor was handed out (only a cursor whose pin was given up can see this):
    its rows have moved.  The caller decides whether to start again."""


class Cursor:
    """An open match_messages/3 stream: the device cursor, the `now` of the first call (the reference captures
    Now when it builds the stream, :290-292) and whether it still holds a pin on the store."""
    __slots__ = ("flt", "pos", "now", "pinned")

    def __init__(self, flt: bytes, now: int):
        self.flt, self.pos, self.now, self.pinned = flt, CURSOR_BEGIN, now, False


class Retainer:
    """store: a factory of stores with the interface of ``_native.Retained`` (put, delete, get, match, expire,
    stats, close); the default makes one on the current device with `store_opts`."""

    def __init__(self, store=None, max_retained_messages: int = 0, batch_read_number: int | None = None,
                 scan_rows: int = 0, **store_opts):
        if store is None:
            from . import _native
            store = lambda: _native.Retained(**store_opts)
        self._factory = store
        self._store = store()
        self.max_retained_messages = max_retained_messages
        # rows a cursor read returns (None: all_remaining, the whole list at once, :296-297); rows a device call
        # examines per filter at most (0: no bound)
        self.batch_read_number = batch_read_number
        self.scan_rows = scan_rows
        self._slot = {}      # topic -> value slot
        self._rows = {}      # value slot -> (topic, msg, expiry_time, timestamp)
        self._free = []
        self._next = 0

    def close(self):
        self._store.close()

    # ---- the callbacks
    def store_retained(self, topic: bytes, msg, expiry_time: int = 0, timestamp: int | None = None) -> bool:
        topic = bytes(topic)
        new = topic not in self._slot
        if new and self.max_retained_messages > 0 and self.size() >= self.max_retained_messages:
            return False   # table_is_full (:210-219)
        slot = self._slot.get(topic)
        if slot is None:
            slot = self._free[-1] if self._free else self._next
        code = int(self._store.put([topic], [slot], [expiry_time])[0])
        if code == 2:
            raise ValueError(f"not a topic name: {topic!r}")   # (nothing stored: the slot is not taken)
        if new:
            self._slot[topic] = slot
            if self._free:
                self._free.pop()
            else:
                self._next += 1
        self._rows[slot] = (topic, msg, expiry_time, _now_ms() if timestamp is None else timestamp)
        return True

    def _drop(self, topics):
        for t in topics:
            slot = self._slot.pop(t)
            del self._rows[slot]
            self._free.append(slot)

    def delete_message(self, topic_or_filter: bytes) -> None:
        t = bytes(topic_or_filter)
        if is_wildcard(t):
            topics = [self._rows[int(v)][0] for v in self._store.match([t], 0)[0]]
        else:
            topics = [t] if t in self._slot else []
        if topics:
            found = self._store.delete(topics)
            assert all(found), "the store and the mirror hold the same topics"
            self._drop(topics)

    def read_message(self, topic: bytes, now: int | None = None) -> list:
        vals, found = self._store.get([bytes(topic)], _now_ms() if now is None else now)
        return [self._rows[int(vals[0])][1]] if found[0] else []

    def match_messages_batch(self, filters, now: int | None = None) -> list:
        now = _now_ms() if now is None else now
        return [[self._rows[int(v)][1] for v in vals] for vals in self._store.match([bytes(f) for f in filters], now)]

    def match_messages(self, flt: bytes, now: int | None = None) -> list:
        return self.match_messages_batch([flt], now)[0]

    # ---- match_messages/3 with its cursor
    def _release(self, cursor: Cursor) -> None:
        if cursor.pinned:
            cursor.pinned = False
            self._store.unpin()

    def match_messages_batch_cursor(self, filters, cursors=None, now: int | None = None):
        """One read of batch_read_number rows for each of many subscribers, each at its own position, in one
        device call per round -> (lists of messages, cursors); a cursor is None once its stream has ended.
        cursors None opens a stream for every filter, with `now`; else it is what the previous call returned, and a
        place that holds None stays ended: ([], None), as match_next(_, _, undefined) gives (:288-289)."""
        n = len(filters)
        if self.batch_read_number is None:   # all_remaining: no cursor comes back (:296-297)
            if cursors is not None:   # ... so what comes in is ended
                return [[] for _ in range(n)], [None] * n
            return self.match_messages_batch(filters, now), [None] * n
        now = _now_ms() if now is None else now
        if cursors is None:
            curs = [Cursor(bytes(f), now) for f in filters]
        else:
            curs = [Cursor(bytes(f), now) if c is None else c for f, c in zip(filters, cursors)]
            for c, given in zip(curs, cursors):
                if given is None:
                    c.pos = CURSOR_DONE
        want = self.batch_read_number
        out = [[] for _ in range(n)]
        todo = [i for i in range(n) if curs[i].pos != CURSOR_DONE]
        try:
            while todo:
                # one `now` and one limit per device call: those that opened together and lack the same number of
                # rows go out together (all of them, when they advance in step)
                key = lambda i: (curs[i].now, want - len(out[i]))
                group = [i for i in todo if key(i) == key(todo[0])]
                limit = want - len(out[group[0]])
                lists, pos, err = self._store.match_page([curs[i].flt for i in group], curs[group[0]].now,
                                                         [curs[i].pos for i in group], limit, self.scan_rows)
                for k, i in enumerate(group):
                    c = curs[i]
                    if int(err[k]) == ERR_STALE:
                        raise StaleCursor(f"the store compacted under the cursor of {c.flt!r}")
                    out[i].extend(self._rows[int(v)][1] for v in lists[k])
                    c.pos = int(pos[k])
                    if c.pos == CURSOR_DONE:
                        self._release(c)
                    elif not c.pinned:      # it opened with rows left: rows keep their places until it ends
                        self._store.pin()
                        c.pinned = True
                # with scan_rows set a page may be short and its cursor live: call again
                rest = [i for i in todo if i not in group]
                todo = rest + [i for i in group if curs[i].pos != CURSOR_DONE and len(out[i]) < want]
        except BaseException:
            for c in curs:
                self._release(c)
            raise
        return out, [None if c.pos == CURSOR_DONE else c for c in curs]

    def match_messages_cursor(self, flt: bytes, cursor: Cursor | None = None, now: int | None = None):
        """match_messages/3 (:288-304) -> (messages, cursor or None).  cursor None opens the stream, with Now fixed
        for all of its reads; a returned cursor of None is the reference's `undefined`.  When exactly
        batch_read_number rows were left the cursor stays open and the next read is ([], None), as
        emqx_utils_stream:consume/2 makes it (:298-304)."""
        out, curs = self.match_messages_batch_cursor([flt], None if cursor is None else [cursor], now)
        return out[0], curs[0]

    def delete_cursor(self, cursor: Cursor | None) -> None:
        """delete_cursor/2 (:306-307): gives up the pin of a cursor that is still open"""
        if cursor is not None:
            self._release(cursor)
            cursor.pos = CURSOR_DONE

    def dispatch(self, flt: bytes, deliver, now: int | None = None) -> None:
        """emqx_retainer_dispatcher's loop (emqx_retainer_dispatcher.erl:248-301) without the limiter: read a page,
        hand it to deliver(messages), stop when that returns false or the stream ends; the cursor is always
        deleted."""
        cursor = None
        try:
            msgs, cursor = self.match_messages_cursor(flt, None, now)
            while msgs:                                   # dispatch_with_cursor(_, [], Cursor, ..) ends (:271-273)
                if deliver(msgs) is False:                # {drop, _} and no_receiver (:279-285)
                    return
                if cursor is None:                        # match_next(_, _, undefined) -> {ok, [], undefined} (:288-289)
                    return
                msgs, cursor = self.match_messages_cursor(flt, cursor)
        finally:
            self.delete_cursor(cursor)

    def clear_expired(self, deadline: int, limit: int | None = None):
        """-> (complete, n cleared); limit None is the reference's `all`"""
        if limit is not None and limit <= 0:
            return False, 0   # fold(_, Acc, 0, S) takes nothing and hands the stream back (:266-267)
        complete, vals = self._store.expire(deadline, 0 if limit is None else limit)
        self._drop([self._rows[int(v)][0] for v in vals])
        return complete, len(vals)

    def page_read(self, flt: bytes | None, deadline: int, page: int, limit: int):
        """-> (has_more, messages): the rows visible at `deadline` (all of them for flt None, :312-313), sorted by
        timestamp (equal timestamps by topic, where the reference has the table's order), page `page` >= 1 of
        `limit`.  has_more is the reference's: the page came back full (:327-331)"""
        if flt is None:
            slots = [s for s, (_, _, exp, _) in self._rows.items() if exp == 0 or exp > deadline]
        else:
            slots = [int(v) for v in self._store.match([bytes(flt)], deadline)[0]]
        rows = sorted((self._rows[s] for s in slots), key=lambda r: (r[3], r[0]))
        skip = (page - 1) * limit
        out = [r[1] for r in rows[skip: skip + limit]]
        return len(out) == limit, out

    def size(self) -> int:
        return len(self._slot)

    def clean(self) -> None:
        self._store.close()
        self._store = self._factory()
        self._slot, self._rows, self._free, self._next = {}, {}, [], 0

    def topics(self) -> list:
        return list(self._slot)
