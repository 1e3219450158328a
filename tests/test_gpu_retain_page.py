"""Match cursors on the device (tm_retained_match_page, tm_retained_pin,
tm_retained_unpin; kernels emqx_amd/csrc/tm_retain_page.hip) against a
restatement of emqx_topic:match/2 (emqx_topic.erl:80-116) and the match path's
expiry rule (expiry == 0 or expiry > now, emqx_retainer_mnesia.erl:464-466).
Through the raw ABI, with canaries around out_hit_offsets (n + 1 words),
out_cursor (n words) and out_err (n bytes) and after out_values[cap].  A drain
(page after page to TM_RET_CURSOR_DONE) must have no duplicate, equal the
restatement's list as a sorted list, and be the same sequence at every page
size; where the scan order is known (an empty base: put order; topics put in
sorted order) the sequence itself is compared.
"""
import ctypes as C
import random

import numpy as np
import pytest

from bytes_vocab import short_vocabulary
from emqx_amd import _native
from emqx_amd._native import RT_TILE, TM_ECAP, TM_EINVAL, TM_OK, pack_strings

pytestmark = pytest.mark.gpu

CANARY32, CANARY64 = 0xC0FFEE11, 0xFEEDFACECAFEBEEF
BEGIN, DONE, ESTALE = 0, 0xFFFFFFFFFFFFFFFF, 3
ROW_MASK = (1 << 40) - 1


# ---- the restatement (independent of emqx_amd.retainer)

def ref_match(topic: bytes, flt: bytes) -> bool:
    t, f = topic.split(b"/"), flt.split(b"/")
    if topic[:1] == b"$" and f[0] in (b"+", b"#"):
        return False
    for i, w in enumerate(f):
        if w == b"#":
            return i == len(f) - 1
        if i >= len(t) or (w != b"+" and w != t[i]):
            return False
    return len(t) == len(f)


def ref_valid(flt: bytes) -> bool:
    return b"#" not in flt.split(b"/")[:-1]


def ref_list(model, flt, now):
    """model: topic -> (value, expiry); the match path's rule"""
    if not ref_valid(flt):
        return []
    return sorted(v for t, (v, e) in model.items() if (e == 0 or e > now) and ref_match(t, flt))


# ---- the raw call, with canaries

def raw_page(store, filters, cursors=None, limit=1000, scan_rows=0, now=0, cap=None):
    """-> (rc, offsets[n + 1], values[:cap], cursors[n], err[n]); cap None: n * limit"""
    lib, h = store._lib, store._h
    blob, offs = pack_strings(filters)
    n = len(filters)
    cap = n * limit if cap is None else cap
    hit = np.full(n + 3, CANARY64, np.uint64)
    cur = np.full(n + 2, CANARY64, np.uint64)
    err = np.full(n + 2, 0xEE, np.uint8)
    vals = np.full(cap + 4, CANARY32, np.uint32)
    cin = None if cursors is None else np.ascontiguousarray(cursors, dtype=np.uint64)
    rc = lib.tm_retained_match_page(h, n, _native._ptr(blob), _native._ptr(offs), now, _native._ptr(cin), limit, scan_rows,
                                    hit[1:].ctypes.data_as(C.c_void_p), _native._ptr(vals), cap,
                                    cur[1:].ctypes.data_as(C.c_void_p), err[1:].ctypes.data_as(C.c_void_p))
    assert hit[0] == CANARY64 and hit[n + 2] == CANARY64, "out_hit_offsets has n + 1 words"
    assert cur[0] == CANARY64 and cur[n + 1] == CANARY64, "out_cursor has n words"
    assert err[0] == 0xEE and err[n + 1] == 0xEE, "out_err has n bytes"
    assert (vals[cap:] == CANARY32).all(), "nothing is written at or past cap"
    assert rc in (TM_OK, TM_ECAP) and hit[1] == 0 and (rc == TM_ECAP) == (int(hit[n + 1]) > cap)
    assert (np.diff(hit[1:n + 2].astype(np.int64)) <= limit).all() and (np.diff(hit[1:n + 2].astype(np.int64)) >= 0).all()
    return rc, hit[1:n + 2].copy(), vals[:cap].copy(), cur[1:n + 1].copy(), err[1:n + 1].copy()


def page1(store, flt, cursor=BEGIN, limit=1000, scan_rows=0, now=0):
    """one filter, one page -> (values, cursor, err)"""
    rc, hit, vals, cur, err = raw_page(store, [flt], [cursor], limit, scan_rows, now)
    assert rc == TM_OK
    return vals[:int(hit[1])].tolist(), int(cur[0]), int(err[0])


def drain(store, flt, limit, scan_rows=0, now=0, cursor=BEGIN):
    """-> (the values in the order they came, the page lengths)"""
    out, sizes = [], []
    while cursor != DONE:
        vals, cursor, err = page1(store, flt, cursor, limit, scan_rows, now)
        assert err == (0 if ref_valid(flt) else 2)
        if not scan_rows:
            assert (cursor != DONE) == (len(vals) == limit), "only a full page leaves a live cursor"
        out += vals
        sizes.append(len(vals))
        assert len(sizes) < 5000
    return out, sizes


def check_drain(store, model, flt, limit, scan_rows=0, now=0):
    seq, _ = drain(store, flt, limit, scan_rows, now)
    assert len(set(seq)) == len(seq), (flt, limit, "a duplicate")
    assert sorted(seq) == ref_list(model, flt, now), (flt, limit, len(seq))
    return seq


def put(store, model, topics, values, expiry=None):
    expiry = [0] * len(topics) if expiry is None else expiry
    codes = store.put(topics, values, expiry)
    for t, v, e, c in zip(topics, values, expiry, codes):
        assert c == (0 if t in model else 1), t
        model[t] = (v, e)


@pytest.fixture
def store():
    made = []

    def make(tail_max=0, initial_rows=64):
        made.append(_native.Retained(initial_rows=initial_rows, tail_max=tail_max))
        return made[-1]
    yield make
    for s in made:
        s.close()


def _rows(n):
    topics = [(b"$m/%d/%d" if i % 13 == 7 else b"m/%d/%d") % (i % 5, i) for i in range(n)]
    values = [0xFFFFFFFF - i for i in range(n)]
    expiry = [0 if i % 4 else 90 + i % 20 for i in range(n)]
    return topics, values, expiry


def _store_600(store, where):
    s = store(tail_max=4000)
    model = {}
    topics, values, expiry = _rows(600)
    first = 300 if where == "both" else 600
    put(s, model, topics[:first], values[:first], expiry[:first])
    if where != "tail":
        s.compact()
    if where == "both":
        put(s, model, topics[300:], values[300:], expiry[300:])
    st = s.stats()
    assert (st["base_rows"], st["tail_rows"]) == {"tail": (0, 600), "base": (600, 0), "both": (300, 300)}[where]
    return s, model


PAGE_FILTERS = [b"#", b"m/#", b"m/+/+", b"m/3/+", b"+/+/17", b"$m/#", b"m/0/0", b"nope/#", b"a/#/b", b"+/4/+"]


# ---- paging is the full match

@pytest.mark.parametrize("where", ["tail", "base", "both"])
def test_paging_is_the_full_match_at_every_page_size(store, where):
    s, model = _store_600(store, where)
    for flt in PAGE_FILTERS:
        for now in (0, 100):
            limits = (1, 255, 256, 257, 1000) if now == 0 else (255, 256, 257, 1000)   # (limit 1: a call per row)
            seqs = {limit: check_drain(s, model, flt, limit, now=now) for limit in limits}
            assert len({tuple(q) for q in seqs.values()}) == 1, (flt, "the sequence does not depend on the page size")
    if where == "both":   # one page crosses from the base to the tail
        vals, cur, _ = page1(s, b"m/#", BEGIN, 400)
        assert len(vals) == 400 and cur & ROW_MASK > 300


def test_scan_order_is_visible(store):
    """with an empty base a '#' drain returns the values in put order"""
    s, model = _store_600(store, "tail")
    in_order = [0xFFFFFFFF - i for i in range(600) if i % 13 != 7]
    for limit in (37, 256, 1000):
        assert drain(s, b"#", limit)[0] == in_order
    assert drain(s, b"$m/3/+", 3)[0] == [0xFFFFFFFF - i for i in range(600) if i % 13 == 7 and i % 5 == 3]


# ---- tile edges

@pytest.mark.parametrize("where", ["tail", "base"])
@pytest.mark.parametrize("n", [255, 256, 257, 512, 513])
def test_tile_edges(store, n, where):
    s = store(tail_max=4000)
    model = {}
    put(s, model, [b"e/%d" % (1000 + i) for i in range(n)], list(range(n)))   # (sorted as they are put)
    if where == "base":
        s.compact()
    seen, cursor, left = [], BEGIN, n
    while cursor != DONE:
        vals, cursor, _ = page1(s, b"e/+", cursor, 256)
        assert len(vals) == min(left, 256)
        assert (cursor != DONE) == (len(vals) == 256), "exactly `limit` rows left: a live cursor, then ([], DONE)"
        if cursor != DONE:
            assert cursor & ROW_MASK == len(seen) + 256, "the row after the limit-th hit, even at the end of the rows"
        seen += vals
        left -= len(vals)
    assert seen == list(range(n))
    assert page1(s, b"e/+", DONE, 256) == ([], DONE, 0)


def test_hits_in_single_waves_of_a_tile(store):
    """tile 0 hits in its first wave only, tile 1 in its last only, tile 2 in all four"""
    s = store(tail_max=4000)
    model = {}
    hit = lambda i: (i % 256 < 64) if i < 256 else (i % 256 >= 192) if i < 512 else i % 3 == 0
    put(s, model, [(b"h/%d" if hit(i) else b"x/%d") % i for i in range(768)], list(range(768)))
    want = [i for i in range(768) if hit(i)]
    for limit in (1, 10, 63, 64, 65, 130, 1000):
        assert drain(s, b"h/+", limit)[0] == want, limit


# ---- cursors that are not on a tile boundary

def test_cursors_inside_tiles_and_across_filters(store):
    s, model = _store_600(store, "both")
    for flt in (b"#", b"m/3/#", b"m/+/+", b"+/4/+"):
        seq = check_drain(s, model, flt, 100)                      # every page starts mid-tile
        assert seq == check_drain(s, model, flt, 1000)
    full = check_drain(s, model, b"m/3/#", 1000)
    st = s.stats()
    # m/3/#'s base range starts at lo > 0: its first page's cursor lies past the rows of m/0 .. m/2
    vals, cur, _ = page1(s, b"m/3/#", BEGIN, 5)
    assert vals == full[:5] and cur & ROW_MASK > 5
    # a cursor is the store's: taken from '#' it is below m/3/#'s range and clamps to its start ...
    _, low, _ = page1(s, b"#", BEGIN, 5)
    assert 0 < low & ROW_MASK < 100
    assert drain(s, b"m/3/#", 1000, cursor=low)[0] == full
    # ... and one past the range (the last base row) skips to the tail
    past = (low & ~ROW_MASK) | (st["base_rows"] - 1)
    tail_only = drain(s, b"m/3/#", 1000, cursor=past)[0]
    want_tail = [v for t, (v, e) in model.items() if ref_match(t, b"m/3/#") and 0xFFFFFFFF - v >= 300]
    assert sorted(tail_only) == sorted(want_tail) and tail_only == full[len(full) - len(tail_only):]
    assert 0 < len(tail_only) < len(full)


# ---- a batch at mixed positions

def test_a_batch_at_mixed_positions(store):
    s, model = _store_600(store, "both")
    pool = [b"m/0/0", b"m/3/#", b"m/+/17", b"+/+/17", b"#", b"a/#/b", b"m/unknown/+", b"m/2/+", b"+/4/+", b"$m/#"]
    limit = 9
    filters, cursors, want, want_cur = [], [], [], []
    for i in range(64):
        flt, cur = pool[i % len(pool)], BEGIN
        for _ in range(i // 10):                                   # a different page of its own drain
            if cur != DONE:
                cur = page1(s, flt, cur, limit)[1]
        if i % 17 == 16:
            cur = DONE
        vals, nxt, _ = page1(s, flt, cur, limit)
        filters.append(flt), cursors.append(cur), want.append(vals), want_cur.append(nxt)
    rc, hit, vals, cur, err = raw_page(s, filters, cursors, limit)
    assert rc == TM_OK
    for i in range(64):
        assert vals[int(hit[i]):int(hit[i + 1])].tolist() == want[i], (i, filters[i])
        assert int(cur[i]) == want_cur[i] and err[i] == (2 if filters[i] == b"a/#/b" else 0)
    assert sum(bool(w) for w in want) >= 25 and sum(c == DONE for c in cursors) >= 3
    # capacity: total - 1 gives TM_ECAP with the true offsets, n * limit never does
    total = int(hit[-1])
    rc, hit2, _, cur2, _ = raw_page(s, filters, cursors, limit, cap=total - 1)
    assert rc == TM_ECAP and hit2.tolist() == hit.tolist()
    assert b"room for %d" % (total - 1) in s._lib.tm_retained_last_error(None)
    rc, hit3, vals3, _, _ = raw_page(s, filters, cursors, limit, cap=total)
    assert rc == TM_OK and vals3.tolist() == vals[:total].tolist()
    assert total < 64 * limit


# ---- expiry, dead rows and '$'

def test_expiry_dead_rows_and_dollar_topics(store):
    s = store(tail_max=6)
    model = {}
    put(s, model, [b"$SYS/a", b"$SYS/b/c", b"t/1", b"t/2", b"t/3", b"t/4", b"u/1", b"u/2"], list(range(1, 9)),
        [0, 0, 0, 1000, 1001, 0, 999, 0])                          # (past tail_max: in the base)
    put(s, model, [b"t/5", b"$SYS/d"], [9, 10], [1000, 0])          # (in the tail)
    assert s.delete([b"t/4", b"u/2"]).all()
    del model[b"t/4"], model[b"u/2"]
    for limit in (1, 2, 100):
        for now in (0, 999, 1000, 1001):
            for flt in (b"#", b"+/+", b"$SYS/#", b"t/+", b"+/1", b"t/4", b"$SYS/+", b"+/#"):
                check_drain(s, model, flt, limit, now=now)
    assert sorted(drain(s, b"#", 2, now=1000)[0]) == [3, 5], "now hides expiry <= now; deleted rows never appear"
    assert sorted(drain(s, b"+/+", 1)[0]) == [3, 4, 5, 7, 9], "no '$' topic under a first-level wildcard"
    assert sorted(drain(s, b"$SYS/#", 1)[0]) == [1, 2, 10]


# ---- scan_rows

def test_scan_rows_gives_short_pages_with_live_cursors(store):
    s = store(tail_max=4000)
    model = {}
    topics = [b"s/%d/%s" % (i, b"leaf" if i % 200 == 77 else b"other") for i in range(2000)]
    put(s, model, topics[:1200], list(range(1200)))
    s.compact()
    put(s, model, topics[1200:], list(range(1200, 2000)))
    seen, cursor, calls = [], BEGIN, 0
    while cursor != DONE:
        vals, cursor, _ = page1(s, b"+/+/leaf", cursor, 1000, scan_rows=256)
        calls += 1
        assert len(vals) < 1000, "every page is short"
        assert (cursor != DONE) == (calls < 8), "seven whole windows and 208 rows: the eighth call reaches the end"
        seen += vals
    assert calls <= -(-2000 // 256) + 1 and sorted(seen) == [i for i in range(2000) if i % 200 == 77] and len(seen) == 10
    for window in (1199, 1200, 1201, 1999, 2000, 2001):            # the window ends at the base's end, at the rows' end
        check_drain(s, model, b"+/+/leaf", 3, scan_rows=window)
    check_drain(s, model, b"s/77/+", 1, scan_rows=100)


# ---- many tiles per filter: past one chunk of the cut

def test_a_filter_of_more_tiles_than_one_chunk_of_the_cut(store):
    """70,000 rows are 274 tiles: the cut's second chunk of 256 tiles.  '#' with limit 69,000, then the last 1,000"""
    n = 70_000
    s = store(tail_max=2 * n)
    assert (s.put([b"k/%d" % i for i in range(n)], np.arange(n, dtype=np.uint32)) == 1).all()
    vals, cur, _ = page1(s, b"#", BEGIN, 69_000)
    assert vals == list(range(69_000)) and cur & ROW_MASK == 69_000
    vals, cur, _ = page1(s, b"#", cur, 69_000)
    assert vals == list(range(69_000, n)) and cur == DONE
    # the cut inside the first chunk: the tiles of the second have nothing to emit
    vals, cur, _ = page1(s, b"k/+", BEGIN, 300)
    assert vals == list(range(300)) and cur & ROW_MASK == 300
    # exactly n: a live cursor at the end of the rows, then nothing and DONE
    vals, cur, _ = page1(s, b"#", BEGIN, n)
    assert len(vals) == n and cur != DONE and cur & ROW_MASK == n
    assert page1(s, b"#", cur, n) == ([], DONE, 0)
    # room for more values than come back with the offsets: the values follow in a copy of their own
    vals, cur, _ = page1(s, b"#", BEGIN, 300_000)
    assert vals == list(range(n)) and cur == DONE


# ---- a batch of more tiles than one launch takes

def test_a_page_batch_of_more_than_2_24_tiles(store):
    """As test_gpu_retain's: 66,000 full-scan filters +/+/L<i % 6000> over 65,000 base rows and 1,000 tail rows are
    258 tiles each, 17.0M in all: two launches per pass.  Row j is g/<j>/L<j % 6000> with value j, and rows are in
    put order, so with limit = 2 filter i gets rows i % 6000 and i % 6000 + 6000 and a live cursor after the second"""
    rows, leaves, n = 66_000, 6_000, 66_000
    s = store(tail_max=rows)
    topics = [b"g/%d/L%d" % (j, j % leaves) for j in range(rows)]
    assert (s.put(topics[:65_000], np.arange(65_000, dtype=np.uint32)) == 1).all()
    s.compact()
    assert (s.put(topics[65_000:], np.arange(65_000, rows, dtype=np.uint32)) == 1).all()
    tiles = n * (-(-65_000 // RT_TILE) + -(-1_000 // RT_TILE))
    assert tiles > 1 << 24
    blob, offs = pack_strings([b"+/+/L%d" % (i % leaves) for i in range(n)])
    hit, vals, cur, err = s.match_page_packed(blob, offs, 0, None, 2)
    assert not err.any() and hit.tolist() == list(range(0, 2 * n + 1, 2))
    first = np.arange(n) % leaves
    sample = np.r_[0:200, n // 2 - 100:n // 2 + 100, n - 200:n]      # both ends and the launches' seam
    assert np.array_equal(vals.reshape(n, 2)[sample].astype(np.int64), np.stack([first, first + leaves], 1)[sample])
    assert (cur != np.uint64(DONE)).all(), "every cursor is live"
    assert np.array_equal((cur & np.uint64(ROW_MASK)).astype(np.int64), first + leaves + 1)


# ---- pins and epochs

def test_pins_hold_compactions_back(store):
    s = store(tail_max=4)
    lib, h = s._lib, s._h
    model = {}
    put(s, model, [b"p/%d" % i for i in range(40)], list(range(40)))   # past tail_max: compacted
    st = s.stats()
    assert (st["tail_rows"], st["compactions"]) == (0, 1)
    assert lib.tm_retained_unpin(h) == TM_EINVAL
    seen, cur, _ = page1(s, b"p/+", BEGIN, 7)
    assert cur != DONE
    s.pin()
    for i in range(10):
        put(s, model, [b"q/%d" % i], [100 + i])
    st = s.stats()
    assert st["compactions"] == 1 and st["tail_rows"] == 10
    assert lib.tm_retained_compact(h) == TM_OK and s.stats()["compactions"] == 1, "due, not done"
    seen += drain(s, b"p/+", 7, cursor=cur)[0]
    assert sorted(seen) == list(range(40)) and len(seen) == 40, "every original row exactly once"
    assert len(check_drain(s, model, b"#", 6)) == 50, "rows written under the pin are in the tail"
    s.unpin()
    st = s.stats()
    assert st["compactions"] == 2 and (st["base_rows"], st["tail_rows"]) == (50, 0)
    assert lib.tm_retained_unpin(h) == TM_EINVAL
    assert b"not pinned" in lib.tm_retained_last_error(None)
    check_drain(s, model, b"#", 6)


def test_a_cursor_of_another_epoch_is_stale(store):
    s, model = _store_600(store, "both")
    vals, cur, _ = page1(s, b"#", BEGIN, 5)
    assert cur != DONE and len(vals) == 5
    s.compact()                                                      # no pin held: the rows move
    rc, hit, vals, out, err = raw_page(s, [b"#", b"#", b"#"], [cur, BEGIN, DONE], 5)
    assert rc == TM_OK and err.tolist() == [ESTALE, 0, 0] and hit.tolist() == [0, 0, 5, 5]
    assert int(out[0]) == BEGIN and int(out[1]) not in (BEGIN, DONE) and int(out[2]) == DONE
    check_drain(s, model, b"#", 64)


# ---- through the mirror

def test_the_mirror_dispatches_in_pages_and_leaves_no_pin():
    from emqx_amd.retainer import Retainer
    rt = Retainer(batch_read_number=10, initial_rows=64, tail_max=8)
    try:
        for i in range(35):
            assert rt.store_retained(b"d/%d" % i, i)
        rt.store_retained(b"other", "x")
        pages = []
        rt.dispatch(b"d/+", lambda ms: pages.append(list(ms)), now=1)
        assert [len(p) for p in pages] == [10, 10, 10, 5] and sorted(sum(pages, [])) == list(range(35))
        assert rt._store._lib.tm_retained_unpin(rt._store._h) == TM_EINVAL, "no pin is left"
        pages = []
        rt.dispatch(b"d/+", lambda ms: (pages.append(list(ms)), False)[1], now=1)
        assert [len(p) for p in pages] == [10]
        assert rt._store._lib.tm_retained_unpin(rt._store._h) == TM_EINVAL, "a deliver that returns false leaves none"
        # eight subscribers in one device call per round equal eight single drains
        filters = [b"d/+", b"#", b"d/7", b"other", b"nothing/#", b"d/+", b"a/#/b", b"+/3"]
        singles = []
        for f in filters:
            got, cur = [], None
            while True:
                ms, cur = rt.match_messages_cursor(f, cur, 1)
                got += ms
                if cur is None:
                    break
            singles.append(got)
        got = [[] for _ in filters]
        lists, curs = rt.match_messages_batch_cursor(filters, None, 1)
        while True:
            for k, l in enumerate(lists):
                got[k] += l
            if all(c is None for c in curs):
                break
            lists, curs = rt.match_messages_batch_cursor(filters, curs)
        assert got == singles and sorted(got[1], key=str) == sorted(list(range(35)) + ["x"], key=str)
        assert rt._store._lib.tm_retained_unpin(rt._store._h) == TM_EINVAL
    finally:
        rt.close()


# ---- random parity under churn

VOCAB = short_vocabulary()


@pytest.mark.parametrize("seed", range(6))
def test_random_parity_under_churn(store, seed):
    r = random.Random(0x50414745 + seed)
    alpha = [b"a", b"b", b"", b"$s"] + r.sample(VOCAB, 4)
    alpha = [w for w in alpha if w not in (b"+", b"#")]
    topic = lambda: b"/".join(r.choice(alpha) for _ in range(r.randint(1, 4))) or b"a"

    def flt():
        n = r.randint(1, 4)
        lv = [r.choices([None, b"+", b"#"], [5, 3, 1])[0] for _ in range(n)]
        lv = [(b"+" if w == b"#" and i != n - 1 else w) for i, w in enumerate(lv)]
        return b"/".join(r.choice(alpha) if w is None else w for w in lv)
    s = store(tail_max=r.choice([8, 16, 32]))
    model = {}
    v = 0
    for step in range(40):
        c = r.random()
        if c < 0.6 or not model:
            ts = [t for t in dict.fromkeys(topic() for _ in range(r.randint(1, 12))) if t]
            put(s, model, ts, [v + k for k in range(len(ts))], [r.choice([0, 0, 90, 110]) for _ in ts])
            v += len(ts)
        elif c < 0.8:
            ts = r.sample(sorted(model), min(3, len(model)))
            assert s.delete(ts).all()
            for t in ts:
                del model[t]
        else:
            complete, gone = s.expire(100)
            assert complete and sorted(gone.tolist()) == sorted(x for x, e in model.values() if e and e < 100)
            model = {t: (x, e) for t, (x, e) in model.items() if not (e and e < 100)}
        for f in (flt(), flt(), flt(), b"#"):
            check_drain(s, model, f, r.randint(1, 20), scan_rows=r.choice([0, 0, 7]), now=r.choice([0, 100]))
    assert s.stats()["compactions"] >= 1
