"""The retained-message store on the device (tm_retained_*, include/tmatch.h;
kernels emqx_amd/csrc/tm_retain.hip) against a restatement of
emqx_topic:match/2 (emqx_topic.erl:80-116) and of the two expiry rules of
emqx_retainer_mnesia (match: expiry == 0 or expiry > now, :464-466; read:
expiry == 0 or expiry >= now, :510).  Every list is compared as a sorted list
with the restatement's (a duplicate or a missing row shows), through the raw
ABI with canaries after out_values[total] and around out_hit_offsets.
"""
import ctypes as C
import json
import random
from pathlib import Path

import numpy as np
import pytest

from bytes_vocab import short_vocabulary
from emqx_amd import _native
from emqx_amd._native import RT_TILE, TM_ECAP, TM_OK, pack_strings

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CANARY32, CANARY64 = 0xC0FFEE11, 0xFEEDFACECAFEBEEF


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

def raw_match(store, filters, now=0, cap=None):
    """-> (rc, offsets[n + 1], values[: min(total, cap)], err[n]); cap None: size with NULL / 0, then fill"""
    lib, h = store._lib, store._h
    blob, offs = pack_strings(filters)
    n = len(filters)
    hit = np.full(n + 3, CANARY64, np.uint64)
    err = np.full(n + 2, 0xEE, np.uint8)
    hp, ep = hit[1:].ctypes.data_as(C.c_void_p), err[1:].ctypes.data_as(C.c_void_p)

    def guards(vals, room):
        assert hit[0] == CANARY64 and hit[n + 2] == CANARY64, "out_hit_offsets has n + 1 words"
        assert err[0] == 0xEE and err[n + 1] == 0xEE, "out_err has n bytes"
        assert vals is None or (vals[room:] == CANARY32).all(), "nothing is written at or past cap"

    if cap is None:
        rc = lib.tm_retained_match(h, n, _native._ptr(blob), _native._ptr(offs), now, hp, None, 0, ep)
        guards(None, 0)
        total = int(hit[n + 1])
        assert rc == (TM_ECAP if total else TM_OK)
        cap = total
    vals = np.full(cap + 4, CANARY32, np.uint32)
    rc = lib.tm_retained_match(h, n, _native._ptr(blob), _native._ptr(offs), now, hp, _native._ptr(vals), cap, ep)
    guards(vals, cap)
    return rc, hit[1:n + 2].copy(), vals[:cap].copy(), err[1:n + 1].copy()


def check(store, model, filters, now=0):
    """every filter's list is the restatement's; -> how many filters matched something"""
    rc, hit, vals, err = raw_match(store, filters, now)
    assert rc == TM_OK and hit[0] == 0 and int(hit[-1]) == len(vals)
    some = 0
    for i, f in enumerate(filters):
        got = sorted(vals[int(hit[i]):int(hit[i + 1])].tolist())
        want = ref_list(model, f, now)
        assert got == want, (f, len(got), len(want))
        assert err[i] == (0 if ref_valid(f) else 2)
        some += bool(want)
    return some


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


# ---- row counts at the kernel's boundaries

ROWS = [0, 1, 63, 64, 65, RT_TILE - 1, RT_TILE, RT_TILE + 1, 2 * RT_TILE + 3]


def _rows(n):
    topics = [(b"$r/%d/%d" if i % 11 == 5 else b"r/%d/%d") % (i % 7, i) for i in range(n)]
    values = [0xFFFFFFFF - i for i in range(n)]                    # any u32 is a value
    expiry = [0 if i % 3 else 1000 + i % 5 for i in range(n)]
    return topics, values, expiry


def _row_filters(n):
    last = max(n - 1, 0)
    return [b"#", b"r/#", b"r/+/+", b"r/3/+", b"+/+/+", b"r/0/0", b"r/+/%d" % last, b"r/%d/%d" % (last % 7, last), b"$r/#",
            b"$r/+/5", b"+/3/#", b"r/3", b"r/3/#", b"r/+", b"nothing/#", b"r/7/+", b"r/+/+/+"]


@pytest.mark.parametrize("where", ["base", "tail"])
@pytest.mark.parametrize("n", ROWS)
def test_row_counts_at_the_tile_boundaries(store, n, where):
    s = store(tail_max=4 * RT_TILE)
    model = {}
    put(s, model, *_rows(n))
    if where == "base":
        s.compact()
    st = s.stats()
    assert (st["base_rows"], st["tail_rows"]) == ((n, 0) if where == "base" else (0, n)) and st["live_rows"] == n
    assert st["rt_tile"] == RT_TILE and st["rt_cols"] == _native.RT_COLS
    for now in (0, 1002):
        some = check(s, model, _row_filters(n), now)
        assert some >= (8 if n >= 63 else 0)
    if n > 64:
        assert st["growths"] >= 1


def test_rows_split_across_base_and_tail(store):
    s = store(tail_max=4 * RT_TILE)
    model = {}
    topics, values, expiry = _rows(RT_TILE + 1)
    put(s, model, topics[:130], values[:130], expiry[:130])
    s.compact()
    put(s, model, topics[130:], values[130:], expiry[130:])
    st = s.stats()
    assert (st["base_rows"], st["tail_rows"]) == (130, RT_TILE + 1 - 130)
    assert check(s, model, _row_filters(RT_TILE + 1), 1002) >= 8


# ---- level counts 1, 7, 8, 9, 12: the last column and the first overflow word

def _chain(k, alt=None):
    """l1/l2/.../lk, level `alt` (1-based) replaced by x<alt>"""
    return b"/".join((b"x%d" if i == alt else b"l%d") % i for i in range(1, k + 1))


@pytest.mark.parametrize("where", ["base", "tail"])
def test_level_counts_around_the_columns(store, where):
    s = store(tail_max=64)
    model = {}
    topics = [_chain(k) for k in (1, 7, 8, 9, 12)]
    topics += [_chain(k, alt) for k in (8, 9, 12) for alt in (1, 7, 8, 9, 12) if alt <= k]
    topics += [_chain(8) + b"/", _chain(7) + b"//l9", b"$" + _chain(9)]
    put(s, model, topics, list(range(len(topics))))
    if where == "base":
        s.compact()
    filters = []
    for d in (8, 9):                                              # a literal, '+' and '#' on level d
        filters += [_chain(d), _chain(d - 1) + b"/+", _chain(d - 1) + b"/#", _chain(d, d), _chain(d) + b"/#",
                    b"+/" + _chain(d).split(b"/", 1)[1], b"+/" + _chain(d - 1).split(b"/", 1)[1] + b"/+",
                    b"+/" + _chain(d - 1).split(b"/", 1)[1] + b"/#"]
    filters += [_chain(7) + b"/+/l9", _chain(7) + b"/+/+", _chain(8) + b"/+/+/+/l12", _chain(8) + b"/+/+/+/x12",
                b"+/" + _chain(12).split(b"/", 1)[1], _chain(12, 9), _chain(12), _chain(11) + b"/#", _chain(12) + b"/#",
                _chain(1), b"+", _chain(1) + b"/#", _chain(6) + b"/#", _chain(7), _chain(13), b"#", b"$l1/#"]
    assert check(s, model, filters) >= len(filters) - 2
    # the '#'-parent at depth 8 and 9: the topic l1/../ld itself is in the list of l1/../ld/#
    for d in (8, 9):
        assert model[_chain(d)][0] in ref_list(model, _chain(d) + b"/#", 0)


# ---- edge topics

def test_dollar_topics_empty_levels_and_byte_words(store):
    vocab = short_vocabulary()
    s = store(tail_max=16)
    model = {}
    topics = [b"$SYS/up", b"$SYS/a/b", b"$SYS", b"$x", b"x", b"a/x", b"/x", b"a//b", b"a/", b"a", b"/", b"//", b"a/b", b"a/c/b",
              b"$/x", b"a/$SYS", b"a+", b"a+/#b", b"+a/x"]
    topics += [b"w/" + w for w in vocab] + [w + b"/w" for w in vocab if w and w[:1] != b"$"]
    topics = list(dict.fromkeys(topics))
    for k in range(0, len(topics), 100):                           # each batch crosses tail_max: a compaction
        put(s, model, topics[k:k + 100], list(range(k, k + len(topics[k:k + 100]))))
    filters = [b"#", b"+/#", b"+/x", b"$SYS/#", b"$SYS/+", b"a/+/b", b"a/+", b"/+", b"+", b"+/+", b"/#", b"a/#", b"$x", b"$x/#",
               b"a+", b"a+/+", b"+a/+", b"w/+", b"+/w", b"w/#", b"", b"/", b"//", b"+/+/+", b"a/#/b", b"#/a", b"a/+/#"]
    filters += [b"w/" + w for w in vocab[::7]] + [w + b"/+" for w in vocab[::9] if w not in (b"+", b"#")]
    assert check(s, model, filters) > len(filters) // 2
    assert s.stats()["compactions"] >= 3
    # no '$' topic under a first-level wildcard; all of them under their own literal
    assert model[b"$SYS/up"][0] not in ref_list(model, b"+/#", 0) and model[b"$SYS/up"][0] in ref_list(model, b"$SYS/+", 0)


# ---- expiry: > under match, >= under get

def test_expiry_rules_of_match_and_get(store):
    now = 10_000
    s = store(tail_max=2)                                          # some rows in the base, some in the tail
    model = {}
    topics = [b"e/never", b"e/past", b"e/now", b"e/future"]
    put(s, model, topics[:3], [1, 2, 3], [0, now - 1, now])         # three rows: compacted into the base
    put(s, model, topics[3:], [4], [now + 1])
    assert (s.stats()["base_rows"], s.stats()["tail_rows"]) == (3, 1)
    for flt in (b"e/+", b"#", b"e/now", b"e/#"):
        check(s, model, [flt], now)
    rc, hit, vals, _ = raw_match(s, [b"e/+"], now)
    assert sorted(vals.tolist()) == [1, 4], "match: expiry > now"
    vals, found = s.get(topics, now)
    assert found.tolist() == [True, False, True, True] and vals[[0, 2, 3]].tolist() == [1, 3, 4], "get: expiry >= now"
    rc, hit, vals, _ = raw_match(s, [b"e/+"], 0)
    assert sorted(vals.tolist()) == [1, 2, 3, 4], "now = 0 shows everything"
    s.compact()
    rc, hit, vals, _ = raw_match(s, [b"e/+", b"e/now", b"e/future"], now)
    assert sorted(vals[:2].tolist()) == [1, 4] and hit.tolist() == [0, 2, 2, 3]


# ---- batches, the no-launch counter, capacity

def _mixed_store(store):
    s = store(tail_max=32)
    model = {}
    topics = [b"dev/%d/%s" % (i, k) for i in range(150) for k in (b"temp", b"hum")] + [b"site/%d" % i for i in range(40)]
    put(s, model, topics, list(range(len(topics))))
    return s, model


@pytest.mark.parametrize("n", [1, 64, 257])
def test_batches_of_mixed_filters(store, n):
    s, model = _mixed_store(store)
    pool = [b"dev/7/temp", b"dev/7/#", b"+/+/temp", b"dev/+/hum", b"site/+", b"dev/7/nope", b"unknown/#", b"site/3/+", b"#",
            b"dev/149/+", b"site/39", b"dev/#/temp"]
    filters = [b"+/+/temp"] if n == 1 else [pool[i % len(pool)] if i % 5 else b"dev/%d/+" % (i % 160) for i in range(n)]
    st0 = s.stats()
    some = check(s, model, filters)
    st1 = s.stats()
    assert some >= max(1, n // 3) and st1["match_launches"] - st0["match_launches"] == 2   # (check sizes, then fills)
    if n > 1:
        assert st1["no_launch_filters"] > st0["no_launch_filters"]


def test_a_batch_the_host_answers_alone_launches_nothing(store):
    s, model = _mixed_store(store)
    st0 = s.stats()
    rc, hit, vals, err = raw_match(s, [b"unknown/#", b"dev/7/nope", b"a/#/b", b"dev/7/temp/deeper/nope"])
    st1 = s.stats()
    assert rc == TM_OK and hit.tolist() == [0] * 5 and err.tolist() == [0, 0, 2, 0]
    assert st1["match_launches"] == st0["match_launches"] and st1["no_launch_filters"] - st0["no_launch_filters"] == 8


def test_capacity(store):
    s, model = _mixed_store(store)
    filters = [b"dev/7/#", b"+/+/temp", b"site/+"]
    rc, hit, vals, _ = raw_match(s, filters)                       # cap = 0 with NULL sizes, the second call fills
    total = int(hit[-1])
    assert rc == TM_OK and total == 2 + 150 + 40
    rc, hit2, _, _ = raw_match(s, filters, cap=total - 1)          # (the canary after cap is checked inside)
    assert rc == TM_ECAP and hit2.tolist() == hit.tolist()
    assert b"room for %d" % (total - 1) in s._lib.tm_retained_last_error(None)
    rc, hit3, vals3, _ = raw_match(s, filters, cap=total + 3)
    assert rc == TM_OK and sorted(vals3[:total].tolist()) == sorted(vals.tolist())


# ---- a batch of more tiles than one launch takes

def test_a_batch_of_more_than_2_24_tiles(store):
    """A launch has fewer than 2^32 threads, 2^24 - 1 tiles of 256 rows: 66,000 full-scan filters over 65,000 base
    rows and 1,000 tail rows are 258 tiles each, 17.0M in all, and go out in two launches per pass.  Filter i is
    +/+/L<i % 6000>; row j is g/<j>/L<j % 6000> with value j: eleven hits each, j = i % 6000 (mod 6000)."""
    rows, leaves, n = 66_000, 6_000, 66_000
    s = store(tail_max=rows)
    topics = [b"g/%d/L%d" % (j, j % leaves) for j in range(rows)]
    assert (s.put(topics[:65_000], np.arange(65_000, dtype=np.uint32)) == 1).all()
    s.compact()
    assert (s.put(topics[65_000:], np.arange(65_000, rows, dtype=np.uint32)) == 1).all()
    st = s.stats()
    assert (st["base_rows"], st["tail_rows"]) == (65_000, 1_000)
    tiles = n * (-(-65_000 // RT_TILE) + -(-1_000 // RT_TILE))
    assert tiles > 1 << 24 and tiles * RT_TILE >= 1 << 32
    blob, offs = pack_strings([b"+/+/L%d" % (i % leaves) for i in range(n)])
    hit, vals, err = s.match_packed(blob, offs, 0)
    assert not err.any() and hit.tolist() == list(range(0, 11 * n + 1, 11))
    got = np.sort(vals.reshape(n, 11).astype(np.int64), axis=1)
    want = (np.arange(n) % leaves)[:, None] + leaves * np.arange(11)[None, :]
    assert np.array_equal(got, want)


# ---- churn: read your writes across compactions and growths

def test_churn_reads_its_writes(store):
    r = random.Random(0x52455431)
    s = store(tail_max=8, initial_rows=64)
    model = {}
    words = [b"a", b"b", b"c", b"", b"$s", b"d1", b"d2", b"d3"]
    topic = lambda: b"/".join(r.choice(words) for _ in range(r.randint(1, 4))) or b"a"
    filters = [b"#", b"+/#", b"a/#", b"+/+", b"a/+/+", b"$s/#", b"b/+", b"+/b/#", b"a/b", b"/#"]
    v = 0
    for step in range(200):
        c = r.random()
        if c < 0.65 or not model:
            ts = list(dict.fromkeys(topic() for _ in range(r.randint(1, 6))))
            put(s, model, ts, [v + k for k in range(len(ts))], [r.choice([0, 0, 50, 150]) for _ in ts])
            v += len(ts)
        elif c < 0.8:                                              # replace: value and expiry in place
            ts = r.sample(sorted(model), min(2, len(model)))
            put(s, model, ts, [v, v + 1][:len(ts)], [r.choice([0, 50, 150]) for _ in ts])
            v += 2
        else:
            ts = r.sample(sorted(model), min(2, len(model))) + [b"never/stored"]
            found = s.delete(ts)
            assert found.tolist() == [t in model for t in ts]
            for t in ts:
                model.pop(t, None)
        check(s, model, r.sample(filters, 4) + [topic()], r.choice([0, 100]))
    st = s.stats()
    assert st["compactions"] >= 3 and st["growths"] >= 2 and st["live_rows"] == len(model)
    before = [raw_match(s, filters, 100)[1:3] for _ in range(1)][0]
    s.compact()
    after = raw_match(s, filters, 100)[1:3]
    assert before[0].tolist() == after[0].tolist()
    for i in range(len(filters)):
        a, b = int(before[0][i]), int(before[0][i + 1])
        assert sorted(before[1][a:b].tolist()) == sorted(after[1][a:b].tolist())
    check(s, model, filters, 100)


# ---- random parity

VOCAB = short_vocabulary()


def _alphabet(r, kind):
    if kind == "ascii":
        return [b"a", b"b", b"c", b"", b"$SYS", b"$a", b"1", b"2"]
    return r.sample(VOCAB, 5) + [b"", b"$" + r.choice(VOCAB), b"\xa4", b"\0"]


def _parity_case(seed, kind):
    r = random.Random(0x454D5158 + 900 + seed)
    alpha = _alphabet(r, kind)
    topics = set()
    while len(topics) < 300:
        t = b"/".join(r.choice(alpha) for _ in range(r.randint(1, 5)))
        if t:
            topics.add(t)
    topics = sorted(topics)
    r.shuffle(topics)
    filters = []
    while len(filters) < 200:
        n = r.randint(1, 5)
        lv = [r.choices([None, b"+", b"#"], [4, 3, 1])[0] for _ in range(n)]
        lv = [(b"+" if w == b"#" and i != n - 1 else w) for i, w in enumerate(lv)]
        filters.append(b"/".join(r.choice(alpha) if w is None else w for w in lv))
    return r, topics, filters


@pytest.mark.parametrize("seed,kind", [(s, "ascii") for s in range(6)] + [(s, "bytes") for s in range(6, 12)])
def test_random_parity(store, seed, kind):
    r, topics, filters = _parity_case(seed, kind)
    s = store(tail_max=r.choice([16, 64, 512]))
    model = {}
    for k in range(0, 300, 50):
        ts = topics[k:k + 50]
        put(s, model, ts, [r.randrange(0, 1 << 32) for _ in ts], [r.choice([0, 0, 90, 110]) for _ in ts])
    share = sum(bool(ref_list(model, f, 100)) for f in filters)
    assert share * 3 >= len(filters), "the filters are drawn so that a third of them match something"
    assert check(s, model, filters, 100) == share
    check(s, model, filters, 0)


# ---- the mirror end to end: the retainer suite's two scenarios

@pytest.mark.parametrize("name", ["t_wildcard_subscription", "t_wildcard_no_$_prefix"])
def test_the_retainer_suites_scenarios_through_the_mirror(name):
    from emqx_amd.retainer import Retainer
    sc = json.loads((ROOT / "tests" / "golden" / "retainer_vectors.json").read_text())["scenarios"][name]
    rt = Retainer(initial_rows=64, tail_max=2)
    try:
        for k, t in enumerate(sc["stored"]):
            assert rt.store_retained(t.encode(), ("msg", t), timestamp=k)
        for flt, want in sc["lookups"]:
            got = rt.match_messages(flt.encode(), now=1)
            assert sorted(m[1] for m in got) == sorted(want), flt
        batch = rt.match_messages_batch([f.encode() for f, _ in sc["lookups"]], now=1)
        assert [sorted(m[1] for m in got) for got in batch] == [sorted(w) for _, w in sc["lookups"]]
        assert rt.read_message(sc["stored"][0].encode(), 1) == [("msg", sc["stored"][0])]
        rt.delete_message(sc["lookups"][0][0].encode())             # a wildcard delete
        assert rt.match_messages(sc["lookups"][0][0].encode(), now=1) == []
        assert rt.size() == len(sc["stored"]) - len(sc["lookups"][0][1])
        rt.clean()
        assert rt.size() == 0 and rt.match_messages(b"#", now=1) == []
    finally:
        rt.close()
