"""The retained-message store without a device: the golden vectors of the
reference's suites (tests/golden/retainer_vectors.json) against a restatement
of emqx_topic:match/2 and against the mirror's matcher; the exports, the ABI
minor, each ctypes signature against the header's prototype, RT_COLS / RT_TILE
in _native and in the device header; the null-handle refusals; and
emqx_amd.retainer.Retainer's host-only behaviour over a pure-Python stand-in
for _native.Retained defined here (table full, wildcard delete, page_read,
clear_expired, the > of match against the >= of read).
"""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from emqx_amd import _native, retainer
from emqx_amd.retainer import Retainer

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "retainer_vectors.json").read_text())
CALLS = ("tm_retained_create", "tm_retained_destroy", "tm_retained_put", "tm_retained_delete", "tm_retained_get",
         "tm_retained_match", "tm_retained_expire", "tm_retained_compact", "tm_retained_stats", "tm_retained_last_error")


# ---- the restatement (emqx_topic.erl:80-116; emqx_retainer_mnesia.erl:464-466, :510), independent of the mirror's

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


def visible_to_match(expiry, now):
    return expiry == 0 or expiry > now


def visible_to_read(expiry, now):
    return expiry == 0 or expiry >= now


class StandIn:
    """_native.Retained's interface in pure Python over the restatement"""

    def __init__(self):
        self.rows = {}   # topic -> (value, expiry), in insertion order
        self.closed = False

    def put(self, topics, values, expiry_ms=None):
        out = []
        for i, t in enumerate(topics):
            if not t or any(w in (b"+", b"#") for w in t.split(b"/")):
                out.append(2)
                continue
            out.append(0 if t in self.rows else 1)
            self.rows[t] = (int(values[i]), int(expiry_ms[i]) if expiry_ms is not None else 0)
        return np.array(out, np.uint8)

    def delete(self, topics):
        return np.array([self.rows.pop(t, None) is not None for t in topics], bool)

    def get(self, topics, now_ms=0):
        rows = [self.rows.get(t) for t in topics]
        found = [r is not None and visible_to_read(r[1], now_ms) for r in rows]
        return np.array([r[0] if f else 0 for r, f in zip(rows, found)], np.uint32), np.array(found, bool)

    def match(self, filters, now_ms=0):
        return [np.array([v for t, (v, e) in self.rows.items() if visible_to_match(e, now_ms) and ref_match(t, f)
                          and b"#" not in f.split(b"/")[:-1]], np.uint32) for f in filters]

    def expire(self, deadline_ms, limit=0):
        gone = [t for t, (v, e) in self.rows.items() if e != 0 and e < deadline_ms]
        take = gone[:limit] if limit else gone
        vals = [self.rows.pop(t)[0] for t in take]
        return (len(take) < limit if limit else True), np.array(vals, np.uint32)

    def stats(self):
        return {"live_rows": len(self.rows)}

    def close(self):
        self.closed = True


# ---- the golden vectors

ROWS = [(name, t, f, m) for name, rows in GOLDEN["match"].items() for t, f, m in rows]


def test_the_fixture_holds_the_suites_rows():
    assert {k: len(v) for k, v in GOLDEN["match"].items()} == {
        "t_match1": 13, "t_match2": 17, "t_match3": 6, "t_sigle_level_match": 9, "t_sys_match": 4, "t_#_match": 5,
        "t_match_tokens": 4}
    assert set(GOLDEN["scenarios"]) == {"t_wildcard_subscription", "t_wildcard_no_$_prefix"}
    assert (ROOT / "tests" / "golden" / "retainer_vectors.json").stat().st_size < 8192


@pytest.mark.parametrize("name,topic,flt,want", ROWS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(ROWS)])
def test_golden_rows_pin_the_restatement_and_the_mirror(name, topic, flt, want):
    assert ref_match(topic.encode(), flt.encode()) is want
    assert retainer.topic_match(topic.encode(), flt.encode()) is want


@pytest.mark.parametrize("name", sorted(GOLDEN["scenarios"]))
def test_golden_scenarios_over_the_stand_in(name):
    sc = GOLDEN["scenarios"][name]
    rt = Retainer(store=StandIn)
    for k, t in enumerate(sc["stored"]):
        assert rt.store_retained(t.encode(), t, timestamp=k)
    for flt, want in sc["lookups"]:
        assert sorted(rt.match_messages(flt.encode(), now=5)) == sorted(want)
        assert sorted(t for t in sc["stored"] if ref_match(t.encode(), flt.encode())) == sorted(want)
    if name == "t_wildcard_no_$_prefix":
        assert sorted(rt.match_messages(b"#", now=5)) == ["/t/3", "t/1", "t/2"]
        assert sorted(rt.match_messages(b"+/+", now=5)) == ["t/1", "t/2"]
        assert rt.match_messages(b"+/t/#", now=5) == ["/t/3"]
        assert len(rt.match_messages(b"$test/#", now=5)) == 2


def test_the_restatement_beyond_the_suites():
    cases = [(b"a", b"a/#", True), (b"a/", b"a/#", True), (b"a/b/c", b"a/#", True), (b"ab", b"a/#", False),
             (b"a+", b"a+", True), (b"ab", b"a+", False), (b"a/b", b"a/#/b", False), (b"", b"", True), (b"/", b"+/+", True),
             (b"$x", b"+", False), (b"$x", b"$x", True), (b"a/$x", b"a/+", True), (b"\xa4x", b"+", True)]
    for t, f, want in cases:
        assert ref_match(t, f) is want and retainer.topic_match(t, f) is want, (t, f)
    assert retainer.is_wildcard(b"a/+/b") and retainer.is_wildcard(b"#") and not retainer.is_wildcard(b"a+/b#")


# ---- the ABI

def test_exports_abi_minor_and_constants():
    lib = _native.load_library()
    for name in CALLS:
        assert name in _native.EXPORTS and hasattr(lib, name), name
    v = lib.tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 24
    dev = (ROOT / "emqx_amd" / "csrc" / "tm_retain.h").read_text()
    assert f"RT_COLS = {_native.RT_COLS};" in dev and f"RT_TILE = {_native.RT_TILE};" in dev
    assert (_native.RT_COLS, _native.RT_TILE) == (8, 256)
    assert hasattr(_native, "Retained") and hasattr(retainer, "Retainer")
    from emqx_amd import build
    assert build.RETAIN_SOURCE == "tm_retain.hip" and build.RETAIN_HOST_SOURCE == "tm_retain_host.cpp"
    assert build.RETAIN_SOURCE not in build.KERNEL_SOURCES and build.RETAIN_HOST_SOURCE not in build.KERNEL_SOURCES
    host = (ROOT / "emqx_amd" / "csrc" / "tm_host.cpp").read_text()
    assert "launch_ret_" not in host and "tm_retain" not in host, "tm_host.cpp calls no new launcher"


def test_the_ctypes_signatures_are_the_headers_prototypes():
    header = (ROOT / "include" / "tmatch.h").read_text()
    lib = _native.load_library()
    plain = {"int": C.c_int, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    res = {"int": C.c_int, "const char *": C.c_char_p}
    counts = {}
    for name in CALLS:
        m = re.search(r"^(int|const char \*) ?%s\((.*?)\);" % name, header, re.S | re.M)
        assert m, f"{name}'s prototype is in the header"
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        fn = getattr(lib, name)
        assert fn.restype == res[m.group(1)], name
        assert len(fn.argtypes) == len(params), name
        for p, a in zip(params, fn.argtypes):
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
                if p.startswith("uint64_t *out_n"):
                    assert a is C.POINTER(C.c_uint64)
                if p.startswith("int *"):
                    assert a is C.POINTER(C.c_int)
            else:
                assert a is plain[p.rsplit(" ", 1)[0]], (name, p)
        counts[name] = len(params)
    assert counts["tm_retained_match"] == 9 and counts["tm_retained_put"] == 7 and counts["tm_retained_expire"] == 7
    # the structs, field by field
    m = re.search(r"typedef struct \{([^{}]*)\} tm_retained_stats_t;", header)
    fields = re.findall(r"\b(\w+)(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in _native.tm_retained_stats_t._fields_] and len(fields) == 12
    assert all(t is C.c_uint64 for _, t in _native.tm_retained_stats_t._fields_)
    assert _native.tm_retained_opts._fields_ == [("initial_rows", C.c_uint32), ("tail_max", C.c_uint32)]
    assert "typedef struct { uint32_t initial_rows" in " ".join(header.split())


def test_every_call_cites_the_reference():
    header = " ".join((ROOT / "include" / "tmatch.h").read_text().replace(" * ", " ").split())
    for name, cite in (("tm_retained_put", ":207-224"), ("tm_retained_delete", ":271-275"), ("tm_retained_get", ":510"),
                       ("tm_retained_match", "emqx_topic.erl:80-116"), ("tm_retained_expire", ":231-234"),
                       ("tm_retained_stats", ":541-542")):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/ int %s\(" % name, header)
        assert m and cite in m.group(1), name


def test_null_handles_are_refused():
    lib = _native.load_library()
    E = _native.TM_EINVAL
    assert lib.tm_retained_create(0, None, None) == E
    assert lib.tm_retained_put(None, 0, None, None, None, None, None) == E
    assert b"tm_retained_put" in lib.tm_retained_last_error(None)
    assert lib.tm_retained_delete(None, 0, None, None, None) == E
    assert lib.tm_retained_get(None, 0, None, None, 0, None, None) == E
    assert lib.tm_retained_match(None, 0, None, None, 0, None, None, 0, None) == E
    assert lib.tm_retained_expire(None, 0, 0, None, 0, None, None) == E
    assert lib.tm_retained_compact(None) == E and lib.tm_retained_stats(None, None) == E
    assert b"tm_retained_stats" in lib.tm_retained_last_error(None)
    assert lib.tm_retained_destroy(None) == E


# ---- the mirror over the stand-in

def test_store_retained_refuses_a_new_topic_when_the_table_is_full():
    rt = Retainer(store=StandIn, max_retained_messages=2)
    assert rt.store_retained(b"a", 1) and rt.store_retained(b"b", 2)
    assert rt.store_retained(b"c", 3) is False and rt.size() == 2 and rt.read_message(b"c", 0) == []
    assert rt.store_retained(b"a", 4) is True and rt.read_message(b"a", 0) == [4], "a stored topic is replaced"
    rt.delete_message(b"b")
    assert rt.store_retained(b"c", 3) is True and sorted(rt.topics()) == [b"a", b"c"]
    unlimited = Retainer(store=StandIn)
    assert all(unlimited.store_retained(b"t/%d" % i, i) for i in range(50)) and unlimited.size() == 50
    with pytest.raises(ValueError):
        unlimited.store_retained(b"t/+", 1)
    # an invalid topic takes no value slot, neither a fresh one nor a freed one
    unlimited.delete_message(b"t/7")
    slots = (list(unlimited._free), unlimited._next)
    for bad in (b"t/+", b"#", b""):
        with pytest.raises(ValueError):
            unlimited.store_retained(bad, 1)
    assert (list(unlimited._free), unlimited._next) == slots
    assert unlimited.store_retained(b"t/new", 5) and unlimited._free == [] and unlimited._next == slots[1]
    assert unlimited.store_retained(b"t/newer", 6) and unlimited._next == slots[1] + 1


def test_a_wildcard_delete_takes_expired_rows_too():
    rt = Retainer(store=StandIn)
    for t, e in ((b"a/1", 0), (b"a/2", 5), (b"a/3/x", 0), (b"b/1", 0), (b"$a/1", 0)):
        rt.store_retained(t, t, expiry_time=e)
    assert rt.match_messages(b"a/+", now=100) == [b"a/1"], "a/2 has expired for a lookup"
    rt.delete_message(b"a/+")                                      # (now = 0: :277)
    assert sorted(rt.topics()) == [b"$a/1", b"a/3/x", b"b/1"]
    rt.delete_message(b"#")
    assert rt.topics() == [b"$a/1"], "'#' does not reach a '$' topic"
    rt.delete_message(b"nothing/here")
    rt.delete_message(b"$a/1")
    assert rt.size() == 0
    assert rt.store_retained(b"z", 9) and rt.read_message(b"z", 0) == [9], "a freed value slot is used again"


def test_match_is_greater_than_and_read_is_greater_or_equal():
    rt = Retainer(store=StandIn)
    now = 1000
    for t, e in ((b"e/never", 0), (b"e/past", now - 1), (b"e/now", now), (b"e/future", now + 1)):
        rt.store_retained(t, t, expiry_time=e)
    assert sorted(rt.match_messages(b"e/+", now)) == [b"e/future", b"e/never"]
    assert [rt.read_message(t, now) for t in (b"e/never", b"e/past", b"e/now", b"e/future")] == \
        [[b"e/never"], [], [b"e/now"], [b"e/future"]]
    assert len(rt.match_messages(b"e/+", 0)) == 4
    assert rt.match_messages_batch([b"e/now", b"e/#", b"x"], now) == [[], rt.match_messages(b"e/#", now), []]


def test_clear_expired_with_and_without_a_limit():
    rt = Retainer(store=StandIn)
    for i in range(6):
        rt.store_retained(b"x/%d" % i, i, expiry_time=10 + i)
    rt.store_retained(b"keep", 7)
    rt.store_retained(b"later", 8, expiry_time=500)
    assert rt.clear_expired(100, 4) == (False, 4) and rt.size() == 4
    assert rt.clear_expired(100, 2) == (False, 2), "exactly `limit` rows: the stream was not seen to end"
    assert rt.clear_expired(100, 2) == (True, 0) and rt.clear_expired(100) == (True, 0)
    assert sorted(rt.topics()) == [b"keep", b"later"]
    assert rt.clear_expired(501) == (True, 1) and rt.topics() == [b"keep"]
    assert rt.clear_expired(10**9, 0) == (False, 0)


def test_page_read_sorts_by_timestamp_and_pages():
    rt = Retainer(store=StandIn)
    stamps = [50, 10, 40, 20, 30, 60, 5]
    for i, ts in enumerate(stamps):
        rt.store_retained(b"p/%d" % i, ts, expiry_time=0 if i != 5 else 100, timestamp=ts)
    rt.store_retained(b"$q/1", 1, timestamp=1)
    assert rt.page_read(b"p/+", 0, 1, 3) == (True, [5, 10, 20])
    assert rt.page_read(b"p/+", 0, 2, 3) == (True, [30, 40, 50])
    assert rt.page_read(b"p/+", 0, 3, 3) == (False, [60])
    assert rt.page_read(b"p/+", 100, 3, 3) == (False, []), "the deadline hides the expired row"
    assert rt.page_read(b"p/+", 0, 1, 7) == (True, sorted(stamps)), "a full page says more, as the reference's does"
    assert rt.page_read(None, 0, 1, 10) == (False, [1] + sorted(stamps)), "no filter: every row, '$' topics too"
    assert rt.page_read(b"#", 0, 1, 10) == (False, sorted(stamps))


def test_clean_starts_a_fresh_store():
    made = []

    def factory():
        made.append(StandIn())
        return made[-1]
    rt = Retainer(store=factory)
    rt.store_retained(b"a", 1)
    rt.clean()
    assert made[0].closed and len(made) == 2 and rt.size() == 0 and rt.match_messages(b"#", 0) == []
    assert "msg_expiry_interval_override" in retainer.__doc__
