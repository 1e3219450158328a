"""Seeded scenarios for the host index compiler, shared by test_image_cpu.py (the
CPU device fake under sanitizers) and test_gpu_image_script.py (the real
library): one generator, two runners.

A scenario is a list of steps -- ``apply`` / ``commit`` (ops, filters, values,
key flags), ``check`` (probe topics with the oracle's answers: counts, CSR, err
flags, first hit) and ``mfcheck`` (filter queries with Oracle.matches_filter's
answers).  write() puts one into the simple binary file
tests/host_cpu/image_check.cpp reads.

Probes.  For every key ever live in the scenario the full probe family is: the
key itself with its wildcards replaced, that topic one level shorter and one
level longer, and that topic with each single level swapped for a word known
elsewhere in the vocabulary and for a word unknown to it.  After a step, the
whole family of every key the step touched is sent (a lost match shows where it
happens); no check is larger than PROBE_CAP topics, so a step that touched many
keys is followed by several check steps -- the probes are split, never thinned
-- and the room the last of them has left takes other keys' families in
rotation.  Script.finish() asserts that every family topic of every key ever
live was sent.  A few fixed odd topics ride along (empty
levels, a '+' level, '$' words).

Each scenario names the constants it crosses; they are read here from the
sources (tm_layout.h, tm_host.cpp), so a changed constant moves the scenario
with it.
"""
from __future__ import annotations

import random
import re
import struct
import zlib
from pathlib import Path

import numpy as np

import bytes_vocab

ROOT = Path(__file__).resolve().parent.parent
_LAYOUT = (ROOT / "emqx_amd" / "csrc" / "tm_layout.h").read_text()
_HOST = (ROOT / "emqx_amd" / "csrc" / "tm_host.cpp").read_text()


def _const(src, name):
    m = re.search(r"constexpr\s+\w+\s+(?:[A-Z_0-9]+\s*=\s*[^,;]+,\s*)*?%s\s*=\s*([0-9xA-Fa-f]+)u?" % name, src)
    assert m, name
    return int(m.group(1), 0)


KINL = _const(_LAYOUT, "KINL")
WIDE_LIT = _const(_LAYOUT, "WIDE_LIT")
PSUM_BLOOM = _const(_LAYOUT, "PSUM_BLOOM")
XINL = _const(_LAYOUT, "XINL")
VINL = _const(_LAYOUT, "VINL")
PATCH_RING = _const(_HOST, "PATCH_RING")
TABLE_FLOOR = 1024          # tm_host.cpp init_tables / reclaim: vocab and exact never shrink below
assert "ix->vocab.h.assign(1024" in _HOST and "ix->exact.h.size() > 1024" in _HOST
assert (KINL, WIDE_LIT, PSUM_BLOOM, XINL, VINL) == (4, 256, 28, 10, 8), "the scenarios' sizes follow these"

PROBE_CAP = 1500
KEY_WORDS, KEY_EMPTY_LIST, KEY_ESCAPED = 1, 2, 4
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

# claims: audit kinds a scenario says it exercises; the driver fails if the count is zero
CLAIMS = ["wide_bitmaps", "hints_both", "qq_saturated", "exact_wrapped", "ctab_wrapped", "wpool_compaction",
          "wseq_compaction", "vocab_shrink", "exact_shrink", "node_reuse", "wid_reuse", "hdesc", "dense_both",
          "mfilter", "wide_to_narrow", "ring_wrap", "rehash_annexed"]


# ---- the hashes of tm_layout.h (scenario 4 picks keys by their home slots)

def mix64(x):
    x ^= x >> 30; x = x * 0xbf58476d1ce4e5b9 & M64
    x ^= x >> 27; x = x * 0x94d049bb133111eb & M64
    return x ^ x >> 31


def child_hash(wid):
    x = (wid + 0x9e3779b9) & M32
    x ^= x >> 16; x = x * 0x7feb352d & M32
    x ^= x >> 15; x = x * 0x846ca68b & M32
    return x ^ x >> 16


def seq_hash(wids):
    h = 0xcbf29ce484222325
    for w in wids:
        h = (h ^ w) * 0x100000001b3 & M64
    return mix64((h + 0x9e3779b97f4a7c15 * (len(wids) + 1)) & M64)


assert "x ^= x >> 16; x *= 0x7feb352du;" in _LAYOUT and "x ^= x >> 15; x *= 0x846ca68bu;" in _LAYOUT
assert "return (h ^ wid) * FNV_PRIME" in _LAYOUT and "mix64(h + 0x9e3779b97f4a7c15ull * (nlev + 1))" in _LAYOUT


# ---- steps

class Step:
    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)


def _pack(items):
    offs = np.zeros(len(items) + 1, np.uint64)
    if items:
        offs[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    blob = np.frombuffer(b"".join(items) + b"\0" * 16, dtype=np.uint8)
    return blob, offs


def topic_of(key: bytes, fill: bytes) -> list:
    """the levels of a topic the filter matches: '+' and a '#' become `fill`"""
    return [fill if w in (b"+", b"#") else w for w in key.split(b"/")]


class Script:
    """Builds one scenario: keeps the oracle in step with the deltas and computes every check's expectations."""

    ODD = [b"", b"/", b"//", b"a//b", b"+/x", b"x/#", b"$SYS/x", b"$x", b"never-seen-word"]

    def __init__(self, name, seed, claims=(), mf=False):
        from pyoracle import Oracle
        self.name, self.r, self.o = name, random.Random(seed), Oracle()
        self.steps, self.claims = [], list(claims)
        assert all(c in CLAIMS for c in claims)
        self.live, self.ever, self._ever = set(), [], set()
        self.touched, self.rot = [], 0
        self.fam, self.sent = {}, set()
        self.words, self._words = [], set()
        self.mf = mf
        self.extra_topics = []
        self.n_deltas = 0

    # deltas: kv = [(key, value)] or [(key, value, flags)]
    def _delta(self, op, kv, commit):
        if not kv:
            return
        keys, vals, flags = [], [], []
        for e in kv:
            k, v, f = (e + (0,))[:3]
            keys.append(k); vals.append(v); flags.append(f)
            if op:
                self.live.add((k, v, f))
            else:
                self.live.discard((k, v, f))
            if not f & KEY_ESCAPED and not f & KEY_EMPTY_LIST:
                if k not in self._ever:
                    self._ever.add(k); self.ever.append(k)
                self.touched.append(k)
                for w in k.split(b"/"):
                    if w not in (b"+", b"#") and w not in self._words:
                        self._words.add(w); self.words.append(w)
        ops = np.full(len(keys), op, np.uint8)
        blob, offs = _pack(keys)
        vals, flags = np.asarray(vals, np.uint32), np.asarray(flags, np.uint8)
        # the oracle never learns the escaped keys: their '/'-, '+'- or '#'-words can match no topic
        keep = [i for i, f in enumerate(flags) if not f & KEY_ESCAPED]
        if keep:
            kb, ko = _pack([keys[i] for i in keep])
            self.o.apply(ops[keep], kb, ko, vals[keep], flags[keep])
        self.steps.append(Step("commit" if commit else "apply", ops=ops, blob=blob, offs=offs, vals=vals, flags=flags))
        self.n_deltas += 1

    def insert(self, kv, commit=False):
        self._delta(1, kv, commit)

    def delete(self, kv, commit=False):
        self._delta(0, kv, commit)

    def mixed(self, ops_kv, commit=False):
        """one delta of mixed ops: [(op, key, value[, flags])], applied in order"""
        run, cur = [], None
        for e in ops_kv:   # (the oracle and the index both take them in order; split into runs of one op)
            if cur is not None and e[0] != cur:
                self._delta(cur, run, commit); run = []
            cur = e[0]; run.append(tuple(e[1:]))
        if run:
            self._delta(cur, run, commit)

    def family(self, key):
        """the probe family of a key, fixed when the key is first seen (the known word is one live then)"""
        if key not in self.fam:
            r = random.Random(zlib.crc32(key))
            lv = topic_of(key, b"fill")
            known = self.words[r.randrange(len(self.words))] if self.words else b"known"
            out = [lv, lv[:-1], lv + [known]]
            for i in range(len(lv)):
                out.append(lv[:i] + [known] + lv[i + 1:])
                out.append(lv[:i] + [b"unknown-%d" % i] + lv[i + 1:])
            self.fam[key] = [b"/".join(t) for t in out if t]
        return self.fam[key]

    def probes(self):
        """-> the check's topics in chunks of at most PROBE_CAP: the odd topics, the whole family of every key
        touched since the last check, then -- in the room the last chunk has left -- other keys' families in rotation"""
        seen, out = set(), []

        def add(ts):
            for t in ts:
                if t not in seen:
                    seen.add(t); out.append(t)
        add(self.ODD + self.extra_topics)
        for k in dict.fromkeys(reversed(self.touched)):
            add(self.family(k))
        self.touched = []
        room = -len(out) % PROBE_CAP
        n, used = len(self.ever), 0
        while used < n and room > 0:
            f = [t for t in self.family(self.ever[(self.rot + used) % n]) if t not in seen]
            if len(f) > room:
                break
            add(f)
            room -= len(f)
            used += 1
        self.rot = (self.rot + used) % n if n else 0
        self.sent.update(out)
        return [out[i:i + PROBE_CAP] for i in range(0, len(out), PROBE_CAP)]

    def check(self, label):
        """one check step per chunk of probes: a step that touched many keys is followed by several checks
        (the probes are never thinned), each within what a GPU test may cost"""
        chunks = self.probes()
        self.o.prepare()
        for i, topics in enumerate(chunks):
            blob, offs = _pack(topics)
            cnt, _, hit, vals = self.o.match_batch(blob, offs)
            found = np.where(cnt == -1, 2, np.where(cnt == -2, 3, (cnt > 0).astype(np.int64))).astype(np.uint8)
            first = np.zeros(len(topics), np.uint32)
            has = cnt > 0
            first[has] = vals[hit[:-1][has].astype(np.int64)]
            part = label if len(chunks) == 1 else "%s, probes %d of %d" % (label, i + 1, len(chunks))
            self.steps.append(Step("check", label=part, topics=topics, blob=blob, offs=offs, cnt=cnt.astype(np.int64),
                                   hit=hit.astype(np.uint64), vals=vals.astype(np.uint32), found=found, first=first))

    def finish(self):
        """every topic of every family of every key ever live was sent in some check, and no check is past the cap"""
        missing = [t for k in self.ever for t in self.family(k) if t not in self.sent]
        assert not missing, (self.name, len(missing), missing[:3])
        assert all(len(st.topics) <= PROBE_CAP for st in self.steps if st.kind == "check")
        assert self.steps[-1].kind in ("check", "mfcheck") and not self.touched
        return self

    def mfcheck(self, label, n=100):
        r = random.Random(len(self.steps))
        qs = []
        pool = self.words[:400] or [b"w"]
        while len(qs) < n:
            ws = [r.choice(pool) for _ in range(r.randint(1, 4))]
            c = r.random()
            if c < 0.5:
                ws[r.randrange(len(ws))] = b"+"
            if c < 0.25 or c > 0.85:
                ws = ws + [b"#"]
            if c > 0.95:
                ws = [b"#"]
            if 0.6 < c < 0.7 and self.ever:
                ws = r.choice(self.ever).split(b"/")
            qs.append(b"/".join(ws))
        hit, vals = [0], []
        for q in qs:
            v = self.o.matches_filter(q)
            vals += v
            hit.append(len(vals))
        blob, offs = _pack(qs)
        self.steps.append(Step("mfcheck", label=label, topics=qs, blob=blob, offs=offs, hit=np.asarray(hit, np.uint64),
                               vals=np.asarray(vals, np.uint32)))


def write(scn: Script, path):
    """The file image_check.cpp reads: little endian, no padding.  'TMIS' u32 version, u32 claim bits, u32 PATCH_RING, the name, then per
    step u32 kind (1 apply, 2 commit, 3 check, 4 mfcheck, 0 end) and its arrays, each array a u64 count + data."""
    def arr(a, dt):
        a = np.ascontiguousarray(a, dt)
        return struct.pack("<Q", len(a)) + a.tobytes()

    def text(s):
        b = s.encode()
        return struct.pack("<Q", len(b)) + b
    bits = sum(1 << CLAIMS.index(c) for c in scn.claims)
    out = [b"TMIS", struct.pack("<III", 2, bits, PATCH_RING), text(scn.name)]
    for s in scn.steps:
        if s.kind in ("apply", "commit"):
            out += [struct.pack("<I", 1 if s.kind == "apply" else 2), arr(s.ops, np.uint8), arr(s.flags, np.uint8),
                    arr(s.vals, np.uint32), arr(s.offs, np.uint64), arr(s.blob, np.uint8)]
        elif s.kind == "check":
            out += [struct.pack("<I", 3), text(s.label), arr(s.offs, np.uint64), arr(s.blob, np.uint8), arr(s.cnt, np.int64),
                    arr(s.hit, np.uint64), arr(s.vals, np.uint32), arr(s.found, np.uint8), arr(s.first, np.uint32)]
        else:
            out += [struct.pack("<I", 4), text(s.label), arr(s.offs, np.uint64), arr(s.blob, np.uint8), arr(s.hit, np.uint64),
                    arr(s.vals, np.uint32)]
    out.append(struct.pack("<I", 0))
    Path(path).write_bytes(b"".join(out))


# ---- the scenarios

def _tails(i):
    """what keeps child i alive, as tests/test_gpu_vocab_hints.py::_family lists: a '#' terminal, an exact
    terminal, a '+' child, a '+' chain, a '#' that is not last (NLIT_HDESC), literals only"""
    return {0: [b"#"], 1: [b""], 2: [b"+"], 3: [b"+/yb"], 4: [b"#/zz"], 5: [b"xa", b"xb/yb"]}.get(i % 10, [b"xa"])


def _kids(prefix, tag, lo, hi, base):
    """the filters below children lo .. hi - 1 of node `prefix`, all in word-list form (trie paths); every
    eighth child word longer than VINL"""
    out = []
    for i in range(lo, hi):
        w = (b"%s-long-kid-%04d" if i % 8 == 7 else b"%s%03d") % (tag, i)
        for j, t in enumerate(_tails(i)):
            k = prefix + b"/" + w + (b"/" + t if t else b"")
            wild = any(x in (b"+", b"#") for x in k.split(b"/"))
            out.append((k, base + 4 * i + j, 0 if wild else KEY_WORDS))   # (a word list: a trie path, not a binary key)
    return out


def _ladder(top):
    """child counts that straddle KINL, PSUM_BLOOM, WIDE_LIT and every table doubling (a table of c slots
    doubles when its c/2-th child arrives) up to `top`"""
    marks = {KINL, PSUM_BLOOM, WIDE_LIT} | {1 << k for k in range(3, 12)}
    pts = sorted({p for m in marks for p in (m - 1, m, m + 1) if 0 < p < top} | {top})
    return pts


def children_of_one_node(top=600):
    """1. Children of one node, 0 -> 600 -> 0, under five parents at once: a literal node, the root's '+'
    child (its saturation shows in the root's psum), a '+' child's '+' child (the QQ half of the root's psum
    and of the slot its grandparent keeps), the '+' child of a literal child of a table-mode node (the QQ half
    of a CSlot.sum) and a child of an annexed wide node (a hint's folded Bloom).  Crosses KINL (4 <-> 5), every
    table doubling, PSUM_BLOOM (28 <-> 29) and WIDE_LIT (255 <-> 256) in both directions, with a check after
    every step that crosses one.  Each parent has its own child words, so none of the wide nodes is dense and
    their bitmaps are audited.  Probes: the family of every key touched by the step, the rest in rotation."""
    s = Script("children", 11, ["wide_bitmaps", "qq_saturated", "hdesc", "wide_to_narrow", "hints_both"])
    parents = [(b"n", b"a"), (b"+", b"b"), (b"+/+", b"c"), (b"t/x/+", b"d"), (b"W/k000", b"e")]
    # a table-mode parent for t/x, and two wide nodes at depth 1 that get the annex slots (W and V)
    s.insert([(b"t/s%d/q" % i, 900_000 + i, KEY_WORDS) for i in range(8)])
    s.insert(_kids(b"W", b"k", 0, WIDE_LIT + 20, 800_000) + _kids(b"V", b"v", 0, WIDE_LIT + 10, 700_000))
    s.check("the frame")
    prev = 0
    for p in _ladder(top):
        s.insert([kv for j, (pre, tag) in enumerate(parents) for kv in _kids(pre, tag, prev, p, 100_000 * (j + 1))])
        s.check("up to %d children" % p)
        prev = p
    for p in reversed([0] + _ladder(top)[:-1]):
        s.delete([kv for j, (pre, tag) in enumerate(parents) for kv in _kids(pre, tag, p, prev, 100_000 * (j + 1))])
        s.check("down to %d children" % p)
        prev = p
    return s.finish()


def dense_and_annex():
    """2. Dense switch and annex.  Two wide nodes at depth 1 (d1, d2) share their 300 child words: each holds
    all of level 1's distinct words -- dense (share >= 3/5), bitmap pointer NONE.  250 other words appear at
    level 1 elsewhere: their share falls to 300/550 < 3/5 -- bitmaps consulted -- and rises again when those
    go.  Both hold the annex slots; a third wide node d3 grows to twice d2's children and takes its slot (the
    vocab rehashes on the way, both slots held); d1 falls below WIDE_LIT and releases its slot, which d2
    takes back.  Probes as in scenario 1."""
    s = Script("dense_annex", 12, ["wide_bitmaps", "hints_both", "dense_both", "wide_to_narrow", "rehash_annexed"])
    n = WIDE_LIT + 44

    def shared(pre, lo, hi, base):   # d1 and d2 use the same child words
        return _kids(pre, b"s", lo, hi, base)
    s.insert(shared(b"d1", 0, n, 100_000) + shared(b"d2", 0, n - 10, 200_000) + [(b"#", 1), (b"+/+/xa", 2), (b"d1/+/xb/yb", 3)])
    s.check("two dense wide nodes")
    other = [(b"o%d/u%03d/xa" % (i % 7, i), 300_000 + i) for i in range(250)]
    s.insert(other)
    s.check("share below 3/5: bitmaps")
    s.delete(other[:125]); s.check("half of the other words gone")
    s.delete(other[125:]); s.check("dense again")
    s.insert(other[:200]); s.check("and not dense")
    third = _kids(b"d3", b"z", 0, 2 * n + 8, 400_000)
    cut = len(third) // 3
    s.insert(third[:cut]); s.check("d3 wide, not twice as wide")
    s.insert(third[cut:]); s.check("d3 took a slot; the vocab rehashed")
    few, gone = shared(b"d1", n - 30, n, 100_000), shared(b"d1", 40, n - 30, 100_000)
    s.delete(few); s.check("d1 narrower, still wide and annexed: d2 keeps the words, their hints for d1 are 0")
    s.delete(gone); s.check("d1 below WIDE_LIT")
    s.insert(gone + few); s.check("d1 wide again")
    s.delete(third); s.check("d3 gone")
    s.delete(other[:200] + shared(b"d2", 0, n - 10, 200_000)); s.check("d2 gone")
    return s.finish()


def table_growth():
    """3. Table growth and shrink.  The vocab passes its growth load (1/4 of TABLE_FLOOR words) and falls
    below its shrink load (1/16 of the doubled table); the exact table likewise (grows at 1/2, shrinks at
    1/8); wpool is compacted (over 64 KiB of long words, more than half erased); wseq is compacted (over
    16 Ki wids of binary keys of 11 and 12 levels, more than half erased), with keys of XINL = 10 levels
    beside them.  matches_filter runs against the oracle after growth and after shrink (snapshot, log replay,
    upload).  Probes: the whole family of every key a step touched (the 2,000 deep keys alone fill some 40
    check steps when they go in), the rest in rotation."""
    s = Script("tables", 13, ["vocab_shrink", "exact_shrink", "wpool_compaction", "wseq_compaction", "mfilter"], mf=True)
    r = s.r
    s.insert([(b"base/+/x", 1), (b"base/#", 2), (b"+/b/c", 3)])
    s.check("small")
    short = [(b"g/w%04d" % i, 10_000 + i, KEY_WORDS) for i in range(TABLE_FLOOR // 4 + 60)]
    s.insert(short[:TABLE_FLOOR // 4 - 40]); s.check("vocab below its growth load")
    s.insert(short[TABLE_FLOOR // 4 - 40:]); s.check("vocab doubled")
    s.mfcheck("after vocab growth")
    binary = [(b"x/k%04d" % (i % 90) + b"/m%d" % (i // 90), 20_000 + i) for i in range(TABLE_FLOOR // 2 + 80)]
    s.insert(binary[:TABLE_FLOOR // 2 - 30]); s.check("exact below its growth load")
    s.insert(binary[TABLE_FLOOR // 2 - 30:]); s.check("exact doubled")
    longw = [(b"lw/" + (b"%04d-" % i) * 48 + b"/#", 30_000 + i) for i in range(290)]   # 240-byte words: 68 KiB
    assert sum((len(k) - 5 + 3) & ~3 for k, _ in longw) > 64 << 10
    s.insert(longw); s.check("long words in")
    pool = [[b"p%d_%d" % (lv, j) for j in range(9)] for lv in range(12)]
    deep, seen = [], set()
    while len(deep) < 2000:
        n = (11, 12, 12, 11, 10)[len(deep) % 5]
        k = b"/".join(r.choice(pool[lv]) for lv in range(n))
        if k not in seen:
            seen.add(k); deep.append((k, 40_000 + len(deep)))
    assert sum(len(k.split(b"/")) for k, _ in deep if len(k.split(b"/")) > XINL) > 16 << 10
    s.insert(deep); s.check("deep binary keys in")
    s.delete(longw[:200]); s.check("wpool compacted")
    s.delete(deep[:1500]); s.check("wseq compacted")
    s.delete(binary[:len(binary) - 100]); s.check("exact shrunk")
    s.delete(short[:len(short) - 20] + longw[200:] + deep[1500:]); s.check("vocab shrunk")
    s.mfcheck("after the shrinks")
    s.insert(short[:50] + binary[:50] + deep[:50]); s.check("and some back")
    return s.finish()


def erase_paths():
    """4. Erase paths: backward-shift erase in `exact` and `ctab` over runs of colliding home slots that wrap
    the table's end.  The index is fresh and every key below brings at most one new word, so a word's wid is
    the order of its first appearance: the generator computes child_hash and seq_hash itself, gives node "c"
    seven children whose home slots in its 16-slot table are 13..15 (the words whose homes are elsewhere go
    to a filler node), and picks binary keys over the known words whose home slots in the TABLE_FLOOR-slot
    exact table are its last three.  It asserts that both runs wrap; every key is then deleted, one delta
    each, in a shuffled order that shifts entries back across the wrap, with a check after each.  Probes:
    every family at every check."""
    s = Script("erase", 14, ["exact_wrapped", "ctab_wrapped"])
    keys, wid = [(b"c/#", 1), (b"f/#", 2)], {b"c": 0, b"f": 1}
    ckids = []
    while len(ckids) < 7:
        w, i = b"w%03d" % len(wid), len(wid)
        wid[w] = i
        if child_hash(i) & 15 >= 13:
            ckids.append(w)
            keys.append((b"c/" + w + b"/#", 100 + i))
        else:
            keys.append((b"f/" + w + b"/#", 100 + i))
    slots = {}
    for w in ckids:   # the table's linear probing, children in insertion order
        p = child_hash(wid[w]) & 15
        while p in slots:
            p = (p + 1) & 15
        slots[p] = w
    assert any(p < (child_hash(wid[w]) & 15) for p, w in slots.items()), "no child slot wraps its table's end"
    s.insert(keys)
    pool, r, xs, seen = sorted(wid, key=wid.get), s.r, [], set()
    for _ in range(2_000_000):
        ws = [r.choice(pool) for _ in range(r.randint(2, 4))]
        k = b"/".join(ws)
        if k not in seen and seq_hash([wid[w] for w in ws]) & (TABLE_FLOOR - 1) >= TABLE_FLOOR - 3:
            seen.add(k)
            xs.append((k, 500 + len(xs)))
            if len(xs) == 8:
                break
    assert len(xs) == 8, "no binary keys found for the exact table's last slots"   # (8 keys, 3 homes: the run wraps)
    s.insert(xs)
    s.check("both runs in place")
    order = xs[:]
    r.shuffle(order)
    for kv in order:
        s.delete([kv]); s.check("binary key %r gone" % kv[0])
    order = [kv for kv in keys if kv[0].startswith(b"c/w")]
    r.shuffle(order)
    for kv in order:
        s.delete([kv]); s.check("child %r gone" % kv[0])
    s.insert(xs[:4] + order[:6]); s.check("some back")
    return s.finish()


def values():
    """5. Values.  Runs going 0 -> 1 (inline, RUN_INLINE) -> 2 -> 40 -> 1 -> 0 on a '#' terminal, on exact
    terminals of word-list keys (a '+' filter and a TM_KEY_WORDS key) and on a binary key; the same value on
    two keys; full-range u32 values (bytes_vocab.full_range_values).  A check after every change of a run's
    form.  Probes: every family, every check."""
    s = Script("values", 15)
    vals = bytes_vocab.full_range_values(s.r, 44)
    keys = [(b"v/a/#", 0), (b"v/+/b", 0), (b"v/c", KEY_WORDS), (b"v/d/e", 0), (b"v/d/e/f0/f1/f2/f3/f4/f5/f6/f7/f8", 0)]
    s.insert([(b"v/a/x", 7), (b"other/#", 7)])   # the same value on two keys
    for lo, hi in ((0, 1), (1, 2), (2, 40)):
        s.insert([(k, v, f) for k, f in keys for v in vals[lo:hi]])
        s.check("runs of %d" % hi)
    s.insert([(k, v, f) for k, f in keys for v in vals[:5]])   # present already: no-ops
    s.check("inserting again changes nothing")
    for lo, hi in ((1, 40), (0, 1)):
        s.delete([(k, v, f) for k, f in keys for v in vals[lo:hi]])
        s.check("runs down to %d" % lo)
    s.delete([(k, v, f) for k, f in keys for v in vals[:3]])   # absent already
    s.insert([(k, vals[41 + i % 3], f) for i, (k, f) in enumerate(keys)])
    s.check("one value each again")
    return s.finish()


def odd_forms():
    """6. '#'-not-last keys and odd forms.  NLIT_HDESC appears on and disappears from a node without '+'
    ancestors (h), below a '+' (+/h2) and on a '+' child (g/+), each beside '+', '#' and literal siblings that
    match, so the seek past the '+' subtree and the cut at the topic's end decide results; escaped word-list
    keys (words "+", "#" and one holding a '/': they match no topic, and leave the image when deleted), the
    empty word list, empty levels in keys and topics, a topic of 65,537 levels (err 2), '+' / '#' topic levels
    (err 1).  matches_filter against the oracle before and after.  Probes: every family, every check."""
    s = Script("odd", 16, ["hdesc", "mfilter"], mf=True)
    s.extra_topics = [b"h", b"h/w", b"h/w/x", b"q/h2", b"q/h2/w", b"g/q", b"g/q/y", b"g/q/w/z", b"/" * 65536, b"/" * 65535,
                      b"a/+", b"#", b"h/#"]
    base = [(b"h/+", 1), (b"h/w", 2), (b"h/#", 3), (b"h/+/x", 4), (b"h/w/x", 5), (b"h", 6, KEY_WORDS), (b"+/h2/+", 7),
            (b"+/h2/w", 8), (b"+/h2", 9), (b"q/h2/w", 10), (b"+/+/w", 11), (b"g/+/y", 12), (b"g/+/+/z", 13), (b"g/+/w/z", 14),
            (b"g/q", 15), (b"#", 16), (b"a//b", 17), (b"/", 18), (b"", 19), (b"+//#", 20), (b"/#", 21), (b"//", 22, KEY_WORDS)]
    s.insert(base); s.check("no '#'-not-last key yet")
    s.mfcheck("before")
    hd = [(b"h/#/x", 30), (b"+/h2/#/y/z", 31), (b"g/+/#/y", 32), (b"h/#/+", 33)]
    for kv in hd:
        s.insert([kv]); s.check("%r in" % kv[0])
    s.mfcheck("with the '#'-not-last keys")
    esc = KEY_WORDS | KEY_ESCAPED
    odd = [(b"e/\\+", 40, esc), (b"e\\/f/g", 41, esc), (b"\\#", 42, esc), (b"e/\\#/x", 43, esc), (b"", 44, KEY_EMPTY_LIST),
           (b"e/pl\\ain", 45, esc)]
    s.insert(odd[:5]); s.check("escaped keys and [] in")
    s.delete(odd[:5]); s.check("and out")
    for kv in hd:
        s.delete([kv]); s.check("%r out" % kv[0])
    s.delete(base[:8]); s.check("half of the base out")
    s.mfcheck("after")
    return s.finish()


def reuse():
    """7. Node and word reuse: a subtree of 300 filters over words of its own is deleted whole, then as many
    different filters over other words are inserted.  The driver asserts that node ids and wids the first
    subtree held were handed out again (ids stay small, so the image shows it).  Probes: the whole family of every key a step touched, the
    rest in rotation."""
    s = Script("reuse", 17, ["node_reuse", "wid_reuse"])
    s.insert([(b"keep/+/k", 1), (b"keep/a/#", 2)])
    one = [(b"r1/a%03d/b%03d" % (i, i % 17) + (b"/#" if i % 3 == 0 else b"/+" if i % 3 == 1 else b""), 1000 + i) for i in range(300)]
    two = [(b"r2/c%03d/d%03d" % (i % 150, i) + (b"/#" if i % 2 == 0 else b""), 5000 + i) for i in range(300)]
    s.insert(one); s.check("the first subtree")
    s.delete(one); s.check("gone")
    s.insert(two); s.check("other filters in its place")
    s.delete(two[:150]); s.insert(one[:100]); s.check("mixed")
    return s.finish()


def churn(n_deltas=3000, every=100):
    """8. Random churn over the byte vocabulary of bytes_vocab.py: `n_deltas` deltas of one to three keys
    (filters of 1 to 4 levels, '+' and '#' mixed in, binary keys, TM_KEY_WORDS keys, second values on live
    filters, deletes of live keys), a check every `every`.  With two copies the driver's alternating commits
    wrap the patch ring (PATCH_RING patches).  Probes: the whole family of every key touched since
    the last check, the rest in rotation."""
    s = Script("churn", 18, ["ring_wrap"])
    r = s.r
    voc = bytes_vocab.short_vocabulary()
    live = []
    for d in range(n_deltas):
        ops = []
        for _ in range(r.randint(1, 3)):
            c = r.random()
            if c < 0.4 and len(live) > 200:
                i = r.randrange(len(live))
                live[i], live[-1] = live[-1], live[i]
                ops.append((0,) + live.pop())
                continue
            if c < 0.5 and live:
                k, _, f = r.choice(live)
                kv = (k, r.randrange(0, 1 << 20), f)
            else:
                ws = [r.choice(voc[:120] if r.random() < 0.7 else voc) for _ in range(r.randint(1, 4))]
                f = 0
                c2 = r.random()
                if c2 < 0.45:
                    ws[r.randrange(len(ws))] = b"+"
                if 0.3 < c2 < 0.55:
                    ws = ws + [b"#"]
                elif c2 > 0.9:
                    f = KEY_WORDS
                kv = (b"/".join(ws), r.randrange(0, 1 << 20), f)
            if kv not in live:
                live.append(kv)
                ops.append((1,) + kv)
        s.mixed(ops)
        if (d + 1) % every == 0:
            s.check("after %d deltas" % (d + 1))
    return s.finish()


SCENARIOS = {
    "children": children_of_one_node,
    "dense_annex": dense_and_annex,
    "tables": table_growth,
    "erase": erase_paths,
    "values": values,
    "odd": odd_forms,
    "reuse": reuse,
    "churn": churn,
}
