"""Shared by test_gpu_patch_log.py and test_gpu_commit.py: an index and the CPU
oracle fed the same deltas in the same order, exact comparison of a batch, and
a deterministic stream of small deltas.

A "patch" below is what one tm_sync makes of the deltas applied since the last
one (tm_host.cpp collect_patch): every dirty word as 16-byte run headers plus
4-byte words in one slot of the patch ring, which each copy of the tables takes
lazily.  tm_stats' `uploads` counts patches and whole-table uploads alike,
`patch_bytes` only a patch's words: a sync across which uploads rose by exactly
one and patch_bytes rose shipped one patch and no whole table.
"""
import random

import numpy as np

from emqx_amd import _native, workload as wl
from pyoracle import Oracle

PATCH_RING = 128            # tm_host.cpp: slots of the patch ring
PATCH_ZC_MAX = 64 << 10     # patches up to this size are read in place from the pinned slot
PATCH_RUN = 64              # words per run (one 16-byte header each)
RUN_HDR = 16


def items_of(strings, vals=None) -> wl.ItemSet:
    blob, offs = _native.pack_strings(strings)
    v = np.arange(len(strings), dtype=np.uint32) if vals is None else np.asarray(vals, np.uint32)
    return wl.ItemSet(blob, offs, v, np.zeros(len(strings), np.uint8))


def topic_of(flt: bytes, fill: bytes = b"w") -> bytes:
    """a topic the filter matches: '+' becomes `fill`, a trailing '#' one more level"""
    return b"/".join(fill if w in (b"+", b"#") else w for w in flt.split(b"/"))


class Pair:
    """one index and the oracle, kept in step"""

    def __init__(self, ix: _native.Index):
        self.ix, self.o = ix, Oracle()

    def apply(self, ops, d: wl.ItemSet, commit: bool = False) -> int:
        ops = np.ascontiguousarray(ops, np.uint8)
        e = self.ix.apply(ops, d.blob, d.offs, d.vals, commit=commit)
        self.o.apply(ops, d.blob, d.offs, d.vals)
        return e

    def insert(self, keys, vals, commit: bool = False) -> int:
        return self.apply(np.ones(len(keys), np.uint8), items_of(keys, vals), commit)

    def delete(self, keys, vals, commit: bool = False) -> int:
        return self.apply(np.zeros(len(keys), np.uint8), items_of(keys, vals), commit)

    def patch(self, ops, d: wl.ItemSet):
        """the deltas as one patch: apply, then tm_sync -> (uploads rise, patch_bytes rise)"""
        s0 = self.ix.stats()
        self.apply(ops, d)
        self.ix.sync()
        s1 = self.ix.stats()
        return s1["uploads"] - s0["uploads"], s1["patch_bytes"] - s0["patch_bytes"]

    def expect(self, topics: wl.ItemSet):
        """the oracle's answer for `topics` as of now (shared by the batches compared with it)"""
        self.o.prepare()
        cnt, _, ohit, ovals = self.o.match_batch(topics.blob, topics.offs)
        return cnt, ohit, ovals

    def check(self, topics: wl.ItemSet, exp=None, what: str = ""):
        """one host batch, bit-exact against the oracle: err flags, hit offsets, values in traversal order"""
        cnt, ohit, ovals = exp if exp is not None else self.expect(topics)
        n = len(topics)   # (buffers that hold the answer and more: one tm_match_batch call, one replica counted)
        out = (np.zeros(n + 1, np.uint64), np.zeros(2 * len(ovals) + 1024, np.uint32), np.zeros(max(n, 1), np.uint8))
        hit, vals, err = self.ix.match_batch(topics.blob, topics.offs, out=out)
        same(hit, vals, err, cnt, ohit, ovals, topics, what)
        return hit, vals


def same(hit, vals, err, cnt, ohit, ovals, topics, what=""):
    assert np.array_equal(err.astype(np.int64), np.where(cnt < 0, -cnt, 0)), f"{what}: badarg / too-deep flags differ"
    bad = np.nonzero(hit.astype(np.uint64) != ohit.astype(np.uint64))[0]
    assert len(bad) == 0, f"{what}: hit offsets differ from topic {int(bad[0]) - 1} ({topics.item(int(bad[0]) - 1)!r}): " \
                          f"gpu {int(hit[bad[0]])} oracle {int(ohit[bad[0]])}"
    bad = np.nonzero(vals != ovals)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(ovals)} values differ, first at {int(bad[0])}: " \
                          f"gpu {int(vals[bad[0]])} oracle {int(ovals[bad[0]])}"


def replica_batches(ix, n):
    return [ix.replica_stats(r)[0] for r in range(n)]


# ----------------------------------------------------- base set and small deltas
#
# Words per level: 30 / 120 / 200 / 250, half of them longer than VINL = 8 bytes
# (their bytes live in wpool).  ~600 words keep the vocab table at 4096 slots
# (it doubles past 1024 words and halves below 256), at most 120 children keep
# every node below WIDE_LIT, ~600 binary keys keep the exact table at 2048
# slots (it doubles past 1024 keys): the small deltas below never rehash a
# table, and every table has half its size again allocated past its end after
# the base's upload, so they never outgrow one either.

def _word(level, i):
    return (b"L%d-long-word-%04d" if i % 2 else b"l%dw%d") % (level, i)


POOL = [[_word(lv, i) for i in range(n)] for lv, n in enumerate((30, 120, 200, 250))]


def base_set(seed: int):
    """-> (keys, vals): ~2,000 mixed filters -- '+' and '#' filters, binary keys of
    2-4 levels, 250 binary keys of 12 levels (past XINL = 10: their wids live in
    wseq), and 600 filters with four ids each"""
    r = random.Random(seed)
    keys, vals, seen = [], [], set()

    def add(k, n_ids=1):
        if k in seen:
            return
        seen.add(k)
        for _ in range(n_ids):
            keys.append(k)
            vals.append(len(vals))

    while len(seen) < 1750:
        ws = [r.choice(POOL[lv]) for lv in range(r.randint(2, 4))]
        c = r.random()
        if c < 0.2:
            pass                                    # a binary key
        elif c < 0.80:
            ws[r.randrange(len(ws))] = b"+"
            if r.random() < 0.3:
                ws[r.randrange(len(ws))] = b"+"
        else:
            ws = ws[:r.randint(1, len(ws) - 1)] + [b"#"]
        add(b"/".join(ws), 4 if len(seen) % 3 == 0 else 1)
    while len(seen) < 2000:
        add(b"/".join(r.choice(POOL[lv % 4]) for lv in range(12)))
    return keys, vals


class Churn:
    """A deterministic stream of one-to-three-key deltas over base_set's keys, each
    changing at least one device word (an insert is of a (key, id) not live, a
    delete of one that is): new '+' filters over known words, filters over a new
    word longer than VINL, new binary keys of 12 levels, a second id on a live
    filter, deletes of base keys and of keys added earlier -- between them
    vocab, wpool, nodes, ctab, vals, exact, xfp and wseq."""

    def __init__(self, keys, vals, seed):
        self.r = random.Random(seed)
        self.live = list(zip(keys, vals))
        self.live_set = set(self.live)
        self.ever = list(dict.fromkeys(keys))     # every key ever live, in order
        self._ever = set(self.ever)
        self.next_val = 1_000_000
        self.n_new_words = 0
        self.kinds = []

    def _fresh(self, key):
        self.next_val += 1
        return key, self.next_val

    def _one(self):
        r = self.r
        c = r.random()
        if c < 0.42 and len(self.live) > 500:
            i = r.randrange(len(self.live))
            self.live[i], self.live[-1] = self.live[-1], self.live[i]
            kv = self.live.pop()
            self.live_set.discard(kv)
            self.kinds.append("delete")
            return 0, kv
        if c < 0.55:
            self.kinds.append("second id")
            kv = self._fresh(r.choice(self.live)[0])
        elif c < 0.67 and self.n_new_words < 60:
            self.n_new_words += 1
            w = b"new-word-longer-than-eight-%04d" % self.n_new_words
            self.kinds.append("new long word")
            kv = self._fresh(b"/".join([r.choice(POOL[0]), w] + ([b"#"] if r.random() < 0.5 else [])))
        elif c < 0.78:
            self.kinds.append("12-level binary key")
            kv = self._fresh(b"/".join(r.choice(POOL[(lv + 1) % 4]) for lv in range(12)))
        else:
            ws = [r.choice(POOL[lv]) for lv in range(r.randint(2, 4))]
            if r.random() < 0.6:
                ws[r.randrange(len(ws))] = b"+"
            self.kinds.append("filter over known words")
            kv = self._fresh(b"/".join(ws))
        self.live.append(kv)
        self.live_set.add(kv)
        if kv[0] not in self._ever:
            self.ever.append(kv[0])
            self._ever.add(kv[0])
        return 1, kv

    def delta(self):
        """-> (ops u8[k], ItemSet) for k in 1..3"""
        ops, ks, vs = [], [], []
        for _ in range(self.r.randint(1, 3)):
            op, (k, v) = self._one()
            ops.append(op)
            ks.append(k)
            vs.append(v)
        return np.array(ops, np.uint8), items_of(ks, vs)

    def probes(self, extra=()):
        """a topic for every key ever live (deleted ones included), plus misses"""
        r = random.Random(5)
        ts = [topic_of(k, r.choice(POOL[1])) for k in self.ever]
        ts += [b"/".join(r.choice(POOL[lv % 4]) for lv in range(r.randint(1, 5))) for _ in range(400)]
        ts += [b"nowhere/at/all", b"new-word-longer-than-eight-9999/x", b"", b"/"]
        return items_of(ts + list(extra))


def run_small_patches(pair: Pair, churn: Churn, n: int, max_bytes: int = 12 << 10):
    """n deltas, each followed by tm_sync; every one must arrive as exactly one
    patch of under max_bytes and no whole-table upload -> uploads rise over the loop"""
    up0 = pair.ix.stats()["uploads"]
    for k in range(n):
        ops, d = churn.delta()
        du, db = pair.patch(ops, d)
        what = f"delta {k} ({', '.join(churn.kinds[-len(ops):])})"
        assert 0 < db < max_bytes, f"{what}: patch_bytes rose by {db}"
        assert du == 1, f"{what}: uploads rose by {du}: a whole-table upload brought every copy up"
    return pair.ix.stats()["uploads"] - up0
