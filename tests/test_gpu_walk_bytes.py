"""The full byte range and full-range u32 values through every walk path.

MQTT topics are UTF-8 and the reference treats them as arbitrary binaries;
every other GPU test feeds ASCII topics and small integer values.  One seeded
case over the byte vocabulary of bytes_vocab.py (every one-byte word, NUL runs
that differ in length alone, the high-bit twins and neighbours of '/', '+',
'#', '$', UTF-8 words of 7-17 bytes, long words differing in their last byte,
words of 251-257 bytes), about 5k filters of at most 6 levels and about 8k
topics.  Stored values are a seeded sample of distinct u32 with the edges of
the signed range; filters repeated under several values give multi-value runs,
the others inline runs (RUN_INLINE: the value itself in the run's offset field).

Every vocabulary word w has a filter lit/<w> with a value of its own and a
topic lit/<w>: a word mistaken for a twin shows as a missing or a foreign
value.  Exact against the CPU oracle on values, order, counts and err flags
through: device pairs, the two-phase device CSR, 4,096-topic host batches on
k_walk_small with 16 and 8 lanes, first_batch, the host CSR in TM_ORDER_SORTED
and matches_filter_batch.  No topic is left out of any comparison.
"""
import random

import numpy as np
import pytest

from bytes_vocab import full_range_values, length_words, short_vocabulary, vocabulary
from emqx_amd import _native
from pyoracle import Oracle
from test_gpu_parity import _sorted_ref
from test_gpu_walk_scan import _check_csr, _check_dev_csr, _check_pairs, _expect, items_of

pytestmark = pytest.mark.gpu

ROOT_FILTERS = (b"#", b"+/#")
LEVELS = (1, 2, 3, 4, 5, 6, 8, 9)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _filters(r, vocab, head):
    """-> filters (bytes) in insertion order: the root filters, lit/<w> for
    every word, fixed edge filters, random ones, then 300 repeats"""
    fs = list(ROOT_FILTERS) + [b"lit/" + w for w in vocab]
    fs += [b"+", b"lit/+", b"lit/#", b"+/+", b"$SYS/#", b"$/+", b"\xa4/#", b"\xa4/+", b"\xa4SYS/#", b"/", b"//", b"/#",
           b"+/", b"\0/#", b"\0\0/+", b"+/+/+/+/+/+", b"+/\xaf/#", b"\xaf/+/\xab"]
    while len(fs) < 5000:
        n = r.randint(1, 6)
        ws = [r.choice(head) if l < 2 else r.choice(vocab) for l in range(n)]
        ws = [b"+" if r.random() < 0.25 else w for w in ws]
        if r.random() < 0.05:
            ws[0] = r.choice([b"$SYS", b"$", b"$\xa4", b"\xa4"])
        if r.random() < 0.3:
            ws = ws[:5] + [b"#"]
        fs.append(b"/".join(ws))
    fs += r.sample(fs[2 + len(vocab):], 300) + r.sample(fs[2:2 + len(vocab)], 40)   # further values: multi-value runs
    return fs


def _topics(r, vocab, head, filters):
    ts = [b"lit/" + w for w in vocab]
    for L in LEVELS:
        for _ in range(900):
            f = r.choice(filters).split(b"/")
            ws = [r.choice(head if l < 2 else vocab) if w in (b"+", b"#") else w for l, w in enumerate(f)][:L]
            while len(ws) < L:
                ws.append(r.choice(vocab))
            if r.random() < 0.1:
                ws[r.randrange(L)] = b""
            if r.random() < 0.05:
                ws[0] = r.choice([b"$SYS", b"$", b"$\xa4", b"\xa4", b"\xa4SYS"])
            ts.append(b"/".join(ws))
    for L, at in ((1, 0), (3, 0), (3, 1), (3, 2), (6, 5), (9, 8)):   # badarg: a lone '+' / '#' level
        for c in (b"+", b"#"):
            for _ in range(20):
                ws = [r.choice(vocab) for _ in range(L)]
                ws[at] = c
                ts.append(b"/".join(ws))
    ts += [b"", b"/", b"//", b"\0", b"\0/\0", b"\0\0/a/b", b"$", b"$/a", b"$SYS/a", b"$\xa4/a", b"\xa4", b"\xa4/a",
           b"\xa4SYS/a/b", b"\xa4x", b"\xaf", b"\xaf/\xaf", b"\xab/\xa3", b"a\xaf/+\xab", b"\xaf/x/\xab", b"\x2e/\x30"]
    r.shuffle(ts)
    return ts


@pytest.fixture(scope="module")
def data():
    """the case without the device: vocabulary, filters and values, topics, the oracle and its expectation"""
    r = random.Random(0xB17E5)
    vocab = vocabulary()
    head = r.sample(short_vocabulary(), 14) + [b"", b"\0", b"\0\0", b"a", b"\xaf", b"\xab", b"\xa3", b"\xa4", b"\x2e", b"\x30"]
    filters = _filters(r, vocab, head)
    vals = full_range_values(r, len(filters))
    r.shuffle(vals)
    fs = items_of(filters, vals)
    o = Oracle()
    o.apply(np.ones(len(fs), np.uint8), fs.blob, fs.offs, fs.vals)
    o.prepare()
    topics = _topics(r, vocab, head, filters)
    ts = items_of(topics)
    return {"vocab": vocab, "filters": filters, "vals": vals, "fs": fs, "o": o, "topics": topics, "ts": ts,
            "exp": _expect(o, ts)}


@pytest.fixture(scope="module")
def case(data):
    ix = _native.Index()
    fs = data["fs"]
    ix.apply(np.ones(len(fs), np.uint8), fs.blob, fs.offs, fs.vals)
    return ix


def test_byte_set_is_what_it_claims(data):
    """the oracle's expectation tells every word from its twins, the set covers
    the byte range and the sizes named above (no device work)"""
    vocab, filters, vals, topics = data["vocab"], data["filters"], data["vals"], data["topics"]
    oerr, ocnt, ohit, ovals = data["exp"]
    assert 5000 <= len(filters) <= 5500 and 7500 <= len(topics) <= 8500
    assert len(set(vals)) == len(vals) == len(filters)
    for e in (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE):
        assert e in vals
    assert max(len(f.split(b"/")) for f in filters) <= 6
    assert len(set(filters)) < len(filters) - 300 + 1        # repeats: several values on one filter
    # lit/<w>: the word's own value, and no other word's
    own = {b"lit/" + w: set() for w in vocab}
    for f, v in zip(filters, vals):
        if f in own:
            own[f].add(v)
    lit_vals = set().union(*own.values())
    at = {t: i for i, t in enumerate(topics)}
    for w in vocab:
        i = at[b"lit/" + w]
        got = set(ovals[int(ohit[i]):int(ohit[i + 1])].tolist())
        assert oerr[i] == 0 and own[b"lit/" + w] and got & lit_vals == own[b"lit/" + w], w
    # every byte but '/' in some topic and in some filter
    for strings in (topics, filters):
        seen = set(b"".join(strings))
        assert seen == set(range(256)), sorted(set(range(256)) - seen)
        words = {w for s in strings for w in s.split(b"/")}
        assert all(bytes([b]) in words for b in range(256) if b not in b"/+#")
    # topics at the staging limit of k_walk_small (SM_TB = 256 bytes), and past 255-byte words
    assert {255, 256, 257} <= {len(t) for t in topics}
    assert {251, 252, 253, 254, 255, 256, 257} <= {len(w) for w in length_words()}
    # a first level beginning with 0xA4 ('$' | 0x80) is an ordinary word; '$' is not
    root = {f: v for f, v in zip(filters, vals) if f in ROOT_FILTERS}
    assert len(root) == 2
    n_a4 = n_dollar = 0
    for i, t in enumerate(topics):
        if oerr[i] or b"/" not in t:
            continue
        got = set(ovals[int(ohit[i]):int(ohit[i + 1])].tolist())
        if t.startswith(b"\xa4"):
            assert set(root.values()) <= got, t
            n_a4 += 1
        elif t.startswith(b"$"):
            assert not set(root.values()) & got, t
            n_dollar += 1
    assert n_a4 > 20 and n_dollar > 20
    assert (oerr != 0).sum() >= 200 and ocnt.max() > 8 and (ocnt > 0).sum() > 7000


def test_byte_set_pairs(torch_dev, case, data):
    _check_pairs(torch_dev, case, data["ts"], data["exp"], "pairs")


def test_byte_set_two_phase(torch_dev, case, data):
    _check_dev_csr(torch_dev, case, data["ts"], data["exp"], "two-phase")


@pytest.mark.parametrize("kind", ["wave", "wave8"])
def test_byte_set_small_kernel(torch_dev, case, data, kind):
    """4,096-topic host batches on k_walk_small with 16 and with 8 lanes per topic"""
    ix, o, topics = case, data["o"], data["topics"]
    ix.debug_set(_native.TM_DEBUG_SMALL_KERNEL, {"wave": _native.SMALL_WAVE, "wave8": _native.SMALL_WAVE8}[kind])
    try:
        for lo in range(0, len(topics), 4096):
            ts = items_of(topics[lo:lo + 4096])
            p0 = ix.debug_get(_native.TM_DEBUG_PATH_SMALL)
            got = ix.match_batch(ts.blob, ts.offs)
            assert ix.debug_get(_native.TM_DEBUG_PATH_SMALL) > p0, f"{kind}: not k_walk_small"
            _check_csr(got, _expect(o, ts), f"{kind} batch at {lo}")
    finally:
        ix.debug_set(_native.TM_DEBUG_SMALL_KERNEL, _native.SMALL_AUTO)


def test_byte_set_first_batch(torch_dev, case, data):
    """match/2: found flags and the first value in traversal order, every topic"""
    o, topics, ts = data["o"], data["topics"], data["ts"]
    val, found = case.first_batch(ts.blob, ts.offs)
    exp = [o.first(t) for t in topics]
    efound = np.array([{-1: 2, -2: 3, 0: 0, 1: 1}[r] for r, _ in exp], np.uint8)
    evals = np.array([v for _, v in exp], np.uint32)
    assert np.array_equal(found, efound)
    hit = efound == 1
    assert hit.sum() > 7000 and np.array_equal(val[hit], evals[hit])


def test_byte_set_sorted_host_csr(torch_dev, case, data):
    """TM_ORDER_SORTED on full-range values: np.sort of the oracle's lists"""
    ts = data["ts"]
    oerr, ocnt, ohit, ovals = data["exp"]
    exp_s, _ = _sorted_ref(ohit, ovals)
    h, v, err = case.match_batch(ts.blob, ts.offs, order=_native.TM_ORDER_SORTED)
    assert np.array_equal(err.astype(np.int64), oerr) and np.array_equal(h, ohit.astype(np.uint64))
    assert np.array_equal(v, exp_s)
    assert (ovals >= 1 << 31).any() and (ovals < 1 << 31).any()


def test_byte_set_matches_filter(torch_dev):
    """200 filter queries over 300 stored filters of the byte vocabulary: the
    word ranks tm_matches_filter compares are in byte order"""
    r = random.Random(0xF117E5)
    vocab = short_vocabulary()
    pool = r.sample(vocab, 12) + [b"", b"\0", b"\0\0", b"a", b"a\0", b"$", b"\xa4", b"\xaf", b"\xab", b"\xa3", b"\x7f", b"\x80",
                                  b"\xff"]

    def flt(wild, hash_anywhere):
        n = r.randint(1, 5)
        out = []
        for i in range(n):
            p = r.choices(["level", "+", "#"], wild)[0]
            if p == "#" and not hash_anywhere and i != n - 1:
                p = "+"
            out.append(b"#" if p == "#" else b"+" if p == "+" else r.choice(pool if r.random() < 0.8 else vocab))
        return b"/".join(out)

    filters = [flt([6, 2, 1], True) for _ in range(300)]
    wf = np.array([1 if r.random() < 0.1 else 0 for _ in filters], np.uint8)
    vals = full_range_values(r, len(filters))
    items = items_of(filters, vals)
    ix, o = _native.Index(), Oracle()
    ix.apply(np.ones(len(items), np.uint8), items.blob, items.offs, items.vals, wf)
    for f, v, w in zip(filters, vals, wf):
        o.insert(f, v, int(w))
    qs = [flt([4, 3, 1], False) for _ in range(200)]
    blob, offs = _native.pack_strings(qs)
    hit, got, err = ix.matches_filter_batch(blob, offs)
    assert not err.any()
    n_hits = 0
    for i, q in enumerate(qs):
        exp = o.matches_filter(q)
        assert got[int(hit[i]):int(hit[i + 1])].tolist() == exp, q
        n_hits += len(exp) > 1
    assert n_hits > 40
