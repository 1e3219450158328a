"""The walk kernels' tokeniser scan (tm_scan.h) and child hash (tm_layout.h
child_hash) on the device, bit-exact against the CPU oracle: values, their
order, counts and err flags.

* a node grown by deltas through the child-table thresholds (4 -> 5 literal
  children: inline -> private table; 28 -> 29: the summaries' Bloom saturates;
  255 -> 257: wide node with a bitmap) and shrunk back, checked after every
  apply;
* one adversarial topic set -- word ends at every byte offset mod 16, words of
  0, 1, 7, 8, 9, 16 and 17 bytes, empty levels, a '$' first level, lone '+' /
  '#' levels at the first, a middle, the last and a past-the-8th level, topics
  of 8, 9, 10, 33 and 65 levels -- through four kernel paths: device pairs
  (k_walk_pairs + k_tail_pairs), the device CSR on the two-phase path
  (k_walk_fast + tails), and 4,096-topic host batches on k_walk_small with 16
  and with 8 lanes per topic (the fallback lane walk).
"""
import random

import numpy as np
import pytest

from emqx_amd import _native, workload as wl
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

WORD_LENS = (0, 1, 7, 8, 9, 16, 17)
LEVELS = (1, 2, 3, 4, 5, 6, 8, 9, 10, 33, 65)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def items_of(strings, vals=None) -> wl.ItemSet:
    blob, offs = _native.pack_strings(strings)
    v = np.arange(len(strings), dtype=np.uint32) if vals is None else np.asarray(vals, np.uint32)
    return wl.ItemSet(blob, offs, v, np.zeros(len(strings), np.uint8))


def _vocab(r):
    """words of every length the scan treats differently (inline up to 8
    bytes, parked by position from 9), a few of each, plus short fillers"""
    out = [b""]
    for n in WORD_LENS[1:] + (2, 3, 4, 5):
        for k in range(4):
            out.append(bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(n)))
    return out


def _filters(r, vocab):
    """about 5k mixed filters of at most 6 levels (so the 8-lane small kernel's
    fallback lane walk applies): literal paths, '+' levels, '#' endings, '$'
    first levels, several IDs on some"""
    fs = [b"#", b"+/#", b"+", b"$SYS/#", b"$SYS/+/x", b"+/+/+/+/+/+", b"/", b"//", b"/#", b"+/"]
    while len(fs) < 5000:
        n = r.randint(1, 6)
        ws = [r.choice(vocab[:12]) if l < 2 else r.choice(vocab) for l in range(n)]
        ws = [b"+" if r.random() < 0.25 else w for w in ws]
        if r.random() < 0.05:
            ws[0] = r.choice([b"$SYS", b"$", b"$share12"])
        if r.random() < 0.3:
            ws = ws[:5] + [b"#"]
        fs.append(b"/".join(ws))
    fs += r.sample(fs, 300)   # the same filter under further IDs: multi-value runs
    return fs


def _topics(r, vocab, filters):
    ts = []
    for L in LEVELS:
        for _ in range(770):
            f = r.choice(filters).split(b"/")
            ws = [r.choice(vocab) if w in (b"+", b"#") else w for w in f][:L]
            while len(ws) < L:
                ws.append(r.choice(vocab))
            if r.random() < 0.1:
                ws[r.randrange(L)] = b""          # an empty level
            if r.random() < 0.05:
                ws[0] = r.choice([b"$SYS", b"$", b"$share12"])
            ts.append(b"/".join(ws))
    # lone '+' / '#' levels (badarg) at the first, a middle, the last and a past-the-8th level
    for L, at in ((1, 0), (3, 0), (3, 1), (3, 2), (8, 7), (10, 8), (10, 9), (33, 20), (33, 32), (65, 64), (65, 40)):
        for c in (b"+", b"#"):
            for _ in range(25):
                ws = [r.choice(vocab[1:]) for _ in range(L)]
                ws[at] = c
                ts.append(b"/".join(ws))
    # '+' / '#' inside a longer word is no wildcard; empty levels at the ends
    ts += [b"", b"/", b"//", b"///", b"a//b", b"/a", b"a/", b"/a/", b"+a/b", b"a+/#b", b"a/#b/c", b"$", b"$/a", b"$SYS",
           b"$SYS/a/x", b"$SYS//x"]
    ts += [b"/".join([w] * k) for w in vocab[:8] for k in (1, 2, 8, 9)]
    r.shuffle(ts)
    return ts


def _expect(o, ts):
    cnt, _, ohit, ovals = o.match_batch(ts.blob, ts.offs)
    return np.where(cnt < 0, -cnt, 0), np.maximum(cnt, 0), ohit, ovals


def _check_csr(got, exp, what):
    hit, vals, err = got
    oerr, ocnt, ohit, ovals = exp
    assert np.array_equal(np.asarray(err).astype(np.int64), oerr), f"{what}: err flags differ"
    assert np.array_equal(np.diff(np.asarray(hit).astype(np.int64)), ocnt), f"{what}: hit counts differ"
    assert np.array_equal(vals, ovals), f"{what}: values / order differ"


def _check_pairs(torch, ix, ts, exp, what):
    """tm_match_batch_dev_pairs: every topic's span holds the oracle's values in order"""
    oerr, ocnt, ohit, ovals = exp
    dev = torch.device("cuda:0")
    n = len(ts)
    cap = int(ohit[-1]) + 4096 * int(ocnt.max() if n else 0)
    blob = torch.from_numpy(ts.blob.copy()).to(dev)
    offs = torch.from_numpy(ts.offs.view(np.int64).copy()).to(dev)
    pairs = torch.full((2 * n + 2,), -1, dtype=torch.int32, device=dev)
    out = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev)
    err = torch.full((max(n, 1),), 7, dtype=torch.uint8, device=dev)
    ix.match_batch_dev_pairs(n, blob.data_ptr(), offs.data_ptr(), pairs.data_ptr(), out.data_ptr(), cap,
                             err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    p = pairs.cpu().numpy().view(np.uint32)
    pr = p[:2 * n].reshape(n, 2).astype(np.int64)
    vals = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(err.cpu().numpy()[:n].astype(np.int64), oerr), f"{what}: err flags differ"
    assert np.array_equal(pr[:, 1], ocnt), f"{what}: hit counts differ"
    assert int(p[2 * n]) == int(ohit[-1]) and int(p[2 * n + 1]) <= cap, f"{what}: total / extent"
    live = np.nonzero(pr[:, 1])[0]
    # gather every span and compare with the oracle's CSR in one go
    idx = np.concatenate([np.arange(pr[i, 0], pr[i, 0] + pr[i, 1]) for i in live]) if len(live) else np.zeros(0, np.int64)
    assert np.array_equal(vals[idx], ovals), f"{what}: values / order differ"
    order = live[np.argsort(pr[live, 0], kind="stable")]
    assert np.all(pr[order[1:], 0] >= (pr[order, 0] + pr[order, 1])[:-1]), f"{what}: spans overlap"


def _check_dev_csr(torch, ix, ts, exp, what):
    """tm_match_batch_dev on the two-phase path (TM_DEBUG_PHASES): k_walk_fast + tails"""
    oerr, ocnt, ohit, ovals = exp
    n, cap = len(ts), int(ohit[-1]) + 1
    d_blob, d_offs = torch.from_numpy(ts.blob.copy()).cuda(), torch.from_numpy(ts.offs.view(np.int64).copy()).cuda()
    d_hit = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_err = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_out = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    ix.debug_set(_native.TM_DEBUG_PHASES, 1)
    p0 = ix.debug_get(_native.TM_DEBUG_PATH_PHASES)
    try:
        ix.match_batch_dev(n, d_blob.data_ptr(), d_offs.data_ptr(), d_hit.data_ptr(), d_out.data_ptr(), cap,
                           d_err.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        ix.debug_set(_native.TM_DEBUG_PHASES, 0)
    assert ix.debug_get(_native.TM_DEBUG_PATH_PHASES) > p0, f"{what}: not the two-phase path"
    _check_csr((d_hit.cpu().numpy().view(np.uint64), d_out.cpu().numpy().view(np.uint32)[:cap - 1], d_err.cpu().numpy()),
               exp, what)


@pytest.fixture(scope="module")
def case():
    r = random.Random(0x5CA11)
    vocab = _vocab(r)
    filters = _filters(r, vocab)
    fs = items_of(filters)
    ix, o = _native.Index(), Oracle()
    for t in (ix, o):
        t.apply(np.ones(len(fs), np.uint8), fs.blob, fs.offs, fs.vals)
    o.prepare()
    topics = _topics(r, vocab, filters)
    return ix, o, topics, len(filters)


def test_adversarial_set_covers_the_scan_cases(case):
    """the set is what the docstring says (no device work)"""
    _, _, topics, _ = case
    assert 8500 <= len(topics) <= 9500
    ts = items_of(topics)
    ends, lens, levels = set(), set(), set()
    for i, t in enumerate(topics):
        beg = int(ts.offs[i])
        ws = t.split(b"/")
        levels.add(len(ws))
        pos = beg
        for w in ws:
            lens.add(len(w))
            pos += len(w)
            ends.add(pos % 16)   # the '/' (or the topic's end) after the word
            pos += 1
    assert ends == set(range(16))
    assert set(WORD_LENS) <= lens and {8, 9, 10, 33, 65} <= levels
    assert any(t.startswith(b"$") for t in topics) and any(b"//" in t for t in topics)


def test_adversarial_set_pairs(torch_dev, case):
    ix, o, topics, _ = case
    ts = items_of(topics)
    exp = _expect(o, ts)
    assert exp[0].any() and exp[1].max() > 8   # badarg topics, and more than RCAP value ranges
    _check_pairs(torch_dev, ix, ts, exp, "pairs")


def test_adversarial_set_two_phase(torch_dev, case):
    ix, o, topics, _ = case
    ts = items_of(topics)
    _check_dev_csr(torch_dev, ix, ts, _expect(o, ts), "two-phase")


@pytest.mark.parametrize("kind", ["wave", "wave8"])
def test_adversarial_set_small_kernel(torch_dev, case, kind):
    """4,096-topic host batches on k_walk_small: 16 lanes per topic, and 8
    lanes with the fallback lane walk for topics past 8 levels"""
    ix, o, topics, _ = case
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


def test_node_grown_and_shrunk_through_the_table_thresholds(torch_dev, case):
    """literal children of `grow` (and of the root's '+' child) added by deltas
    through 4 -> 5, 28 -> 29 and 255 -> 257 and erased back, every step checked
    on the host CSR, the device pairs and the two-phase path"""
    ix, o, _, base = case
    kids = [b"c%d" % i for i in range(257)]

    def fam(i):
        return [b"grow/" + kids[i], b"grow/" + kids[i] + b"/t%d" % (i % 5), b"+/" + kids[i] + b"/#",
                b"grow/+/" + kids[i]]

    probe = [b"grow/" + k for k in kids] + [b"grow/" + k + b"/t%d" % j for k in kids[::7] for j in range(5)] + \
            [b"zz/" + k + b"/q" for k in kids[::5]] + [b"grow/x/" + k for k in kids[::3]] + \
            [b"grow", b"grow/", b"grow/nochild", b"grow/c1/none", b"grow/c300"]
    pts = items_of(probe)
    have = 0
    for target in (4, 5, 28, 29, 255, 257, 255, 29, 28, 5, 4, 0):
        ids = range(have, target) if target > have else range(target, have)
        strings = [f for i in ids for f in fam(i)]
        vals = [base + 4 * i + k for i in ids for k in range(4)]
        d = items_of(strings, vals)
        op = np.full(len(strings), 1 if target > have else 0, np.uint8)
        ix.apply(op, d.blob, d.offs, d.vals)
        o.apply(op, d.blob, d.offs, d.vals)
        o.prepare()
        have = target
        exp = _expect(o, pts)
        _check_csr(ix.match_batch(pts.blob, pts.offs), exp, f"host CSR at {target} children")
        _check_pairs(torch_dev, ix, pts, exp, f"pairs at {target} children")
        _check_dev_csr(torch_dev, ix, pts, exp, f"two-phase at {target} children")
