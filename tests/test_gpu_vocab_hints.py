"""Vocab-entry hints (tm_layout.h HINT_*): the main walks skip the child-table
probe of an annexed node when the hint carried by the level word's vocab entry
says the child is absent or cannot matter.  Every batch below is compared
bit-exactly with the CPU oracle fed the same deltas, in the pairs form
(k_walk_pairs) and the CSR form (k_walk_fast) at 70,000 topics -- the smallest
batch that takes those kernels -- and after every delta batch of a churn that
moves the hints: children appearing and vanishing under the annexed nodes,
summaries changing below them, a slot re-designated, the vocab rehashed, an
annexed node dropping below WIDE_LIT.  TM_DEBUG_HINT_AUDIT compares every hint
in the host image with the child slot it copies after each step.
"""
import random

import numpy as np
import pytest

from emqx_amd import _native
from delta_transport import Pair, items_of

pytestmark = pytest.mark.gpu

N_TOPICS = 70_000
NW = 320                      # children of each annexed node (WIDE_LIT = 256)
UNUSED = (1 << 64) - 1


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _w(i):
    """level-2 words: every eighth one longer than VINL = 8 bytes (no hint: probed as before)"""
    return b"long-child-%04d" % i if i % 8 == 7 else b"w%03d" % i


def _family(prefix, i, base):
    """the filters below child _w(i) of node `prefix`: what keeps the child alive differs by i"""
    w, k = _w(i), i % 10
    tails = {0: [b"#"],                       # a '#' terminal
             1: [b""],                        # an exact terminal (topics of depth + 1 levels end there)
             2: [b"+"],                       # a '+' child
             3: [b"+/yb"],
             4: [b"#/zz"],                    # a '#' that is not last: NLIT_HDESC on the child
             5: [b"xa", b"xb/yb"]}.get(k, [b"xa"])   # literals only
    return [(prefix + b"/" + w + (b"/" + t if t else b""), base + 8 * i + j) for j, t in enumerate(tails)]


def _base():
    fs = []
    for i in range(NW):
        fs += _family(b"+/+", i, 100_000)     # (+,+): the widest node, slot 0
        fs += _family(b"a/+", i, 200_000)     # (a,+): slot 1
    fs += [(b"#", 1), (b"+/#", 2), (b"a/b/w001/xa", 3), (b"a/b/w002", 4), (b"$SYS/+/w003/xa", 5), (b"+/+/+/xa", 6),
           (b"a/b/+/+/yb", 7), (b"b/c/w000", 8)]
    fs += [(b"q/" + b"x%c" % c, 300 + c) for c in b"abcdz"] + [(b"q/q/q/yb", 320), (b"q/q/q/zz", 321)]
    return fs


def _topics(seed=7):
    """every case of the level-2 word under both annexed nodes: absent, present but
    dead, alive through each kind of filter, long words, words unknown to the vocab;
    3 to 6 levels; '$'-topics"""
    r = random.Random(seed)
    l0 = [b"a", b"a", b"b", b"c", b"$SYS", b"$other", b"never-seen-0"]
    l1 = [b"b", b"c", b"q", b"never-seen-1", b""]
    l2 = [_w(i) for i in range(NW)] * 3 + [b"w%03d" % i for i in range(NW, NW + 60)] + \
         [b"long-child-%04d" % i for i in range(NW, NW + 40)] + [b"xa", b"yb", b"q", b"", b"unknown-word", b"nope"] + \
         [b"v%03d" % i for i in range(0, 700, 9)] + [b"nw%04d" % i for i in range(0, 3000, 97)]
    l3 = [b"xa", b"xa", b"xb", b"yb", b"zz", b"never-seen-3", b"", b"q"]
    l4 = [b"yb", b"zz", b"xa", b"never-seen-4"]
    ts = []
    for _ in range(N_TOPICS - 8):
        n = r.choice((3, 3, 4, 4, 4, 5, 6))
        ws = [r.choice(l0), r.choice(l1), r.choice(l2)]
        if n > 3:
            ws.append(r.choice(l3))
        if n > 4:
            ws += [r.choice(l4) for _ in range(n - 4)]
        ts.append(b"/".join(ws))
    ts += [b"", b"/", b"a", b"a/b", b"+/b/w000", b"a/b/#", b"a//w000/xa", b"a/b/w000/xa/yb/zz/q/q/q"]
    return items_of(ts)


def _check(torch, pair, topics, what):
    """one oracle answer; the device pairs batch and the device CSR batch equal it"""
    ix = pair.ix
    assert ix.debug_get(_native.TM_DEBUG_HINT_AUDIT) == 0, f"{what}: hints and child slots disagree in the host image"
    cnt, ohit, ovals = pair.expect(topics)
    paths0 = [ix.debug_get(k) for k in (_native.TM_DEBUG_PATH_PHASES, _native.TM_DEBUG_PATH_SMALL)]
    dev, n = torch.device("cuda:0"), len(topics)
    stream = torch.cuda.current_stream().cuda_stream
    d_blob = torch.from_numpy(topics.blob.copy()).to(dev)
    d_offs = torch.from_numpy(topics.offs.view(np.int64).copy()).to(dev)
    cap = 2 * int(ohit[-1]) + 4096
    d_vals = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_err = torch.zeros(n, dtype=torch.uint8, device=dev)
    want_err = np.where(cnt < 0, -cnt, 0)
    # pairs
    d_pairs = torch.zeros(2 * n + 2, dtype=torch.int32, device=dev)
    ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_vals.data_ptr(), cap,
                             d_err.data_ptr(), stream)
    torch.cuda.synchronize()
    pr = d_pairs.cpu().numpy().view(np.uint32).astype(np.int64)
    pv = d_vals.cpu().numpy().view(np.uint32)
    assert np.array_equal(d_err.cpu().numpy().astype(np.int64), want_err), f"{what}: pairs err flags"
    assert int(pr[2 * n]) == int(ohit[-1]), f"{what}: pairs total {int(pr[2 * n])} oracle {int(ohit[-1])}"
    want_cnt = np.diff(ohit.astype(np.int64))
    bad = np.nonzero(pr[1:2 * n:2] != want_cnt)[0]
    assert len(bad) == 0, f"{what}: pairs: {len(bad)} topics' counts differ, first {topics.item(int(bad[0]))!r}: " \
                          f"gpu {int(pr[2 * bad[0] + 1])} oracle {int(want_cnt[bad[0]])}"
    pos = np.repeat(pr[0:2 * n:2] - ohit[:-1].astype(np.int64), want_cnt) + np.arange(len(ovals))
    bad = np.nonzero(pv[pos] != ovals)[0]
    assert len(bad) == 0, f"{what}: pairs: {len(bad)} of {len(ovals)} values differ"
    # CSR
    d_hit = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_vals.zero_()
    d_err.zero_()
    ix.match_batch_dev(n, d_blob.data_ptr(), d_offs.data_ptr(), d_hit.data_ptr(), d_vals.data_ptr(), cap,
                       d_err.data_ptr(), stream)
    torch.cuda.synchronize()
    hit = d_hit.cpu().numpy().view(np.uint64)
    assert np.array_equal(d_err.cpu().numpy().astype(np.int64), want_err), f"{what}: CSR err flags"
    bad = np.nonzero(hit != ohit.astype(np.uint64))[0]
    assert len(bad) == 0, f"{what}: CSR: hit offsets differ from topic {topics.item(int(bad[0]) - 1)!r}"
    bad = np.nonzero(d_vals.cpu().numpy().view(np.uint32)[:len(ovals)] != ovals)[0]
    assert len(bad) == 0, f"{what}: CSR: {len(bad)} of {len(ovals)} values differ"
    # both batches took the main walks (k_walk_pairs / k_walk_fast), not the one-launch kernel
    paths = [ix.debug_get(k) for k in (_native.TM_DEBUG_PATH_PHASES, _native.TM_DEBUG_PATH_SMALL)]
    assert [a - b for a, b in zip(paths, paths0)] == [2, 0], (what, paths0, paths)


def _annex(ix):
    """-> [(depth, children) or None per slot]"""
    out = []
    for k in (_native.TM_DEBUG_ANNEX0, _native.TM_DEBUG_ANNEX1):
        v = ix.debug_get(k)
        out.append(None if v == UNUSED else (v >> 32, v & 0xFFFFFFFF))
    return out


@pytest.mark.parametrize("copies,commit", [(1, False), (2, True)])
def test_hints_follow_the_child_slots(torch_dev, copies, commit):
    ix = _native.Index(copies=copies)
    pair = Pair(ix)
    topics = _topics()
    step = 0

    def ins(kv):
        pair.insert([k for k, _ in kv], [v for _, v in kv], commit=commit)

    def dele(kv):
        pair.delete([k for k, _ in kv], [v for _, v in kv], commit=commit)

    def check(what):
        nonlocal step
        step += 1
        _check(torch_dev, pair, topics, f"step {step} ({what}, copies={copies}, commit={commit})")

    base = _base()
    pair.insert([k for k, _ in base], [v for _, v in base])
    assert _annex(ix) == [(2, NW), (2, NW)], _annex(ix)   # (+,+) and (a,+), both at depth 2
    check("the base")
    # a subscribe that creates a child under each annexed node
    new_kids = [(b"+/+/w%03d/xa" % (NW + 1), 400_001), (b"a/+/w%03d/xa" % (NW + 2), 400_002),
                (b"+/+/long-child-%04d/xa" % (NW + 3), 400_003), (b"+/+/unknown-word", 400_004)]
    ins(new_kids)
    assert sorted(_annex(ix)) == [(2, NW + 1), (2, NW + 3)]
    check("children created under the annexed nodes")
    # a literal, a '#' and a '+' below existing literal-only children (k = 6..9), and an exact terminal
    below = [(b"+/+/" + _w(6) + b"/yb", 400_010), (b"+/+/" + _w(8) + b"/#", 400_011), (b"+/+/" + _w(9) + b"/+", 400_012),
             (b"a/+/" + _w(16) + b"/zz", 400_013), (b"a/+/" + _w(18) + b"/+/yb", 400_014), (b"+/+/" + _w(19), 400_015),
             (b"+/+/" + _w(26) + b"/#/q", 400_016)]
    for kv in below:
        ins([kv])
    check("summaries changed below existing children")
    # the matching unsubscribes, down to the children vanishing
    dele(below)
    check("those filters gone again")
    dele(new_kids)
    dele(_family(b"+/+", 5, 100_000)[:1])           # one of two filters below a child: it stays
    # the child's only filters: it vanishes
    dele(_family(b"+/+", 12, 100_000) + _family(b"a/+", 13, 200_000) + _family(b"a/+", 14, 200_000))
    assert sorted(_annex(ix)) == [(2, NW - 2), (2, NW - 1)]
    check("children vanished")
    # vocab growth across a rehash (3,000 new short words: the table quadruples at least once)
    grow = [(b"nw%04d/x" % i, 500_000 + i) for i in range(3000)]
    ins(grow)
    check("vocab rehashed")
    # a third family outgrows the narrower annexed node, (a,+), by 2x: re-designation
    third = [(b"b/+/v%03d/xa" % i, 600_000 + i) for i in range(2 * NW + 10)]
    ins(third[:NW])
    assert sorted(_annex(ix)) == [(2, NW - 2), (2, NW - 1)]   # not yet twice as wide: the slots keep their nodes
    ins(third[NW:])
    assert sorted(_annex(ix)) == [(2, NW - 1), (2, 2 * NW + 10)], _annex(ix)
    check("(b,+) took a slot")
    # (+,+) drops below WIDE_LIT: its slot is released and goes to the widest node left without one
    gone = [kv for i in range(70) if i not in (5, 12) for kv in _family(b"+/+", i, 100_000)]
    dele(gone[:len(gone) // 2])
    check("(+,+) narrower, still wide")
    dele(gone[len(gone) // 2:])
    assert sorted(_annex(ix)) == [(2, NW - 2), (2, 2 * NW + 10)], _annex(ix)   # (a,+) is back, (+,+) is out
    check("(+,+) below WIDE_LIT")
    ins(gone)
    assert sorted(_annex(ix)) == [(2, NW - 2), (2, 2 * NW + 10)], _annex(ix)   # wide again, but not twice (a,+)
    check("(+,+) wide again")
    dele(grow)
    check("the new words erased")
    ix.close()
