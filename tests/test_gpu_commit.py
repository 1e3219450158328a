"""tm_commit (include/tmatch.h): its contract called directly, and epoch
snapshots of concurrent callers while commits ship structural deltas with
every copy of the tables busy.  The reference is the CPU oracle fed the same
deltas in the same order; every comparison is bit-exact.
"""
import random
import threading

import numpy as np
import pytest

from emqx_amd import _native
from delta_transport import POOL, Churn, Pair, base_set, items_of, same, topic_of

pytestmark = pytest.mark.gpu

COUNTERS = (_native.TM_DEBUG_COMMITS, _native.TM_DEBUG_COMMIT_WAITS, _native.TM_DEBUG_COMMIT_FORCED)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _counters(ix):
    """-> [commits, commit_waits, commit_forced]"""
    return [ix.debug_get(k) for k in COUNTERS]


def _rise(ix, before):
    return [a - b for a, b in zip(_counters(ix), before)]


# ------------------------------------------------------------ 6. direct contract

def _first_hits(pair, topics):
    """tm_first_batch against the oracle's first value in traversal order"""
    cnt, ohit, ovals = pair.expect(topics)
    val, found = pair.ix.first_batch(topics.blob, topics.offs)
    assert np.array_equal(found == 2, cnt < 0)
    assert np.array_equal(found == 1, cnt > 0)
    has = cnt > 0
    assert np.array_equal(val[has], ovals[ohit[:-1][has].astype(np.int64)])


def _dev_pairs(torch, pair, topics):
    """tm_match_batch_dev_pairs on device buffers: per topic the oracle's values in its order"""
    cnt, ohit, ovals = pair.expect(topics)
    dev, n = torch.device("cuda:0"), len(topics)
    d_blob = torch.from_numpy(topics.blob.copy()).to(dev)
    d_offs = torch.from_numpy(topics.offs.view(np.int64).copy()).to(dev)
    cap = 2 * int(ohit[-1]) + 4096
    d_pairs = torch.zeros(2 * n + 2, dtype=torch.int32, device=dev)
    d_vals = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_err = torch.zeros(n, dtype=torch.uint8, device=dev)
    pair.ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_vals.data_ptr(), cap,
                                  d_err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pr = d_pairs.cpu().numpy().view(np.uint32)
    pv = d_vals.cpu().numpy().view(np.uint32)
    assert np.array_equal(d_err.cpu().numpy().astype(np.int64), np.where(cnt < 0, -cnt, 0))
    assert int(pr[2 * n]) == int(ohit[-1]) and int(pr[2 * n + 1]) <= cap
    for i in range(n):
        p, c = int(pr[2 * i]), int(pr[2 * i + 1])
        assert np.array_equal(pv[p:p + c], ovals[int(ohit[i]):int(ohit[i + 1])]), f"pairs: topic {topics.item(i)!r}"


@pytest.mark.parametrize("copies", [1, 2])
def test_commit_contract(torch_dev, copies):
    """n = 0 and a delta that changes no device word ship nothing; every commit
    with n > 0 advances the epoch by one and returns it; with one copy every
    shipping commit is forced, with an idle second copy none is and none waits;
    the first batch after a commit -- host CSR, first hit, device pairs --
    holds its delta; plain applies before and after a commit reach the batch
    with it."""
    ix = _native.Index(copies=copies)
    pair = Pair(ix)
    keys, vals = base_set(400)
    pair.insert(keys, vals)
    ix.sync()
    gone = (5, 9)   # deleted by hand below: not the small deltas' to delete again
    churn = Churn([k for i, k in enumerate(keys) if i not in gone], [v for i, v in enumerate(vals) if i not in gone], 401)
    extra = [b"l0w0/c6/a", b"l0w0/c6/b", b"l0w2/c6/c/d", b"c6-first-level-word/x", b"l0w4/c6/e", b"l0w4/c6/f/g"]
    probes = churn.probes(extra)
    pair.check(probes, what="the base")
    shipped = 0

    def commit(ops, ks, vs, ships=True):
        nonlocal shipped
        e0, c0 = ix.epoch()[0], _counters(ix)
        e = pair.apply(np.array(ops, np.uint8), items_of(ks, vs), commit=True)
        assert e == e0 + 1 and ix.epoch()[0] == e, (e0, e, ix.epoch())
        exp = [1, 0, 1 if copies == 1 else 0] if ships else [0, 0, 0]
        assert _rise(ix, c0) == exp, (ks, _rise(ix, c0), exp)
        shipped += ships

    # n = 0: no epoch, no patch
    e0, c0, s0 = ix.epoch()[0], _counters(ix), ix.stats()
    e = ix.apply(np.zeros(0, np.uint8), np.zeros(16, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), commit=True)
    s1 = ix.stats()
    assert e == e0 == ix.epoch()[0] and _rise(ix, c0) == [0, 0, 0]
    assert (s1["uploads"], s1["patch_bytes"]) == (s0["uploads"], s0["patch_bytes"])
    # a live (key, id) inserted again: an epoch, but nothing to ship
    commit([1], [keys[0]], [vals[0]], ships=False)
    assert ix.stats()["patch_bytes"] == s0["patch_bytes"]
    pair.check(probes, what="after the commits that ship nothing")
    # the first batch after a commit, through each entry point
    commit([1, 0], [b"l0w0/c6/+", keys[5]], [7_000_001, vals[5]])
    pair.check(probes, what="tm_match_batch after a commit")
    commit([1, 1, 0], [b"l0w2/c6/#", b"c6-first-level-word/x", keys[9]], [7_000_002, 7_000_003, vals[9]])
    _first_hits(pair, probes)
    commit([0, 1], [b"l0w0/c6/+", b"l0w0/c6/b"], [7_000_001, 7_000_004])
    _dev_pairs(torch_dev, pair, probes)
    pair.check(probes, what="after the three entry points")
    # apply; commit; apply; batch
    s0 = ix.stats()
    pair.insert([b"l0w4/c6/+"], [7_000_005])
    commit([1], [b"l0w4/c6/f/#"], [7_000_006])
    pair.delete([b"l0w2/c6/#"], [7_000_002])
    pair.check(probes, what="apply, commit, apply")
    assert ix.stats()["uploads"] - s0["uploads"] == 2   # the commit's patch carried the apply before it
    # small deltas as commits, a batch after each few
    for k in range(20):
        ops, d = churn.delta()
        e0, c0 = ix.epoch()[0], _counters(ix)
        assert pair.apply(ops, d, commit=True) == e0 + 1
        assert _rise(ix, c0) == [1, 0, 1 if copies == 1 else 0]
        shipped += 1
        if k % 4 == 3:
            pair.check(probes, what=f"after small commit {k}")
    assert _counters(ix) == [shipped, 0, shipped if copies == 1 else 0]
    ix.close()


# --------------------------------- 7. epoch snapshots under commit, copies busy

N_THREADS, BATCH, EPOCHS, N_SETS = 12, 4096, 24, 4


def _payload():
    """the structural payload: 3,000 filters over 3,000 new words (the vocab
    doubles twice, and halves back when they are deleted), half of them binary
    keys (the exact table), and 300 children under one node (a child bitmap)"""
    words = [(b"pay-long-word-%05d" if i % 4 == 0 else b"pw%05d") % i for i in range(3000)]
    ks = [(b"pay/%s/x" if i % 2 else b"pay/%s/+") % w for i, w in enumerate(words)]
    ks += [b"pwide/%s/+" % w for w in words[:300]]
    return ks, [500_000 + i for i in range(len(ks))]


@pytest.mark.parametrize("copies", [2, 3])
def test_snapshots_under_commit_with_busy_copies(torch_dev, copies):
    """12 host threads keep 4,096-topic batches in flight on 2 or 3 copies while
    the main thread ships 24 epochs with tm_commit.  Every epoch inserts a
    marker 'probe/+' -> 900000 + e, so the probe topic of a batch says how many
    epochs it saw; every third epoch also inserts (or deletes again) the
    structural payload, which makes the commit's own collect upload whole
    tables -- witnessed by tm_stats' uploads rising by more than the one patch.
    A batch queued while the committer waits for a copy to drain must still
    see whole epochs only: every batch equals the oracle after exactly the
    epochs its probe shows, and a thread's batches never go back in time.

    A race test without false positives: a pass does not prove that no window
    is left, a failure is a real bug."""
    ix = _native.Index(copies=copies)
    pair = Pair(ix)
    keys, vals = base_set(700)
    pair.insert(keys, vals)
    ix.sync()
    r = random.Random(701)
    pay_keys, pay_vals = _payload()
    uniq = list(dict.fromkeys(keys))
    usets = []   # (four distinct batches among the 12 threads: the oracle's share of the test is a quarter)
    for t in range(N_SETS):
        ts = [topic_of(r.choice(uniq), r.choice(POOL[1])) for _ in range(BATCH - 200)]
        ts += [b"/".join(r.choice(POOL[lv % 4]) for lv in range(r.randint(1, 5))) for _ in range(100)]
        ts += [topic_of(k, b"y") for k in r.sample(pay_keys, 100)]
        r.shuffle(ts)
        usets.append(items_of(ts + [b"probe/x"]))
    tsets = [usets[t % N_SETS] for t in range(N_THREADS)]
    base_kv = r.sample(list(zip(keys, vals)), EPOCHS * 60)   # each unsubscribed once
    ep_ops, structural = [], []
    for e in range(EPOCHS):
        fl, vs, ops = [b"probe/+"], [900_000 + e], [1]
        for i in range(60):   # new filters that match some batch topics
            ws = tsets[r.randrange(N_THREADS)].item(r.randrange(BATCH)).split(b"/")
            k = r.randrange(len(ws))
            ws[k] = b"+" if r.random() < 0.5 else ws[k]
            fl.append(b"/".join(ws[: k + 1]) + (b"/#" if r.random() < 0.3 else b""))
            vs.append(100_000 + e * 1000 + i)
            ops.append(1)
        for k, v in base_kv[e * 60:(e + 1) * 60]:
            fl.append(k)
            vs.append(v)
            ops.append(0)
        structural.append(e % 3 == 0)
        if e % 3 == 0:
            fl += pay_keys
            vs += pay_vals
            ops += [1 if e % 6 == 0 else 0] * len(pay_keys)
        ep_ops.append((np.array(ops, np.uint8), items_of(fl, vs)))
    # the oracle after e epochs, for every distinct batch
    expected = []
    for e in range(EPOCHS + 1):
        if e:
            ops, d = ep_ops[e - 1]
            pair.o.apply(ops, d.blob, d.offs, d.vals)
        pair.o.prepare()
        expected.append([pair.o.match_batch(ts.blob, ts.offs) for ts in usets])
    vcap = max(len(x[3]) for ex in expected for x in ex) + 64
    results = [[] for _ in range(N_THREADS)]
    stop = threading.Event()
    batch_done = threading.Semaphore(0)
    errors = []

    def caller(t):
        try:
            ts = tsets[t]
            n = len(ts)
            if t % 2:   # pageable caller buffers
                bufs = (np.zeros(n + 1, np.uint64), np.zeros(vcap, np.uint32), np.zeros(n, np.uint8))
                blob, offs = ts.blob, ts.offs
            else:       # tm_host_alloc buffers: in place
                nb = int(ts.offs[-1])
                blob = ix.host_array(nb + 16, np.uint8)
                blob[:nb] = ts.blob[:nb]
                offs = ix.host_array(n + 1, np.uint64)
                offs[:] = ts.offs
                bufs = (ix.host_array(n + 1, np.uint64), ix.host_array(vcap, np.uint32), ix.host_array(n, np.uint8))
            while not stop.is_set() or len(results[t]) < 3:
                hit, vs_, err = ix.match_batch(blob, offs, out=bufs)
                results[t].append((hit.copy(), vs_.copy(), err.copy()))
                batch_done.release()
        except BaseException as e:   # noqa: BLE001 - reported below
            errors.append(repr(e))
            batch_done.release(10_000)

    def let_batches_finish(k):   # (paces the epochs by the callers' progress, not by the clock)
        for _ in range(k):
            assert batch_done.acquire(timeout=60)

    th = [threading.Thread(target=caller, args=(t,)) for t in range(N_THREADS)]
    for x in th:
        x.start()
    rises = []
    for (ops, d), st in zip(ep_ops, structural):
        let_batches_finish(N_THREADS)
        up0 = ix.stats()["uploads"]
        ix.apply(ops, d.blob, d.offs, d.vals, commit=True)
        rises.append(ix.stats()["uploads"] - up0)
    let_batches_finish(2 * N_THREADS)
    stop.set()
    for x in th:
        x.join(timeout=60)
    assert not any(x.is_alive() for x in th), "a caller thread did not end"
    assert not errors, errors
    commits, waits, forced = _counters(ix)
    print(f"commit under load, {copies} copies: commits {commits} waits {waits} forced {forced}; "
          f"uploads per epoch {rises}; batches {sum(len(x) for x in results)}")
    for e, (rise, st) in enumerate(zip(rises, structural)):   # (only commits collect while they hold batches off)
        assert rise > 1 if st else rise >= 1, f"epoch {e}: uploads rose by {rise} (structural: {st})"
    assert commits > 0
    seen = set()
    for t in range(N_THREADS):
        last = -1
        for hit, vs_, err in results[t]:
            probe = [v for v in vs_[int(hit[-2]):int(hit[-1])].tolist() if v >= 900_000]
            e = len(probe)
            assert sorted(probe) == [900_000 + k for k in range(e)], "a batch saw part of an epoch"
            assert e >= last, "a thread's batches went back in time"
            last = e
            seen.add(e)
            cnt, _, ohit, ovals = expected[e][t % N_SETS]
            same(hit, vs_, err, cnt, ohit, ovals, tsets[t], f"thread {t}, a batch that saw {e} epochs")
    assert len(seen) >= 4, seen          # the batches did interleave with the epochs
    ix.close()


# ------------------- 8. a commit that changes the cached view, every copy busy

def test_view_changing_commit_with_every_copy_busy(torch_dev):
    """The window of test 7 made to open: both copies of the tables are kept
    busy by queued device batches (stream 1 on copy 0; a first commit makes
    copy 1 the serving copy; stream 2 on copy 1) while a commit deletes the
    only binary key of 20 levels and the only filter of 24 (DevIndex::xlen_mask
    loses a bit, DevIndex::depth falls from 24 to 4 -- the cached view changes,
    no table is uploaded whole; topics of more levels than the one-launch walk
    has lanes resolve only need_levels() of them) and a thread keeps small
    host batches coming.
    Such a commit has no idle copy to publish on and must not leave batches to
    run with the new view over tables that lack its patch while it waits for
    one: it publishes at once (TM_DEBUG_COMMIT_FORCED, no TM_DEBUG_COMMIT_WAITS),
    and every host batch -- before, during and after -- equals the oracle after
    exactly the epochs its probe shows."""
    torch = torch_dev
    ix = _native.Index(copies=2)
    pair = Pair(ix)
    keys, vals = base_set(800)
    deep = b"/".join(POOL[lv % 4][3] for lv in range(20))
    filt = b"/".join(POOL[lv % 4][5] for lv in range(23)) + b"/+"
    pair.insert(keys + [deep, filt], vals + [600_000, 600_001])
    ix.sync()
    r = random.Random(801)
    uniq = list(dict.fromkeys(keys))
    small = items_of([deep, topic_of(filt), deep + b"/x", topic_of(filt) + b"/x"] +
                     [topic_of(r.choice(uniq), r.choice(POOL[1])) for _ in range(200)] + [b"probe/x"])
    pair.check(small, what="the base")
    # device batches that keep a copy busy: 2M topics each (milliseconds on the device, a fraction of one to
    # queue, so a stream's backlog grows while it is being queued), as many as take ~300 ms on an idle device.
    # The commit below starts once both streams are queued and three small host batches have run; that both
    # streams still had work when it returned is asserted
    big = items_of([topic_of(r.choice(uniq), r.choice(POOL[1])) for _ in range(20_000)] * 100)
    dev, n = torch.device("cuda:0"), len(big)
    d_blob = torch.from_numpy(big.blob.copy()).to(dev)
    d_offs = torch.from_numpy(big.offs.view(np.int64).copy()).to(dev)
    streams = [torch.cuda.Stream() for _ in range(2)]
    cap = 8 * n
    bufs = [(torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev),
             torch.zeros(n, dtype=torch.uint8, device=dev)) for _ in streams]

    def queue(k, count):
        hit, out, err = bufs[k]
        for _ in range(count):
            ix.match_batch_dev(n, d_blob.data_ptr(), d_offs.data_ptr(), hit.data_ptr(), out.data_ptr(), cap,
                               err.data_ptr(), streams[k].cuda_stream)

    queue(0, 1)   # (workspace allocated)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(streams[0]):
        t0.record()
        queue(0, 4)
        t1.record()
    torch.cuda.synchronize()
    count = int(min(max(300.0 / max(t0.elapsed_time(t1) / 4, 1e-3), 8), 4000))
    exp = {}
    results, errors = [], []
    started, stop = threading.Event(), threading.Event()

    def caller():
        try:
            out = (np.zeros(len(small) + 1, np.uint64), np.zeros(50_000, np.uint32), np.zeros(len(small), np.uint8))
            while not stop.is_set():
                hit, vs_, err = ix.match_batch(small.blob, small.offs, out=out)
                results.append((hit.copy(), vs_.copy(), err.copy()))
                if len(results) == 3:
                    started.set()
        except BaseException as e:   # noqa: BLE001 - reported below
            errors.append(repr(e))
            started.set()

    before = [ix.replica_stats(k)[0] for k in range(2)]
    queue(0, count)                                         # copy 0 busy
    pair.insert([b"probe/+"], [900_000], commit=True)       # published on copy 1, the idle one
    exp[1] = pair.expect(small)
    queue(1, count)                                         # copy 1, now the serving copy, busy
    served = [ix.replica_stats(k)[0] - b for k, b in enumerate(before)]
    assert served == [count, count], f"the device batches did not keep to their copies: {served}"
    th = threading.Thread(target=caller)
    th.start()
    started.wait(timeout=60)
    c0, up0 = _counters(ix), ix.stats()["uploads"]
    pair.apply(np.array([0, 0, 1], np.uint8), items_of([deep, filt, b"probe/+"], [600_000, 600_001, 900_001]), commit=True)
    rise, up = _rise(ix, c0), ix.stats()["uploads"] - up0
    still_busy = [not st.query() for st in streams]
    stop.set()
    th.join(timeout=60)
    assert not th.is_alive(), "the caller thread did not end"
    torch.cuda.synchronize()
    exp[2] = pair.expect(small)
    assert not errors, errors
    print(f"view-changing commit, both copies busy with {count} device batches each: "
          f"[commits, waits, forced] rose by {rise}, {len(results)} host batches")
    assert up == 1, f"uploads rose by {up}: a whole-table upload drained the device, no copy was busy"
    assert all(still_busy), f"a stream ran out of queued batches before the commit returned ({still_busy}): not the case meant"
    last = 0
    for k, (hit, vs_, err) in enumerate(results):
        probe = sorted(v for v in vs_[int(hit[-2]):int(hit[-1])].tolist() if v >= 900_000)
        e = len(probe)
        assert probe == [900_000, 900_001][:e] and e >= max(last, 1), f"host batch {k} saw probe ids {probe} after {last} epochs"
        last = e
        cnt, ohit, ovals = exp[e]
        same(hit, vs_, err, cnt, ohit, ovals, small, f"host batch {k} of {len(results)}, which saw {e} epochs")
    assert rise == [1, 0, 1], f"[commits, waits, forced] rose by {rise}: the commit found an idle copy, or waited for one"
    pair.check(small, exp[2], "after the commit")
    ix.close()
