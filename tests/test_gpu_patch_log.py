"""The delta transport of tm_host.cpp, single-threaded and deterministic: the
ring of PATCH_RING = 128 logged patches wrapping while a copy of the tables
lags, whole-table uploads between logged patches, the copied-patch path and its
slot buffer's growth, and patch sizes at the in-place limit -- every batch
bit-exact against the CPU oracle fed the same deltas in the same order.

One patch is `ix.apply(...)` followed by `ix.sync()`: tm_sync collects the
dirty words and brings up the first copy on the current device, so copy 0 (or
replica 0) takes every patch as it is made and any other copy lags until a
batch reads it, tm_commit picks it, or its oldest missing patch's slot is
needed again.  Every test asserts through tm_stats / tm_replica_stats /
tm_debug_get that it went the way it describes (delta_transport.py says how the
counters tell a patch from a whole-table upload).
"""
import numpy as np
import pytest

from emqx_amd import _native, workload as wl
from delta_transport import (PATCH_RING, PATCH_RUN, PATCH_ZC_MAX, RUN_HDR, Churn, Pair, base_set, items_of,
                             replica_batches, run_small_patches, topic_of)

pytestmark = pytest.mark.gpu

N_DELTAS = 300   # > 2 * PATCH_RING: every slot of the ring is reused at least once


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _based(ix, seed):
    """the base set on `ix` and in the oracle, uploaded (the first sync ships whole tables)"""
    pair = Pair(ix)
    keys, vals = base_set(seed)
    pair.insert(keys, vals)
    ix.sync()
    return pair, Churn(keys, vals, seed + 1)


def _ring_wrap(ix, seed, zc=1):
    ix.debug_set(_native.TM_DEBUG_PATCH_ZC, zc)
    assert ix.debug_get(_native.TM_DEBUG_PATCH_ZC) == zc
    pair, churn = _based(ix, seed)
    rose = run_small_patches(pair, churn, N_DELTAS)
    assert rose >= N_DELTAS > 2 * PATCH_RING
    assert {"delete", "second id", "new long word", "12-level binary key", "filter over known words"} <= set(churn.kinds)
    return pair, churn


# ------------------------------------------------- 1. ring wrap, lagging replica

@pytest.mark.parametrize("zc", [1, 0])
def test_ring_wrap_with_a_lagging_replica(torch_dev, zc):
    """Two replicas on device 0, 300 small patches taken by replica 0 alone: the
    ring wraps twice, replica 1 is dragged along only as far as each reused
    slot demands and takes the last 128 patches in one go before its first
    batch.  In place from the pinned slots (TM_DEBUG_PATCH_ZC 1) and through
    the per-slot device buffers (0)."""
    ix = _native.Index(devices=[0, 0])
    pair, churn = _ring_wrap(ix, 100, zc)
    probes = churn.probes()
    exp = pair.expect(probes)
    before = replica_batches(ix, 2)
    for k in range(2):   # consecutive host batches alternate between the replicas
        pair.check(probes, exp, f"batch {k}")
    assert [a - b for a, b in zip(replica_batches(ix, 2), before)] == [1, 1]
    ix.close()


# ----------------------------------------------- 2. ring wrap, copies and commits

@pytest.mark.parametrize("copies", [2, 3, 4])
def test_ring_wrap_with_copies_then_commits(torch_dev, copies):
    """The same 300 patches on one replica with 2-4 copies: copy 0 takes them,
    the others lag.  tm_commit then picks the idle copy that lags most (copy
    1), brings it up over the wrapped ring and makes it the serving copy: the
    next batch reads copy 1, and so does the one after copy 0 has caught up.
    12 further commits, a batch after each, walk through every copy."""
    ix = _native.Index(copies=copies)
    pair, churn = _ring_wrap(ix, 200)
    probes = churn.probes([b"l0w0/commit/0"] + [b"l0w2/commit/%d" % k for k in range(12)])
    get = ix.debug_get
    c0 = [get(k) for k in (_native.TM_DEBUG_COMMITS, _native.TM_DEBUG_COMMIT_FORCED, _native.TM_DEBUG_COMMIT_WAITS)]
    before = replica_batches(ix, copies)
    pair.insert([b"l0w0/commit/+"], [2_000_000], commit=True)
    pair.check(probes, what="after the commit")
    c1 = [get(k) for k in (_native.TM_DEBUG_COMMITS, _native.TM_DEBUG_COMMIT_FORCED, _native.TM_DEBUG_COMMIT_WAITS)]
    assert [a - b for a, b in zip(c1, c0)] == [1, 0, 0], (c0, c1)
    served = [a - b for a, b in zip(replica_batches(ix, copies), before)]
    assert served == [0, 1] + [0] * (copies - 2), f"the batch after the commit did not read copy 1: {served}"
    ix.sync()   # copy 0 is up to date again, and comes first: only as the serving copy does copy 1 keep the batches
    pair.check(probes, what="after the commit, every copy up to date")
    served = [a - b for a, b in zip(replica_batches(ix, copies), before)]
    assert served == [0, 2] + [0] * (copies - 2), f"copy 1 is not the serving copy: {served}"
    for k in range(12):
        if k % 2:
            pair.delete([b"l0w2/commit/%d" % (k - 1)], [2_000_100 + k - 1], commit=True)
        else:
            pair.insert([b"l0w2/commit/%d" % k, b"l0w2/commit/+"], [2_000_100 + k, 2_000_200 + k], commit=True)
        pair.check(probes, what=f"after further commit {k}")
    c2 = [get(k) for k in (_native.TM_DEBUG_COMMITS, _native.TM_DEBUG_COMMIT_FORCED, _native.TM_DEBUG_COMMIT_WAITS)]
    assert [a - b for a, b in zip(c2, c1)] == [12, 0, 0], (c1, c2)
    served = [a - b for a, b in zip(replica_batches(ix, copies), before)]
    assert sum(served) == 14 and min(served) >= 1, f"batches per copy {served}"
    ix.close()


# ------------------------------------ 3. a lagging copy across whole-table uploads

def test_lagging_replica_across_whole_table_uploads(torch_dev):
    """40 patches only replica 0 has taken, then one delta that rehashes the
    vocab and outgrows tables (whole-table uploads: every replica must take the
    logged patches first, or a later bring-up would write old words over the
    new tables), 40 more patches, a batch per replica; then the 6,000 keys are
    deleted again (the shrink rehash of reclaim), 10 more patches, a batch per
    replica."""
    ix = _native.Index(devices=[0, 0])
    pair, churn = _based(ix, 300)
    run_small_patches(pair, churn, 40)
    grow = [(b"l0w%d/grown-word-%05d/+" if i % 2 else b"l0w%d/grown-word-%05d/leaf") % (i % 30 // 2 * 2, i)
            for i in range(6000)]
    gvals = [3_000_000 + i for i in range(6000)]
    words0 = ix.stats()["n_words"]
    du, db = pair.patch(np.ones(6000, np.uint8), items_of(grow, gvals))
    assert du > 1 and ix.stats()["n_words"] >= words0 + 6000, (du, db)   # whole tables, and the rest as a patch
    run_small_patches(pair, churn, 40)
    probes = churn.probes([topic_of(k) for k in grow[::7]] + [b"l0w0/grown-word-99999/leaf"])
    exp = pair.expect(probes)
    before = replica_batches(ix, 2)
    for k in range(2):
        pair.check(probes, exp, f"after the growth, batch {k}")
    assert [a - b for a, b in zip(replica_batches(ix, 2), before)] == [1, 1]
    du, db = pair.patch(np.zeros(6000, np.uint8), items_of(grow, gvals))
    assert du > 1 and ix.stats()["n_words"] < words0 + 100, (du, db)     # the vocab shrank back: shipped whole
    run_small_patches(pair, churn, 10)
    exp = pair.expect(probes)
    before = replica_batches(ix, 2)
    for k in range(2):
        pair.check(probes, exp, f"after the shrink, batch {k}")
    assert [a - b for a, b in zip(replica_batches(ix, 2), before)] == [1, 1]
    ix.close()


# ----------------------------------- 4. large patches and the slot buffer's growth

# Measured on an MI355X (base: 200,002 C3 filters, then new filters of the same
# generator): the first 600 make patch_bytes rise by 260,360 (one patch, no
# table shipped whole); the 9,000 after the 127 one-key patches by 1,863,416
# -- an incremental patch above 1 MiB, as the slot buffer's first allocation
# is: no table comes near half dirty (the vocab outgrows its allocation in
# that sync and is shipped whole beside the patch).  A one-key patch is 72
# bytes of words, or the whole child table of a node that outgrew it (131,656).
BIG_1, BIG_2 = 600, 9000


def test_large_patches_grow_the_slot_buffer(torch_dev):
    """A patch above 64 KiB is copied to a device buffer of its ring slot even
    with TM_DEBUG_PATCH_ZC on; the buffer is allocated at max(2 x bytes, 1 MiB)
    on first use.  127 one-key patches later the ring is back at that slot, and
    a patch above 1 MiB has to replace the buffer.  A batch after each large
    patch and at the end, exact on a 5k-topic probe set."""
    nf = 200_000
    fs = wl.filters(3, nf)
    more = wl.filters(3, nf + BIG_1 + BIG_2 + PATCH_RING)   # the same generator: filters nf .. are new keys
    ix = _native.Index(hint_keys=len(fs) + BIG_1 + BIG_2 + PATCH_RING)
    pair = Pair(ix)
    pair.apply(np.ones(len(fs), np.uint8), fs)
    ix.sync()
    new = [more.item(i) for i in range(nf, len(more) - 2)]
    nvals = [5_000_000 + i for i in range(len(new))]
    ts = wl.topics(3, nf, 3000)
    probes = items_of(ts.items() + [topic_of(k) for k in new[::6]])
    assert 4500 < len(probes) < 5500

    def one(lo, hi):
        return pair.patch(np.ones(hi - lo, np.uint8), items_of(new[lo:hi], nvals[lo:hi]))

    du, db = one(0, BIG_1)
    print(f"large patch 1: {BIG_1} keys, patch_bytes +{db}, uploads +{du}")
    assert db > PATCH_ZC_MAX, (du, db)
    pair.check(probes, what="after the first large patch")
    at = BIG_1
    for k in range(PATCH_RING - 1):
        du, sb = one(at, at + 1)
        assert du >= 1 and sb > 0, (k, du, sb)   # one patch each: the ring moves on one slot
        at += 1
    du, db2 = one(at, at + BIG_2)
    print(f"large patch 2: {BIG_2} keys, patch_bytes +{db2}, uploads +{du}")
    assert db2 > 1 << 20, (du, db2)      # past the slot buffer's first allocation
    pair.check(probes, what="after the second large patch")
    at += BIG_2
    du, sb = one(at, at + 1)
    assert du >= 1 and sb > 0
    pair.check(probes, what="at the end")
    ix.close()


# --------------------------------------------- 5. patch sizes at the in-place limit

# One filter with n ids inserted in ascending order into an index that held none
# of its words dirties one contiguous stretch of `vals` -- the run's blocks of
# 1, 2, 4, ... 8192 words, each filled before the next is taken from the
# table's end: 8191 + n words for 4096 < n <= 8192 -- and a few words of nodes,
# ctab and vocab.  A patch of nw words in nr runs is 4 nw + 16 nr bytes, with
# ceil(nw / 64) <= nr <= ceil(nw / 64) + SLACK_RUNS (a run is short only at the
# end of a dirty stretch; this delta has a handful).  Measured on an MI355X:
# 7,080 ids -> patch_bytes + 61,436 (a patch of 65,276 .. 65,532 bytes by the
# bounds above), 7,142 ids -> + 61,684 (65,540 or more), four bytes more per
# id in between.  With the copy of the copied path left out (a scratch build),
# 7,117 ids were the last to arrive, 7,118 the first lost: this delta has six
# short runs, so 7,117 ids are a patch of exactly 65,536 bytes, the largest
# read in place, and 7,118 one of 65,540, the smallest copied.
SLACK_RUNS = 16
N_UNDER, N_OVER = 7080, 7142


def _patch_bounds(db):
    nw = db // 4
    lo = db + RUN_HDR * -(-nw // PATCH_RUN)
    return lo, lo + RUN_HDR * SLACK_RUNS


@pytest.mark.parametrize("zc", [1, 0])
def test_patch_sizes_at_the_in_place_limit(torch_dev, zc):
    """A patch at most SLACK_RUNS run headers below PATCH_ZC_MAX = 64 KiB (read
    in place when ZC is on), one above it (copied), and with ZC on one at every
    size in between, four bytes apart: the pinned slot's mapped range and the
    copy's length must both cover the patch's last word."""
    ix = _native.Index()
    ix.debug_set(_native.TM_DEBUG_PATCH_ZC, zc)
    pair = Pair(ix)
    # a vals table far larger than the patches (a table more than half dirty is shipped whole)
    # (and a few hundred nodes, so that a patch's three is not half of that table either)
    pad = [b"pad%d/p%d/+" % (i % 10, i) for i in range(300)]
    pair.insert([b"base/+"] * 40_000 + [b"base/x", b"lim/#"] + pad, list(range(40_302)))
    ix.sync()
    probes = items_of([b"lim/%d/t" % n for n in range(N_UNDER, N_OVER + 1)] + [b"base/x", b"lim", b"other/1/t"])
    sizes = range(N_UNDER, N_OVER + 1) if zc else (N_UNDER, N_OVER)
    seen = {}
    for n in sizes:
        key, ids = b"lim/%d/+" % n, list(range(100_000, 100_000 + n))
        du, db = pair.patch(np.ones(n, np.uint8), items_of([key] * n, ids))
        assert du == 1, (n, du, db)
        seen[n] = db
        pair.check(probes, what=f"{n} ids ({db} bytes of words)")
        du, _ = pair.patch(np.zeros(n, np.uint8), items_of([key] * n, ids[::-1]))   # (frees its blocks for the next one)
        assert du == 1
    print(f"limit patches: {N_UNDER} ids -> patch_bytes +{seen[N_UNDER]}, {N_OVER} ids -> +{seen[N_OVER]}")
    assert _patch_bounds(seen[N_UNDER])[1] <= PATCH_ZC_MAX, (seen[N_UNDER], _patch_bounds(seen[N_UNDER]))
    assert _patch_bounds(seen[N_OVER])[0] > PATCH_ZC_MAX, (seen[N_OVER], _patch_bounds(seen[N_OVER]))
    if zc:   # the sizes in between leave no gap wider than one id and one run header
        steps = np.diff([seen[n] for n in sizes])
        assert steps.min() >= 4 and steps.max() <= 4 + RUN_HDR, (steps.min(), steps.max())
    pair.check(probes, what="at the end")
    ix.close()
