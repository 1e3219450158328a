"""The host API's one run-and-retry loop and its one way back under the lock,
through every CSR host entry point whose launch has a look-back.

A forced look-back failure (TM_DEBUG_LB_FAIL_BLOCK / TM_DEBUG_LB_LAUNCHES: a
block of k_walk_small acts as if its wait expired and raises the flag the host
reads; nothing faults) must run the batch again once, with identical results,
and a second failure must be a device error for the whole call that leaves the
lane released.  The counters say what ran: TM_DEBUG_FAILED_BATCHES,
TM_DEBUG_RETRIED_BATCHES, TM_DEBUG_PATH_SMALL.  (The pairs launches --
tm_match_batch32_pairs, tm_route_batch32 in place -- have no look-back.)

200 topics at 16 per block (the `wave` kernel) are 13 blocks; block 1 fails.

The growth tests: 300 values under '#' and 250 topics are 75,000 hits, just
over the 65,536 entries a lane's value scratch starts with, so the first call
runs twice (the scratch grown in between) and the second once.
"""
import numpy as np
import pytest

from emqx_amd import _native
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

N_TOPICS, N_DESTS, CAP = 200, 5, 4096
FAILED, RETRIED = _native.TM_DEBUG_FAILED_BATCHES, _native.TM_DEBUG_RETRIED_BATCHES
SMALL, PHASES = _native.TM_DEBUG_PATH_SMALL, _native.TM_DEBUG_PATH_PHASES


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _filters():
    fs = []
    for i in range(12):
        fs += [f"a{i}/+/c{i % 3}", f"a{i}/#", f"+/b{i}/#", f"a{i}/b{i}/c{i % 3}"]
    fs += ["#", "+/+/+"]
    return [f.encode() for f in fs]


def _topics(n=N_TOPICS):
    out = [f"a{i % 14}/b{i % 13}/c{i % 4}".encode() for i in range(n)]
    out[7], out[150] = b"a1/+/c1", b"#"   # badarg
    return out


def _index(filters, values):
    ix = _native.Index()
    values = np.asarray(values, np.uint32)
    ix.set_dests(values, (values % (N_DESTS + 1)).astype(np.uint32))   # (dest N_DESTS: not routed)
    blob, offs = _native.pack_strings(filters)
    ix.apply(np.ones(len(filters), np.uint8), blob, offs, values)
    return ix


class Case:
    """one entry point over one index and the 200 topics: call() -> the results, copied"""

    def __init__(self, kind):
        fs = _filters()
        self.kind, self.ix = kind, _index(fs, np.arange(len(fs)))
        ix = self.ix
        ix.debug_set(_native.TM_DEBUG_SMALL_KERNEL, _native.SMALL_WAVE)
        self.blob, self.offs = _native.pack_strings(_topics())
        n, nb = N_TOPICS, int(self.offs[-1])
        if kind in ("match_in_place", "match32", "match32_combined"):
            odt = np.uint64 if kind == "match_in_place" else np.uint32
            blob = ix.host_array(nb + 16, np.uint8)
            blob[:nb] = self.blob[:nb]
            offs = ix.host_array(n + 1, odt)
            offs[:] = self.offs.astype(odt)
            self.blob, self.offs = blob, offs
            self.out = (ix.host_array(n + 1, odt), ix.host_array(CAP, np.uint32), ix.host_array(n, np.uint8))
        if kind == "match32":
            ix.debug_set(_native.TM_DEBUG_COMBINE, 0)
        if kind == "match32_combined":
            ix.debug_set(_native.TM_DEBUG_COMBINE, 1)

    def call(self):
        ix = self.ix
        if self.kind == "match_staged":
            r = ix.match_batch(self.blob, self.offs, cap=CAP)
        elif self.kind == "match_in_place":
            r = ix.match_batch(self.blob, self.offs, out=self.out)
        elif self.kind in ("match32", "match32_combined"):
            r = ix.match_batch32(self.blob, self.offs, self.out)
        else:
            r = ix.route_batch(self.blob, self.offs, N_DESTS, cap=CAP)
        return tuple(np.array(a) for a in r)

    def counters(self):
        return tuple(self.ix.debug_get(k) for k in (FAILED, RETRIED, SMALL))


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["match_staged", "match_in_place", "match32", "match32_combined", "route"])
def test_failed_launch_is_retried_once_then_a_device_error(gpu, kind):
    c = Case(kind)
    ix = c.ix
    c0 = c.counters()
    ref = c.call()
    c1 = c.counters()
    assert int(ref[0][-1]) > N_TOPICS, "the batch has hits"
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (0, 0, 1), "a normal run: one one-launch walk, no failure"
    ix.debug_set(_native.TM_DEBUG_LB_FAIL_BLOCK, 1)
    ix.debug_set(_native.TM_DEBUG_LB_LAUNCHES, 1)     # the first launch fails, the retry succeeds
    got = c.call()
    c2 = c.counters()
    assert _same(got, ref), "the retried batch differs"
    assert (c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]) == (1, 1, 2)
    ix.debug_set(_native.TM_DEBUG_LB_LAUNCHES, 2)     # both fail: a device error
    with pytest.raises(_native.DeviceError):
        c.call()
    c3 = c.counters()
    assert (c3[0] - c2[0], c3[1] - c2[1]) == (2, 1)
    # the same call again, from the same thread: the lane was released, the hook is spent
    assert _same(c.call(), ref)
    c4 = c.counters()
    assert (c4[0] - c3[0], c4[1] - c3[1], c4[2] - c3[2]) == (0, 0, 1)
    ix.close()


# ---- growth through the shared relock()

N_VALUES, N_GROW = 300, 250


@pytest.fixture(scope="module")
def grow_ref():
    """the oracle's CSR of the 250 topics over 300 values under '#'"""
    o = Oracle()
    for v in range(N_VALUES):
        o.insert(b"#", v)
    o.prepare()
    blob, offs = _native.pack_strings([b"t/%d" % i for i in range(N_GROW)])
    cnt, _, hit, vals = o.match_batch(blob, offs)
    assert int(hit[-1]) == N_VALUES * N_GROW == 75_000 and (cnt == N_VALUES).all()
    return blob, offs, hit, vals


def _launches(ix):
    return ix.debug_get(SMALL) + ix.debug_get(PHASES)   # (every run of a batch is one match launch)


def test_match_batch_staging_grows_and_is_kept(gpu, grow_ref):
    blob, offs, ohit, ovals = grow_ref
    ix = _index([b"#"] * N_VALUES, np.arange(N_VALUES))
    for runs in (2, 1):   # grown and run again, once; then the grown size is kept
        l0 = _launches(ix)
        hit, vals, err = ix.match_batch(blob, offs, cap=80_000)
        assert _launches(ix) - l0 == runs
        assert np.array_equal(hit, ohit) and np.array_equal(vals, ovals) and not err.any()
    assert ix.debug_get(FAILED) == 0 and ix.debug_get(RETRIED) == 0
    ix.close()


def test_route_batch_scratch_grows_and_is_kept(gpu, grow_ref):
    blob, offs, ohit, ovals = grow_ref
    ix = _index([b"#"] * N_VALUES, np.arange(N_VALUES))
    # the definition: a stable sort of the CSR's (topic, value) entries by destination
    topic = np.repeat(np.arange(N_GROW, dtype=np.uint32), np.diff(ohit.astype(np.int64)))
    bucket = ovals % (N_DESTS + 1)
    order = np.argsort(bucket, kind="stable")
    edoff = np.concatenate([np.searchsorted(bucket[order], np.arange(N_DESTS + 1)), [len(ovals)]]).astype(np.uint64)
    for runs in (2, 1):
        l0 = _launches(ix)
        doff, t, v, err = ix.route_batch(blob, offs, N_DESTS, cap=80_000)
        assert _launches(ix) - l0 == runs
        assert np.array_equal(doff, edoff) and np.array_equal(t, topic[order]) and np.array_equal(v, ovals[order])
        assert not err.any()
    assert ix.debug_get(FAILED) == 0 and ix.debug_get(RETRIED) == 0
    ix.close()
