"""tm_share_pick_dev driven directly: synthetic aggregated (topic, value) arrays
and slot tables built in numpy, exact against the numpy definition
(shared_sub.pick_batch_ref) -- no index content involved (the pattern of
test_gpu_dispatch.py).

The passes run on G = TM_DEBUG_FANOUT_GRID one-wave blocks over the E entries
(chunk = ceil(E / G) rounded up to 64) and over the N ranked ones: up to 64 G a
block owns one 64-wide step, from 64 G + 1 on two.  The inputs hold exactly E
entries and the pool exactly pool_len words (one spare word keeps an empty
tensor from being a null pointer); out_member is filled with a sentinel that
must survive at and past E; the inputs and the tables are compared after the
run; the state array is compared with the definition's.
"""
import numpy as np
import pytest

from emqx_amd import _native, shared_sub
from emqx_amd.shared_sub import NONE, UNDEF, pick_batch_ref

pytestmark = pytest.mark.gpu

CANARY = 0xC0FFEE22
TAIL = 64
RANKED = (shared_sub.ROUND_ROBIN, shared_sub.ROUND_ROBIN_PER_GROUP, shared_sub.STICKY)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def index(torch_dev):
    """an empty index: tm_share_pick_dev needs a handle for its scratch (and its own tables) only"""
    ix = _native.Index()
    yield ix
    torch_dev.cuda.synchronize()
    ix.close()


@pytest.fixture(scope="module")
def G(index):
    g = index.debug_get(_native.TM_DEBUG_FANOUT_GRID)
    assert g >= 64 and g % 64 == 0
    return g


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)]).view(np.int32 if a.itemsize == 4 else np.int64)).cuda()


def _host(x, n, dtype=np.uint32):
    return x.cpu().numpy().view(dtype)[:n]


class Tables:
    def __init__(self, slot_of, rec, pool, state):
        self.slot_of = np.asarray(slot_of, np.uint32)
        self.rec = np.asarray(rec, np.uint32).reshape(-1)
        self.pool = np.asarray(pool, np.uint32)
        self.state = np.asarray(state, np.uint32)
        assert len(self.rec) == 4 * len(self.state)


def make_tables(rng, n_slots, cnts=(2, 3, 4, 5), strategies=range(7), n_values=None, none_every=0, c0s=(UNDEF, 0, 1, 7)):
    """n_slots slots with lists of the given counts, cycling through the strategies"""
    cnt = np.asarray(cnts, np.int64)[np.arange(n_slots) % len(cnts)]
    pos = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    strat = np.asarray(list(strategies), np.int64)[(np.arange(n_slots) // 3) % len(list(strategies))]
    init = np.asarray([shared_sub.RANDOM, shared_sub.LOCAL, shared_sub.HASH_TOPIC, shared_sub.HASH_CLIENTID, 9],
                      np.int64)[(np.arange(n_slots) // 5) % 5]
    n_local = (np.arange(n_slots) // 7) % 4
    rec = np.stack([pos, cnt, n_local, strat | init << 8], axis=1).astype(np.uint32)
    pool = rng.integers(0, 0xFFFFFFFF, int(cnt.sum()), dtype=np.uint32)
    state = np.asarray(c0s, np.uint32)[np.arange(n_slots) % len(c0s)]
    n_values = n_slots if n_values is None else n_values
    slot_of = (np.arange(n_values) % max(n_slots, 1)).astype(np.uint32)
    if none_every:
        slot_of[::none_every] = NONE
    return Tables(slot_of, rec, pool, state)


def run_pick(torch, ix, tab, topic, value, cap=None, doff_total=None, keys=True, n_topics=None, seed=0x5EED, own=False,
             stream=None):
    """one call against the definition -> (member, head, state after).  own: the
    index's tables (tab = the host model of them, state included)"""
    topic, value = np.asarray(topic, np.uint32), np.asarray(value, np.uint32)
    total = len(topic) if doff_total is None else doff_total
    cap = len(topic) if cap is None else cap
    n_dests = 3
    doff = np.array([0, total // 3, total // 2, total, total], np.uint64)
    E = min(total, cap)
    topic, value = topic[:E].copy(), value[:E].copy()          # no position at or past E exists
    nt = (int(topic.max()) + 1 if E else 1) if n_topics is None else n_topics
    rng = np.random.default_rng(E + 17)
    kc = rng.integers(0, 1 << 32, nt, dtype=np.uint32) if keys else None
    kt = rng.integers(0, 1 << 32, nt, dtype=np.uint32) if keys else None
    want, whead, wstate = pick_batch_ref(n_dests, doff, topic, value, cap, tab.slot_of, tab.rec, tab.pool, tab.state, kc,
                                         kt, nt, seed)
    d_doff, d_t, d_v = _dev(torch, doff), _dev(torch, topic), _dev(torch, value)
    d_kc = _dev(torch, kc) if keys else None
    d_kt = _dev(torch, kt) if keys else None
    d_head = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    d_out = torch.from_numpy(np.full(E + TAIL, CANARY, np.uint32).view(np.int32)).cuda()
    ins = [(d_doff, doff), (d_t, topic), (d_v, value)] + ([(d_kc, kc), (d_kt, kt)] if keys else [])
    kw = {}
    if not own:
        d_so, d_rec, d_pool, d_state = _dev(torch, tab.slot_of), _dev(torch, tab.rec), _dev(torch, tab.pool), \
            _dev(torch, tab.state)
        kw = dict(d_slot_of=d_so.data_ptr(), slot_of_len=len(tab.slot_of), d_slot_rec=d_rec.data_ptr(),
                  n_slots=len(tab.state), d_pool=d_pool.data_ptr(), pool_len=len(tab.pool), d_state=d_state.data_ptr())
        ins += [(d_so, tab.slot_of), (d_rec, tab.rec), (d_pool, tab.pool)]
    torch.cuda.synchronize()
    ix.share_pick_dev(n_dests, d_doff.data_ptr(), d_t.data_ptr(), d_v.data_ptr(), cap, d_head.data_ptr(),
                      d_out.data_ptr(), d_key_clientid=d_kc.data_ptr() if keys else None,
                      d_key_topic=d_kt.data_ptr() if keys else None, n_topics=nt, seed=seed,
                      stream=stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    out = _host(d_out, E + TAIL)
    head = tuple(int(x) for x in d_head.cpu().numpy())
    assert head == whead
    assert np.array_equal(out[:E], want)
    assert (out[E:] == CANARY).all(), "written at or past E"
    for d, h in ins:
        assert np.array_equal(_host(d, len(h), h.dtype), h), "an input was modified"
    if own:
        slots = np.arange(len(tab.state), dtype=np.uint32)
        got_state = ix.share_state_get(slots)
    else:
        got_state = _host(d_state, len(tab.state))
    assert np.array_equal(got_state, wstate)
    return out[:E], head, wstate


def _values(rng, E, layout, tab):
    nv = len(tab.slot_of)
    if layout == "one":
        return np.full(E, 4, np.uint32) % max(nv, 1)
    if layout == "own":
        return (np.arange(E) % max(nv, 1)).astype(np.uint32)
    if layout == "alternating":
        return np.where(np.arange(E) % 2 == 0, 4, 5).astype(np.uint32)
    if layout == "runs":                                        # runs of 100 over 7 slots: a slot's entries lie apart
        return (4 + (np.arange(E) // 100) % 7).astype(np.uint32)
    v = rng.integers(0, nv + 40, E).astype(np.uint32)           # mixed: values past the table, values without a slot
    return v


@pytest.mark.parametrize("layout", ["one", "own", "alternating", "runs", "mixed"])
@pytest.mark.parametrize("size", ["0", "1", "63", "64", "65", "64G-1", "64G", "64G+1"])
def test_sizes_and_layouts(torch_dev, index, G, size, layout):
    E = {"64G-1": 64 * G - 1, "64G": 64 * G, "64G+1": 64 * G + 1}.get(size) or int(size)
    rng = np.random.default_rng(E * 31 + len(layout))
    n_slots = max(E, 16) if layout == "own" else 300
    # slots 4 .. 10 (the layouts' slots) are ranked ones: the rank runs up to E - 1
    tab = make_tables(rng, n_slots, none_every=11 if layout == "mixed" else 0,
                      strategies=RANKED if layout in ("one", "alternating", "runs") else range(8))
    topic = np.sort(rng.integers(0, max(E // 2, 1), E)).astype(np.uint32)
    value = _values(rng, E, layout, tab)
    member, head, _ = run_pick(torch_dev, index, tab, topic, value)
    if E and layout != "mixed":
        assert head[0] == E
    if layout == "one" and E > 1:
        assert head == (E, E) and len(set(member.tolist())) > 1


@pytest.mark.parametrize("n_slots", [500, 100_000, (1 << 20) + 1])
def test_slot_ids_needing_one_two_and_three_digit_passes(torch_dev, index, n_slots):
    rng = np.random.default_rng(n_slots)
    tab = make_tables(rng, n_slots, strategies=RANKED + (shared_sub.RANDOM,))
    E = 20_000
    value = rng.integers(0, n_slots, E).astype(np.uint32)
    value[:64] = n_slots - 1                                    # the highest slot, ranked 0 .. 63 and beyond
    value[100:4000:3] = n_slots - 2
    value[1::5] = rng.integers(0, 50, len(value[1::5]))         # long runs in a few slots
    topic = np.sort(rng.integers(0, 9000, E)).astype(np.uint32)
    run_pick(torch_dev, index, tab, topic, value)


def test_counts_strategies_and_start_states(torch_dev, index):
    """every count x every strategy byte (two unknown ones) x every start state the
    header names, n_local 0, 1, 2 and one past cnt, a span outside the pool"""
    rng = np.random.default_rng(5)
    cnts = [0, 1, 2, 3, 64, 65, 100_000]
    rows, state = [], []
    pos = 0
    for cnt in cnts:
        for strat in list(range(8)) + [255]:
            for j, c0 in enumerate((UNDEF, 0, max(cnt, 1) - 1, cnt, cnt + 5, 0xFFFFFFFE)):
                n_local = (0, 1, 2, cnt + 1)[(j + strat) % 4]
                init = (shared_sub.RANDOM, shared_sub.LOCAL, shared_sub.HASH_TOPIC, shared_sub.HASH_CLIENTID, 77)[(j + cnt) % 5]
                rows.append((pos if cnt < 100_000 else 0, cnt, n_local, strat | init << 8))
                state.append(c0)
                if cnt < 100_000:
                    pos += cnt
    pool_len = max(pos, 100_000)
    outside = len(rows)
    rows += [(pool_len - 2, 3, 1, shared_sub.ROUND_ROBIN), (0xFFFFFFF0, 0x20, 0, shared_sub.RANDOM)]   # spans outside the pool
    state += [3, 3]
    n_slots = len(rows)
    pool = rng.integers(0, 0xFFFFFFFF, pool_len, dtype=np.uint32)
    tab = Tables(np.arange(n_slots, dtype=np.uint32), np.array(rows, np.uint32), pool, state)
    value = np.repeat(np.arange(n_slots), 5)
    rng.shuffle(value)
    topic = np.sort(rng.integers(0, 700, len(value))).astype(np.uint32)
    member, head, after = run_pick(torch_dev, index, tab, topic, value)
    assert head[0] == len(value)
    assert (member[np.isin(value, [outside, outside + 1])] == NONE).all()
    assert after[outside] == 3 and after[outside + 1] == 3
    # NULL key arrays, and topic indices at or past n_topics: the key is 0
    run_pick(torch_dev, index, tab, topic, value, keys=False)
    run_pick(torch_dev, index, tab, topic, value, n_topics=350)


def test_the_cap_cut_and_a_total_below_the_arrays(torch_dev, index):
    rng = np.random.default_rng(6)
    tab = make_tables(rng, 200)
    E = 9000
    value = rng.integers(0, 200, E).astype(np.uint32)
    topic = np.sort(rng.integers(0, 3000, E)).astype(np.uint32)
    run_pick(torch_dev, index, tab, topic, value, cap=4097)              # cap cuts the total
    run_pick(torch_dev, index, tab, topic, value, cap=20_000, doff_total=7001)   # the total cuts cap
    run_pick(torch_dev, index, tab, topic, value, cap=0)


def test_three_calls_in_a_row_equal_one_run_over_the_concatenation(torch_dev, index):
    rng = np.random.default_rng(8)
    tab = make_tables(rng, 64, cnts=(2, 3, 5, 64))
    E = 3 * 5000
    value = rng.integers(0, 64, E).astype(np.uint32)
    topic = np.arange(E, dtype=np.uint32)                       # (random's hash sees the topic index: keep them distinct)
    doff = np.array([0, 0, 0, E, E], np.uint64)
    kc = np.random.default_rng(1).integers(0, 1 << 32, E, dtype=np.uint32)
    whole, _, wstate = pick_batch_ref(3, doff, topic, value, E, tab.slot_of, tab.rec, tab.pool, tab.state, kc, kc, E, 3)
    torch = torch_dev
    d_so, d_rec, d_pool, d_state = (_dev(torch, a) for a in (tab.slot_of, tab.rec, tab.pool, tab.state))
    d_kc = _dev(torch, kc)
    d_head = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = []
    for part in range(3):
        lo, hi = part * 5000, (part + 1) * 5000
        d_doff = _dev(torch, np.array([0, 0, 0, 5000, 5000], np.uint64))
        d_t, d_v = _dev(torch, topic[lo:hi]), _dev(torch, value[lo:hi])
        d_out = torch.zeros(5000, dtype=torch.int32, device="cuda")
        # the key arrays are indexed by topic: the whole arrays every time
        index.share_pick_dev(3, d_doff.data_ptr(), d_t.data_ptr(), d_v.data_ptr(), 5000, d_head.data_ptr(),
                             d_out.data_ptr(), d_key_clientid=d_kc.data_ptr(), d_key_topic=d_kc.data_ptr(), n_topics=E,
                             seed=3, d_slot_of=d_so.data_ptr(), slot_of_len=len(tab.slot_of), d_slot_rec=d_rec.data_ptr(),
                             n_slots=64, d_pool=d_pool.data_ptr(), pool_len=len(tab.pool), d_state=d_state.data_ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got.append(_host(d_out, 5000))
    assert np.array_equal(np.concatenate(got), whole)
    assert np.array_equal(_host(d_state, 64), wstate)


def test_two_streams_share_one_round_robin_per_group_slot(torch_dev, index):
    """both calls' whole transitions are atomic: together they pick every idx of
    [c0, c0 + m1 + m2) once, each call's picks consecutive in its own order"""
    torch = torch_dev
    m1, m2, c0, cnt = 6000, 5000, 17, 20_000
    rec = np.array([0, cnt, 0, shared_sub.ROUND_ROBIN_PER_GROUP], np.uint32)
    pool = np.arange(cnt, dtype=np.uint32)                      # member id = idx
    d_so, d_rec, d_pool = _dev(torch, np.zeros(1, np.uint32)), _dev(torch, rec), _dev(torch, pool)
    d_state = _dev(torch, np.array([c0], np.uint32))
    calls = []
    for m in (m1, m2):
        calls.append((m, _dev(torch, np.array([0, 0, 0, m, m], np.uint64)), _dev(torch, np.arange(m, dtype=np.uint32)),
                      _dev(torch, np.zeros(m, np.uint32)), torch.zeros(2, dtype=torch.int64, device="cuda"),
                      torch.zeros(m, dtype=torch.int32, device="cuda"), torch.cuda.Stream()))
    torch.cuda.synchronize()
    for m, d_doff, d_t, d_v, d_head, d_out, st in calls:
        index.share_pick_dev(3, d_doff.data_ptr(), d_t.data_ptr(), d_v.data_ptr(), m, d_head.data_ptr(), d_out.data_ptr(),
                             d_slot_of=d_so.data_ptr(), slot_of_len=1, d_slot_rec=d_rec.data_ptr(), n_slots=1,
                             d_pool=d_pool.data_ptr(), pool_len=cnt, d_state=d_state.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    a, b = (_host(c[5], c[0]).astype(np.int64) for c in calls)
    for x in (a, b):
        assert (np.diff(x) == 1).all()                          # consecutive in its own order
    assert sorted(np.concatenate([a, b]).tolist()) == list(range(c0, c0 + m1 + m2))
    assert int(_host(d_state, 1)[0]) == c0 + m1 + m2
    for c in calls:
        index.release_stream(c[6].cuda_stream)


def test_the_index_tables_and_state(torch_dev):
    """set_share_slots / set_share_members / share_state_set / _get against a host
    model: set, longer, shorter, empty, a slot twice in one call, the state array
    growing with its contents kept, and the calls' TM_EINVALs on a live index"""
    torch = torch_dev
    ix = _native.Index()
    try:
        rng = np.random.default_rng(9)
        n_values = 300
        slot_of = np.full(n_values, NONE, np.uint32)
        lists, meta, n_local, state = {}, {}, {}, {}

        def model():
            n_slots = max(list(lists) + [-1]) + 1
            rec, pool = np.zeros((n_slots, 4), np.uint32), []
            for s in range(n_slots):
                ids = lists.get(s, [])
                rec[s] = (len(pool), len(ids), n_local.get(s, 0), meta.get(s, 0))
                pool.extend(ids)
            st = np.array([state.get(s, UNDEF) for s in range(n_slots)], np.uint32)
            return Tables(slot_of, rec, np.array(pool, np.uint32), st)

        def set_members(slots, ls, strat):
            ix.set_share_members(slots, ls, [min(len(x), 1) for x in ls], [strat] * len(slots))
            for s, x in zip(slots, ls):
                lists[s], meta[s], n_local[s] = list(x), strat, min(len(x), 1)

        def pick(E=4000):
            value = rng.integers(0, n_values + 5, E).astype(np.uint32)
            topic = np.sort(rng.integers(0, 1500, E)).astype(np.uint32)
            _, _, after = run_pick(torch, ix, model(), topic, value, own=True)
            for s, w in enumerate(after.tolist()):
                if w != UNDEF or s in state:
                    state[s] = w

        run_pick(torch, ix, model(), [1, 2], [0, 1], own=True)   # nothing set: no slot anywhere
        vals = np.arange(0, n_values, 2, dtype=np.uint32)
        slot_of[vals] = vals % 40
        ix.set_share_slots(vals, slot_of[vals])
        set_members(list(range(40)), [rng.integers(0, 1 << 31, 2 + s % 5).tolist() for s in range(40)],
                    shared_sub.ROUND_ROBIN)
        pick()
        before = dict(state)
        set_members([3, 4], [rng.integers(0, 1 << 31, 70).tolist(), [5]], shared_sub.ROUND_ROBIN_PER_GROUP)   # longer, shorter
        set_members([5], [[]], shared_sub.STICKY)                # empty
        set_members([6, 6], [[1, 2, 3], [9, 8]], shared_sub.STICKY)   # a slot twice: the last list
        assert ix.share_state_get(list(range(40))).tolist() == [before.get(s, UNDEF) for s in range(40)], \
            "set_share_members touched a state"
        pick()
        ix.share_state_set([3, 7, 39], [2, UNDEF, 0xFFFFFFFE])
        state.update({3: 2, 7: UNDEF, 39: 0xFFFFFFFE})
        pick()
        # the state array grows (a slot far past its first allocation) with its contents kept
        slot_of[1] = 20_000
        ix.set_share_slots([1], [20_000])
        set_members([20_000], [[11, 12, 13]], shared_sub.ROUND_ROBIN_PER_GROUP)
        pick()
        assert ix.share_state_get([20_000, 3_000_000]).tolist()[1] == UNDEF
        ix.share_state_set([60_000], [5])                        # ... and through state_set
        state[60_000] = 5
        assert ix.share_state_get([60_000, 3]).tolist() == [5, state[3]]
        pick()
        # the TM_EINVALs decided before any work, on a live handle
        lib, h, p = ix._lib, ix._h, _native._ptr
        one, E = np.zeros(4, np.uint32), _native.TM_EINVAL
        assert lib.tm_set_share_slots(h, 1, None, p(one)) == E
        assert lib.tm_set_share_members(h, 1, p(one), p(np.array([2, 1], np.uint64)), p(one), p(one), p(one)) == E
        assert lib.tm_set_share_members(h, 1, p(one), p(np.array([0, 1], np.uint64)),
                                        p(np.array([NONE], np.uint32)), p(one), p(one)) == E
        assert lib.tm_set_share_members(h, 1, p(one), p(np.array([0, 1], np.uint64)), None, p(one), p(one)) == E
        assert lib.tm_set_share_members(h, 1, p(one), p(np.array([0, 0], np.uint64)), None, None, p(one)) == E
        assert lib.tm_share_state_set(h, 1, p(np.array([NONE], np.uint32)), p(one)) == E
        assert lib.tm_share_state_get(h, 5, 1, p(one), p(one)) == E
        d = torch.zeros(64, dtype=torch.int32, device="cuda")
        a = d.data_ptr()
        for n_dests, kw in ((0, {}), (65537, {}), (1, dict(doff=None)), (1, dict(head=None)), (1, dict(out=None)),
                            (1, dict(rec=a + 8)), (1, dict(state=None)), (1, dict(pool=None))):
            g = dict(doff=a, head=a, out=a, rec=a, state=a, pool=a)
            g.update(kw)
            assert lib.tm_share_pick_dev(h, n_dests, g["doff"], a, a, 4, None, None, 0, 0, a, 4, g["rec"], 2, g["pool"],
                                         4, g["state"], g["head"], g["out"], None) == E, (n_dests, kw)
        pick()                                                   # nothing of that changed anything
    finally:
        torch.cuda.synchronize()
        ix.close()
