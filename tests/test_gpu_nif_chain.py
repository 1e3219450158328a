"""The NIF's publish chain on the real library: c_src/tmatch_nif_share.c
(tmn_publish), tmatch_nif_deliver.c (tmn_deliver) and
tmatch_nif_publish_deliver.c (tmn_publish_deliver), linked with the four older
units and tests/native/nif_chain_shim.c against emqx_amd/libtmatch.so and run
on the device -- what the stand-in libtmatch of the CPU tests cannot vouch for:
the sizes of the first call's buffers, the words read back after TM_ECAP, the
rerun decided from them, and what the reruns do to the shared-subscription
state words.

The references are never the code under test:
  - the STAGED 64-bit calls (Index.publish_batch, deliver_batch,
    publish_deliver_batch, dispatch_batch, route_batch) on the same index,
    topics, keys and seed, with capacities so large that each is ONE library
    call, run from the same start state of the slots (share_state_set before,
    share_state_get after);
  - the numpy definitions tests/group_ref.py and tests/group_picks_ref.py over
    those calls' ungrouped outputs;
  - for the sizes of the forced reruns, the oracle (oracle/pyoracle.py) and the
    tables in plain numpy (nif_chain_shapes.py), asserted against the first
    capacities before the device is asked.
Every comparison is exact and whole: every slice through tmn_route_dest, every
member through tmn_picks, every delivery through tmn_deliveries, every group
through tmn_groups, tmn_direct, every err flag, every slot's state word.

A fresh set's first capacity is what tmn_get hands back for TMN_IDS_PER_TOPIC *
n + 1024 words (twice that for tmn_publish_deliver's deliveries); both numbers
come from the shim (shim_ids_per_topic, shim_first_cap), and the asserted
`reruns` says whether a shape landed where it was meant to.
"""
import threading
from collections import Counter

import numpy as np
import pytest

from emqx_amd import _native, shared_sub
from emqx_amd.shared_sub import NONE, UNDEF
from group_picks_ref import group_picks_ref
from group_ref import group_ref
from nif_chain import DELIVERIES, ENTRIES, GROUPS, Caller, load
from nif_chain_shapes import CASES, SHAPES, FatTables, check_case, topics_of
from test_gpu_publish_batch import _topics
from test_gpu_publish_deliver_batch32 import N_MEMBERS, Env, _keys, world   # noqa: F401  (world: a fixture)

pytestmark = pytest.mark.gpu

AGGRE, VRAM = _native.TM_ROUTE_AGGRE, _native.TM_ALLOC_VRAM
OK, ECAP, EINVAL = _native.TM_OK, _native.TM_ECAP, _native.TM_EINVAL
BIG = 1 << 18                 # the references' capacities: one library call each
SEED = 0x5EED
P_ONE, P_GRID = _native.TM_DEBUG_PUBLISH_ONE, _native.TM_DEBUG_PUBLISH_GRID
D_ONE, D_GRID = _native.TM_DEBUG_DELIVER_ONE, _native.TM_DEBUG_DELIVER_GRID
PD_ONE, PD_GRID = _native.TM_DEBUG_PUBLISH_DELIVER_ONE, _native.TM_DEBUG_PUBLISH_DELIVER_GRID
COUNTERS = (_native.TM_DEBUG_ROUTE_ONE, _native.TM_DEBUG_ROUTE_GRID, _native.TM_DEBUG_DISPATCH_ONE,
            _native.TM_DEBUG_DISPATCH_GRID, P_ONE, P_GRID, D_ONE, D_GRID, PD_ONE, PD_GRID,
            _native.TM_DEBUG_PATH_SMALL, _native.TM_DEBUG_PATH_PHASES)
FO1_ENTRIES, GP1_DELIVERIES, GS1_DELIVERIES = 16384, _native.GP1_DELIVERIES, _native.GS1_DELIVERIES


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def nif(tmp_path_factory, gpu):
    return load(tmp_path_factory.mktemp("nifchain"))


def _counters(ix, keys=COUNTERS):
    return np.array([ix.debug_get(k) for k in keys], np.int64)


# ---- the references: one staged call each, and the numpy definitions over them

def ref_publish(env, topics, kc, kt, seed, calls=1):
    """Index.publish_batch `calls` times from the state the slots are in -> [(route, deliveries, member, state after)]"""
    blob, offs = _native.pack_strings(topics)
    out = []
    for _ in range(calls):
        route, dl, member = env.ix.publish_batch(blob, offs, env.n_dests, env.local, cap=BIG, dcap=BIG, key_clientid=kc,
                                                 key_topic=kt, seed=seed)
        out.append((route, dl, member, env.state()))
    return out


def ref_deliver(env, topics, aggre):
    """Index.deliver_batch, checked against group_ref over Index.dispatch_batch -> (route, grouped deliveries, groups)"""
    blob, offs = _native.pack_strings(topics)
    route, dl, groups = env.ix.deliver_batch(blob, offs, env.n_dests, env.local, cap=BIG, dcap=BIG, gcap=BIG, aggre=aggre)
    _, (dt, dv, ds) = env.ix.dispatch_batch(blob, offs, env.n_dests, env.local, cap=BIG, dcap=BIG, aggre=aggre)
    T = len(dt)
    (G, W), et, ev, es, _, egs, ego = group_ref([0, T], dt, dv, ds, T, BIG)
    assert (W, G) == (len(dl[0]), len(groups[0])), "the staged call and the definition disagree"
    for a, b in zip(dl + groups, (et, ev, es, egs, ego)):
        assert np.array_equal(a, b), "the staged call and the definition disagree"
    return route, dl, groups


def ref_publish_deliver(env, topics, kc, kt, seed):
    """Index.publish_deliver_batch, once, from the state the slots are in -> (route, merged and grouped deliveries,
    member, groups, T, state after); the definition (group_picks_ref) over Index.publish_batch's output of the
    same batch from the same state must give the same lists"""
    blob, offs = _native.pack_strings(topics)
    start = env.state()
    route, dl, member, groups, T = env.ix.publish_deliver_batch(blob, offs, env.n_dests, env.local, cap=BIG, dcap=BIG,
                                                                gcap=BIG, key_clientid=kc, key_topic=kt, seed=seed)
    state = env.state()
    env.reset(start)
    (xroute, (xdt, xdv, xds), xmember, xstate), = ref_publish(env, topics, kc, kt, seed)
    assert np.array_equal(xstate, state) and np.array_equal(xmember, member), "the two staged calls disagree"
    K = len(member)
    (G, N), et, ev, es, _, egs, ego, W, _ = group_picks_ref([0, len(xdt)], xdt, xdv, xds, BIG, env.n_dests, xroute[0],
                                                            xroute[1], xroute[2], xmember, K, env.sub_of, BIG, BIG)
    assert W == T and N == len(dl[0]) and G == len(groups[0]), "the staged call and the definition disagree"
    for a, b in zip(dl + groups, (et, ev, es, egs, ego)):
        assert np.array_equal(a, b), "the staged call and the definition disagree"
    return route, dl, member, groups, T, state


def same_route(c, n, n_dests, route):
    rc, doff, t, v, err = c.slices(n, n_dests)
    assert rc == 0
    assert np.array_equal(doff, route[0]), "the slices' bounds"
    assert np.array_equal(t, route[1]) and np.array_equal(v, route[2]), "the slices' entries"
    assert np.array_equal(err, route[3]), "the err flags"


def same_deliveries(c, dl):
    rc, dt, dv, ds = c.deliveries()
    assert rc == 0 and len(dt) == len(dl[0]), "the delivery count"
    assert np.array_equal(dt, dl[0]) and np.array_equal(dv, dl[1]) and np.array_equal(ds, dl[2]), "the deliveries"


def same_groups(c, groups):
    rc, gs, go = c.groups()
    assert rc == 0 and len(gs) == len(groups[0]), "the group count"
    assert np.array_equal(gs, groups[0]) and np.array_equal(go, groups[1]), "the groups"


def same_picks(c, member):
    rc, m = c.picks()
    assert rc == 0 and len(m) == len(member), "the pick count"
    assert np.array_equal(m, member), "the picked members"


def run_publish(c, env, topics, kc, kt, seed, ref, state):
    """tmn_share_keys + tmn_pack + tmn_publish from the state the slots are in; everything against `ref`
    (route, deliveries, member) and the state words against `state`"""
    n = len(topics)
    assert c.pack(topics) == 0 and c.keys(n, kc, kt) == 0
    assert c.publish(n, env.n_dests, env.local, seed) == 0, env.ix._lib.tm_last_error(env.ix._h)
    same_route(c, n, env.n_dests, ref[0])
    same_deliveries(c, ref[1])
    same_picks(c, ref[2])
    assert c.groups()[0] == EINVAL and c.direct == 0 and c.dispatched == 2
    assert np.array_equal(env.state(), state), "the state words afterwards"


def run_deliver(c, env, topics, aggre, ref):
    n = len(topics)
    assert c.pack(topics) == 0
    assert c.deliver(n, env.n_dests, env.local, AGGRE if aggre else 0) == 0, env.ix._lib.tm_last_error(env.ix._h)
    same_route(c, n, env.n_dests, ref[0])
    same_deliveries(c, ref[1])
    same_groups(c, ref[2])
    assert c.picks()[0] == EINVAL and c.direct == 0 and c.dispatched == 3


def run_publish_deliver(c, env, topics, kc, kt, seed, ref):
    """... tmn_publish_deliver from the state the slots are in, against ref_publish_deliver's tuple"""
    n = len(topics)
    assert c.pack(topics) == 0 and c.keys(n, kc, kt) == 0
    assert c.publish_deliver(n, env.n_dests, env.local, seed) == 0, env.ix._lib.tm_last_error(env.ix._h)
    same_route(c, n, env.n_dests, ref[0])
    same_deliveries(c, ref[1])
    same_picks(c, ref[2])
    same_groups(c, ref[3])
    assert c.direct == ref[4] and c.dispatched == 4, "tmn_direct"
    assert np.array_equal(env.state(), ref[5]), "the state words afterwards"


# ---- A1. plain parity on the 76-filter world, every strategy

@pytest.fixture(scope="module")
def seven(world):   # noqa: F811
    """test_gpu_publish_deliver_batch32's world with member lists of 1 to 6 ids and EVERY strategy: slot s
    picks by strategy s % 7 (random, round_robin, round_robin_per_group, sticky, local, hash_clientid,
    hash_topic; sticky starts by hash_topic)"""
    w = world
    rng = np.random.default_rng(78)
    slots = list(range(w.n_slots))
    w.set_members(slots, [rng.permutation(N_MEMBERS)[:1 + s % 6].tolist() for s in slots],
                  [s % 7 | shared_sub.HASH_TOPIC << 8 for s in slots])
    return w


@pytest.fixture(scope="module")
def warm(seven, nif):
    """one set for the parity cases, its buffers grown by a first batch of each call: the world matches far
    more than TMN_IDS_PER_TOPIC entries per topic, so a FRESH set reruns (asserted here, and the rerun's
    results are compared like any other); the cases after it must not rerun again"""
    w = seven
    c = Caller(nif, w.ix, VRAM)
    topics = _topics(300, seed=4)
    kc, kt = _keys(len(topics), 4)
    w.env.reset()
    ref = ref_publish_deliver(w.env, topics, kc, kt, SEED)
    w.env.reset()
    run_publish_deliver(c, w.env, topics, kc, kt, SEED, ref)
    assert c.reruns >= 1, "the world's first batch fitted a fresh set: no rerun was exercised"
    r = c.reruns
    run_deliver(c, w.env, topics, True, ref_deliver(w.env, topics, True))
    w.env.reset()
    (route, dl, member, state), = ref_publish(w.env, topics, kc, kt, SEED)
    w.env.reset()
    run_publish(c, w.env, topics, kc, kt, SEED, (route, dl, member), state)
    assert c.reruns == r, "the sizes are sticky: the other two calls found the buffers grown"
    yield c
    c.close()


@pytest.mark.parametrize("n", [64, 300])
@pytest.mark.parametrize("keys", ["both", "clientid", "topic", "none"])
def test_plain_parity_every_strategy_and_key_choice(seven, warm, keys, n):
    """tmn_publish / tmn_deliver / tmn_publish_deliver == ONE Index.publish_batch / deliver_batch /
    publish_deliver_batch each (and the definitions group_ref / group_picks_ref), from UNDEF and from a moved
    start state; no rerun on the warm set; 64 topics end in the one-workgroup kernels (TM_DEBUG_*_ONE)"""
    w, c, env, ix = seven, warm, seven.env, seven.ix
    topics = _topics(n, seed=n + 5)
    kc, kt = _keys(n, n)
    kc, kt = (kc if keys in ("both", "clientid") else None), (kt if keys in ("both", "topic") else None)
    blob, offs = _native.pack_strings(topics)
    total = int(ix.route_batch(blob, offs, env.n_dests)[0][-1])
    r0 = c.reruns
    start = None
    for _ in range(2):
        env.reset(start)
        ref = ref_publish_deliver(env, topics, kc, kt, SEED)
        K, T = len(ref[2]), ref[4]
        env.reset(start)
        c0 = _counters(ix)
        run_publish_deliver(c, env, topics, kc, kt, SEED, ref)
        refp = ref_publish_state(env, topics, kc, kt, start)
        c1 = _counters(ix)
        run_publish(c, env, topics, kc, kt, SEED, refp, ref[5])
        c2 = _counters(ix)
        refd = ref_deliver(env, topics, True)
        c3 = _counters(ix)
        run_deliver(c, env, topics, True, refd)
        c4 = _counters(ix)
        dpd, dp, dd = dict(zip(COUNTERS, c1 - c0)), dict(zip(COUNTERS, c2 - c1)), dict(zip(COUNTERS, c4 - c3))
        assert dpd[PD_ONE] + dpd[PD_GRID] == 1 and dp[P_ONE] + dp[P_GRID] == 1 and dd[D_ONE] + dd[D_GRID] == 1
        if n == 64:
            assert total <= FO1_ENTRIES and T + K <= GP1_DELIVERIES and T <= GS1_DELIVERIES
            assert (dpd[PD_ONE], dp[P_ONE], dd[D_ONE]) == (1, 1, 1), "the one-workgroup endings, in place"
        assert not np.array_equal(ref[5], env_start(env, start)), "no state word moved: nothing was picked"
        start = ref[5]
    assert c.reruns == r0, "a rerun on a warm set"
    member = ref[2]
    picked = ref[0][2][member != NONE]
    used = {w.meta[int(s)] & 0xFF for s in w.slot_of[picked]}
    assert used == set(range(7)), "a strategy without a pick"
    local = member[member != NONE]
    assert (env.sub_of[local] != NONE).any() and (env.sub_of[local] == NONE).any(), "local and remote picks"


def env_start(env, start):
    return np.full(len(env.slots), UNDEF, np.uint32) if start is None else start


def ref_publish_state(env, topics, kc, kt, start):
    """ONE Index.publish_batch from `start` -> (route, deliveries, member); the slots are put back to `start`"""
    env.reset(start)
    (route, dl, member, _), = ref_publish(env, topics, kc, kt, SEED)
    env.reset(start)
    return route, dl, member


# ---- A2-A5. forced reruns on the smallest indexes that do it (nif_chain_shapes.py)

class Fat:
    """a shape of nif_chain_shapes.py (FatTables) on the device, and the slots its picks may move"""

    def __init__(self, shape):
        self.tab = tab = FatTables(**SHAPES[shape])
        self.ix = ix = _native.Index()
        vals = np.arange(tab.nv, dtype=np.uint32)
        routed = np.nonzero(tab.dest_of != NONE)[0].astype(np.uint32)
        ix.set_dests(routed, tab.dest_of[routed])
        ix.set_route_filters(vals, tab.filt_of)
        blob, offs = _native.pack_strings([tab.flt] * tab.nv)
        ix.apply(np.ones(tab.nv, np.uint8), blob, offs, vals)
        ix.set_subscribers(list(tab.subs), [tab.subs[v] for v in tab.subs])
        slots = list(range(len(tab.members)))
        ix.set_share_slots(tab.slot_values, slots)
        ix.set_share_members(slots, tab.members, tab.n_local, tab.meta)
        ix.set_member_subs(np.arange(len(tab.sub_of), dtype=np.uint32), tab.sub_of)
        self.env = Env(ix, tab.n_dests, tab.local, slots, tab.sub_of)

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.ix.close()


@pytest.fixture(scope="module")
def fats(gpu):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Fat(shape)
        return made[shape]
    yield get
    for f in made.values():
        f.close()


def planned(nif, fat, case):
    """the case's totals from the oracle and the tables alone (no device) against the first capacities the shim
    reports on this index; printed, so a run's log holds the (total, K, T, G, capacity) tuple of every case"""
    p = check_case(case, nif.shim_ids_per_topic(), lambda words: nif.shim_first_cap(fat.ix._h, words))
    print(f"planned {case}: {p}")
    return p


def test_publish_reruns_from_the_entries(nif, fats):
    """a fresh set, total > the first capacity, T below it: ONE rerun; members and state equal ONE
    Index.publish_batch (the first call picked nothing); TM_DEBUG_PUBLISH_ONE moves by 0 (a call under TM_ECAP
    from cap counts on neither leg) + 1"""
    fat = fats("thick")
    env, n = fat.env, CASES["publish-entries"][1]
    p = planned(nif, fat, "publish-entries")
    topics = topics_of(n)
    kc, kt = _keys(n, 21)
    env.reset()
    (route, dl, member, state), = ref_publish(env, topics, kc, kt, SEED)
    assert (int(route[0][-1]), len(dl[0])) == (p["K"], p["T"]), "the plan's totals are the device's"
    assert not np.array_equal(state, env_start(env, None))
    c = Caller(nif, fat.ix, VRAM)
    try:
        env.reset()
        c0 = _counters(fat.ix, (P_ONE, P_GRID))
        run_publish(c, env, topics, kc, kt, SEED, (route, dl, member), state)
        assert c.reruns == 1
        assert (_counters(fat.ix, (P_ONE, P_GRID)) - c0).tolist() == [1, 0]
        assert c.cap(ENTRIES) >= p["total"] and c.cap(DELIVERIES) == p["cap"], "only the entry buffers grew"
    finally:
        c.close()


def test_publish_reruns_from_the_deliveries_alone_and_picks_twice(nif, fats):
    """the entries fit, T > the first dcap: ONE rerun that picks AGAIN -- the members are those of the SECOND
    of two Index.publish_batch calls from the same start state and the state is the state after two; the same
    batch again on the same set: no rerun (sticky sizes), the THIRD call's members and state"""
    fat = fats("deliveries")
    env, n = fat.env, CASES["publish-deliveries"][1]
    p = planned(nif, fat, "publish-deliveries")
    topics = topics_of(n)
    kc, kt = _keys(n, 22)
    env.reset()
    refs = ref_publish(env, topics, kc, kt, SEED, calls=3)
    assert len(refs[0][1][0]) == p["T"] and int(refs[0][0][0][-1]) == p["K"]
    assert not np.array_equal(refs[0][2], refs[1][2]) and not np.array_equal(refs[1][2], refs[2][2]), \
        "the calls pick alike: the test could not tell one pick from two"
    assert len({tuple(r[3].tolist()) for r in refs}) == 3
    c = Caller(nif, fat.ix, VRAM)
    try:
        env.reset()
        c0 = _counters(fat.ix, (P_ONE, P_GRID))
        run_publish(c, env, topics, kc, kt, SEED, refs[1][:3], refs[1][3])
        assert c.reruns == 1
        assert (_counters(fat.ix, (P_ONE, P_GRID)) - c0).tolist() == [2, 0], "both calls picked, in place"
        assert c.cap(ENTRIES) == p["cap"] and c.cap(DELIVERIES) >= p["T"], "only the delivery buffers grew"
        run_publish(c, env, topics, kc, kt, SEED, refs[2][:3], refs[2][3])
        assert c.reruns == 1, "the sizes are sticky"
        assert (_counters(fat.ix, (P_ONE, P_GRID)) - c0).tolist() == [3, 0]
    finally:
        c.close()


@pytest.mark.parametrize("kind,shape,reruns", [("entries", "thin", 1), ("deliveries", "deliveries", 1), ("both", "thick", 2)])
def test_publish_deliver_reruns_and_a_round_robin_advances_once(nif, fats, kind, shape, reruns):
    """total > cap, T + K > dcap, and one after the other (two reruns): members, merged and grouped deliveries,
    groups, tmn_direct and the state equal ONE Index.publish_deliver_batch -- no call under TM_ECAP picked.
    Every call ends in the one workgroup (TM_DEBUG_PUBLISH_DELIVER_ONE counts a TM_ECAP that moved nothing)"""
    fat = fats(shape)
    env, n = fat.env, CASES["pd-" + kind][1]
    p = planned(nif, fat, "pd-" + kind)
    topics = topics_of(n)
    kc, kt = _keys(n, 23)
    env.reset()
    ref = ref_publish_deliver(env, topics, kc, kt, SEED)
    assert (len(ref[2]), ref[4]) == (p["K"], p["T"]), "the plan's totals are the device's"
    assert len(ref[1][0]) > ref[4] > 0 and not np.array_equal(ref[5], env_start(env, None))
    c = Caller(nif, fat.ix, VRAM)
    try:
        env.reset()
        c0 = _counters(fat.ix, (PD_ONE, PD_GRID))
        run_publish_deliver(c, env, topics, kc, kt, SEED, ref)
        assert c.reruns == reruns
        assert (_counters(fat.ix, (PD_ONE, PD_GRID)) - c0).tolist() == [1 + reruns, 0]
        assert (c.cap(ENTRIES) > p["cap"]) == (kind != "deliveries"), "the entry buffers grew exactly when they were short"
        assert (c.cap(DELIVERIES) > p["pd_dcap"]) == (kind != "entries"), "the delivery buffers likewise"
        assert c.cap(GROUPS) >= c.cap(DELIVERIES), "room for a group per delivery slot"
        env.reset(ref[5])                                        # the same batch again: sticky sizes, one call
        again = ref_publish_deliver(env, topics, kc, kt, SEED)
        env.reset(ref[5])
        run_publish_deliver(c, env, topics, kc, kt, SEED, again)
        assert c.reruns == reruns and (_counters(fat.ix, (PD_ONE, PD_GRID)) - c0).tolist() == [2 + reruns, 0]
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["entries", "deliveries", "groups"])
def test_deliver_reruns_of_each_kind(nif, fats, kind):
    """tmn_deliver == Index.deliver_batch and group_ref.  entries: total > cap.  deliveries: T > dcap with more
    distinct subscribers than the first gcap -- the rerun's groups have room for a group per delivery, so it is
    the last.  groups alone: the set's delivery buffers are large from an earlier tmn_dispatch of a fat batch,
    its group buffers still unallocated, and the batch has more distinct subscribers than the first gcap"""
    fat = fats("thin" if kind == "entries" else "wide")
    env, ix = fat.env, fat.ix
    n = CASES["deliver-" + kind][1]
    p = planned(nif, fat, "deliver-" + kind)
    topics = topics_of(n)
    aggre = kind == "entries"
    ref = ref_deliver(env, topics, aggre)
    assert (int(ref[0][0][-1]), len(ref[1][0]), len(ref[2][0])) == (p["K" if aggre else "total"], p["T"], p["G"]), \
        "the plan's totals are the device's"
    c = Caller(nif, ix, VRAM)
    try:
        before = 0
        if kind == "groups":
            fatter = topics_of(2)
            p2 = planned(nif, fat, "deliver-groups-dispatch-before")
            blob, offs = _native.pack_strings(fatter)
            route, dl = ix.dispatch_batch(blob, offs, env.n_dests, env.local, cap=BIG, dcap=BIG)
            assert c.pack(fatter) == 0 and c.dispatch(2, env.n_dests, env.local, 0) == 0
            same_route(c, 2, env.n_dests, route)
            same_deliveries(c, dl)
            assert c.picks()[0] == EINVAL and c.groups()[0] == EINVAL and c.direct == 0
            before = c.reruns
            assert before == 1 and c.cap(DELIVERIES) >= p2["T"] >= p["T"] and c.cap(GROUPS) == 0
        c0 = _counters(ix, (D_ONE, D_GRID))
        run_deliver(c, env, topics, aggre, ref)
        assert c.reruns - before == 1
        d = _counters(ix, (D_ONE, D_GRID)) - c0
        assert d.sum() == 2 and d[0] >= 1, "two calls, the one that stands in the one workgroup"
        if kind == "deliveries":
            assert c.cap(GROUPS) >= p["T"], "a group per delivery"
        if kind == "groups":
            assert p["cap"] < p["G"] <= c.cap(GROUPS) and c.cap(DELIVERIES) >= p2["T"]
        run_deliver(c, env, topics, aggre, ref)                  # sticky sizes
        assert c.reruns - before == 1
    finally:
        c.close()


# ---- A6. one set through every entry point in turn

def test_one_set_through_every_entry_point_in_turn(seven, nif):
    """tmn_route, tmn_dispatch, tmn_publish, tmn_deliver, tmn_publish_deliver, tmn_match, tmn_first and back to
    tmn_publish_deliver on ONE set, whose buffers they share: each equals its staged call (route_batch,
    dispatch_batch, publish_batch, deliver_batch, publish_deliver_batch; match_batch / first_batch here -- the
    match half against the oracle is tests/test_gpu_nif_match.py), and the readers refuse the wrong kind"""
    w, env, ix = seven, seven.env, seven.ix
    topics = _topics(64, seed=61)
    n, nd, local = len(topics), env.n_dests, env.local
    kc, kt = _keys(n, 61)
    blob, offs = _native.pack_strings(topics)
    c = Caller(nif, ix, VRAM)
    try:
        assert c.slices(n, nd)[0] == EINVAL and c.deliveries()[0] == EINVAL and c.picks()[0] == EINVAL
        assert c.groups()[0] == EINVAL and c.direct == 0, "a set that has run nothing has nothing to read"
        assert c.pack(topics) == 0
        # tmn_route (no aggre), tmn_route_aggre
        assert c.route(n, nd) == 0
        same_route(c, n, nd, ix.route_batch(blob, offs, nd, cap=BIG))
        assert c.deliveries()[0] == EINVAL and c.picks()[0] == EINVAL and c.groups()[0] == EINVAL and c.direct == 0
        assert c.route(n, nd, aggre=True) == 0
        same_route(c, n, nd, ix.route_batch(blob, offs, nd, cap=BIG, aggre=True))
        # tmn_dispatch
        route, dl = ix.dispatch_batch(blob, offs, nd, local, cap=BIG, dcap=BIG, aggre=True)
        assert c.dispatch(n, nd, local, AGGRE) == 0
        same_route(c, n, nd, route)
        same_deliveries(c, dl)
        assert c.picks()[0] == EINVAL and c.groups()[0] == EINVAL and c.direct == 0 and c.dispatched == 1
        # tmn_publish
        env.reset()
        (route, dl, member, state), = ref_publish(env, topics, kc, kt, SEED)
        env.reset()
        run_publish(c, env, topics, kc, kt, SEED, (route, dl, member), state)
        # tmn_deliver
        run_deliver(c, env, topics, True, ref_deliver(env, topics, True))
        run_deliver(c, env, topics, False, ref_deliver(env, topics, False))
        # tmn_publish_deliver
        env.reset(state)
        ref = ref_publish_deliver(env, topics, kc, kt, SEED)
        env.reset(state)
        run_publish_deliver(c, env, topics, kc, kt, SEED, ref)
        assert c.direct == ref[4] > 0
        # tmn_match, every order, and tmn_first: the value, err and offset buffers are the ones the chain used
        for order in (_native.TM_ORDER_TRAVERSAL, _native.TM_ORDER_SORTED, _native.TM_ORDER_UNIQUE):
            uc = np.zeros(n, np.uint32)
            unique = order == _native.TM_ORDER_UNIQUE
            hit, vals, err = ix.match_batch(blob, offs, order=order, unique_counts=uc if unique else None)
            assert c.match(n, order) == 0
            flags, cnt, got = c.rows(n, order)
            exp_cnt = uc.astype(np.int64) if unique else np.diff(hit.astype(np.int64))
            assert np.array_equal(flags, err) and np.array_equal(cnt, exp_cnt)
            lo = hit[:-1].astype(np.int64)
            at = np.repeat(lo - np.concatenate(([0], np.cumsum(exp_cnt)[:-1])), exp_cnt) + np.arange(int(exp_cnt.sum()))
            assert np.array_equal(got, vals[at]), "tmn_row's values"
        val, found = ix.first_batch(blob, offs)
        assert c.first(n) == 0
        gf, gv = c.firsts(n)
        assert np.array_equal(gf, found) and np.array_equal(gv[found == 1], val[found == 1]) and (found == 1).any()
        # and back: the same state, the same answer
        env.reset(state)
        run_publish_deliver(c, env, topics, kc, kt, SEED, ref)
    finally:
        c.close()


# ---- A7. refusals before any device work

@pytest.mark.parametrize("entry", ["publish", "deliver", "publish_deliver"])
def test_refusals_before_any_device_work(seven, nif, entry):
    """keys set for another n (the two picking calls), n_dests of 0 or 65537, local_dest == n_dests: TM_EINVAL,
    no debug counter moves, the state words are unchanged, nothing is left to read, and the set still works"""
    w, env, ix = seven, seven.env, seven.ix
    topics = _topics(40, seed=71)
    n, nd, local = len(topics), env.n_dests, env.local
    kc, kt = _keys(n, 71)
    c = Caller(nif, ix, VRAM)
    try:
        env.reset()
        ref = ref_publish_deliver(env, topics, kc, kt, SEED)
        start = ref[5]                                           # (a moved state: a word put back would show)
        env.reset(start)
        assert c.pack(topics) == 0 and c.keys(n, kc, kt) == 0
        assert c.publish_deliver(n, nd, local, SEED) == 0        # something to read, which a refusal must take away
        r0 = c.reruns
        env.reset(start)
        call = {"publish": lambda n_, nd_, l_: c.publish(n_, nd_, l_, SEED),
                "deliver": lambda n_, nd_, l_: c.deliver(n_, nd_, l_, AGGRE),
                "publish_deliver": lambda n_, nd_, l_: c.publish_deliver(n_, nd_, l_, SEED)}[entry]
        bad = [(n, 0, 0), (n, 65537, local), (n, nd, nd)]
        if entry != "deliver":                                   # the keys are set for n topics
            bad += [(n - 1, nd, local), (n + 1, nd, local)]
        c0 = _counters(ix)
        for args in bad:
            assert call(*args) == EINVAL, args
            assert c.slices(n, nd)[0] == EINVAL and c.deliveries()[0] == EINVAL and c.picks()[0] == EINVAL
            assert c.groups()[0] == EINVAL and c.direct == 0 and c.dispatched == 0
        assert np.array_equal(_counters(ix), c0), "a refused call reached the library's batch paths"
        assert np.array_equal(env.state(), start), "a refused call moved a state word"
        assert c.reruns == r0
        again = ref_publish_deliver(env, topics, kc, kt, SEED)
        env.reset(start)
        run_publish_deliver(c, env, topics, kc, kt, SEED, again)
    finally:
        c.close()


# ---- A8. empty and tiny batches

@pytest.mark.parametrize("topics", [[], [b"no/such/topic/anywhere/at/all/x"], [b"+"]], ids=["n0", "no-match", "plus"])
def test_empty_and_tiny_batches(nif, fats, topics):
    """n = 0, one topic without a match (the 'tiny' shape's filters are 'a/+'), one topic that is a '+' level
    (err 1): the three calls equal their staged calls, with nothing or next to nothing to read"""
    fat = fats("tiny")
    env, n = fat.env, len(topics)
    kc, kt = _keys(n, 8)
    kc, kt = (kc[:n], kt[:n]) if n else (None, None)
    c = Caller(nif, fat.ix, VRAM)
    try:
        env.reset()
        ref = ref_publish_deliver(env, topics, kc, kt, SEED)
        env.reset()
        run_publish_deliver(c, env, topics, kc, kt, SEED, ref)
        (route, dl, member, state), = ref_publish(env, topics, kc, kt, SEED)
        env.reset(ref[5])
        run_publish(c, env, topics, kc, kt, SEED, (route, dl, member), state)
        run_deliver(c, env, topics, False, ref_deliver(env, topics, False))
        assert c.reruns == 0
        rc, doff, t, v, err = c.slices(n, env.n_dests)
        assert int(doff[-1]) == 0 and err.tolist() == ([1] if topics == [b"+"] else [0] * n)
        assert c.deliveries()[1].size == 0 and c.groups()[1].size == 0 and c.groups()[2].tolist() == [0]
    finally:
        c.close()


# ---- A9. eight callers and a writer

def test_eight_threads_one_pool_and_a_writer(nif, fats):
    """eight threads, each with its own set from ONE pool, run 20 tmn_publish_deliver batches on one index; a
    ninth applies and removes filters no topic matches.  The reference is the single-threaded
    Index.publish_deliver_batch of each thread's batch.  Slot 0 is round_robin_per_group with five REMOTE
    members and is shared by all: its picks are no thread's own to predict, so they are compared as a multiset
    over all threads -- those of as many sequential calls -- and its word must have advanced by exactly the
    picks made on it; every other slot picks by a hash of the keys, statelessly, and every slice, member,
    delivery and group of every batch is the reference's"""
    fat = fats("threads")
    env, ix, tab = fat.env, fat.ix, fat.tab
    THREADS, ROUNDS, c0 = 8, 20, 3
    rr_values = set(np.asarray(tab.slot_values)[:1].tolist())        # slot 0's value
    rr_members = np.asarray(tab.members[0], np.uint32)
    batches = [[b"t/%d/%d" % (i, k) for k in range(12)] for i in range(THREADS)]
    keys = [_keys(12, 90 + i) for i in range(THREADS)]
    refs = []
    for i in range(THREADS):
        env.reset()
        refs.append(ref_publish_deliver(env, batches[i], keys[i][0], keys[i][1], SEED))
    per_batch = int(np.isin(refs[0][0][2], list(rr_values)).sum())
    assert per_batch == 12 and all(np.array_equal(env_start(env, None)[1:], r[5][1:]) for r in refs), \
        "a stateful slot besides slot 0"
    pool = nif.shim_pool_new(ix._h, VRAM)
    callers = [Caller(nif, ix, pool=pool) for _ in range(THREADS)]
    picks, errors, stop = [[] for _ in range(THREADS)], [], threading.Event()

    def work(i):
        try:
            c, ref = callers[i], refs[i]
            on_rr = np.isin(ref[0][2], list(rr_values))
            for _ in range(ROUNDS):
                assert c.pack(batches[i]) == 0 and c.keys(12, *keys[i]) == 0
                assert c.publish_deliver(12, env.n_dests, env.local, SEED) == 0
                same_route(c, 12, env.n_dests, ref[0])
                same_deliveries(c, ref[1])
                same_groups(c, ref[3])
                rc, m = c.picks()
                assert rc == 0 and len(m) == len(ref[2]) and np.array_equal(m[~on_rr], ref[2][~on_rr])
                assert c.direct == ref[4] and c.reruns == 0
                picks[i].extend(m[on_rr].tolist())
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    def write():
        try:
            fs = [b"zz/%d/+" % k for k in range(16)]
            blob, offs = _native.pack_strings(fs)
            vals = np.arange(1000, 1016, dtype=np.uint32)
            for _ in range(200):
                if stop.is_set():
                    break
                ix.apply(np.ones(16, np.uint8), blob, offs, vals)
                ix.apply(np.zeros(16, np.uint8), blob, offs, vals)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
    try:
        ix.share_state_set([0], [c0])
        o0 = _counters(ix, (PD_ONE, PD_GRID))
        ths = [threading.Thread(target=work, args=(i,)) for i in range(THREADS)]
        wr = threading.Thread(target=write)
        wr.start()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        stop.set()
        wr.join()
        assert not errors, errors
        total = THREADS * ROUNDS * per_batch
        assert (_counters(ix, (PD_ONE, PD_GRID)) - o0).tolist() == [THREADS * ROUNDS, 0]
        got = Counter(p for ps in picks for p in ps)
        assert sum(got.values()) == total
        assert got == Counter(int(rr_members[(c0 + k) % len(rr_members)]) for k in range(total))
        assert ix.share_state_get([0]).tolist() == [(c0 + total - 1) % len(rr_members) + 1]
        assert np.array_equal(env.state()[1:], env_start(env, None)[1:])
    finally:
        for c in callers:
            c.close()
        assert nif.shim_pool_count(pool) == THREADS, "every set is back in the pool"
        nif.shim_pool_free(pool)
