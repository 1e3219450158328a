"""CPU-side checks of the shared-subscription pick: the new calls are exported
and refuse a null handle (the argument checks need a live handle: the GPU files); the numpy definition of
tm_share_pick_dev (shared_sub.pick_batch_ref) equals SharedSubs.pick -- the
transcription of pick/6, do_pick/7 and pick_subscriber/6 -- called once per
message in message order, over seeded histories that interleave subscribe and
unsubscribe between batches, for every strategy (random and local are made
comparable by giving the transcription the definition's hash as its
rand:uniform); and the special cases the header names."""
import random

import numpy as np
import pytest

from emqx_amd import _native, build, shared_sub
from emqx_amd.shared_sub import NONE, UNDEF, SharedSubs, pick_batch_ref

NEW = ("tm_set_share_slots", "tm_set_share_members", "tm_share_state_set", "tm_share_state_get", "tm_share_pick_dev",
       "tm_publish_batch")


def test_new_calls_are_exported_and_refuse_a_null_handle():
    build.build_tmatch()
    lib = _native.load_library()
    for name in NEW:
        assert name in _native.EXPORTS and hasattr(lib, name)
    # No index can be created without a device, so only the null-handle refusal is
    # reachable here, once per call.  The argument checks proper -- decreasing
    # offsets, member id 0xFFFFFFFF, tm_publish_batch without TM_ROUTE_AGGRE,
    # local_dest >= n_dests, null and misaligned buffers -- are asserted on a live
    # handle in tests/test_gpu_share.py and tests/test_gpu_publish_batch.py.
    E = _native.TM_EINVAL
    assert lib.tm_set_share_slots(None, 0, None, None) == E
    assert lib.tm_set_share_members(None, 0, None, None, None, None, None) == E
    assert lib.tm_share_state_set(None, 0, None, None) == E
    assert lib.tm_share_state_get(None, 0, 0, None, None) == E
    assert lib.tm_share_pick_dev(None, 1, None, None, None, 0, None, None, 0, 0, None, 0, None, 0, None, 0, None, None,
                                 None, None) == E
    assert lib.tm_publish_batch(None, 0, None, None, 1, 0, _native.TM_ROUTE_AGGRE, None, None, None, 0, None, None, None,
                                None, 0, None, None, 0, None, None) == E


def test_abi_minor_version_and_constants():
    v = _native.load_library().tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 18
    assert _native.TM_SHARE_NONE == _native.TM_SHARE_UNDEF == 0xFFFFFFFF == NONE == UNDEF
    names = ("RANDOM", "ROUND_ROBIN", "ROUND_ROBIN_PER_GROUP", "STICKY", "LOCAL", "HASH_CLIENTID", "HASH_TOPIC")
    for i, n in enumerate(names):
        assert getattr(_native, "TM_SHARE_" + n) == getattr(shared_sub, n) == i
        assert shared_sub.STRATEGIES[n.lower()] == i
    header = (build.ROOT / "include" / "tmatch.h").read_text()
    for i, n in enumerate(names):
        assert f"TM_SHARE_{n} = {i}" in header


# ---- the definition against the transcription

class DeviceModel:
    """what the on_change hook of SharedSubs keeps on the device: records, pool, state"""

    def __init__(self):
        self.rec, self.pool, self.state = [], [], []

    def on_change(self, slot, ids, n_local, meta, state):
        while len(self.rec) <= slot:
            self.rec.append((0, 0, 0, 0))
            self.state.append(UNDEF)
        self.rec[slot] = (len(self.pool), len(ids), n_local, meta)
        self.pool.extend(ids)
        if state is not None:
            self.state[slot] = state

    def arrays(self):
        return (np.array(self.rec, dtype=np.uint32).reshape(-1), np.array(self.pool, dtype=np.uint32),
                np.array(self.state, dtype=np.uint32))


def _run_batch(subs, dev, msgs, key_c, key_t):
    """msgs: [(message index, group, topic)] in entry order -> checks the
    definition against one SharedSubs.pick per message; the model's state moves"""
    rec, pool, state = dev.arrays()
    n_slots = len(state)
    slot_of = np.arange(n_slots + 3, dtype=np.uint32)
    slot_of[n_slots:] = NONE                                   # values without a slot
    slots = [subs.slot(g, t) for _, g, t in msgs]
    value = np.array([n_slots + 1 if s is None else s for s in slots], dtype=np.uint32)
    topic = np.array([m for m, _, _ in msgs], dtype=np.uint32)
    doff = np.array([0, len(msgs), len(msgs)], dtype=np.uint64)
    member, head, after = pick_batch_ref(1, doff, topic, value, len(msgs), slot_of, rec, pool, state, key_c, key_t,
                                         len(key_c), subs.seed)
    for g, t in {(g, t) for _, g, t in msgs if subs.slot(g, t) is not None}:
        subs.adopt_state(g, t, int(state[subs.slot(g, t)]))   # the host's tables hold what the device held
    want = []
    for m, g, t in msgs:
        r = subs.pick(g, t, int(key_c[m]), int(key_t[m]), None, m)
        want.append(subs.pid_id(r[1]) if r else NONE)
    assert member.tolist() == want
    assert head == (sum(s is not None for s in slots), sum(w != NONE for w in want))
    for g, t in {(g, t) for _, g, t in msgs if subs.slot(g, t) is not None}:
        s = subs.slot(g, t)
        mem, _ = subs.members(g, t)
        stateful = subs.strategy(g) in SharedSubs.STATEFUL
        if stateful and len(mem) >= 2:
            assert int(after[s]) == subs.device_state(g, t), (g, t, subs.strategy(g))
        elif not (subs.strategy(g) == "sticky" and len(mem) == 1):
            assert int(after[s]) == int(state[s])              # the singleton rule, the stateless strategies
    dev.state = after.tolist()


@pytest.mark.parametrize("strategy,initial", [
    ("round_robin", None), ("round_robin_per_group", None), ("hash_clientid", None), ("hash_topic", None),
    ("sticky", "hash_clientid"), ("sticky", "hash_topic"), ("sticky", "random"), ("sticky", "local"),
    ("random", None), ("local", None)])
def test_definition_equals_sequential_picks_over_histories(strategy, initial):
    rng = random.Random(f"{strategy}/{initial}")
    dev = DeviceModel()
    subs = SharedSubs(node="n1", on_change=dev.on_change, seed=rng.getrandbits(32))
    groups = [b"g1", b"g2", b"g3"]
    for g in groups:
        subs.set_strategy(g, strategy, initial)
    topics = [b"t/1", b"t/+", b"#"]
    pids = [("n1" if i % 3 else "n2", i) for i in range(80)]
    for step in range(40):
        for _ in range(rng.randrange(0, 12)):                   # subscriptions change between batches
            g, t, p = rng.choice(groups), rng.choice(topics), rng.choice(pids[:10 if step % 2 else 80])
            if rng.random() < 0.55:
                subs.subscribe(g, t, p)
            else:
                subs.unsubscribe(g, t, p)
        if step == 20:                                          # a pid goes down everywhere
            subs.down(pids[1])
        n = rng.choice((1, 5, 64, 200))
        key_c = np.array([rng.getrandbits(32) for _ in range(n)], dtype=np.uint32)
        key_t = np.array([rng.getrandbits(32) for _ in range(n)], dtype=np.uint32)
        msgs = []
        for m in range(n):                                      # aggre/1: one entry per (message, {Group, To})
            for g in groups:
                for t in topics:
                    if rng.random() < 0.3:
                        msgs.append((m, g, t))
        msgs.sort(key=lambda x: (x[1], x[0]))                   # the fan-out's order: bucket-major, message order within
        _run_batch(subs, dev, msgs, key_c, key_t)


def _one_slot(cnt, strategy, c0, n_entries, n_local=0, init=0, seed=7, keys=None):
    rec = np.array([0, cnt, n_local, strategy | init << 8], dtype=np.uint32)
    pool = np.arange(100, 100 + max(cnt, 1), dtype=np.uint32)
    topic = np.arange(n_entries, dtype=np.uint32)
    value = np.zeros(n_entries, dtype=np.uint32)
    doff = np.array([0, n_entries, n_entries], dtype=np.uint64)
    kc = kt = keys
    member, head, after = pick_batch_ref(1, doff, topic, value, n_entries, [0], rec, pool, [c0], kc, kt,
                                         0 if keys is None else len(keys), seed)
    return member, head, int(after[0])


@pytest.mark.parametrize("cnt", [0, 1, 2, 3, 64])
def test_counts_and_the_singleton_rule(cnt):
    for strategy in range(7):
        for c0 in (UNDEF, 0, 5, 0xFFFFFFFE):
            member, head, after = _one_slot(cnt, strategy, c0, 9)
            if cnt == 0:
                assert (member == NONE).all() and head == (9, 0) and after == c0
            elif cnt == 1:
                # pick_subscriber(.., [Sub]) -> Sub: no strategy code runs, no state changes
                assert (member == 100).all() and head == (9, 9)
                assert after == (0 if strategy == shared_sub.STICKY else c0)
            else:
                assert ((member >= 100) & (member < 100 + cnt)).all() and head == (9, 9)
    member, head, after = _one_slot(3, 7, 0, 4)                 # an unknown strategy byte
    assert (member == NONE).all() and head == (4, 0) and after == 0


def test_round_robins_step_by_step():
    # round_robin: Rem = (N + 1) rem Count, Nth = Rem + 1
    member, _, after = _one_slot(3, shared_sub.ROUND_ROBIN, 0, 5)
    assert member.tolist() == [101, 102, 100, 101, 102] and after == 2
    # a list that shrank below its counter: (N + 1) rem Count all the same
    member, _, after = _one_slot(3, shared_sub.ROUND_ROBIN, 7, 2)
    assert member.tolist() == [102, 100] and after == 0
    member, _, after = _one_slot(2, shared_sub.ROUND_ROBIN, 0xFFFFFFFE, 2)    # 64-bit sums
    assert member.tolist() == [100 + 0xFFFFFFFF % 2, 100 + 0x100000000 % 2] and after == 0
    # undefined: a start drawn from [0, Count), then round robin
    member, _, after = _one_slot(64, shared_sub.ROUND_ROBIN, UNDEF, 3)
    first = shared_sub.mix(7, NONE, 0) % 64
    assert member.tolist() == [100 + (first + k) % 64 for k in range(3)] and after == (first + 2) % 64
    # round_robin_per_group: the counter lives in [0, Count]; c <- c + 1, 1 past Count; a missing one starts at 0
    for c0, want, end in ((0, [100, 101, 102, 100], 1), (UNDEF, [100, 101, 102, 100], 1), (2, [102, 100, 101, 102], 3),
                          (3, [100, 101, 102, 100], 1), (8, [100, 101, 102, 100], 1)):
        member, _, after = _one_slot(3, shared_sub.ROUND_ROBIN_PER_GROUP, c0, 4)
        assert member.tolist() == want and after == end, c0


def test_counter_reset_on_subscribe_and_delete_on_last_unsubscribe():
    dev = DeviceModel()
    subs = SharedSubs(node="n1", on_change=dev.on_change, default_strategy="round_robin_per_group")
    a, b, c = ("n1", 1), ("n1", 2), ("n2", 3)
    subs.subscribe(b"g", b"t", a)
    subs.subscribe(b"g", b"t", b)
    s = subs.slot(b"g", b"t")
    assert dev.state[s] == 0
    dev.state[s] = 2                                             # the device picked twice
    subs.subscribe(b"g", b"t", c)                                # a remote member: no ets:insert here
    assert dev.state[s] == 2
    subs.subscribe(b"g", b"t", ("n1", 4))                        # a local one: {GT, 0} is inserted again
    assert dev.state[s] == 0 and subs.rr_counter[(b"g", b"t")] == 0
    for p in (a, b):
        subs.unsubscribe(b"g", b"t", p)
    assert (b"g", b"t") in subs.rr_counter
    subs.unsubscribe(b"g", b"t", ("n1", 4))                      # the last local one: the counter is deleted
    assert (b"g", b"t") not in subs.rr_counter and dev.state[s] == UNDEF
    assert subs.subscribers(b"g", b"t") == [c]


@pytest.mark.parametrize("strategy", [shared_sub.RANDOM, shared_sub.LOCAL])
def test_random_and_local_stay_inside_their_lists(strategy):
    for cnt, n_local in ((2, 0), (3, 1), (64, 2), (64, 17), (5, 9)):
        member, head, after = _one_slot(cnt, strategy, 3, 500, n_local=n_local, seed=99)
        again, _, _ = _one_slot(cnt, strategy, 3, 500, n_local=n_local, seed=99)
        other, _, _ = _one_slot(cnt, strategy, 3, 500, n_local=n_local, seed=100)
        assert np.array_equal(member, again) and after == 3 and head == (500, 500)
        hi = cnt if strategy == shared_sub.RANDOM or n_local == 0 else min(n_local, cnt)
        assert ((member >= 100) & (member < 100 + hi)).all()
        if hi > 1:
            assert not np.array_equal(member, other)
            assert len(set(member.tolist())) == min(hi, len(set(member.tolist())))
            assert len(set(member.tolist())) > 1
