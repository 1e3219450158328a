"""Tab.route_kids32 / dispatch_kids32 / publish_kids32 without a device: the
pooled buffer sets and the retry policy on TM_ECAP, against a stand-in index
(Tab(index=fake)) whose three 32-bit calls fill the outputs from a scripted
result and raise TmError(TM_ECAP), offsets and head filled in, when the arrays
they are given are short.

The policy: the entry arrays grow from dest_offsets[n_dests + 1], the delivery
arrays from head[1], one retry; a publish whose deliveries alone were short
keeps its route outputs and its picks (the state has moved) and fetches only
the dispatch again, through dispatch_batch32.
"""
import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.topic_index import ROUTE_POOL_SETS, Tab

TOPICS = [b"a/b", b"c"]
N, N_DESTS, LOCAL = 2, 2, 1
FIRST = 1024 + 1024 // 4   # entries / deliveries a fresh set has room for: max(4 n, 1024) and a quarter


class FakeIndex:
    """host_array / host_free on plain numpy, and the three calls.  The result: E entries over
    the buckets (topic q % 2, value 7 q), T deliveries (topic k % 2, value 3 k, subscriber k + 1),
    err flags (0, 1); a publish that has room for the entries picks member 1000 state + q for
    entry q and moves the state word."""

    def __init__(self, E, T, grow=0):
        self.E, self.T, self.grow = E, T, grow   # grow: the totals rise by that much with every call
        self.state = 0
        self.calls = []                          # (name, cap, dcap) per library call
        self.live = {}                           # id -> array handed out and not freed
        self.allocs = self.frees = 0

    def host_array(self, n, dtype, vram=False):
        a = np.zeros(max(int(n), 1), dtype)
        self.live[id(a)] = a
        self.allocs += 1
        return a

    def host_free(self, a):
        assert id(a) in self.live, "freed twice, or never handed out"
        del self.live[id(a)]
        self.frees += 1

    def _inputs(self, blob, offs, out, n_dests):
        blob0, offs0 = _native.pack_strings(TOPICS)
        assert offs.dtype == np.uint32 and np.array_equal(offs, offs0)
        assert np.array_equal(blob[:int(offs0[-1])], blob0[:int(offs0[-1])]) and n_dests == N_DESTS
        assert all(id(a) in self.live for a in out), "every output comes from host_array"

    def _route(self, out, cap):
        doff, topic, vals, err = out[:4]
        E = self.E
        doff[:N_DESTS + 2] = (0, E // 3, E // 2, E)
        k = min(E, cap)
        topic[:k], vals[:k] = np.arange(k) % 2, 7 * np.arange(k)
        err[:N] = (0, 1)
        return E > cap

    def _dispatch(self, out, dcap):
        head, dt, dv, ds = out[4:]
        T = self.T
        head[:2] = (self.E // 2 - self.E // 3, T)
        k = min(T, dcap)
        dt[:k], dv[:k], ds[:k] = np.arange(k) % 2, 3 * np.arange(k), np.arange(k) + 1
        return T > dcap

    def _done(self, short):
        self.E, self.T = self.E + self.grow, self.T + self.grow
        if short:
            raise _native.TmError(_native.TM_ECAP, "scripted: does not fit")

    def route_batch32(self, blob, offs, n_dests, out, cap=None, aggre=False):
        self._inputs(blob, offs, out, n_dests)
        cap = min(len(out[1]), len(out[2]))
        self.calls.append(("route", cap, None))
        E = self.E
        self._done(self._route(out, cap))
        return out[0][:N_DESTS + 2], out[1][:E], out[2][:E], out[3][:N]

    def dispatch_batch32(self, blob, offs, n_dests, local_dest, out, cap=None, dcap=None, aggre=False):
        self._inputs(blob, offs, out, n_dests)
        assert local_dest == LOCAL
        cap, dcap = min(len(out[1]), len(out[2])), min(len(a) for a in out[5:])
        self.calls.append(("dispatch", cap, dcap))
        short = self._route(out, cap)
        E, T = self.E, self.T
        self._done(self._dispatch(out, dcap) or short)
        return (out[0][:N_DESTS + 2], out[1][:E], out[2][:E], out[3][:N]), tuple(a[:T] for a in out[5:])

    def publish_batch32(self, blob, offs, n_dests, local_dest, out, member, key_clientid=None, key_topic=None,
                        seed=0, cap=None, dcap=None):
        self._inputs(blob, offs, out + (member,), n_dests)
        assert local_dest == LOCAL
        self.keys = tuple(None if k is None else k[:N].tolist() for k in (key_clientid, key_topic)) + (seed,)
        assert all(k is None or id(k.base if k.base is not None else k) in self.live for k in (key_clientid, key_topic))
        cap, dcap = min(len(out[1]), len(out[2]), len(member)), min(len(a) for a in out[5:])
        self.calls.append(("publish", cap, dcap))
        short = self._route(out, cap)
        E, T = self.E, self.T
        if not short:
            member[:E] = 1000 * self.state + np.arange(E)
            self.state += 1
        self._done(self._dispatch(out, dcap) or short)
        return (out[0][:N_DESTS + 2], out[1][:E], out[2][:E], out[3][:N]), tuple(a[:T] for a in out[5:]), member[:E]


def _route_exp(E):
    q = np.arange(E)
    return np.array([0, E // 3, E // 2, E], np.uint64), (q % 2).astype(np.uint32), (7 * q).astype(np.uint32), \
        np.array([0, 1], np.uint8)


def _dl_exp(T):
    k = np.arange(T)
    return (k % 2).astype(np.uint32), (3 * k).astype(np.uint32), (k + 1).astype(np.uint32)


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and np.array_equal(g, e)


def _pool_holds_everything(tab, fake):
    """what host_array handed out is freed or in an idle set; the results are copies"""
    assert len(tab._route_pool) <= ROUTE_POOL_SETS
    pooled = {id(a) for s in tab._route_pool for a in s.values()}
    assert pooled == set(fake.live) and fake.allocs - fake.frees == len(fake.live)


def _call(tab, kind, **kw):
    if kind == "route":
        return (tab.route_kids32(TOPICS, N_DESTS),)
    if kind == "dispatch":
        return tab.dispatch_kids32(TOPICS, N_DESTS, LOCAL)
    return tab.publish_kids32(TOPICS, N_DESTS, LOCAL, **kw)


def _grown(x):
    return x + x // 4


SHORT = {"fits": (10, 20), "entries": (3000, 20), "deliveries": (10, 5000), "both": (3000, 5000)}


@pytest.mark.parametrize("kind", ["route", "dispatch"])
@pytest.mark.parametrize("case", list(SHORT))
def test_route_and_dispatch_retry_once_from_the_offsets_and_the_head(kind, case):
    E, T = SHORT[case]
    fake = FakeIndex(E, T)
    tab = Tab(index=fake)
    res = _call(tab, kind)
    _same(res[0], _route_exp(E))
    if kind == "dispatch":
        _same(res[1], _dl_exp(T))
    assert not any(id(a) in fake.live for part in res for a in part), "copies, not the pooled buffers"
    cap1 = _grown(E) if E > FIRST else FIRST
    dcap1 = _grown(T) if T > FIRST else FIRST
    if kind == "route":
        exp = [("route", FIRST, None)] + ([("route", cap1, None)] if E > FIRST else [])
        sets = 6
    else:
        exp = [("dispatch", FIRST, FIRST)] + ([("dispatch", cap1, dcap1)] if E > FIRST or T > FIRST else [])
        sets = 10
    assert fake.calls == exp
    grown = (2 if E > FIRST else 0) + (3 if kind == "dispatch" and T > FIRST else 0)
    assert (fake.allocs, fake.frees) == (sets + grown, grown), "only the arrays that were short are replaced"
    _pool_holds_everything(tab, fake)
    # the set is reused as it stands: one call, nothing allocated
    a0 = fake.allocs
    fake.calls.clear()
    _same(_call(tab, kind)[0], _route_exp(E))
    assert len(fake.calls) == 1 and fake.allocs == a0 and len(tab._route_pool) == 1
    _pool_holds_everything(tab, fake)


@pytest.mark.parametrize("case", list(SHORT))
def test_publish_keeps_the_picks_when_the_deliveries_alone_were_short(case):
    E, T = SHORT[case]
    fake = FakeIndex(E, T)
    tab = Tab(index=fake)
    route, dl, member = tab.publish_kids32(TOPICS, N_DESTS, LOCAL, key_clientid=[5, 6, 99], key_topic=None, seed=9)
    _same(route, _route_exp(E))
    _same(dl, _dl_exp(T))
    # the state word has moved once, and the members are those of the call that picked (state 0)
    assert fake.state == 1 and member.dtype == np.uint32 and np.array_equal(member, np.arange(E))
    assert fake.keys == ([5, 6], None, 9)
    cap1 = _grown(E) if E > FIRST else FIRST
    dcap1 = _grown(T) if T > FIRST else FIRST
    exp = [("publish", FIRST, FIRST)]
    if E > FIRST:
        exp.append(("publish", cap1, dcap1))       # no pick was made: the call once more
    elif T > FIRST:
        exp.append(("dispatch", cap1, dcap1))      # the picks stand: only the dispatch again
    assert fake.calls == exp
    grown = (3 if E > FIRST else 0) + (3 if T > FIRST else 0)
    assert (fake.allocs, fake.frees) == (13 + grown, grown)
    assert not any(id(a) in fake.live for a in route + dl + (member,))
    _pool_holds_everything(tab, fake)


@pytest.mark.parametrize("kind", ["route", "dispatch", "publish"])
def test_a_second_ecap_propagates(kind):
    fake = FakeIndex(3000, 5000, grow=4000)   # the retry's arrays are short again
    tab = Tab(index=fake)
    with pytest.raises(_native.TmError) as e:
        _call(tab, kind)
    assert e.value.code == _native.TM_ECAP and len(fake.calls) == 2 and fake.state == 0
    _pool_holds_everything(tab, fake)


def test_a_second_ecap_of_the_dispatch_after_a_publish_propagates():
    fake = FakeIndex(10, 5000, grow=4000)
    tab = Tab(index=fake)
    with pytest.raises(_native.TmError) as e:
        _call(tab, "publish")
    assert e.value.code == _native.TM_ECAP and fake.state == 1
    assert [c[0] for c in fake.calls] == ["publish", "dispatch"]
    _pool_holds_everything(tab, fake)


def test_another_error_is_not_retried():
    fake = FakeIndex(10, 20)
    tab = Tab(index=fake)

    def fails(*a, **k):
        fake.calls.append(("route", 0, None))
        raise _native.DeviceError(_native.TM_EDEVICE, "scripted")
    fake.route_batch32 = fails
    with pytest.raises(_native.DeviceError):
        tab.route_kids32(TOPICS, N_DESTS)
    assert len(fake.calls) == 1
    _pool_holds_everything(tab, fake)


@pytest.mark.parametrize("keys", [{"key_clientid": [1]}, {"key_topic": [1]}, {"key_clientid": [1, 2], "key_topic": []}])
def test_a_key_array_shorter_than_the_batch_is_a_value_error(keys):
    fake = FakeIndex(10, 20)
    tab = Tab(index=fake)
    with pytest.raises(ValueError):
        tab.publish_kids32(TOPICS, N_DESTS, LOCAL, **keys)
    assert fake.calls == [] and fake.state == 0
    _pool_holds_everything(tab, fake)


def test_idle_sets_beyond_the_pool_are_freed():
    """callers that overlap each take a set; at most ROUTE_POOL_SETS stay, the others are freed"""
    fake = FakeIndex(10, 20)
    tab = Tab(index=fake)
    sets = [tab._route_set(N, 4, N_DESTS, 1024) for _ in range(ROUTE_POOL_SETS + 2)]
    for s in sets:
        tab._route_put(s)
    assert len(tab._route_pool) == ROUTE_POOL_SETS and fake.frees == 2 * 6
    _pool_holds_everything(tab, fake)
