"""tm_publish_deliver_batch32: the 32-bit, in-place route + local dispatch +
shared-subscription pick + merge and grouping by subscriber for a NIF's
micro-batches.

Two references.  The unchanged tm_publish_deliver_batch on the same index,
topics, caps, keys and seed, run from the same start state of the slots: the
return code, the bucket offsets, both heads and every output array -- each
filled with a canary first and compared WHOLE, tail included, so a word written
past min(total, cap), K, min(N, dcap), min(G, gcap) or out_goff[min(G, gcap)]
fails the comparison; out_goff and the bucket offsets are compared after
narrowing -- and the state words afterwards.  And the numpy definition
(tests/group_picks_ref.py) applied to tm_publish_batch32's output of the same
batch from the same start state.  The inputs are compared after every run, and
TM_DEBUG_PUBLISH_DELIVER_ONE / _GRID say which ending finished the call: the
one workgroup (k_pd_gate, k_sh_one, k_gp_one), or the grid kernels / the staged
path.

Two indexes.  test_gpu_publish_deliver_batch.py's world (76 wildcard filters,
400 members, about half of them local).  And a synthetic one in which the sizes
are chosen word by word: '$p/+', '$q/+' and '$s/+' deliver three subscriber
lists of any length (T), '$g<i>/+' is one entry with its own slot of one member
(a pick each; sub_of says which of them are local and whose), '$m<j>/+' and
'$m<j>/#' give one subscriber a direct and a picked delivery of the same
message.  k_gp_one gives each of its 16 waves ceil(N / 16) codes rounded up to
64: N = 1,024 fills every wave's first step exactly, 1,025 takes a second;
8,192 merged deliveries (T + K) is the compiled bound.
"""
import threading
from collections import Counter

import numpy as np
import pytest

from emqx_amd import _native, shared_sub
from emqx_amd.shared_sub import NONE, UNDEF
from group_picks_ref import group_picks_ref

pytestmark = pytest.mark.gpu

FO1_TOPICS, FO1_ENTRIES, GP1_DELIVERIES = 8192, 16384, _native.GP1_DELIVERIES   # emqx_amd/csrc/tm_dev.h
CANARY, OFFC, ERRC, HEADC, TAIL = 0xC0FFEE55, 0xDEADBEEF, 0xEE, 0xABCDEF0123456789, 64
ONE, GRID = _native.TM_DEBUG_PUBLISH_DELIVER_ONE, _native.TM_DEBUG_PUBLISH_DELIVER_GRID
GP1_MAX, GS1_MAX, DP1_MAX = _native.TM_DEBUG_GP1_MAX, _native.TM_DEBUG_GS1_MAX, _native.TM_DEBUG_DP1_MAX
RUN, SKIPPED = _native.TM_DEBUG_GROUP_PASSES_RUN, _native.TM_DEBUG_GROUP_PASSES_SKIPPED
AGGRE = _native.TM_ROUTE_AGGRE
OK, ECAP, EINVAL = _native.TM_OK, _native.TM_ECAP, _native.TM_EINVAL
P = _native._ptr
SEED = 0x5EED
NAMES = ("rc", "bucket offsets", "topic", "values", "member", "head", "dtopic", "dvalue", "dsub", "ghead", "gsub", "goff",
         "err")
RR, PG, STICKY = shared_sub.ROUND_ROBIN, shared_sub.ROUND_ROBIN_PER_GROUP, shared_sub.STICKY


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, max(n, 1), dtype=np.uint32), rng.integers(0, 1 << 32, max(n, 1), dtype=np.uint32)


# ---- the reference and the call under test, both on canary-filled outputs

def _reference(ix, topics, n_dests, local, cap, dcap, gcap, kc, kt, seed=SEED):
    """tm_publish_deliver_batch -> NAMES' tuple, the arrays whole (doff and goff u64)"""
    blob, offs = _native.pack_strings(topics)
    n = len(topics)
    doff, head, ghead = np.zeros(n_dests + 2, np.uint64), np.full(2, HEADC, np.uint64), np.full(2, HEADC, np.uint64)
    t, v, m = (np.full(cap + TAIL, CANARY, np.uint32) for _ in range(3))
    dt, dv, ds = (np.full(dcap + TAIL, CANARY, np.uint32) for _ in range(3))
    gsub, goff = np.full(gcap + TAIL, CANARY, np.uint32), np.full(gcap + 1 + TAIL, OFFC, np.uint64)
    err = np.zeros(max(n, 1), np.uint8)
    rc = ix._lib.tm_publish_deliver_batch(ix._h, n, P(blob), P(offs), n_dests, local, AGGRE, P(doff), P(t), P(v), cap,
                                          P(head), P(dt), P(dv), P(ds), dcap, P(kc), P(kt), seed, P(m), P(ghead), P(gsub),
                                          P(goff), gcap, P(err))
    assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
    return rc, doff, t, v, m, head, dt, dv, ds, ghead, gsub, goff, err[:n]


class Bufs:
    """one caller's batch buffers: host_array (pinned; the inputs and keys optionally TM_ALLOC_VRAM), those in
    `plain` numpy; x*: a second set for the tm_publish_batch32 / tm_deliver_batch32 call of the same batch"""

    def __init__(self, ix, nmax, bytes_max, dmax, cap_max, dcap_max, gcap_max=None, vram_inputs=False, plain=()):
        def alloc(name, k, dt, vram=False):
            if name in plain:
                return np.zeros(max(k, 1), dt)
            a = ix.host_array(k, dt, vram=vram)
            self.owned.append(a)
            return a
        gcap_max = dcap_max if gcap_max is None else gcap_max
        self.ix, self.cap_max, self.dcap_max, self.gcap_max, self.owned = ix, cap_max, dcap_max, gcap_max, []
        self.vram_inputs = vram_inputs
        self.blob = alloc("blob", bytes_max + 48, np.uint8, vram_inputs)
        self.offs = alloc("offs", nmax + 1, np.uint32, vram_inputs)
        self.kc, self.kt = (alloc(k, nmax + 1, np.uint32, vram_inputs) for k in ("kc", "kt"))
        self.doff, self.err = alloc("doff", dmax + 2 + TAIL, np.uint32), alloc("err", nmax + TAIL, np.uint8)
        self.topic, self.vals, self.member = (alloc(k, cap_max + TAIL, np.uint32) for k in ("topic", "vals", "member"))
        self.xmember = alloc("xmember", cap_max + TAIL, np.uint32)
        self.head, self.ghead, self.xhead, self.xghead = (alloc(k, 2, np.uint64) for k in ("head", "ghead", "xhead", "xghead"))
        self.dt, self.dv, self.ds = (alloc(k, dcap_max + TAIL, np.uint32) for k in ("dt", "dv", "ds"))
        self.xdt, self.xdv, self.xds = (alloc(k, dcap_max + TAIL, np.uint32) for k in ("xdt", "xdv", "xds"))
        self.gsub, self.goff = alloc("gsub", gcap_max + TAIL, np.uint32), alloc("goff", gcap_max + 1 + TAIL, np.uint32)
        self.xgsub, self.xgoff = alloc("xgsub", gcap_max + TAIL, np.uint32), alloc("xgoff", gcap_max + 1 + TAIL, np.uint32)

    def free(self):
        for a in self.owned:
            self.ix.host_free(a)

    def _load(self, topics, kc, kt, shift=0):
        blob, offs = _native.pack_strings(topics)
        n, nb = len(topics), int(offs[-1])
        assert n + 1 <= len(self.offs) and nb + shift <= len(self.blob)
        self.blob[shift:shift + nb] = blob[:nb]
        self.offs[:n + 1] = offs
        self.doff[:], self.topic[:], self.vals[:], self.err[:] = OFFC, CANARY, CANARY, ERRC
        keys = []
        for mine, k in ((self.kc, kc), (self.kt, kt)):
            if k is not None:
                mine[:n] = k[:n]
            keys.append(None if k is None else mine)
        return blob, offs, n, nb, keys

    def publish32(self, topics, n_dests, local, cap, dcap, kc, kt, seed=SEED):
        """tm_publish_batch32 of the same batch -> (rc, doff, topic, values, member, head, dtopic, dvalue, dsub)"""
        _, _, n, _, keys = self._load(topics, kc, kt)
        ix = self.ix
        rc = ix._lib.tm_publish_batch32(ix._h, n, P(self.blob), P(self.offs), n_dests, local, AGGRE, P(self.doff),
                                        P(self.topic), P(self.vals), cap, P(self.xhead), P(self.xdt), P(self.xdv),
                                        P(self.xds), dcap, P(keys[0]), P(keys[1]), seed, P(self.xmember), P(self.err))
        assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
        K, w = min(int(self.doff[n_dests + 1]), cap), min(int(self.xhead[1]), dcap)
        return rc, self.doff[:n_dests + 2].copy(), self.topic[:K].copy(), self.vals[:K].copy(), self.xmember[:K].copy(), \
            self.xhead.copy(), self.xdt[:w].copy(), self.xdv[:w].copy(), self.xds[:w].copy()

    def deliver32(self, topics, n_dests, local, cap, dcap, gcap):
        """tm_deliver_batch32 of the same batch (aggre) -> (rc, head, dtopic, dvalue, dsub, ghead, gsub, goff), whole"""
        _, _, n, _, _ = self._load(topics, None, None)
        self.xdt[:], self.xdv[:], self.xds[:], self.xgsub[:], self.xgoff[:] = CANARY, CANARY, CANARY, CANARY, OFFC
        ix = self.ix
        rc = ix._lib.tm_deliver_batch32(ix._h, n, P(self.blob), P(self.offs), n_dests, local, AGGRE, P(self.doff),
                                        P(self.topic), P(self.vals), cap, P(self.xhead), P(self.xdt), P(self.xdv),
                                        P(self.xds), dcap, P(self.xghead), P(self.xgsub), P(self.xgoff), gcap, P(self.err))
        assert rc in (OK, ECAP), ix._lib.tm_last_error(ix._h)
        return rc, self.xhead.copy(), self.xdt[:dcap + TAIL].copy(), self.xdv[:dcap + TAIL].copy(), \
            self.xds[:dcap + TAIL].copy(), self.xghead.copy(), self.xgsub[:gcap + TAIL].copy(), \
            self.xgoff[:gcap + 1 + TAIL].copy()

    def call(self, topics, n_dests, local, cap, dcap, gcap, kc, kt, seed=SEED, shift=0, flags=AGGRE, ok=(OK, ECAP)):
        """tm_publish_deliver_batch32 -> what _reference returns (doff and goff as u32), arrays whole up to cap + TAIL"""
        assert cap <= self.cap_max and dcap <= self.dcap_max and gcap <= self.gcap_max
        blob, offs, n, nb, keys = self._load(topics, kc, kt, shift)
        self.member[:], self.dt[:], self.dv[:], self.ds[:] = CANARY, CANARY, CANARY, CANARY
        self.head[:], self.ghead[:], self.gsub[:], self.goff[:] = HEADC, HEADC, CANARY, OFFC
        ix = self.ix
        rc = ix._lib.tm_publish_deliver_batch32(ix._h, n, P(self.blob[shift:]), P(self.offs), n_dests, local, flags,
                                                P(self.doff), P(self.topic), P(self.vals), cap, P(self.head), P(self.dt),
                                                P(self.dv), P(self.ds), dcap, P(keys[0]), P(keys[1]), seed, P(self.member),
                                                P(self.ghead), P(self.gsub), P(self.goff), gcap, P(self.err))
        assert rc in ok, ix._lib.tm_last_error(ix._h)
        if not self.vram_inputs:   # (device memory is never read back by the host)
            assert np.array_equal(self.blob[shift:shift + nb], blob[:nb]) and np.array_equal(self.offs[:n + 1], offs), \
                "the inputs changed"
            assert all(k is None or np.array_equal(mine[:n], k[:n]) for mine, k in ((self.kc, kc), (self.kt, kt)))
        if rc in (OK, ECAP):
            assert (self.doff[n_dests + 2:] == OFFC).all(), "offsets: canary"
            assert (self.err[n:] == ERRC).all(), "err: canary"
            for a, c in ((self.topic, cap), (self.vals, cap), (self.member, cap), (self.dt, dcap), (self.dv, dcap),
                         (self.ds, dcap), (self.gsub, gcap)):
                assert (a[c:] == CANARY).all(), "written past the capacity"
            assert (self.goff[gcap + 1:] == OFFC).all(), "written past out_goff[gcap]"
        c = lambda a, k: a[:k + TAIL].copy()
        return rc, self.doff[:n_dests + 2].copy(), c(self.topic, cap), c(self.vals, cap), c(self.member, cap), \
            self.head.copy(), c(self.dt, dcap), c(self.dv, dcap), c(self.ds, dcap), self.ghead.copy(), c(self.gsub, gcap), \
            c(self.goff, gcap + 1), self.err[:n].copy()


def _same(got, ref):
    for name, g, r in zip(NAMES, got, ref):
        if name == "rc":
            assert g == r, f"return code {g}, tm_publish_deliver_batch's {r}"
        elif name == "goff":   # narrowed: the written part equal, the canary tails each whole
            written = np.nonzero(r != OFFC)[0]
            k = int(written[-1]) + 1 if len(written) else 0
            assert np.array_equal(g[:k].astype(np.uint64), r[:k]) and (r[:k] < 1 << 32).all(), name
            assert (g[k:] == OFFC).all() and len(g) == len(r), "past out_goff[min(G, gcap)]"
        else:
            assert np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(r).astype(np.uint64)), name


class Env:
    """an index with the slots a case's picks may move and the member-subs table it holds"""

    def __init__(self, ix, n_dests, local, slots, sub_of):
        self.ix, self.n_dests, self.local = ix, n_dests, local
        self.slots, self.sub_of = np.asarray(slots, np.uint32), np.asarray(sub_of, np.uint32)

    def reset(self, words=None):
        if len(self.slots):
            self.ix.share_state_set(self.slots, np.full(len(self.slots), UNDEF, np.uint32) if words is None else words)

    def state(self):
        return self.ix.share_state_get(self.slots) if len(self.slots) else np.zeros(0, np.uint32)


def _check(env, b, topics, leg, cap=None, dcap=None, gcap=None, keys=True, seed=SEED, shift=0, definition=True, start=None):
    """the reference from the start state, the definition over tm_publish_batch32's output from the same start
    state, then the call under test from the same start state: every output, the state afterwards and the
    ending's counter (leg: ONE or GRID must rise by one, the other stay put).  -> a dict of the figures"""
    ix, n = env.ix, len(topics)
    cap = b.cap_max if cap is None else cap
    dcap = b.dcap_max if dcap is None else dcap
    gcap = b.gcap_max if gcap is None else gcap
    kc, kt = _keys(n, seed) if keys else (None, None)
    env.reset(start)
    before = env.state()
    ref = _reference(ix, topics, env.n_dests, env.local, cap, dcap, gcap, kc, kt, seed)
    ref_state = env.state()
    env.reset(start)
    c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
    got = b.call(topics, env.n_dests, env.local, cap, dcap, gcap, kc, kt, seed, shift)
    c1 = (ix.debug_get(ONE), ix.debug_get(GRID))
    state = env.state()
    _same(got, ref)
    assert np.array_equal(state, ref_state), "the state words afterwards"
    assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if leg == ONE else (0, 1)), "which ending finished the call"
    rc, doff, t, v, m, head, dt, dv, ds, ghead, gsub, goff = got[:12]
    total, T, G, N = int(doff[-1]), int(head[1]), int(ghead[0]), int(ghead[1])
    out = dict(rc=rc, total=total, T=T, G=G, N=N, moved=not np.array_equal(state, before), got=got)
    if total > cap or T + total > dcap:   # (under total > cap the un-aggregated total: the staged call's ECAP all the same)
        assert rc == ECAP and (G, N) == (0, 0) and not out["moved"], "a call to repeat moved something"
        for a in (m, dt, dv, ds, gsub):
            assert (a == CANARY).all(), "a call to repeat wrote a delivery, a pick or a group"
        assert (goff == OFFC).all()
        return out
    K = total
    assert rc == (ECAP if G > gcap else OK) and T <= N <= T + K and G <= N
    assert (m[K:] == CANARY).all() and (dt[N:] == CANARY).all() and (gsub[min(G, gcap):] == CANARY).all()
    if definition:
        env.reset(start)
        xrc, xdoff, xt, xv, xm, xhead, xdt, xdv, xds = b.publish32(topics, env.n_dests, env.local, cap, dcap, kc, kt, seed)
        assert xrc == OK and np.array_equal(env.state(), ref_state) and np.array_equal(xm, m[:K])
        (eG, eN), et, ev, es, _, egs, ego, W, Pn = group_picks_ref([0, T], xdt, xdv, xds, T, env.n_dests, xdoff, xt, xv, xm,
                                                                   K, env.sub_of, T + K, gcap)
        assert (G, N) == (eG, eN), "the definition's [G, N]"
        assert np.array_equal(dt[:N], et) and np.array_equal(dv[:N], ev) and np.array_equal(ds[:N], es), "the definition"
        assert np.array_equal(gsub[:len(egs)], egs) and np.array_equal(goff[:len(ego)].astype(np.uint64), ego)
        out["P"] = Pn
    return out


# ---- 1. the synthetic index

S_DESTS, NG, NM = 3, 700, 4
G_VAL, MD_VAL, MP_VAL = 100, 5000, 6000     # values of '$g<i>/+', '$m<j>/+' (direct) and '$m<j>/#' (picked)
G_MEMBER, M_MEMBER = 1000, 2000             # member ids of slot i / of the tie slots NG + j


class Synth:
    def __init__(self):
        self.ix = ix = _native.Index()
        fs = [b"$p/+", b"$q/+", b"$r/+", b"$s/+"] + [b"$g%d/+" % i for i in range(NG)]
        fs += [b"$m%d/+" % j for j in range(NM)] + [b"$m%d/#" % j for j in range(NM)]
        vals = [0, 1, 2, 3] + [G_VAL + i for i in range(NG)] + [MD_VAL + j for j in range(NM)] + [MP_VAL + j for j in range(NM)]
        dests = [0, 0, 1, 0] + [1 + i % 2 for i in range(NG)] + [0] * NM + [1] * NM
        vals = np.asarray(vals, np.uint32)
        ix.set_dests(vals, np.asarray(dests, np.uint32))
        ix.set_route_filters(vals, vals)                           # every filter its own id: aggre/1 keeps everything
        blob, offs = _native.pack_strings(fs)
        ix.apply(np.ones(len(fs), np.uint8), blob, offs, vals)
        ix.set_subscribers([2], [[9, 8, 7]])
        slots = list(range(NG + NM))
        ix.set_share_slots([G_VAL + i for i in range(NG)] + [MP_VAL + j for j in range(NM)], slots)
        ix.set_share_members(slots, [[G_MEMBER + i] for i in range(NG)] + [[M_MEMBER + j] for j in range(NM)],
                             [0] * len(slots), [(RR, PG, STICKY | 5 << 8)[s % 3] for s in slots])
        self.env = Env(ix, S_DESTS, 0, slots, np.full(M_MEMBER + NM, NONE, np.uint32))
        self.b = Bufs(ix, 1200, 1200 * 10, 16, 2000, 9000)
        self.member_subs({})

    def member_subs(self, sub_of):
        """{member: local subscriber id}; every other member is remote"""
        tab = np.full(M_MEMBER + NM, NONE, np.uint32)
        for m, s in sub_of.items():
            tab[m] = s
        self.ix.set_member_subs(np.arange(len(tab), dtype=np.uint32), tab)
        self.env.sub_of = tab

    def batch(self, ids, picks, ties=0):
        """the direct deliveries' subscribers are `ids` (three lists, the middle one the longest), `picks`
        entries '$g<i>/x' spread around them, `ties` topics '$m<j>/x' -> the topics"""
        ids = np.asarray(ids, np.uint32)
        a = len(ids) // 5
        self.ix.set_subscribers([0, 1, 3], [ids[:a], ids[a:len(ids) - a], ids[len(ids) - a:]])
        g = [b"$g%d/x" % i for i in range(picks)]
        h = picks // 2
        return g[:h:2] + [b"$p/x"] + g[1:h:2] + [b"$m%d/x" % j for j in range(ties)] + [b"$q/x", b"$r/x", b"none"] + g[h:] \
            + [b"$s/x"]


@pytest.fixture(scope="module")
def synth(gpu):
    s = Synth()
    yield s
    s.b.free()
    s.ix.close()


def _random_ids(W, bound, seed):
    return np.random.default_rng(seed).integers(0, bound, W, dtype=np.uint64).astype(np.uint32)


def _digits_that_differ(x, digits=4):
    x = np.asarray(x, np.uint32)
    return sum(len(np.unique((x >> (8 * p)) & 255)) > 1 for p in range(digits)) if len(x) else 0


def _sized(synth, N, local_every=1, bound=1 << 16, seed=0):
    """a batch of N = T + P merged deliveries: P = N // 3 picks '$g<i>/x', every local_every-th of them local
    (the others remote: K > P) -- onto the direct deliveries' subscribers and onto ids of their own"""
    Pn = N // 3
    T = N - Pn
    ids = _random_ids(T, bound, N + seed)
    picks = Pn * local_every
    assert picks <= NG
    rng = np.random.default_rng(N + 1 + seed)
    own = _random_ids(Pn, bound, N + 2 + seed)
    synth.member_subs({G_MEMBER + i * local_every: int(ids[rng.integers(0, T)]) if T and i % 2 else int(own[i])
                       for i in range(Pn)})
    return synth.batch(ids, picks), T, Pn, picks


def _check_passes(synth, topics, leg, **kw):
    """_check, and the pass counters' deltas around the call under test alone against the rule: the picks'
    messages are sorted on their two low digits, the merged subscriber ids on four, a digit all agree on
    skipped; four passes are accounted for per sort"""
    ix = synth.ix
    out = _check(synth.env, synth.b, topics, leg, **kw)
    if leg != ONE or out["rc"] == ECAP and out["N"] == 0:
        return out
    # (the counters are read around one more call from the same start state: _check's own bracket holds
    # the reference's passes too)
    synth.env.reset()
    kc, kt = _keys(len(topics), SEED)
    p0 = (ix.debug_get(RUN), ix.debug_get(SKIPPED))
    got = synth.b.call(topics, S_DESTS, 0, kw.get("cap", synth.b.cap_max), kw.get("dcap", synth.b.dcap_max),
                       kw.get("gcap", synth.b.gcap_max), kc, kt)
    p1 = (ix.debug_get(RUN), ix.debug_get(SKIPPED))
    _same(got, out["got"])
    K, N = out["total"], out["N"]
    member, et = got[4][:K], got[2][:K]
    local = env_local(synth.env.sub_of, member)
    run = _digits_that_differ(et[local], 2) + _digits_that_differ(got[8][:N])
    assert (p1[0] - p0[0], p1[1] - p0[1]) == (run, 8 - run), "digit passes run / skipped"
    out["run"], out["msg_run"] = run, _digits_that_differ(et[local], 2)
    return out


def env_local(sub_of, member):
    ok = member < len(sub_of)
    ok[ok] = sub_of[member[ok]] != NONE
    return ok


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1023, 1024, 1025])
def test_sizes_in_place(synth, N):
    topics, T, Pn, K = _sized(synth, N)
    out = _check_passes(synth, topics, ONE)
    assert out["rc"] == OK and (out["T"], out["P"], out["N"], out["total"]) == (T, Pn, N, K + 4)   # ('$p/x', '$q/x', '$r/x', '$s/x')
    assert out["moved"] == (K > 0)


@pytest.mark.parametrize("d,leg", [(-1, ONE), (0, ONE), (1, GRID)])
def test_the_compiled_bound_counts_every_pick_local_or_not(synth, d, leg):
    """T + K = GP1_DELIVERIES - 1, exactly, + 1: a few topics under long subscriber lists, 330 picks on more than
    256 messages (the picks' sort runs both of its passes), every third of them local"""
    picks, every = 330, 3
    T = GP1_DELIVERIES + d - picks - 4                          # (four entries without a slot: '$p/x' .. '$s/x')
    ids = _random_ids(T, 1 << 32, 7 + d)
    synth.member_subs({G_MEMBER + i: int(ids[i * 5]) if i % 2 else 77_000 + i for i in range(0, picks, every)})
    topics = synth.batch(ids, picks)
    out = _check_passes(synth, topics, leg)
    assert out["rc"] == OK and out["T"] + out["total"] == GP1_DELIVERIES + d and out["P"] == picks // every
    assert out["N"] == T + picks // every and out["moved"]
    if leg == ONE:
        assert out["msg_run"] == 2, "more than 256 messages: two digit passes over the picks"


def test_the_bound_lowered_and_the_smallest_of_the_three_wins(synth):
    ix = synth.ix
    assert ix.debug_get(GP1_MAX) == GP1_DELIVERIES
    ix.debug_set(GP1_MAX, 1 << 40)
    assert ix.debug_get(GP1_MAX) == GP1_DELIVERIES, "clamped to the compiled bound"
    ix.debug_set(GP1_MAX, 64)
    try:
        assert ix.debug_get(GP1_MAX) == 64
        for N, leg in ((64, ONE), (65, GRID)):
            T, Pn = N - 24, 20                                  # K = 24: the picks and '$p/x' .. '$s/x'; every pick local
            ids = _random_ids(T, 1 << 32, N)
            synth.member_subs({G_MEMBER + i: int(ids[i]) for i in range(Pn)})
            out = _check(synth.env, synth.b, synth.batch(ids, Pn), leg)
            assert out["rc"] == OK and out["T"] + out["total"] == N and out["N"] == N - 4
        ix.debug_set(GP1_MAX, GP1_DELIVERIES)
        for key, full in ((GS1_MAX, 16384), (DP1_MAX, _native.DP1_DELIVERIES)):
            ix.debug_set(key, 100)                              # bounds T alone
            try:
                for T, leg in ((100, ONE), (101, GRID)):
                    ids = _random_ids(T, 1 << 16, T)
                    synth.member_subs({G_MEMBER + i: int(ids[i]) for i in range(10)})
                    out = _check(synth.env, synth.b, synth.batch(ids, 10), leg)
                    assert out["rc"] == OK and out["T"] == T and out["N"] == T + 10
            finally:
                ix.debug_set(key, full)
    finally:
        ix.debug_set(GP1_MAX, GP1_DELIVERIES)


def test_no_local_pick_the_groups_are_tm_deliver_batch32s(synth):
    """P = 0, every member remote: the grouped arrays and the group outputs are bit-equal to
    tm_deliver_batch32's for the same batch; the picks are made all the same"""
    ids = _random_ids(1500, 1 << 16, 3)
    synth.member_subs({})
    topics = synth.batch(ids, 200)
    b = synth.b
    out = _check(synth.env, b, topics, ONE)
    assert out["rc"] == OK and out["P"] == 0 and out["N"] == out["T"] == 1500 and out["moved"]
    got = out["got"]
    assert (got[4][:out["total"]] != NONE).sum() == 200
    d = b.deliver32(topics, S_DESTS, 0, b.cap_max, b.dcap_max, b.gcap_max)
    for mine, theirs in zip((got[5], got[6], got[7], got[8], got[9], got[10], got[11]), d[1:]):
        assert np.array_equal(mine, theirs)


def test_picks_only(synth):
    """T = 0: 300 picks, two of three local, onto 40 subscribers"""
    synth.member_subs({G_MEMBER + i: 500 + i % 40 for i in range(300) if i % 3})
    out = _check_passes(synth, synth.batch([], 300), ONE)
    assert out["rc"] == OK and out["T"] == 0 and out["N"] == out["P"] == 200 and out["G"] == 40


def test_the_tie_rule_direct_before_picked_inside_one_message(synth):
    """'$m<j>/x': subscriber 40 + j gets message j's direct delivery (value 5000 + j) and its pick (6000 + j)"""
    ids = _random_ids(50, 1 << 8, 9)
    synth.member_subs({M_MEMBER + j: 40 + j for j in range(NM)} | {G_MEMBER + i: 40 + i % NM for i in range(30)})
    synth.ix.set_subscribers([MD_VAL + j for j in range(NM)], [[40 + j, 3000 + j] for j in range(NM)])
    topics = synth.batch(ids, 30, ties=NM)
    out = _check(synth.env, synth.b, topics, ONE)
    assert out["rc"] == OK and out["P"] == 30 + NM
    got = out["got"]
    N = out["N"]
    dt, dv, ds = got[6][:N], got[7][:N], got[8][:N]
    for j in range(NM):
        mine = np.nonzero(ds == 40 + j)[0]
        at = np.nonzero(dv[mine] == MD_VAL + j)[0]
        assert len(at) == 1 and dv[mine][at[0] + 1] == MP_VAL + j and dt[mine][at[0]] == dt[mine][at[0] + 1]
        assert (np.diff(dt[mine].astype(np.int64)) >= 0).all(), "a subscriber's messages ascend"


def test_subscriber_ids_at_both_ends(synth):
    """ids 0 and 0xFFFFFFFE direct and picked, 0xFFFFFFFF direct only (as a pick's target it means: not local)"""
    ids = np.array([0, 0xFFFFFFFF, 5, 0xFFFFFFFE, 0, 0xFFFFFFFF, 0xFFFFFFFE, 6, 0xFFFFFFFF, 0], np.uint32)
    synth.member_subs({G_MEMBER + i: (0, 0xFFFFFFFE, 5)[i % 3] for i in range(12)})
    out = _check_passes(synth, synth.batch(ids, 14), ONE)
    assert out["rc"] == OK and out["P"] == 12 and out["N"] == 22 and out["G"] == 5
    got = out["got"]
    assert got[10][:5].tolist() == [0, 5, 6, 0xFFFFFFFE, 0xFFFFFFFF] and got[11][5] == 22


def test_dcap_one_short_moves_nothing_and_the_exact_retry_succeeds(synth):
    topics, T, Pn, K = _sized(synth, 900, local_every=2)
    K += 4
    out = _check(synth.env, synth.b, topics, ONE, dcap=T + K - 1)
    assert out["rc"] == ECAP and not out["moved"] and (out["T"], out["total"]) == (T, K)
    assert synth.b.ghead.tolist() == [0, 0]
    out = _check(synth.env, synth.b, topics, ONE, dcap=int(synth.b.head[1]) + int(synth.b.doff[S_DESTS + 1]))
    assert out["rc"] == OK and out["moved"] and out["N"] == 900


def test_cap_short_moves_nothing(synth):
    topics, T, Pn, K = _sized(synth, 900)
    out = _check(synth.env, synth.b, topics, ONE, cap=K // 2)
    assert out["rc"] == ECAP and not out["moved"] and out["total"] == K + 4
    assert (synth.b.topic == CANARY).all(), "entries were written under total > cap with aggre"


def test_gcap_short_the_picks_stand(synth):
    topics, T, Pn, K = _sized(synth, 900)
    G = _check(synth.env, synth.b, topics, ONE)["G"]
    assert G > 100
    for gcap in (0, G - 1):
        out = _check(synth.env, synth.b, topics, ONE, gcap=gcap)
        assert out["rc"] == ECAP and out["moved"] and (out["G"], out["N"]) == (G, 900)
    ix = synth.ix                                               # the wrapper reads the bounds off the sorted dsub
    b = synth.b
    blob, offs = _native.pack_strings(topics)
    b.blob[:len(blob)], b.offs[:len(offs)] = blob, offs
    outs = (b.doff, b.topic, b.vals, b.err, b.head, b.dt, b.dv, b.ds, b.ghead, b.gsub, b.goff)
    full = ix.publish_deliver_batch32(b.blob, b.offs[:len(offs)], S_DESTS, 0, outs, b.member)
    gs, go = full[3][0].copy(), full[3][1].copy()
    cut = ix.publish_deliver_batch32(b.blob, b.offs[:len(offs)], S_DESTS, 0, outs, b.member, gcap=G - 1)
    assert len(gs) == G and np.array_equal(cut[3][0], gs) and np.array_equal(cut[3][1], go) and cut[4] == T


def test_dp1_too_large_nothing_is_picked_twice(synth):
    ix = synth.ix
    topics, T, Pn, K = _sized(synth, 900)
    ix.debug_set(DP1_MAX, 10)
    try:
        out = _check(synth.env, synth.b, topics, GRID)
        assert out["rc"] == OK and out["T"] == T > 10 and out["N"] == 900 and out["moved"]
        out = _check(synth.env, synth.b, topics, ONE, dcap=T + K)   # (K + 4 entries: short, decided by the gate)
        assert out["rc"] == ECAP and not out["moved"]
    finally:
        ix.debug_set(DP1_MAX, _native.DP1_DELIVERIES)


def test_einval(synth):
    ix, b = synth.ix, synth.b
    topics, T, Pn, K = _sized(synth, 30)
    synth.env.reset()
    before = synth.env.state()
    kc, kt = _keys(len(topics), 1)
    call = lambda **kw: b.call(topics, kw.pop("n_dests", S_DESTS), kw.pop("local", 0), 100, 100, 100, kc, kt,
                               ok=(EINVAL,), **kw)[0]
    assert call(flags=0) == EINVAL and call(flags=AGGRE | 2) == EINVAL and call(local=S_DESTS) == EINVAL
    assert call(n_dests=0) == EINVAL
    args = lambda member=P(b.member), head=P(b.head), ghead=P(b.ghead), gsub=P(b.gsub), goff=P(b.goff), gcap=16: (
        ix._h, len(topics), P(b.blob), P(b.offs), S_DESTS, 0, AGGRE, P(b.doff), P(b.topic), P(b.vals), 16, head, P(b.dt),
        P(b.dv), P(b.ds), 16, None, None, 0, member, ghead, gsub, goff, gcap, P(b.err))
    f = ix._lib.tm_publish_deliver_batch32
    assert f(*args(member=None)) == EINVAL and f(*args(head=None)) == EINVAL and f(*args(ghead=None)) == EINVAL
    assert f(*args(goff=None)) == EINVAL and f(*args(gsub=None)) == EINVAL
    odd = P(b.gsub[1:])                                        # 4 mod 8
    assert f(*args(ghead=odd)) == EINVAL and f(*args(head=odd)) == EINVAL
    assert f(*args(gsub=None, gcap=0)) == ECAP                 # (allowed; 16 entries are too few)
    assert np.array_equal(synth.env.state(), before), "a refused call moved a state"


# ---- 2. the staged arm and other memory

def test_a_plain_numpy_buffer_takes_the_staged_arm(synth):
    topics, T, Pn, K = _sized(synth, 700, local_every=2)
    for plain in ("goff", "member", "kc"):
        b = Bufs(synth.ix, 800, 800 * 10, 16, 1500, 1500, plain=(plain,))
        try:
            out = _check(synth.env, b, topics, GRID)
            assert out["rc"] == OK and out["N"] == 700 and out["moved"]
        finally:
            b.free()


def test_misaligned_topic_bytes_take_the_staged_arm(synth):
    topics, T, Pn, K = _sized(synth, 700)
    out = _check(synth.env, synth.b, topics, GRID, shift=4)
    assert out["rc"] == OK and out["N"] == 700
    out = _check(synth.env, synth.b, topics, GRID, shift=4, dcap=T + K)
    assert out["rc"] == ECAP and not out["moved"]


def test_inputs_and_keys_in_vram(synth):
    topics, T, Pn, K = _sized(synth, 700, local_every=2)
    b = Bufs(synth.ix, 800, 800 * 10, 16, 1500, 1500, vram_inputs=True)
    try:
        out = _check(synth.env, b, topics, ONE)
        assert out["rc"] == OK and out["N"] == 700
    finally:
        b.free()


def test_lookback_retry_moves_the_state_once(synth):
    """the look-back lives in the CSR walk of the staged arm (the in-place arm's pairs walk has none): a plain
    buffer takes the call there, the forced failure runs the batch again, and the state still moves once"""
    ix, env = synth.ix, synth.env
    topics, T, Pn, K = _sized(synth, 700)
    b = Bufs(ix, 800, 800 * 10, 16, 1500, 1500, plain=("member",))
    try:
        kc, kt = _keys(len(topics), 7)
        env.reset()
        ref = _reference(ix, topics, S_DESTS, 0, 1500, 1500, 1500, kc, kt)
        ref_state = env.state()
        env.reset()
        start = env.state()
        r0, g0 = ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES), ix.debug_get(GRID)
        ix.debug_set(_native.TM_DEBUG_LB_FAIL_BLOCK, 3)
        ix.debug_set(_native.TM_DEBUG_LB_LAUNCHES, 1)            # the first launch fails, the retry succeeds
        got = b.call(topics, S_DESTS, 0, 1500, 1500, 1500, kc, kt)
        assert ix.debug_get(_native.TM_DEBUG_RETRIED_BATCHES) == r0 + 1, "the look-back hook made no batch retry"
        assert ix.debug_get(GRID) == g0 + 1
        _same(got, ref)
        assert np.array_equal(env.state(), ref_state) and not np.array_equal(ref_state, start)
    finally:
        b.free()


# ---- 3. more than one workgroup's entries, a value scratch that grows

def test_a_value_scratch_that_grows_then_more_than_fo1_entries(gpu):
    """a fresh index: its lane's first value scratch (65536 words) is too small for 7,000 topics under ten '#'
    filters, so the batch runs twice; both runs have too many entries for the one-workgroup kernels, the gate
    keeps k_sh_one and k_gp_one out of both, and the grid pick and merge run once.  Then 2,000 topics: 20,000
    entries fit the scratch but not k_fo_one -- the grid kernels on the same pairs, one walk"""
    ix = _native.Index()
    try:
        vals = np.arange(10, dtype=np.uint32)
        ix.set_dests(vals, vals % 2)
        ix.set_route_filters(vals, vals)
        blob, offs = _native.pack_strings([b"#"] * 10)
        ix.apply(np.ones(10, np.uint8), blob, offs, vals)
        ix.set_subscribers([0, 3], [[1, 2], [3]])
        ix.set_share_slots(vals, vals % 4)
        ix.set_share_members([0, 1, 2, 3], [[10, 11, 12], [20, 21], [30, 31, 32, 33, 34], [40]], [0, 0, 0, 0],
                             [RR, PG, STICKY | 5 << 8, RR])
        sub_of = np.full(41, NONE, np.uint32)
        sub_of[[10, 12, 20, 31, 40]] = [2, 50, 3, 1, 51]
        ix.set_member_subs(np.arange(41, dtype=np.uint32), sub_of)
        env = Env(ix, 2, 0, [0, 1, 2, 3], sub_of)
        n, cap, dcap = 7000, 80_000, 100_000
        topics = [b"t/%d" % i for i in range(n)]
        kc, kt = _keys(n, SEED)
        b = Bufs(ix, n + 8, n * 8, 16, cap, dcap, gcap_max=64)
        keys = (_native.TM_DEBUG_PATH_PHASES, _native.TM_DEBUG_PATH_SMALL)
        env.reset()
        p0, g0, o0 = sum(ix.debug_get(k) for k in keys), ix.debug_get(GRID), ix.debug_get(ONE)
        got = b.call(topics, 2, 0, cap, dcap, 64, kc, kt)       # FIRST on this index: the scratch is still small
        assert sum(ix.debug_get(k) for k in keys) == p0 + 2, "the batch did not run twice"
        assert (ix.debug_get(GRID), ix.debug_get(ONE)) == (g0 + 1, o0)
        state = env.state()
        env.reset()
        ref = _reference(ix, topics, 2, 0, cap, dcap, 64, kc, kt)
        _same(got, ref)
        assert got[0] == OK and int(got[1][-1]) == 10 * n and int(got[9][0]) == 5
        assert np.array_equal(env.state(), state) and state[1] != UNDEF, "the state moved other than once"
        p0 = sum(ix.debug_get(k) for k in keys)
        out = _check(env, b, topics[:2000], GRID, gcap=64, definition=False)
        assert sum(ix.debug_get(k) for k in keys) == p0 + 2, "a second walk (the reference's is the other one)"
        assert out["rc"] == OK and out["total"] == 20_000 > FO1_ENTRIES and out["T"] == 4000 and out["moved"]
        out = _check(env, b, topics[:2000], GRID, gcap=64, dcap=23_999, definition=False)
        assert out["rc"] == ECAP and not out["moved"]
        b.free()
    finally:
        import torch
        torch.cuda.synchronize()
        ix.close()


# ---- 4. the 76-filter world: 400 members, about half of them local

N_MEMBERS = 400


@pytest.fixture(scope="module")
def world(gpu):
    from test_gpu_publish_batch import World
    w = World()
    rng = np.random.default_rng(77)
    slots = list(range(w.n_slots))
    strategies = (shared_sub.ROUND_ROBIN, shared_sub.HASH_CLIENTID, shared_sub.ROUND_ROBIN_PER_GROUP, shared_sub.STICKY,
                  shared_sub.HASH_TOPIC)
    w.set_members(slots, [rng.permutation(N_MEMBERS)[:s % 6].tolist() for s in slots],
                  [strategies[s % 5] | shared_sub.HASH_TOPIC << 8 for s in slots])
    n_sub_ids = len(w.subs._pids)
    sub_of = np.where(rng.random(N_MEMBERS) < 0.5, rng.integers(0, n_sub_ids, N_MEMBERS), NONE).astype(np.uint32)
    w.ix.set_member_subs(np.arange(N_MEMBERS, dtype=np.uint32), sub_of)
    w.env = Env(w.ix, w.n_dests, w.local, slots, sub_of)
    w.b = Bufs(w.ix, 1100, 1100 * 12, 16, 140_000, 90_000, gcap_max=2000)
    yield w
    w.b.free()
    w.close()


@pytest.mark.parametrize("n", [0, 1, 64, 1000])
def test_the_world_in_place(world, n):
    from test_gpu_publish_batch import _topics
    w = world
    topics = _topics(n, seed=n + 5)
    blob, offs = _native.pack_strings(topics)
    total = K = T = 0
    if n:
        total = int(w.ix.route_batch(blob, offs, w.n_dests)[0][-1])   # the un-aggregated total: what cap must hold
        K = int(w.ix.route_batch(blob, offs, w.n_dests, aggre=True)[0][-1])
        T = len(w.ix.dispatch_batch(blob, offs, w.n_dests, w.local, aggre=True)[1][0])
    one = total <= FO1_ENTRIES and T + K <= GP1_DELIVERIES
    print(f"n={n}: total={total} K={K} T={T} ending={'one workgroup' if one else 'grid'}")
    assert one == (n <= 64)
    out = _check(w.env, w.b, topics, ONE if one else GRID)
    assert out["rc"] == OK and (out["T"], out["total"]) == (T, K)
    if n >= 64:
        assert 0 < out["P"] < K and out["moved"]
        got = out["got"]
        m = got[4][:K]
        local = env_local(w.env.sub_of, m.copy())
        direct = set(got[8][:out["N"]].tolist())
        assert (m == NONE).sum() > 0 and ((m != NONE) & ~local).sum() > 0, "no entry without a pick / no remote pick"
        assert set(w.env.sub_of[m[local]].tolist()) & direct


def test_five_consecutive_batches_with_members_and_member_subs_changed_in_between(world):
    """the reference's five from the start state, then the call's five: every batch's outputs and the words
    after it are equal"""
    from test_gpu_publish_batch import _topics
    w, ix, b = world, world.ix, world.b
    topics = _topics(64, seed=31)
    rng = np.random.default_rng(12)
    first_lists = [list(w.lists[s]) for s in w.env.slots.tolist()]
    first_meta = [w.meta[s] for s in w.env.slots.tolist()]
    first_sub_of = w.env.sub_of.copy()
    changes = []
    for _ in range(5):
        slots = rng.choice(w.env.slots, 3, replace=False).tolist()
        changes.append((slots, [rng.permutation(N_MEMBERS)[:int(rng.integers(0, 7))].tolist() for _ in slots],
                        [int(rng.integers(0, 5)) | 6 << 8 for _ in slots],
                        (rng.integers(0, N_MEMBERS, 40), np.where(rng.random(40) < 0.5, rng.integers(0, 30, 40), NONE))))

    def run(call):
        w.set_members(w.env.slots.tolist(), first_lists, first_meta)
        ix.set_member_subs(np.arange(N_MEMBERS, dtype=np.uint32), first_sub_of)
        w.env.reset()
        outs = []
        for k in range(5):
            kc, kt = _keys(len(topics), 300 + k)
            outs.append((call(kc, kt, 40 + k), w.env.state()))
            slots, lists, meta, (members, subs) = changes[k]
            w.set_members(slots, lists, meta)
            ix.set_member_subs(members.astype(np.uint32), subs.astype(np.uint32))
        return outs
    try:
        ref = run(lambda kc, kt, seed: _reference(ix, topics, w.n_dests, w.local, b.cap_max, b.dcap_max, b.gcap_max, kc, kt,
                                                  seed))
        o0 = ix.debug_get(ONE)
        got = run(lambda kc, kt, seed: b.call(topics, w.n_dests, w.local, b.cap_max, b.dcap_max, b.gcap_max, kc, kt, seed))
        assert ix.debug_get(ONE) == o0 + 5
        for (g, gs), (r, rs) in zip(got, ref):
            _same(g, r)
            assert np.array_equal(gs, rs)
        assert len({tuple(s.tolist()) for _, s in ref}) == 5, "the words never moved"
        assert len({tuple(r[8][:int(r[9][1])].tolist()) for r, _ in ref}) > 1, "the member-subs changes changed nothing"
    finally:
        w.set_members(w.env.slots.tolist(), first_lists, first_meta)
        ix.set_member_subs(np.arange(N_MEMBERS, dtype=np.uint32), first_sub_of)


# ---- 5. concurrency

def test_four_threads_share_one_round_robin_per_group_slot(synth):
    """4 x 50 calls of one entry each on one slot of five members, three of them local: each call's transition
    is one compare-and-swap loop on the device-resident word, so the 200 picks are those of 200 sequential
    calls, as a multiset -- and each call's merged delivery is its own pick's"""
    ix = synth.ix
    topic = [b"$g7/x"]
    members = np.array([100, 101, 102, 103, 104], np.uint32)
    ix.set_share_members([7], [members], [0], [PG])
    synth.member_subs({100: 9000, 102: 9002, 103: 9003})
    sub_of = synth.env.sub_of
    c0 = 3
    try:
        ix.share_state_set([7], [c0])
        o0 = ix.debug_get(ONE)
        bs = [Bufs(ix, 4, 64, 16, 64, 64) for _ in range(4)]
        picks, errors = [[] for _ in bs], []

        def work(i):
            try:
                for _ in range(50):
                    rc, doff, t, v, m, head, dt, dv, ds, ghead = bs[i].call(topic, S_DESTS, 0, 64, 64, 64, None, None)[:10]
                    assert rc == OK and int(doff[-1]) == 1 and int(head[1]) == 0
                    s = int(sub_of[int(m[0])])
                    assert ghead.tolist() == ([1, 1] if s != NONE else [0, 0])
                    assert s == NONE or (int(ds[0]), int(dv[0]), int(dt[0])) == (s, G_VAL + 7, 0)
                    picks[i].append(int(m[0]))
            except BaseException as e:   # noqa: BLE001
                errors.append(e)
        ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        for b in bs:
            b.free()
        assert not errors, errors
        assert ix.debug_get(ONE) == o0 + 200
        want = Counter(int(members[(c0 + i) % 5]) for i in range(200))
        assert Counter(p for ps in picks for p in ps) == want
        assert ix.share_state_get([7]).tolist() == [(c0 + 199) % 5 + 1]
    finally:
        ix.set_share_members([7], [[G_MEMBER + 7]], [0], [(RR, PG, STICKY | 5 << 8)[7 % 3]])


# ---- 6. the layers: Router(route_in_place=True).match_routes_publish_deliver and the Broker through it

def _layers(in_place):
    """test_gpu_publish_deliver_batch.py's router over a real device mirror, staged or in place: four wildcard
    filters routed to n1 and n2, four groups with members on n1 (some of which also subscribe directly) and n2,
    an exact-topic $share route in the host bag"""
    from emqx_amd.router import Router
    from emqx_amd.shared_sub import SharedSubs
    from emqx_amd.subscribers import LocalSubs
    ss = SharedSubs(node="n1")
    r = Router(node="n1", local_subs=LocalSubs(), shared_subs=ss, route_in_place=in_place)
    ss.set_strategy(b"rr", "round_robin")
    ss.set_strategy(b"pg", "round_robin_per_group")
    ss.set_strategy(b"hc", "hash_clientid")
    ss.set_strategy(b"st", "sticky", "hash_topic")
    filters = (b"a1/#", b"+/b2/+", b"a1/b2/+", b"#")
    pid = 0
    for g in (b"rr", b"pg", b"hc", b"st"):
        for f in filters + (b"a1/b2/c3",):
            for k in range(2 + (len(f) + len(g)) % 3):
                p = ("n1" if k % 3 != 2 else "n2", pid)
                ss.subscribe(g, f, p)
                if k == 0 and f != b"a1/b2/c3":
                    r.local_subs.subscribe(f, p)                 # a member that subscribes directly as well
                pid += 1
            r.add_route(f, (g, "n2"))
    r.add_route(b"#", (b"empty", "n3"))                          # a pair without members: no pick
    for f in filters:
        r.add_route(f, "n2")
        r.add_route(f, "n1")
        r.local_subs.subscribe(f, ("local", f))
    return r


def test_router_and_broker_in_place_equal_the_staged_ones(gpu):
    from emqx_amd.broker import Broker, Message
    from test_gpu_publish_batch import _topics
    staged, inplace, b_staged, b_inplace = _layers(False), _layers(True), _layers(False), _layers(True)
    try:
        topics = [t for t in _topics(300, seed=71) if b"+" not in t and b"#" not in t]
        topics[5] = b"a1/b2/c3"
        n = len(topics)
        ix = inplace._mirror._index
        for batch in range(3):                                   # the state carries from batch to batch
            kc, kt = _keys(n, 80 + batch)
            e = staged.match_routes_publish_deliver(topics, kc[:n], kt[:n], seed=batch)
            o0, g0 = ix.debug_get(ONE), ix.debug_get(GRID)
            g = inplace.match_routes_publish_deliver(topics, kc[:n], kt[:n], seed=batch)
            # (the first batch sizes the pooled buffers: a call that moved nothing, then the one that stands)
            assert ix.debug_get(ONE) - o0 in ((1, 2) if batch == 0 else (1,)) and ix.debug_get(GRID) == g0, \
                "the router did not go through tm_publish_deliver_batch32 in place"
            assert dict(g[0]) == dict(e[0]) and g[1] == e[1] and g[2] == e[2] and g[3] == e[3] and len(e[1]) > n
            direct = {p for _, _, p in e[1]}
            local = {p for rows in e[2].values() for _, _, p in rows if p is not None and staged.member_is_local(p)}
            assert direct & local, "no subscriber with both kinds"
        kc, kt = _keys(n, 99)
        msgs = [Message(t, i) for i, t in enumerate(topics)]
        one, two = [], []

        def broker(r, log):
            return Broker(r, share_on_device=True, share_grouped=True, share_seed=9,
                          share_keys=lambda m: (int(kc[m.payload]), int(kt[m.payload])),
                          share_send=lambda p, to, m: log.append((p, to, m.payload)) or "ok",
                          deliver=lambda p, to, m: log.append((p, to, m.payload)),
                          deliver_batch=lambda p, items: log.append(("batch", p, [(to, m.payload) for to, m in items])),
                          share_dispatch=lambda g, to, m: 1 / 0)
        plans, errors = broker(b_staged, one).publish_batch_by_dest(msgs)
        bix = b_inplace._mirror._index
        o0, g0 = bix.debug_get(ONE), bix.debug_get(GRID)
        plans2, errors2 = broker(b_inplace, two).publish_batch_by_dest(msgs)
        assert bix.debug_get(ONE) - o0 in (1, 2) and bix.debug_get(GRID) == g0
        assert plans2 == plans and errors2 == errors == {}
        assert two == one and len([x for x in two if x[0] == "batch"]) > 4
    finally:
        gpu.cuda.synchronize()
        for r in (staged, inplace, b_staged, b_inplace):
            r._mirror._index.close()
