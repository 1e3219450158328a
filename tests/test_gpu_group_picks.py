"""tm_group_picks_dev driven directly: synthetic deliveries, aggregated entries,
picked members and a member -> subscriber table built in numpy, exact against
the numpy definition in include/tmatch.h (tests/group_picks_ref.py) -- no index
content involved (the pattern of test_gpu_group.py).

Every input holds a poisoned tail past W / E / sub_of_len (deliveries of a
subscriber nobody else has, members that would be local picks): a read past the
bounds changes the outputs.  Every output buffer is filled with a sentinel that
must survive at and past min(N, out_cap), at and past Gw in out_gsub, past
out_goff[Gw] and past ghead[1]; the inputs are compared after the run.
"""
import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.shared_sub import pick_batch_ref
from group_picks_ref import group_picks_ref
from group_ref import group_ref

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CANARY = 0xC0FFEE11
OFFS_CANARY = -77
TAIL = 64
POISON = 32


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def index(torch_dev):
    """an empty index: the call needs a handle for its scratch only"""
    ix = _native.Index()
    yield ix
    torch_dev.cuda.synchronize()
    ix.close()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.itemsize == 4 else np.int64)).cuda()


def _canary32(torch, n):
    return torch.from_numpy(np.full(n, CANARY, np.uint32).view(np.int32)).cuda()


def make(W, E, p_local, n_msgs, n_subs=40, n_dests=3, seed=0, one_sub_one_msg=False, big_ids=False):
    """-> dict of inputs: W deliveries in ascending message order, E entries in
    n_dests buckets (ascending message inside a bucket, as the fan-out leaves
    them), a member per entry: NONE (no pick), remote (sub_of NONE), beyond the
    table, or -- a share p_local -- a local subscriber"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(1 << 20)[:n_subs].astype(np.uint32) if big_ids else np.arange(n_subs, dtype=np.uint32)
    ids = ids.copy()
    ids[0], ids[1] = 0, 0xFFFFFFFE
    topic = np.sort(rng.integers(0, n_msgs, W)).astype(np.uint32)
    value = rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)
    sub = ids[rng.integers(0, n_subs, W)]
    if W > 3:
        sub[W // 2] = NONE                       # a direct delivery may carry 0xFFFFFFFF
    cuts = np.sort(rng.integers(0, E + 1, n_dests))
    doff = np.concatenate([[0], cuts, [E]]).astype(np.uint64)   # n_dests + 2: the last bucket unrouted
    etopic = np.zeros(E, np.uint32)
    for b in range(n_dests + 1):
        lo, hi = int(doff[b]), int(doff[b + 1])
        etopic[lo:hi] = np.sort(rng.integers(0, n_msgs, hi - lo))
    evalue = rng.integers(0, 1 << 32, E, dtype=np.uint64).astype(np.uint32)
    n_members = 3 * n_subs
    sub_of = np.full(n_members, NONE, np.uint32)
    sub_of[:n_subs] = ids[rng.permutation(n_subs)]            # members 0 .. n_subs - 1 are local
    kind = rng.random(E)
    member = np.where(kind < p_local, rng.integers(0, n_subs, E),
                      np.where(kind < p_local + (1 - p_local) / 3, rng.integers(n_subs, n_members, E),
                               np.where(kind < p_local + 2 * (1 - p_local) / 3, n_members + rng.integers(0, 5, E),
                                        NONE))).astype(np.uint32)
    if one_sub_one_msg:                          # pure ties: every pick to one subscriber in one message
        etopic[:] = n_msgs // 2
        member[:] = 0
    return dict(topic=topic, value=value, sub=sub, doff=doff, n_dests=n_dests + 0, etopic=etopic, evalue=evalue,
                member=member, sub_of=sub_of)


class Run:
    """one tm_group_picks_dev call's device buffers (kept alive until checked)"""

    def __init__(self, torch, ix, d, T=None, cap=None, K=None, ecap=None, out_cap=None, gcap=None, src=True, stream=None):
        W0, E0 = len(d["sub"]), len(d["member"])
        T = W0 if T is None else T
        cap = T if cap is None else cap
        ecap = E0 if ecap is None else ecap
        doff = d["doff"].copy()
        if K is not None:
            doff[-1] = K
        W, E = min(T, cap), min(int(doff[-1]), ecap)
        assert W <= W0 and E <= E0
        head = np.array([4242, T], np.uint64)
        full = group_picks_ref(head, d["topic"], d["value"], d["sub"], cap, d["n_dests"], doff, d["etopic"], d["evalue"],
                               d["member"], ecap, d["sub_of"], 1 << 40, 1 << 40)
        G, N = full[0]
        out_cap = N if out_cap is None else out_cap
        gcap = G if gcap is None else gcap
        self.exp = group_picks_ref(head, d["topic"], d["value"], d["sub"], cap, d["n_dests"], doff, d["etopic"],
                                   d["evalue"], d["member"], ecap, d["sub_of"], out_cap, gcap)
        # the inputs as the device gets them: exact below W / E, poison behind
        pz = np.zeros(POISON, np.uint32)
        ins = [np.concatenate([d["topic"][:W], pz]), np.concatenate([d["value"][:W], pz]),
               np.concatenate([d["sub"][:W], np.full(POISON, 0xFFFFFFFD, np.uint32)]),
               np.concatenate([d["etopic"][:E], pz]), np.concatenate([d["evalue"][:E], pz]),
               np.concatenate([d["member"][:E], pz]),                                   # member 0 is local
               np.concatenate([d["sub_of"], np.full(POISON, 0xFFFFFFFD, np.uint32)])]   # members beyond: "local"
        self.torch, self.ins, self.src, self.keep = torch, ins, src, min(N, out_cap)
        Gw = min(G, gcap)
        with torch.cuda.stream(stream) if stream is not None else _Null():
            self.d_head, self.d_doff = _dev(torch, head), _dev(torch, doff)
            self.d_in = [_dev(torch, a) for a in ins]
            self.o_ghead = torch.full((2 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.o_goff = torch.full((Gw + 1 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.o_gsub = _canary32(torch, Gw + TAIL)
            self.o_t, self.o_v, self.o_s, self.o_p = (_canary32(torch, self.keep + TAIL) for _ in range(4))
            t, v, s, et, ev, m, so = (a.data_ptr() for a in self.d_in)
            ix.group_picks_dev(self.d_head.data_ptr(), t, v, s, cap, d["n_dests"], self.d_doff.data_ptr(), et, ev, m, ecap,
                               self.o_ghead.data_ptr(), self.o_gsub.data_ptr(), self.o_goff.data_ptr(), gcap,
                               self.o_t.data_ptr(), self.o_v.data_ptr(), self.o_s.data_ptr(), out_cap,
                               d_out_src=self.o_p.data_ptr() if src else None, d_sub_of=so, sub_of_len=len(d["sub_of"]),
                               stream=torch.cuda.current_stream().cuda_stream)

    def outputs(self):
        self.torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (self.o_ghead, self.o_goff, self.o_gsub, self.o_t, self.o_v, self.o_s, self.o_p)]

    def check(self, what):
        """exact outputs, sentinels, inputs unmodified -> (G, N, W, P)"""
        (G, N), e_t, e_v, e_s, e_p, e_gsub, e_goff, W, P = self.exp
        Gw, keep = len(e_gsub), self.keep
        ghead, g_goff, g_gsub, g_t, g_v, g_s, g_p = self.outputs()
        g_gsub, g_t, g_v, g_s, g_p = (x.view(np.uint32) for x in (g_gsub, g_t, g_v, g_s, g_p))
        print(f"{what}: W={W} P={P} N={N} G={G} Gw={Gw} keep={keep} ghead={ghead[:2].tolist()}")
        assert ghead[:2].view(np.uint64).tolist() == [G, N], f"{what}: ghead is {ghead[:2].tolist()}, not {[G, N]}"
        assert (ghead[2:] == OFFS_CANARY).all(), f"{what}: wrote past ghead[1]"
        assert np.array_equal(g_goff[:Gw + 1].view(np.uint64), e_goff), f"{what}: group offsets differ"
        assert (g_goff[Gw + 1:] == OFFS_CANARY).all(), f"{what}: wrote past out_goff[Gw]"
        assert np.array_equal(g_gsub[:Gw], e_gsub), f"{what}: group subscribers differ"
        assert (g_gsub[Gw:] == CANARY).all(), f"{what}: wrote at or past Gw in out_gsub"
        bad = np.nonzero((g_t[:keep] != e_t) | (g_v[:keep] != e_v) | (g_s[:keep] != e_s))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {keep} merged deliveries differ, first at {bad[0]}"
        if self.src:
            assert np.array_equal(g_p[:keep], e_p), f"{what}: out_src differs"
        else:
            assert (g_p == CANARY).all(), f"{what}: out_src was NULL"
        for g in (g_t, g_v, g_s) + ((g_p,) if self.src else ()):
            assert (g[keep:] == CANARY).all(), f"{what}: wrote at or past min(N, out_cap)"
        for dev, host in zip(self.d_in, self.ins):
            assert np.array_equal(dev.cpu().numpy().view(np.uint32), host), f"{what}: an input was written"
        return G, N, W, P


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("n_msgs", [200, 1000])
@pytest.mark.parametrize("W,E,p_local", [(0, 0, 0.5), (1, 1, 1.0), (1023, 90, 0.7), (1025, 100, 0.65), (5000, 4500, 0.67),
                                         (0, 300, 0.5), (1, 2, 0.0), (777, 63, 1.0), (778, 65, 1.0)])
def test_sizes(torch_dev, index, W, E, p_local, n_msgs):
    """W around GS_TILE and over many blocks of the merge's searches, P from 0 to about 3,000;
    messages below 256 (one digit pass over the picks) and up to 1,000 (two)"""
    d = make(W, E, p_local, n_msgs, seed=W + E)
    G, N, w, P = Run(torch_dev, index, d).check(f"W={W} E={E} msgs={n_msgs}")
    assert w == W and (P == E if p_local == 1.0 else P <= E)
    if (W, E) == (5000, 4500):
        assert 2500 < P < 3500


def test_no_local_pick_equals_group_subs_dev(torch_dev, index):
    """P = 0, every member NONE, remote or beyond the table: bit-equal to tm_group_subs_dev on the same deliveries"""
    torch = torch_dev
    d = make(3000, 500, 0.0, 300, seed=11)
    r = Run(torch, index, d)
    G, N, W, P = r.check("P = 0")
    assert P == 0 and N == W == 3000
    ghead = torch.full((2,), OFFS_CANARY, dtype=torch.int64, device="cuda")
    goff = torch.full((G + 1,), OFFS_CANARY, dtype=torch.int64, device="cuda")
    gsub, ot, ov, os_, op = (_canary32(torch, n) for n in (G, W, W, W, W))
    index.group_subs_dev(r.d_head.data_ptr(), r.d_in[0].data_ptr(), r.d_in[1].data_ptr(), r.d_in[2].data_ptr(), W,
                         ghead.data_ptr(), gsub.data_ptr(), goff.data_ptr(), G, ot.data_ptr(), ov.data_ptr(),
                         os_.data_ptr(), d_out_perm=op.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for a, b in ((ghead, r.o_ghead[:2]), (goff, r.o_goff[:G + 1]), (gsub, r.o_gsub[:G]), (ot, r.o_t[:W]), (ov, r.o_v[:W]),
                 (os_, r.o_s[:W]), (op, r.o_p[:W])):
        assert torch.equal(a, b)
    e = group_ref([0, W], d["topic"], d["value"], d["sub"], W, G)
    assert np.array_equal(ot.cpu().numpy().view(np.uint32), e[1])


def test_pure_ties_and_interleaving(torch_dev, index):
    d = make(2000, 700, 1.0, 100, seed=5, one_sub_one_msg=True)
    G, N, W, P = Run(torch_dev, index, d).check("all picks to one subscriber in one message")
    assert P == 700
    # one subscriber with direct deliveries and picks interleaved over the messages
    W, E = 600, 600
    d = make(W, E, 1.0, 1000, n_subs=4, seed=6)
    d["topic"] = (2 * np.arange(W)).astype(np.uint32)            # even messages direct, odd ones picked, one tie
    d["sub"][:] = 7
    d["etopic"] = (2 * np.arange(E) + 1).astype(np.uint32)
    d["etopic"][5] = 10
    d["doff"] = np.array([0, E, E, E, E], np.uint64)
    d["sub_of"][:] = 7
    r = Run(torch_dev, index, d)
    assert r.check("interleaved")[0] == 1
    src = r.exp[4]
    assert src[0] == 0 and src[1] >= W and src[2] == 1            # direct, pick, direct ...
    big = make(1500, 1200, 0.6, 900, n_subs=300, seed=8, big_ids=True)
    Run(torch_dev, index, big).check("ids up to 2^20: three digit passes over the subscribers")


def test_caps(torch_dev, index):
    d = make(3000, 2000, 0.6, 500, seed=21)
    full = Run(torch_dev, index, d)
    G, N, W, P = full.check("room for everything")
    Run(torch_dev, index, d, T=3000, cap=1700).check("cap < head[1]")
    Run(torch_dev, index, d, T=9000, cap=3000).check("cap < head[1], every input position used")
    Run(torch_dev, index, d, ecap=1100).check("ecap < the entry total")
    Run(torch_dev, index, d, K=5000, ecap=2000).check("ecap < the entry total, every entry position used")
    Run(torch_dev, index, d, K=900).check("the entry total below the arrays")
    Run(torch_dev, index, d, cap=0, ecap=0, T=0).check("cap = ecap = 0")
    for out_cap in (N - 1, N // 2, 1, 0):
        g, n, _, _ = Run(torch_dev, index, d, out_cap=out_cap).check(f"out_cap = {out_cap} < N = {N}")
        assert (g, n) == (G, N)
    for gcap in (G - 1, G // 2, 1, 0):
        g, n, _, _ = Run(torch_dev, index, d, gcap=gcap).check(f"gcap = {gcap} < G = {G}")
        assert (g, n) == (G, N)
    Run(torch_dev, index, d, gcap=G + 9, out_cap=N + 9).check("caps above G and N")
    Run(torch_dev, index, d, src=False).check("out_src NULL")


def test_two_runs_give_identical_bytes(torch_dev, index):
    d = make(4000, 3000, 0.7, 800, seed=31)
    a, b = Run(torch_dev, index, d), Run(torch_dev, index, d)
    for x, y in zip(a.outputs(), b.outputs()):
        assert x.tobytes() == y.tobytes()
    a.check("first run")


def test_scratch_reuse_and_release(torch_dev, index):
    s = torch_dev.cuda.Stream()
    for W, E in ((50, 20), (20000, 9000), (50, 20), (0, 9000), (3, 0)):
        Run(torch_dev, index, make(W, E, 0.5, 250, seed=W), stream=s).check(f"scratch reuse W={W} E={E}")
    index.release_stream(s.cuda_stream)


def test_chained_behind_dispatch_and_pick_with_the_indexs_own_tables(torch_dev):
    """tm_dispatch_dev -> tm_share_pick_dev -> tm_group_picks_dev on one stream with the index's own
    tables (tm_set_subscribers, tm_set_share_*, tm_set_member_subs), no host synchronisation in between"""
    torch = torch_dev
    ix = _native.Index()
    rng = np.random.default_rng(17)
    n_vals, n_slots, n_members, M = 60, 6, 30, 500
    lists = [rng.integers(0, 25, int(k)).astype(np.uint32) for k in rng.integers(0, 6, n_vals)]
    ix.set_subscribers(np.arange(n_vals, dtype=np.uint32), lists)
    slot_of = np.full(n_vals, NONE, np.uint32)
    slot_of[40:] = rng.integers(0, n_slots, n_vals - 40)
    ix.set_share_slots(np.arange(n_vals, dtype=np.uint32), slot_of)
    mlists = [rng.permutation(n_members)[:int(k)].astype(np.uint32) for k in (0, 1, 3, 4, 7, 2)]
    meta = np.array([_native.TM_SHARE_ROUND_ROBIN, _native.TM_SHARE_HASH_TOPIC, _native.TM_SHARE_ROUND_ROBIN_PER_GROUP,
                     _native.TM_SHARE_STICKY | _native.TM_SHARE_HASH_CLIENTID << 8, _native.TM_SHARE_HASH_CLIENTID,
                     _native.TM_SHARE_ROUND_ROBIN], np.uint32)
    ix.set_share_members(np.arange(n_slots, dtype=np.uint32), mlists, np.zeros(n_slots, np.uint32), meta)
    state0 = np.array([2, 0, 1, NONE, 0, 0], np.uint32)
    ix.share_state_set(np.arange(n_slots, dtype=np.uint32), state0)
    sub_of = np.where(rng.random(n_members) < 0.6, rng.integers(0, 25, n_members), NONE).astype(np.uint32)
    ix.set_member_subs(np.arange(n_members, dtype=np.uint32), sub_of)
    # bucket 0: this node's routes (values below 40), bucket 1: the groups' (values from 40)
    n0 = 300
    t = np.concatenate([np.sort(rng.integers(0, 200, n0)), np.sort(rng.integers(0, 200, M - n0))]).astype(np.uint32)
    v = np.concatenate([rng.integers(0, 40, n0), rng.integers(40, n_vals, M - n0)]).astype(np.uint32)
    doff = np.array([0, n0, M, M], np.uint64)
    kc, kt = (rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    e_sub = np.concatenate([lists[x] for x in v[:n0]] + [np.zeros(0, np.uint32)])
    lens = np.array([len(lists[x]) for x in v[:n0]])
    e_t, e_v = np.repeat(t[:n0], lens), np.repeat(v[:n0], lens)
    T = len(e_sub)
    rec = np.zeros((n_slots, 4), np.uint32)
    pool = np.concatenate(mlists).astype(np.uint32)
    rec[:, 0] = np.concatenate([[0], np.cumsum([len(x) for x in mlists])[:-1]])
    rec[:, 1] = [len(x) for x in mlists]
    rec[:, 3] = meta
    e_member, _, e_state = pick_batch_ref(2, doff, t, v, M, slot_of, rec, pool, state0, kc, kt, 200, 9)
    exp = group_picks_ref([n0, T], e_t, e_v, e_sub, T, 2, doff, t, v, e_member, M, sub_of, T + M, T + M)
    (G, N), x_t, x_v, x_s, x_p, x_gsub, x_goff, W, P = exp
    assert 0 < P < M - n0 and (e_member == NONE).any() and G > 5
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_doff, d_t, d_v, d_kc, d_kt = (_dev(torch, a) for a in (doff, t, v, kc, kt))
        head = torch.full((2,), OFFS_CANARY, dtype=torch.int64, device="cuda")
        phead = torch.full((2,), OFFS_CANARY, dtype=torch.int64, device="cuda")
        dt, dv, ds = (_canary32(torch, T + 1) for _ in range(3))
        mem = _canary32(torch, M)
        ghead = torch.full((2,), OFFS_CANARY, dtype=torch.int64, device="cuda")
        goff = torch.full((T + M + 1,), OFFS_CANARY, dtype=torch.int64, device="cuda")
        gsub, ot, ov, os_, op = (_canary32(torch, T + M) for _ in range(5))
        ix.dispatch_dev(2, d_doff.data_ptr(), 0, d_t.data_ptr(), d_v.data_ptr(), M, head.data_ptr(), dt.data_ptr(),
                        dv.data_ptr(), ds.data_ptr(), T, stream=s.cuda_stream)
        ix.share_pick_dev(2, d_doff.data_ptr(), d_t.data_ptr(), d_v.data_ptr(), M, phead.data_ptr(), mem.data_ptr(),
                          d_key_clientid=d_kc.data_ptr(), d_key_topic=d_kt.data_ptr(), n_topics=200, seed=9,
                          stream=s.cuda_stream)
        ix.group_picks_dev(head.data_ptr(), dt.data_ptr(), dv.data_ptr(), ds.data_ptr(), T, 2, d_doff.data_ptr(),
                           d_t.data_ptr(), d_v.data_ptr(), mem.data_ptr(), M, ghead.data_ptr(), gsub.data_ptr(),
                           goff.data_ptr(), T + M, ot.data_ptr(), ov.data_ptr(), os_.data_ptr(), T + M,
                           d_out_src=op.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert head.cpu().numpy().view(np.uint64).tolist() == [n0, T]
    assert np.array_equal(mem.cpu().numpy().view(np.uint32), e_member)
    assert ghead.cpu().numpy().view(np.uint64).tolist() == [G, N]
    for got, want in ((ot, x_t), (ov, x_v), (os_, x_s), (op, x_p), (gsub, x_gsub)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32)[:len(want)], want)
        assert (got.cpu().numpy().view(np.uint32)[len(want):] == CANARY).all()
    assert np.array_equal(goff.cpu().numpy().view(np.uint64)[:G + 1], x_goff)
    assert np.array_equal(ix.share_state_get(np.arange(n_slots, dtype=np.uint32)), e_state)
    ix.release_stream(s.cuda_stream)
    ix.close()


def test_refusals_name_the_entry_point(torch_dev, index):
    """one row per TM_EINVAL cause; nothing is queued (the sentinels stay)"""
    torch = torch_dev
    lib = _native.load_library()
    a32 = [_canary32(torch, 16) for _ in range(12)]
    a64 = [torch.full((8,), OFFS_CANARY, dtype=torch.int64, device="cuda") for _ in range(4)]
    P32, P64 = [a.data_ptr() for a in a32], [a.data_ptr() for a in a64]
    #        head    topic   value   sub    cap nd doff    etopic  evalue  member ecap sub_of len
    good = [P64[0], P32[0], P32[1], P32[2], 4, 1, P64[1], P32[3], P32[4], P32[5], 2, P32[6], 4,
            # ghead gsub    goff  gcap out_t   out_v   out_s    src     out_cap
            P64[2], P32[7], P64[3], 4, P32[8], P32[9], P32[10], P32[11], 6]
    rows = [("null d_head", 0, None), ("null d_topic with cap > 0", 1, None), ("null d_sub with cap > 0", 3, None),
            ("n_dests 0", 5, 0), ("n_dests above 65536", 5, 65537), ("null d_dest_offsets", 6, None),
            ("null d_etopic with ecap > 0", 7, None), ("null d_member with ecap > 0", 9, None),
            ("sub_of_len above 2^32 - 1", 12, 1 << 32), ("null d_out_ghead", 13, None),
            ("null d_out_gsub with gcap > 0", 14, None), ("null d_out_goff", 15, None),
            ("null d_out_topic with out_cap > 0", 17, None), ("null d_out_sub with out_cap > 0", 19, None),
            ("d_head not 8-byte aligned", 0, P64[0] + 4), ("d_out_ghead not 8-byte aligned", 13, P64[2] + 4),
            ("d_out_goff not 8-byte aligned", 15, P64[3] + 4), ("cap + ecap above 2^32 - 1", 4, (1 << 32) - 2)]
    for what, at, bad in rows:
        args = list(good)
        args[at] = bad
        rc = lib.tm_group_picks_dev(index._h, *args, torch.cuda.current_stream().cuda_stream)
        assert rc == _native.TM_EINVAL, f"{what}: {rc}"
        assert b"tm_group_picks_dev" in lib.tm_last_error(None), what
    assert lib.tm_group_picks_dev(None, *good, None) == _native.TM_EINVAL   # a null handle
    torch.cuda.synchronize()
    for a in a32:
        assert (a.cpu().numpy().view(np.uint32) == CANARY).all()
    for a in a64:
        assert (a.cpu().numpy() == OFFS_CANARY).all()
    # allowed: no arrays with cap == ecap == out_cap == 0, no out_gsub with gcap == 0, the index's own (empty) table
    a64[1].zero_()
    index.group_picks_dev(P64[0], None, None, None, 0, 1, P64[1], None, None, None, 0, P64[2], None, P64[3], 0, None,
                          None, None, 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert a64[2].cpu().numpy()[:2].tolist() == [0, 0] and a64[3].cpu().numpy()[0] == 0
