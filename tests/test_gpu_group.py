"""tm_group_subs_dev driven directly: synthetic delivery arrays built in numpy,
exact against the numpy definition in include/tmatch.h (tests/group_ref.py) --
no index content involved (the pattern of test_gpu_dispatch.py).

The sort runs on a fixed grid of B = TM_DEBUG_GROUP_GRID blocks; block k owns
chunk = ceil(W / B) rounded up to K = TM_DEBUG_GROUP_TILE positions and ranks K
keys at a time, so up to B K deliveries (about 1M) a block owns one tile and
from there on several.  The
inputs hold exactly W deliveries (one spare word keeps an empty tensor from
being a null pointer); every output buffer is filled with a sentinel that must
survive at and past W, at and past Gw in out_gsub, past out_goff[Gw] and past
ghead[1]; the inputs are compared after the run.
"""
import numpy as np
import pytest

from emqx_amd import _native
from group_ref import group_ref

pytestmark = pytest.mark.gpu

CANARY = 0xC0FFEE11
OFFS_CANARY = -77
TAIL = 64


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def index(torch_dev):
    """an empty index: tm_group_subs_dev needs a handle for its scratch only"""
    ix = _native.Index()
    yield ix
    torch_dev.cuda.synchronize()
    ix.close()


@pytest.fixture(scope="module")
def K(index):
    k = index.debug_get(_native.TM_DEBUG_GROUP_TILE)
    assert k >= 64 and k % 64 == 0
    return k


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def _dev(torch, a):
    return torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)]).view(np.int32 if a.itemsize == 4 else np.int64)).cuda()


def _canary32(torch, n):
    return torch.from_numpy(np.full(n, CANARY, np.uint32).view(np.int32)).cuda()


def _payload(n, seed=0):
    i = np.arange(n, dtype=np.uint32)
    return (i * np.uint32(2654435761)) ^ np.uint32(0x1234 + seed), i * np.uint32(40503) + np.uint32(7 + seed)


class Run:
    """one tm_group_subs_dev call's device buffers (kept alive until checked)"""

    def __init__(self, torch, ix, sub, T=None, cap=None, gcap=None, perm=True, stream=None, d_head=None, seed=0):
        """T: head[1] (default len(sub)); cap / gcap default to room for everything;
        d_head: a head already on the device (T then says what it will hold)"""
        sub = np.asarray(sub, np.uint32)
        T = len(sub) if T is None else T
        cap = T if cap is None else cap
        W = min(T, cap)
        assert W <= len(sub)
        sub = sub[:W].copy()   # no position at or past W exists
        topic, value = _payload(W, seed)
        head = np.array([12345, T], np.uint64)
        G = len(np.unique(sub))
        gcap = G if gcap is None else gcap
        self.exp = group_ref(head, topic, value, sub, cap, gcap)
        self.torch, self.ins, self.W, self.perm = torch, (topic, value, sub), W, perm
        Gw = min(G, gcap)
        with torch.cuda.stream(stream) if stream is not None else _Null():
            self.d_head = _dev(torch, head) if d_head is None else d_head
            self.d_t, self.d_v, self.d_s = _dev(torch, topic), _dev(torch, value), _dev(torch, sub)
            self.o_ghead = torch.full((2 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.o_goff = torch.full((Gw + 1 + TAIL,), OFFS_CANARY, dtype=torch.int64, device="cuda")
            self.o_gsub = _canary32(torch, Gw + TAIL)
            self.o_t, self.o_v, self.o_s, self.o_p = (_canary32(torch, W + TAIL) for _ in range(4))
            ix.group_subs_dev(self.d_head.data_ptr(), self.d_t.data_ptr(), self.d_v.data_ptr(), self.d_s.data_ptr(), cap,
                              self.o_ghead.data_ptr(), self.o_gsub.data_ptr(), self.o_goff.data_ptr(), gcap,
                              self.o_t.data_ptr(), self.o_v.data_ptr(), self.o_s.data_ptr(),
                              d_out_perm=self.o_p.data_ptr() if perm else None,
                              stream=torch.cuda.current_stream().cuda_stream)

    def check(self, what):
        """exact outputs, sentinels, inputs unmodified -> (G, W)"""
        topic, value, sub = self.ins
        self.torch.cuda.synchronize()
        (G, W), e_t, e_v, e_s, e_p, e_gsub, e_goff = self.exp
        Gw = len(e_gsub)
        ghead = self.o_ghead.cpu().numpy()
        print(f"{what}: W={W} G={G} Gw={Gw} ghead={ghead[:2].tolist()}")
        assert ghead[:2].view(np.uint64).tolist() == [G, W], f"{what}: ghead is {ghead[:2].tolist()}, not {[G, W]}"
        assert (ghead[2:] == OFFS_CANARY).all(), f"{what}: wrote past ghead[1]"
        g_goff = self.o_goff.cpu().numpy()
        assert np.array_equal(g_goff[:Gw + 1].view(np.uint64), e_goff), f"{what}: group offsets differ"
        assert (g_goff[Gw + 1:] == OFFS_CANARY).all(), f"{what}: wrote past out_goff[Gw]"
        g_gsub = self.o_gsub.cpu().numpy().view(np.uint32)
        assert np.array_equal(g_gsub[:Gw], e_gsub), f"{what}: group subscribers differ"
        assert (g_gsub[Gw:] == CANARY).all(), f"{what}: wrote at or past Gw in out_gsub"
        g_t, g_v, g_s, g_p = (x.cpu().numpy().view(np.uint32) for x in (self.o_t, self.o_v, self.o_s, self.o_p))
        bad = np.nonzero((g_t[:W] != e_t) | (g_v[:W] != e_v) | (g_s[:W] != e_s))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {W} grouped deliveries differ, first at {bad[0]}"
        if self.perm:
            assert np.array_equal(g_p[:W], e_p), f"{what}: the permutation differs"
            if Gw == G and W:   # stability, stated on its own: positions strictly increase inside every group
                up = np.diff(g_p[:W].astype(np.int64)) > 0
                up[e_goff[1:-1].astype(np.int64) - 1] = True   # (between two groups anything goes)
                assert up.all(), f"{what}: a group is not in input order"
        else:
            assert (g_p == CANARY).all(), f"{what}: out_perm was NULL"
        for g in (g_t, g_v, g_s) + ((g_p,) if self.perm else ()):
            assert (g[W:] == CANARY).all(), f"{what}: wrote at or past W"
        assert np.array_equal(self.d_t.cpu().numpy().view(np.uint32)[:-1], topic), f"{what}: the topics were written"
        assert np.array_equal(self.d_v.cpu().numpy().view(np.uint32)[:-1], value), f"{what}: the values were written"
        assert np.array_equal(self.d_s.cpu().numpy().view(np.uint32)[:-1], sub), f"{what}: the subscribers were written"
        return G, W


def _passes(ix):
    return ix.debug_get(_native.TM_DEBUG_GROUP_PASSES_RUN), ix.debug_get(_native.TM_DEBUG_GROUP_PASSES_SKIPPED)


# ---------------------------------------------------------------- the key sets

def _keysets(n, seed=3):
    """name -> n keys (u32)"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.uint64)
    sets = {
        "all equal": np.full(n, 0xDEADBEEF, np.uint64),
        "ascending distinct": i * 3 + 5,
        "descending distinct": (n - i) * 7 + 1,
        "two ids alternating": np.where(i % 2 == 0, 0x80000001, 0x00000100),
        "0 and 0xFFFFFFFF": rng.choice(np.array([0, 0xFFFFFFFF, 17], np.uint64), n),
        "one id holding 90 %": np.where(rng.random(n) < 0.9, np.uint64(424242), rng.integers(0, 1 << 32, n, dtype=np.uint64)),
        "random below 2^8": rng.integers(0, 1 << 8, n, dtype=np.uint64),
        "random below 2^16": rng.integers(0, 1 << 16, n, dtype=np.uint64),
        "random below 2^32": rng.integers(0, 1 << 32, n, dtype=np.uint64),
    }
    for b in range(4):   # ids that differ in exactly byte b
        sets[f"one byte differs: byte {b}"] = np.uint64(0x5A5A5A5A & ~(0xFF << (8 * b))) | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * b))
    return {k: v.astype(np.uint32) for k, v in sets.items()}


SETS = sorted(_keysets(1))


@pytest.mark.parametrize("name", SETS)
def test_key_sets(torch_dev, index, K, name):
    """every key set at 5 K + 17 deliveries: six blocks with keys, the last one's tile ragged"""
    n = 5 * K + 17
    Run(torch_dev, index, _keysets(n)[name]).check(name)


@pytest.mark.parametrize("size", ["0", "1", "2", "63", "64", "65", "K-1", "K", "K+1", "2K+1"])
def test_sizes(torch_dev, index, K, size):
    W = {"K-1": K - 1, "K": K, "K+1": K + 1, "2K+1": 2 * K + 1}[size] if "K" in size else int(size)
    for name in ("random below 2^32", "two ids alternating", "random below 2^8", "0 and 0xFFFFFFFF"):
        Run(torch_dev, index, _keysets(W, seed=W)[name]).check(f"W={size} {name}")


def test_a_million_deliveries_every_block_owns_several_tiles(torch_dev, index, K):
    B = index.debug_get(_native.TM_DEBUG_GROUP_GRID)
    n = B * K + (B * K) // 4 + 77          # 1.3M: chunks of two tiles, the last block's ragged
    assert (n + B - 1) // B > K and n < 1_500_000
    for name in ("random below 2^32", "random below 2^16", "two ids alternating"):
        Run(torch_dev, index, _keysets(n, seed=9)[name]).check(f"1M {name}")


def test_dense_ids_skip_passes_with_identical_results(torch_dev, index, K):
    """the counters' differences around one call each; the results are checked against the same definition"""
    n = 3 * K + 5
    for name, run, skipped in (("random below 2^8", 1, 3), ("random below 2^16", 2, 2), ("random below 2^32", 4, 0),
                               ("all equal", 0, 4), ("one byte differs: byte 2", 1, 3)):
        torch_dev.cuda.synchronize()
        r0, s0 = _passes(index)
        Run(torch_dev, index, _keysets(n)[name]).check(name)
        r1, s1 = _passes(index)
        print(f"{name}: passes run {r1 - r0}, skipped {s1 - s0}")
        assert (r1 - r0, s1 - s0) == (run, skipped), f"{name}: ran {r1 - r0} and skipped {s1 - s0} passes"


def test_cap_below_T_and_cap_zero(torch_dev, index, K):
    sub = _keysets(2 * K + 100)["random below 2^16"]
    Run(torch_dev, index, sub, T=len(sub), cap=K + 3).check("cap < T")
    Run(torch_dev, index, sub, T=len(sub) + 1000, cap=len(sub)).check("cap < T, every input position used")
    Run(torch_dev, index, sub, T=len(sub), cap=0).check("cap = 0")
    Run(torch_dev, index, sub, T=5, cap=len(sub)).check("T < cap")


def test_gcap_below_G_and_gcap_zero(torch_dev, index, K):
    sub = _keysets(2 * K + 100)["random below 2^16"]
    G = len(np.unique(sub))
    for gcap in (G - 1, G // 2, 1, 0):
        g, w = Run(torch_dev, index, sub, gcap=gcap).check(f"gcap = {gcap} < G = {G}")
        assert (g, w) == (G, len(sub))
    Run(torch_dev, index, sub, gcap=G + 50).check("gcap > G")


def test_out_perm_null(torch_dev, index, K):
    Run(torch_dev, index, _keysets(K + 9)["random below 2^32"], perm=False).check("out_perm NULL")


def test_chained_behind_dispatch_dev_without_a_synchronisation(torch_dev, index, K):
    """tm_dispatch_dev and tm_group_subs_dev queued back to back on one stream; the head stays on the device"""
    torch = torch_dev
    rng = np.random.default_rng(5)
    n_vals, M = 50, 700
    lengths = rng.integers(0, 9, n_vals)
    lengths[7] = 2 * K + 3                     # one broadcast list
    span = np.zeros(2 * n_vals, np.uint32)
    span[1::2] = lengths
    span[0::2] = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    pool = rng.integers(0, 40, int(lengths.sum()), dtype=np.uint64).astype(np.uint32)   # few pids: fan-in
    t = np.sort(rng.integers(0, 64, M)).astype(np.uint32)
    v = rng.integers(0, n_vals, M).astype(np.uint32)
    doff = np.array([0, M, M], np.uint64)
    e_sub = np.concatenate([pool[span[2 * x]: span[2 * x] + span[2 * x + 1]] for x in v] + [np.zeros(0, np.uint32)])
    e_t, e_v = np.repeat(t, lengths[v]), np.repeat(v, lengths[v])
    T = len(e_sub)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = [_dev(torch, a) for a in (doff, t, v, span, pool)]
        head = torch.full((2,), OFFS_CANARY, dtype=torch.int64, device="cuda")
        dt, dv, ds = (_canary32(torch, T + 1) for _ in range(3))
        ghead = torch.full((2,), OFFS_CANARY, dtype=torch.int64, device="cuda")
        goff = torch.full((41,), OFFS_CANARY, dtype=torch.int64, device="cuda")
        gsub, ot, ov, os_, op = (_canary32(torch, n) for n in (40, T, T, T, T))
        index.dispatch_dev(1, d[0].data_ptr(), 0, d[1].data_ptr(), d[2].data_ptr(), M, head.data_ptr(), dt.data_ptr(),
                           dv.data_ptr(), ds.data_ptr(), T, d_sub_span=d[3].data_ptr(), span_len=n_vals,
                           d_sub_pool=d[4].data_ptr(), pool_len=len(pool), stream=s.cuda_stream)
        index.group_subs_dev(head.data_ptr(), dt.data_ptr(), dv.data_ptr(), ds.data_ptr(), T, ghead.data_ptr(),
                             gsub.data_ptr(), goff.data_ptr(), 40, ot.data_ptr(), ov.data_ptr(), os_.data_ptr(),
                             d_out_perm=op.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert head.cpu().numpy().view(np.uint64).tolist() == [M, T]
    (G, W), x_t, x_v, x_s, x_p, x_gsub, x_goff = group_ref([M, T], e_t, e_v, e_sub, T, 40)
    assert ghead.cpu().numpy().view(np.uint64).tolist() == [G, W] and W == T
    for got, want in ((ot, x_t), (ov, x_v), (os_, x_s), (op, x_p), (gsub, x_gsub)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32)[:len(want)], want)
    assert np.array_equal(goff.cpu().numpy().view(np.uint64)[:G + 1], x_goff)


def test_two_streams_at_once_each_with_its_own_scratch(torch_dev, index, K):
    torch = torch_dev
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    n = 40 * K + 11
    runs = []
    for rep in range(3):
        runs.append((Run(torch, index, _keysets(n, seed=rep)["random below 2^32"], stream=s1, seed=rep), f"stream 1 #{rep}"))
        runs.append((Run(torch, index, _keysets(n + 5, seed=50 + rep)["random below 2^16"], stream=s2, seed=rep),
                     f"stream 2 #{rep}"))
    for r, what in runs:
        r.check(what)
    for s in (s1, s2):
        index.release_stream(s.cuda_stream)


def test_scratch_reuse_small_large_small(torch_dev, index, K):
    s = torch_dev.cuda.Stream()
    for n in (100, 70 * K + 3, 100, 2 * K, 0, 7):
        Run(torch_dev, index, _keysets(n, seed=n)["random below 2^32"], stream=s).check(f"scratch reuse, W = {n}")
    index.release_stream(s.cuda_stream)


def test_refusals_name_the_entry_point(torch_dev, index):
    """one row per TM_EINVAL cause; nothing is queued (the sentinels stay)"""
    torch = torch_dev
    lib = _native.load_library()
    a32 = [_canary32(torch, 16) for _ in range(7)]
    a64 = [torch.full((8,), OFFS_CANARY, dtype=torch.int64, device="cuda") for _ in range(3)]
    P32, P64 = [a.data_ptr() for a in a32], [a.data_ptr() for a in a64]
    #        head    topic   value   sub     cap ghead   gsub    goff  gcap out_t   out_v   out_s   perm
    good = [P64[0], P32[0], P32[1], P32[2], 4, P64[1], P32[3], P64[2], 4, P32[4], P32[5], P32[6], None]
    rows = [("null d_head", 0, None), ("null d_topic with cap > 0", 1, None), ("null d_value with cap > 0", 2, None),
            ("null d_sub with cap > 0", 3, None), ("null d_out_ghead", 5, None), ("null d_out_gsub with gcap > 0", 6, None),
            ("null d_out_goff", 7, None), ("null d_out_topic with cap > 0", 9, None),
            ("null d_out_value with cap > 0", 10, None), ("null d_out_sub with cap > 0", 11, None),
            ("d_head not 8-byte aligned", 0, P64[0] + 4), ("d_out_ghead not 8-byte aligned", 5, P64[1] + 4),
            ("d_out_goff not 8-byte aligned", 7, P64[2] + 4)]
    for what, at, bad in rows:
        args = list(good)
        args[at] = bad
        with pytest.raises(_native.TmError) as e:
            index.group_subs_dev(*args[:12], d_out_perm=args[12], stream=torch.cuda.current_stream().cuda_stream)
        assert e.value.code == _native.TM_EINVAL and "tm_group_subs_dev" in str(e.value), f"{what}: {e.value}"
    assert lib.tm_group_subs_dev(None, *good, None) == _native.TM_EINVAL   # a null handle
    assert b"tm_group_subs_dev" in lib.tm_last_error(None)
    torch.cuda.synchronize()
    for a in a32:
        assert (a.cpu().numpy().view(np.uint32) == CANARY).all()
    for a in a64:
        assert (a.cpu().numpy() == OFFS_CANARY).all()
    # the null pointers that are allowed: no arrays with cap == 0, no out_gsub with gcap == 0
    index.group_subs_dev(P64[0], None, None, None, 0, P64[1], None, P64[2], 0, None, None, None,
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert a64[1].cpu().numpy()[:2].tolist() == [0, 0] and a64[2].cpu().numpy()[0] == 0
