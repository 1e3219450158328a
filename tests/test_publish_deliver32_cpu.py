"""tm_publish_deliver_batch32 without a device: the export, the ABI minor, the
debug keys and the ctypes signature against the header, the header's contract
lines, every argument check that needs no GPU, Tab.publish_deliver_kids32 over
a stub index, the Router's route_in_place choice over the stub mirror of
tests/test_publish_deliver_cpu.py, and the NIF core's publish-deliver half
(c_src/tmatch_nif_publish_deliver.c) against the stand-in libtmatch
(tests/native/fake_tmatch*.c with fake_tmatch_publish_deliver.c): slices,
picks, merged and grouped deliveries, one rerun per kind of TM_ECAP with the
stand-in's state moved once, err 4 -> TM_EDEVICE, buffers released with the
set.

The same cases, with tmn_give and the pool's destruction, run once more in a
stand-alone C program (tests/native/nif_publish_deliver_check.c) built with
-fsanitize=address,undefined and started as a subprocess; nothing sanitised is
loaded into Python.
"""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from emqx_amd import _native
from emqx_amd.broker import Broker, Message
from group_picks_ref import NONE, group_picks_ref
from test_publish_deliver_cpu import KC, KT, TOPICS, PublishMirror, _host_grouping
from test_publish_deliver_cpu import _world as _staged_world

ROOT = Path(__file__).resolve().parent.parent
TM_OK, TM_EINVAL, TM_EDEVICE, TM_ECAP = 0, -1, -3, -4
NATIVE = ROOT / "tests" / "native"
SOURCES = [ROOT / "c_src" / f"tmatch_nif_{u}.c" for u in ("core", "route", "dispatch", "share", "deliver", "publish_deliver")]
SOURCES += [NATIVE / f"fake_tmatch{u}.c" for u in ("", "_route", "_dispatch", "_share", "_deliver", "_publish_deliver")]


def test_export_abi_minor_and_debug_keys():
    lib = _native.load_library()
    assert "tm_publish_deliver_batch32" in _native.EXPORTS and hasattr(lib, "tm_publish_deliver_batch32")
    v = lib.tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 23
    keys = (("TM_DEBUG_GP1_MAX", 44), ("TM_DEBUG_PUBLISH_DELIVER_ONE", 45), ("TM_DEBUG_PUBLISH_DELIVER_GRID", 46))
    header = (ROOT / "include" / "tmatch.h").read_text()
    for name, key in keys:
        assert getattr(_native, name) == key and f"{name} = {key}" in header
    assert hasattr(_native.Index, "publish_deliver_batch32")
    from emqx_amd.topic_index import Tab
    assert hasattr(Tab, "publish_deliver_kids32")
    dev = (ROOT / "emqx_amd" / "csrc" / "tm_dev.h").read_text()
    assert f"GP1_DELIVERIES = {_native.GP1_DELIVERIES};" in dev and _native.GP1_DELIVERIES == 8192


def test_the_ctypes_signature_is_the_headers_prototype():
    header = (ROOT / "include" / "tmatch.h").read_text()
    protos = {}
    for name in ("tm_publish_deliver_batch32", "tm_publish_deliver_batch"):
        m = re.search(r"int %s\((.*?)\);" % name, header, re.S)
        assert m, "the prototype is in the header"
        protos[name] = [" ".join(p.split()) for p in m.group(1).split(",")]
    params = protos["tm_publish_deliver_batch32"]
    kinds = {"tm_index *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}

    def ctype(p):
        return C.c_void_p if "*" in p else kinds[p.replace("const ", "").rsplit(" ", 1)[0]]
    lib = _native.load_library()
    assert lib.tm_publish_deliver_batch32.restype == C.c_int32
    assert list(lib.tm_publish_deliver_batch32.argtypes) == [ctype(p) for p in params] and len(params) == 25
    # tm_publish_deliver_batch's prototype with exactly three changes
    wide = protos["tm_publish_deliver_batch"]
    changed = [(a, b) for a, b in zip(wide, params) if a != b]
    assert changed == [("const uint64_t *topic_offsets", "const uint32_t *topic_offsets"),
                       ("uint64_t *out_dest_offsets", "uint32_t *out_dest_offsets"), ("uint64_t *out_goff", "uint32_t *out_goff")]
    assert "uint64_t *out_ghead" in params and "uint64_t *out_head" in params


def test_null_handle_is_einval():
    lib = _native.load_library()
    offs = (C.c_uint32 * 2)(0, 1)
    doff = (C.c_uint32 * 3)()
    head, ghead = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    goff = (C.c_uint32 * 1)()
    err = (C.c_uint8 * 1)()
    assert lib.tm_publish_deliver_batch32(None, 1, b"a" * 16, offs, 1, 0, _native.TM_ROUTE_AGGRE, doff, None, None, 0, head,
                                          None, None, None, 0, None, None, 0, None, ghead, None, goff, 0, err) == TM_EINVAL


def test_the_header_states_the_contract():
    header = " ".join((ROOT / "include" / "tmatch.h").read_text().replace(" * ", " ").split())
    m = re.search(r"/\* tm_publish_deliver_batch32 \(ABI minor 23\)(.*?)\*/ int tm_publish_deliver_batch32", header)
    assert m, "the call's comment stands above its prototype"
    text = m.group(1)
    for line in ("the return code, every route output, out_head = [M, T], out_member[0 .. K)",
                 "and the state words afterwards are tm_publish_deliver_batch's",
                 "out_goff narrowed to u32 (gcap + 1 words",
                 "out_head and out_ghead stay u64[2] and must be 8-byte aligned",
                 "Nothing is written at or past min(total, cap)", "K in out_member", "min(N, dcap) in the three delivery arrays",
                 "min(G, gcap) in out_gsub", "nor past out_goff[min(G, gcap)]",
                 "total > cap no pick, no state", "T + K > dcap no pick, no state", "out_ghead = [0, 0]",
                 "G > gcap alone the picks stand and the state has moved once",
                 "whatever tm_publish_batch32 refuses, a null out_ghead or out_goff, a null out_gsub with gcap > 0, a "
                 "misaligned out_ghead",
                 "one synchronisation", "it is the run's own snapshot, which is stricter than",
                 "never looser", "at most 8192 merged deliveries", "never a second walk",
                 "does everything or moves nothing"):
        assert line in text, line


def test_the_wrapper_refuses_wrong_buffers_before_any_call():
    """Index.publish_deliver_batch32's own checks raise before the library (or a device) is touched"""
    ix = _native.Index.__new__(_native.Index)                    # (no handle: nothing below reaches the library)
    u32, u8, u64 = (lambda k: np.zeros(k, np.uint32)), (lambda k: np.zeros(k, np.uint8)), (lambda k: np.zeros(k, np.uint64))
    blob, offs = u8(16), np.array([0, 1], np.uint32)
    good = lambda: (u32(3), u32(8), u32(8), u8(1), u64(2), u32(8), u32(8), u32(8), u64(2), u32(8), u32(9))
    call = ix.publish_deliver_batch32
    bad = [
        lambda: call(blob, offs.astype(np.uint64), 1, 0, good(), u32(8)),                        # u64 topic offsets
        lambda: call(blob, offs, 1, 0, good()[:8], u32(8)),                                      # no group arrays
        lambda: call(blob, offs, 1, 0, good()[:8] + (u32(2), u32(8), u32(9)), u32(8)),           # a u32 group head
        lambda: call(blob, offs, 1, 0, good()[:9] + (u32(8), u64(9)), u32(8)),                   # u64 group offsets
        lambda: call(blob, offs, 1, 0, good()[:9] + (u64(8), u32(9)), u32(8)),                   # u64 subscribers
        lambda: call(blob, offs, 1, 0, good()[:10] + (u32(0),), u32(8)),                         # no room for entry 0
        lambda: call(blob, offs, 1, 0, good(), u32(8), gcap=9),                                  # gcap beyond gsub
        lambda: call(blob, offs, 1, 0, good()[:10] + (u32(8),), u32(8), gcap=8),                 # goff holds gcap + 1
        lambda: call(blob, offs, 1, 0, good(), u32(8), dcap=9),                                  # dcap beyond the arrays
        lambda: call(blob, offs, 1, 0, good(), u32(7), cap=8),                                   # cap beyond the members
        lambda: call(blob, offs, 1, 0, good(), u64(8)),                                          # u64 members
        lambda: call(blob, offs, 1, 0, good(), u32(8), key_clientid=u64(1)),                     # u64 key words
        lambda: call(blob, offs, 1, 0, good(), u32(8), key_topic=u32(0)),                        # a key word per topic
        lambda: call(blob, offs, 1, 0, good()[:4] + (u64(1),) + good()[5:], u32(8)),             # a one-word head
        lambda: call(blob, offs, 1, 0, (u32(2),) + good()[1:], u32(8)),                          # n_dests + 2 offsets
    ]
    for c in bad:
        with pytest.raises(ValueError):
            c()


# ---- Tab.publish_deliver_kids32 over a stub index: the pooled buffers, the sizes, the one retry

class StubIndex:
    """host_array is numpy; publish_deliver_batch32 records the capacities it is given and raises TM_ECAP
    until they hold `total` entries and T + total deliveries, writing the sizes the library would"""

    def __init__(self, total, T):
        self.total, self.T, self.log, self.live, self.never = total, T, [], 0, False

    def host_array(self, n, dtype, vram=False):
        self.live += 1
        return np.zeros(max(n, 1), dtype)

    def host_free(self, a):
        self.live -= 1

    def set_member_subs(self, members, subs):
        self.log.append("member_subs")

    def publish_deliver_batch32(self, blob, offs, n_dests, local, out, member, kc=None, kt=None, seed=0):
        doff, topic, vals, err, head, dt, dv, ds, ghead, gsub, goff = out
        cap, dcap, gcap = min(len(topic), len(vals), len(member)), min(len(dt), len(dv), len(ds)), min(len(gsub), len(goff) - 1)
        self.log.append((cap, dcap, gcap, None if kc is None else kc.tolist(), None if kt is None else kt.tolist(), seed))
        assert gcap >= dcap, "room for a group per delivery"
        doff[n_dests + 1], head[1] = self.total, self.T
        if self.never or self.total > cap or self.T + self.total > dcap:
            raise _native.TmError(TM_ECAP, "short")
        N = self.T + 1
        dt[:N], ds[:N], member[: self.total] = 7, 9, 5
        gsub[0], goff[:2] = 9, (0, N)
        return (doff[: n_dests + 2], topic[: self.total], vals[: self.total], err[: len(offs) - 1]), \
            (dt[:N], dv[:N], ds[:N]), member[: self.total], (gsub[:1], goff[:2]), self.T


def test_the_tab_sizes_the_pooled_buffers_and_retries_once():
    from emqx_amd.topic_index import Tab
    ix = StubIndex(total=5000, T=3000)
    t = Tab(index=ix)
    t.set_member_sub(4, 40)
    topics = [b"a/b", b"c"]
    route, (dt, dv, ds), member, (gsub, goff), T = t.publish_deliver_kids32(topics, 2, 1, [1, 2], None, seed=3)
    assert ix.log[0] == "member_subs", "the member-subs table is shipped ahead of the call"
    first, second = ix.log[1], ix.log[2]
    assert len(ix.log) == 3 and first[0] < 5000 and second[0] >= 5000 and second[1] >= 8000 and first[3:] == ([1, 2], None, 3)
    assert T == 3000 and len(dt) == 3001 and len(member) == 5000 and route[0].dtype == np.uint64 and goff.dtype == np.uint64
    assert gsub.tolist() == [9] and goff.tolist() == [0, 3001] and int(route[0][3]) == 5000
    # copies: the buffers are back in the pool, and the next call of the size needs no retry
    dt[:] = 1
    again = t.publish_deliver_kids32(topics, 2, 1, [1, 2], None, seed=3)
    assert len(ix.log) == 4 and (again[1][0] == 7).all()
    ix.never = True
    with pytest.raises(_native.TmError):                         # a call that never fits: one retry, then the error
        t.publish_deliver_kids32(topics, 2, 1)
    assert len(ix.log) == 6
    with pytest.raises(ValueError):
        t.publish_deliver_kids32(topics, 2, 1, [1], None)        # a key word per topic


# ---- the Router's route_in_place choice

class PublishMirror32(PublishMirror):
    """test_publish_deliver_cpu's stub with the in-place call: publish_deliver_kids under another name, recorded"""

    def publish_deliver_kids32(self, topics, n_dests, local, kc=None, kt=None, seed=0):
        out = self.publish_deliver_kids(topics, n_dests, local, kc, kt, seed)
        self.calls[-1] = "publish_deliver32"
        return out

    def route_kids32(self, topics, n_dests, aggre=False):
        return self.route_kids(topics, n_dests, aggre)


def _world(in_place):
    """test_publish_deliver_cpu._world over the mirror with the in-place call"""
    import test_publish_deliver_cpu as base
    saved = base.PublishMirror
    base.PublishMirror = PublishMirror32
    try:
        return base._world(in_place)
    finally:
        base.PublishMirror = saved


def test_the_router_takes_publish_deliver_kids32_when_made_in_place():
    (r1, m1, _, _), (r2, m2, _, _), (r3, m3, _, _) = _staged_world(), _world(False), _world(True)
    for batch in range(3):                                 # the state carries from batch to batch
        e = r1.match_routes_publish_deliver(TOPICS, KC, KT, seed=batch)
        g = r2.match_routes_publish_deliver(TOPICS, KC, KT, seed=batch)
        h = r3.match_routes_publish_deliver(TOPICS, KC, KT, seed=batch)
        assert (m1.calls[-1], m2.calls[-1], m3.calls[-1]) == ("publish_deliver", "publish_deliver", "publish_deliver32")
        for x in (g, h):                                   # what the call returns: unchanged
            assert dict(x[0]) == dict(e[0]) and x[1] == e[1] and x[2] == e[2] and x[3] == e[3]
        assert h[3] == _host_grouping(r1, e[1], e[2]) and len(e[1]) > 20
        assert m1.state == m3.state
    # a mirror without the in-place call keeps the staged one
    r4, m4, _, _ = _staged_world(True)
    r4.match_routes_publish_deliver(TOPICS, KC, KT)
    assert m4.calls[-1] == "publish_deliver"


def test_the_broker_gets_the_in_place_call_through_the_router():
    r, m, _, _ = _world(True)
    msgs = [Message(t, n) for n, t in enumerate(TOPICS)]
    log = []
    b = Broker(r, share_on_device=True, share_grouped=True, share_send=lambda p, to, mm: "ok", share_seed=3,
               share_keys=lambda mm: (KC[mm.payload], KT[mm.payload]), share_dispatch=lambda g, to, mm: 1 / 0,
               deliver=lambda p, to, mm: log.append(p), deliver_batch=lambda p, items: log.append(p))
    b.publish_batch_by_dest(msgs)
    assert "publish_deliver32" in m.calls and len(log) == len(set(log)) > 3
    assert Broker(r).share_grouped is False                # the defaults stay off


# ---- the NIF half against the stand-in libtmatch

@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("nifpd") / "libnifpd.so"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out)] + [str(s) for s in SOURCES],
                   check=True)
    lib = C.CDLL(str(out))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    p32, p64 = C.POINTER(u32), C.POINTER(u64)
    lib.fake_pool_new.restype = vp
    lib.fake_pool_free.argtypes = [vp]
    lib.fake_count.restype = C.c_long
    lib.tmn_take.restype = vp
    lib.tmn_take.argtypes = [vp]
    lib.tmn_give.argtypes = [vp, vp]
    lib.tmn_pack.argtypes = [vp, vp, u32, vp, vp]
    lib.tmn_share_keys.argtypes = [vp, vp, u32, vp, vp]
    lib.tmn_publish.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_publish_deliver.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_route_dest.argtypes = [vp, u32, p64, p64]
    lib.tmn_deliveries.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), C.POINTER(p32), p64]
    lib.tmn_groups.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), p64]
    lib.tmn_picks.argtypes = [vp, C.POINTER(p32), p64]
    for f in (lib.fake_set_vals, lib.fake_set_route_topics):
        f.argtypes, f.restype = [vp], p32
    for f in (lib.fake_set_reruns, lib.fake_pd_direct, lib.fake_pd_group_room, lib.fake_set_delivery_cap):
        f.argtypes, f.restype = [vp], u64
    lib.fake_pd_count.restype = lib.fake_pd_moves.restype = C.c_long
    for f in (lib.fake_pd_cap, lib.fake_pd_dcap, lib.fake_pd_gcap):
        f.argtypes, f.restype = [C.c_long], u64
    lib.fake_dispatch_mult.argtypes = [u32]
    lib.fake_pd_direct_sub.argtypes, lib.fake_pd_direct_sub.restype = [u32, u32], u32
    lib.fake_pd_member.argtypes, lib.fake_pd_member.restype = [u32, u32, u32, u32, C.c_long], u32
    lib.fake_pd_local.argtypes, lib.fake_pd_local.restype = [u32], u32
    yield lib
    lib.fake_dispatch_mult(1)


H = C.c_void_p(1)


def pack(lib, s, topics):
    arr = (C.c_char_p * len(topics))(*topics)
    lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
    return lib.tmn_pack(s, H, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))


def keys(lib, s, n, kc, kt):
    a = None if kc is None else (C.c_uint32 * n)(*kc)
    b = None if kt is None else (C.c_uint32 * n)(*kt)
    return lib.tmn_share_keys(s, H, n, a, b)


def results(lib, s, n_dests):
    """-> (slices [(topic, value)] per destination, (rc, deliveries), (rc, members), (rc, subscribers, offsets))"""
    vals, tops = lib.fake_set_vals(s), lib.fake_set_route_topics(s)
    out = []
    for d in range(n_dests + 1):
        b, e = C.c_uint64(), C.c_uint64()
        assert lib.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
        out.append([(tops[k], vals[k]) for k in range(b.value, e.value)])
    t, v, ds = (C.POINTER(C.c_uint32)() for _ in range(3))
    dc = C.c_uint64(99)
    rc = lib.tmn_deliveries(s, C.byref(t), C.byref(v), C.byref(ds), C.byref(dc))
    mem, mc = C.POINTER(C.c_uint32)(), C.c_uint64(99)
    prc = lib.tmn_picks(s, C.byref(mem), C.byref(mc))
    gs, go, gc = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64(99)
    grc = lib.tmn_groups(s, C.byref(gs), C.byref(go), C.byref(gc))
    return out, (rc, [(t[k], v[k], ds[k]) for k in range(dc.value)]), (prc, mem[:mc.value] if prc == 0 else []), \
        (grc, gs[:gc.value] if grc == 0 else [], go[:gc.value + 1] if grc == 0 else [])


def expected(lib, topics, n_dests, local, kc, kt, seed, moves, mult=1):
    """the fakes' rules: value 1000 i + k per byte, bucket v % (n_dests + 1); ((v % 1000) % 7) * mult direct
    deliveries, delivery r to fake_pd_direct_sub(v, r); the pick of an entry none when v % 5 == 0, else
    fake_pd_member; the header's definition (group_picks_ref) over them with sub_of = fake_pd_local"""
    out = [[] for _ in range(n_dests + 1)]
    for i, t in enumerate(topics):
        if t[:1] == b"+":
            continue
        for k in range(len(t)):
            out[(1000 * i + k) % (n_dests + 1)].append((i, 1000 * i + k))
    entries = [e for bucket in out for e in bucket]
    dl = [(i, v, lib.fake_pd_direct_sub(v, r)) for i, v in out[local] for r in range((v % 1000) % 7 * mult)]
    member = [NONE if v % 5 == 0 else lib.fake_pd_member(v, kc[i] if kc else 0, kt[i] if kt else 0, seed, moves)
              for i, v in entries]
    ids = sorted(set(m for m in member if m != NONE))
    dense = {m: j for j, m in enumerate(ids)}                    # (member ids reach 2^31: a dense table of them)
    sub_of = np.array([lib.fake_pd_local(m) for m in ids], np.uint32)
    T, K = len(dl), len(entries)
    doff = np.zeros(n_dests + 2, np.uint64)
    doff[-1] = K
    (G, N), g_t, g_v, g_s, _, gsub, goff, _, P = group_picks_ref(
        [0, T], [d[0] for d in dl], [d[1] for d in dl], [d[2] for d in dl], T, n_dests, doff, [e[0] for e in entries],
        [e[1] for e in entries], [dense.get(m, NONE) for m in member], K, sub_of, T + K, T + K)
    return out, list(zip(g_t.tolist(), g_v.tolist(), g_s.tolist())), member, gsub.tolist(), goff.tolist(), T, P


def test_slices_picks_and_merged_grouped_deliveries(core):
    core.fake_dispatch_mult(1)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    topics = [b"abcde", b"+x", b"", b"xyz", b"0123456789"]
    n = len(topics)
    assert pack(core, s, topics) == TM_OK
    assert results(core, s, -1)[1:] == ((TM_EINVAL, []), (TM_EINVAL, []), (TM_EINVAL, [], []))    # nothing yet
    for local, kc, kt in ((0, None, None), (1, [11, 22, 33, 44, 55], [5, 4, 3, 2, 1]), (2, [9, 8, 7, 6, 5], None)):
        assert keys(core, s, n, kc, kt) == TM_OK
        c0 = core.fake_pd_count()
        assert core.tmn_publish_deliver(s, H, n, 3, local, 40 + local) == TM_OK
        assert core.fake_pd_count() - c0 == 1 and core.fake_set_reruns(s) == 0
        exp, exp_dl, exp_m, exp_gs, exp_go, T, P = expected(core, topics, 3, local, kc, kt, 40 + local,
                                                            core.fake_pd_moves() - 1)
        got, dl, picks, groups = results(core, s, 3)
        assert got == exp and dl == (0, exp_dl) and picks == (0, exp_m) and groups == (0, exp_gs, exp_go)
        assert core.fake_pd_direct(s) == T and len(exp_dl) == T + P and P > 0 and T > 0
        assert 1 < len(exp_gs) < len(exp_dl), "subscribers with several deliveries"
        assert core.fake_pd_gcap(c0) == core.fake_pd_dcap(c0) <= core.fake_pd_group_room(s), "a group per delivery slot"
    assert core.tmn_publish_deliver(s, H, n - 1, 3, 0, 0) == TM_EINVAL                # the keys are for n topics
    assert core.tmn_publish_deliver(s, H, n, 3, 3, 0) == TM_EINVAL                    # local_dest >= n_dests
    assert results(core, s, -1)[1:] == ((TM_EINVAL, []), (TM_EINVAL, []), (TM_EINVAL, [], []))
    # a plain tmn_publish on the same set: picks, no groups; then merged and grouped again
    assert core.tmn_publish(s, H, n, 3, 1, 0) == TM_OK
    got, dl, picks, groups = results(core, s, 3)
    assert dl[0] == 0 and picks[0] == 0 and groups[0] == TM_EINVAL and core.fake_pd_direct(s) == 0
    assert core.tmn_publish_deliver(s, H, n, 3, 1, 0) == TM_OK and results(core, s, 3)[3][0] == 0
    core.tmn_give(pool, s)
    a0, f0 = core.fake_count(0), core.fake_count(1)
    core.fake_pool_free(pool)
    # blob, offs, vals, err, rdoff, rtopic, dhead, dtopic, dvalue, dsub, skc, skt, smember, ghead, gsub, goff
    assert core.fake_count(1) - f0 >= 16
    assert core.fake_count(0) == a0 == core.fake_count(1), "buffers released with the set"


@pytest.mark.parametrize("kind", ["cap", "dcap", "both"])
def test_ecap_reruns_once_per_kind_and_the_state_moves_once(core, kind):
    """total > cap: ONE rerun with room for out_dest_offsets[n_dests + 1] entries; T + K > dcap: ONE rerun
    with room for out_head[1] + out_dest_offsets[n_dests + 1] deliveries and as many groups; both: one after
    the other (K is exact only once the entries fit).  No call under TM_ECAP picked: the stand-in's state
    has moved once when tmn_publish_deliver returns"""
    topics = [b"abcdefg", b"hijklmn"] if kind == "dcap" else [b"x" * 3000, b"y" * 200]
    mult = {"cap": 1, "dcap": 400, "both": 3}[kind]
    n_dests, local = {"cap": (15, 2), "dcap": (1, 0), "both": (1, 0)}[kind]
    core.fake_dispatch_mult(mult)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    assert pack(core, s, topics) == TM_OK
    c0, m0 = core.fake_pd_count(), core.fake_pd_moves()
    assert core.tmn_publish_deliver(s, H, 2, n_dests, local, 5) == TM_OK
    calls = core.fake_pd_count() - c0
    assert calls == (3 if kind == "both" else 2) and core.fake_set_reruns(s) == calls - 1
    assert core.fake_pd_moves() - m0 == 1, "a call that had to be repeated moved the state"
    exp, exp_dl, exp_m, exp_gs, exp_go, T, P = expected(core, topics, n_dests, local, None, None, 5, m0, mult)
    K = sum(map(len, exp))
    caps = [core.fake_pd_cap(c0 + k) for k in range(calls)]
    dcaps = [core.fake_pd_dcap(c0 + k) for k in range(calls)]
    gcaps = [core.fake_pd_gcap(c0 + k) for k in range(calls)]
    assert gcaps == dcaps, "room for a group per delivery slot in every call"
    assert (caps[0] < K) == (kind != "dcap") and caps[-1] >= K and (dcaps[0] < T + K) == (kind != "cap")
    assert dcaps[-1] >= T + K
    if kind == "cap":
        assert dcaps[1] == dcaps[0] and caps[1] > caps[0]
    if kind == "dcap":
        assert caps[1] == caps[0] and dcaps[1] > dcaps[0]
    if kind == "both":                                           # the entries first, then the deliveries
        assert caps[1] > caps[0] and dcaps[1] == dcaps[0] and caps[2] == caps[1] and dcaps[2] > dcaps[1]
    got, dl, picks, groups = results(core, s, n_dests)
    assert got == exp and dl == (0, exp_dl) and picks == (0, exp_m) and groups == (0, exp_gs, exp_go)
    c0 = core.fake_pd_count()
    assert core.tmn_publish_deliver(s, H, 2, n_dests, local, 5) == TM_OK
    assert core.fake_pd_count() - c0 == 1 and core.fake_set_reruns(s) == calls - 1   # sticky sizes: no rerun
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
    assert core.fake_count(0) == core.fake_count(1)
    core.fake_dispatch_mult(1)


def test_device_failure_is_a_device_error(core):
    core.fake_dispatch_mult(1)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    for topics in ([b"ab", b"!x", b"cd"], [b"ab", b"~x"]):                          # err flag 4; TM_EDEVICE
        assert pack(core, s, topics) == TM_OK
        assert core.tmn_publish_deliver(s, H, len(topics), 2, 0, 0) == TM_EDEVICE
        b, e = C.c_uint64(), C.c_uint64()
        assert core.tmn_route_dest(s, 0, C.byref(b), C.byref(e)) == TM_EINVAL       # no result to slice
        assert results(core, s, -1)[1:] == ((TM_EINVAL, []), (TM_EINVAL, []), (TM_EINVAL, [], []))
    topics = [b"abcdefgh", b"+x"]
    assert pack(core, s, topics) == TM_OK
    assert core.tmn_publish_deliver(s, H, 2, 2, 1, 0) == TM_OK
    exp, exp_dl, exp_m, exp_gs, exp_go, T, P = expected(core, topics, 2, 1, None, None, 0, core.fake_pd_moves() - 1)
    got, dl, picks, groups = results(core, s, 2)
    assert got == exp and dl == (0, exp_dl) and picks == (0, exp_m) and groups == (0, exp_gs, exp_go)
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
    assert core.fake_count(0) == core.fake_count(1)


def test_the_header_contrasts_the_reruns_with_tmn_publish():
    text = " ".join((ROOT / "c_src" / "tmatch_nif_publish_deliver.h").read_text().replace(" * ", " ").split())
    for line in ("NEITHER has moved state", "a round robin advances once",
                 "unlike tmn_publish's rerun for the deliveries alone", "picks twice",
                 "G > gcap cannot occur"):
        assert line in text, line
    doc = (ROOT / "INTEGRATION.md").read_text()
    assert "tmn_publish_deliver" in doc and "tmatch_nif_publish_deliver" in doc


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler (gcc) to build the NIF publish-deliver check")
    exe = tmp_path / "nif_publish_deliver_check"
    b = subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}",
                        "-o", str(exe)] + [str(s) for s in SOURCES] +
                       [str(NATIVE / "nif_publish_deliver_check.c")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok"
