"""tm_deliver_batch32 without a device: the export, the ABI minor, the debug
keys and the ctypes signature against the header, every argument check that
needs no GPU, the Router's route_in_place choice over the stub mirror of
tests/test_aggre_cpu.py, and the NIF core's deliver half
(c_src/tmatch_nif_deliver.c) against the stand-in libtmatch
(tests/native/fake_tmatch.c + fake_tmatch_route.c + fake_tmatch_dispatch.c +
fake_tmatch_deliver.c): slices, groups and grouped deliveries, one rerun per
kind of TM_ECAP, err 4 -> TM_EDEVICE, buffers released with the set.

The same cases, with tmn_give and the pool's destruction, run once more in a
stand-alone C program (tests/native/nif_deliver_check.c) built with
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
from emqx_amd.subscribers import LocalSubs
from group_ref import group_ref
from test_aggre_cpu import MirrorRouter, UnroutedMirror

ROOT = Path(__file__).resolve().parent.parent
TM_OK, TM_EINVAL, TM_EDEVICE, TM_ECAP = 0, -1, -3, -4
SOURCES = [ROOT / "c_src" / "tmatch_nif_core.c", ROOT / "c_src" / "tmatch_nif_route.c",
           ROOT / "c_src" / "tmatch_nif_dispatch.c", ROOT / "c_src" / "tmatch_nif_deliver.c",
           ROOT / "tests" / "native" / "fake_tmatch.c", ROOT / "tests" / "native" / "fake_tmatch_route.c",
           ROOT / "tests" / "native" / "fake_tmatch_dispatch.c", ROOT / "tests" / "native" / "fake_tmatch_deliver.c"]


def test_export_abi_minor_and_debug_keys():
    lib = _native.load_library()
    assert "tm_deliver_batch32" in _native.EXPORTS and hasattr(lib, "tm_deliver_batch32")
    v = lib.tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 21
    assert (_native.TM_DEBUG_DELIVER_ONE, _native.TM_DEBUG_DELIVER_GRID, _native.TM_DEBUG_GS1_MAX) == (41, 42, 43)
    header = (ROOT / "include" / "tmatch.h").read_text()
    for name, key in (("TM_DEBUG_DELIVER_ONE", 41), ("TM_DEBUG_DELIVER_GRID", 42), ("TM_DEBUG_GS1_MAX", 43)):
        assert f"{name} = {key}" in header
    assert hasattr(_native.Index, "deliver_batch32")
    from emqx_amd.topic_index import Tab
    assert hasattr(Tab, "deliver_kids32")
    dev = (ROOT / "emqx_amd" / "csrc" / "tm_dev.h").read_text()
    assert f"GS1_DELIVERIES = {_native.GS1_DELIVERIES};" in dev


def test_the_ctypes_signature_is_the_headers_prototype():
    header = (ROOT / "include" / "tmatch.h").read_text()
    m = re.search(r"int tm_deliver_batch32\((.*?)\);", header, re.S)
    assert m, "the prototype is in the header"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    kinds = {"tm_index *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}

    def ctype(p):
        return C.c_void_p if "*" in p else kinds[p.replace("const ", "").rsplit(" ", 1)[0]]
    lib = _native.load_library()
    assert lib.tm_deliver_batch32.restype == C.c_int32
    assert list(lib.tm_deliver_batch32.argtypes) == [ctype(p) for p in params] and len(params) == 21
    names = [p.rsplit(" ", 1)[1].lstrip("*") for p in params]
    assert names[15:20] == ["dcap", "out_ghead", "out_gsub", "out_goff", "gcap"] and names[20] == "out_err"
    assert "uint32_t *out_goff" in params and "uint64_t *out_ghead" in params and "uint64_t *out_head" in params


def test_null_handle_is_einval():
    lib = _native.load_library()
    offs = (C.c_uint32 * 2)(0, 1)
    doff = (C.c_uint32 * 3)()
    head, ghead = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    goff = (C.c_uint32 * 1)()
    err = (C.c_uint8 * 1)()
    assert lib.tm_deliver_batch32(None, 1, b"a" * 16, offs, 1, 0, 0, doff, None, None, 0, head, None, None, None, 0, ghead,
                                  None, goff, 0, err) == TM_EINVAL


def test_the_wrapper_refuses_wrong_buffers_before_any_call():
    """Index.deliver_batch32's own checks raise before the library (or a device) is touched"""
    ix = _native.Index.__new__(_native.Index)                    # (no handle: nothing below reaches the library)
    u32, u8, u64 = (lambda k: np.zeros(k, np.uint32)), (lambda k: np.zeros(k, np.uint8)), (lambda k: np.zeros(k, np.uint64))
    blob, offs = u8(16), np.array([0, 1], np.uint32)
    good = lambda: (u32(3), u32(8), u32(8), u8(1), u64(2), u32(8), u32(8), u32(8), u64(2), u32(8), u32(9))
    bad = [
        lambda: ix.deliver_batch32(blob, offs.astype(np.uint64), 1, 0, good()),                  # u64 topic offsets
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good()[:8]),                                # no group arrays
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good()[:8] + (u32(2), u32(8), u32(9))),     # a u32 group head
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good()[:9] + (u32(8), u64(9))),             # u64 group offsets
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good()[:9] + (u64(8), u32(9))),             # u64 subscribers
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good()[:10] + (u32(0),)),                   # no room for entry 0
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good(), gcap=9),                            # gcap beyond gsub
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good()[:10] + (u32(8),), gcap=8),           # goff holds gcap + 1
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good(), dcap=9),                            # dcap beyond the arrays
        lambda: ix.deliver_batch32(blob, offs, 1, 0, good()[:4] + (u64(1),) + good()[5:]),       # a one-word head
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()


# ---- the Router's route_in_place choice

class DeliverMirror(UnroutedMirror):
    """test_aggre_cpu's stub with the local dispatch and both deliver calls: the header's definition
    applied to the deliveries; deliver_kids32 is deliver_kids under another name, recorded"""

    def __init__(self, hidden=()):
        super().__init__(hidden)
        self.sub_fn = None
        self.calls = []

    def _deliver(self, topics, n_dests, local, aggre):
        doff, tidx, kids, err = self.route_kids(topics, n_dests, aggre)
        t, k, s = [], [], []
        for q in range(int(doff[local]), int(doff[local + 1])):
            for sub in self.sub_fn(self.order[int(kids[q])]):
                t.append(int(tidx[q])), k.append(int(kids[q])), s.append(sub)
        t, k, s = (np.array(a, dtype=np.uint32) for a in (t, k, s))
        _, g_t, g_k, g_s, _, gsub, goff = group_ref([0, len(s)], t, k, s, len(s), len(s))
        return (doff, tidx, kids, err), (g_t, g_k, g_s), (gsub, goff)

    def deliver_kids(self, topics, n_dests, local, aggre=False):
        self.calls.append("deliver")
        return self._deliver(topics, n_dests, local, aggre)

    def deliver_kids32(self, topics, n_dests, local, aggre=False):
        self.calls.append("deliver32")
        return self._deliver(topics, n_dests, local, aggre)

    def route_kids32(self, topics, n_dests, aggre=False):   # (a Broker with the defaults, over an in-place router)
        return self.route_kids(topics, n_dests, aggre)


def _world(in_place):
    subs = LocalSubs(shards=3, shard_after=4)
    m = DeliverMirror()
    r = MirrorRouter(node="n1", mirror=m, local_subs=subs, route_in_place=in_place)
    for i in range(7):
        subs.subscribe(b"a/+", "p%d" % i)
    for p in ("p1", "p9", "p0"):
        subs.subscribe(b"a/#", p)
    subs.subscribe(b"#", "p1")
    subs.subscribe(b"exact/t", "p1")
    for f, d in ((b"a/+", "n1"), (b"a/+", "n2"), (b"a/#", "n1"), (b"#", "n1"), (b"exact/t", "n1"), (b"exact/t", "n2")):
        r.add_route(f, d)
    return r, m


def test_the_router_takes_deliver_kids32_when_made_in_place():
    topics = [b"exact/t", b"other", b"exact/t"]
    (plain, pm), (inplace, im) = _world(False), _world(True)
    for aggre in (False, True):
        e = plain.match_routes_deliver(topics, aggre=aggre)
        g = inplace.match_routes_deliver(topics, aggre=aggre)
        assert dict(g[0]) == dict(e[0]) and g[1] == e[1] and g[2] == e[2] and len(g[1]) > 10   # what it returns: unchanged
    assert pm.calls == ["deliver"] * 2 and im.calls == ["deliver32"] * 2


def test_the_broker_gets_the_in_place_leg_through_the_router():
    r, m = _world(True)
    msgs = [Message(t, n) for n, t in enumerate([b"exact/t", b"other"])]
    calls = []
    Broker(r, deliver_grouped=True, deliver_batch=lambda p, items: calls.append(p)).publish_batch_by_dest(msgs)
    assert m.calls == ["deliver32"] and len(calls) == len(set(calls)) > 2
    m.calls.clear()
    b = Broker(r)                                  # the defaults stay off
    assert b.deliver_grouped is False
    b.publish_batch_by_dest(msgs)
    assert m.calls == []


# ---- the NIF half against the stand-in libtmatch

@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("nifdeliver") / "libnifdeliver.so"
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
    lib.tmn_dispatch.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_deliver.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_route_dest.argtypes = [vp, u32, p64, p64]
    lib.tmn_deliveries.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), C.POINTER(p32), p64]
    lib.tmn_groups.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), p64]
    for f in (lib.fake_set_vals, lib.fake_set_route_topics):
        f.argtypes, f.restype = [vp], p32
    for f in (lib.fake_set_reruns, lib.fake_set_delivery_cap, lib.fake_set_route_cap, lib.fake_set_group_cap):
        f.argtypes, f.restype = [vp], u64
    lib.fake_deliver_count.restype = C.c_long
    for f in (lib.fake_deliver_cap, lib.fake_deliver_dcap, lib.fake_deliver_gcap):
        f.argtypes, f.restype = [C.c_long], u64
    lib.fake_dispatch_mult.argtypes = [u32]
    lib.fake_deliver_mod.argtypes = [u32]
    lib.fake_deliver_sub.argtypes, lib.fake_deliver_sub.restype = [u32, u32], u32
    yield lib
    lib.fake_dispatch_mult(1)
    lib.fake_deliver_mod(13)


H = C.c_void_p(1)


def pack(lib, s, topics):
    arr = (C.c_char_p * len(topics))(*topics)
    lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
    return lib.tmn_pack(s, H, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))


def results(lib, s, n_dests):
    """-> (slices [(topic, value)] per destination, (rc, deliveries), (rc, subscribers, offsets))"""
    vals, tops = lib.fake_set_vals(s), lib.fake_set_route_topics(s)
    out = []
    for d in range(n_dests + 1):
        b, e = C.c_uint64(), C.c_uint64()
        assert lib.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
        out.append([(tops[k], vals[k]) for k in range(b.value, e.value)])
    t, v, ds = (C.POINTER(C.c_uint32)() for _ in range(3))
    dc = C.c_uint64(99)
    rc = lib.tmn_deliveries(s, C.byref(t), C.byref(v), C.byref(ds), C.byref(dc))
    gs, go, gc = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64(99)
    grc = lib.tmn_groups(s, C.byref(gs), C.byref(go), C.byref(gc))
    return out, (rc, [(t[k], v[k], ds[k]) for k in range(dc.value)]), \
        (grc, gs[:gc.value] if grc == 0 else [], go[:gc.value + 1] if grc == 0 else [])


def expected(lib, topics, n_dests, local, mult=1):
    """the fakes' rules: value 1000 i + k per byte, bucket v % (n_dests + 1); ((v % 1000) % 7) * mult
    deliveries, delivery r to fake_deliver_sub(v, r); the header's definition over them"""
    out = [[] for _ in range(n_dests + 1)]
    for i, t in enumerate(topics):
        if t[:1] == b"+":
            continue
        for k in range(len(t)):
            out[(1000 * i + k) % (n_dests + 1)].append((i, 1000 * i + k))
    dl = [(i, v, lib.fake_deliver_sub(v, r)) for i, v in out[local] for r in range((v % 1000) % 7 * mult)]
    T = len(dl)
    _, g_t, g_v, g_s, _, gsub, goff = group_ref([0, T], [d[0] for d in dl], [d[1] for d in dl], [d[2] for d in dl], T, T)
    return out, list(zip(g_t.tolist(), g_v.tolist(), g_s.tolist())), gsub.tolist(), goff.tolist()


def test_slices_groups_and_grouped_deliveries(core):
    core.fake_dispatch_mult(1)
    core.fake_deliver_mod(13)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    topics = [b"abcde", b"+x", b"", b"xyz", b"0123456789"]
    n = len(topics)
    assert pack(core, s, topics) == TM_OK
    assert results(core, s, -1)[2][0] == TM_EINVAL                                   # nothing delivered yet
    for local in (0, 1, 2):
        c0 = core.fake_deliver_count()
        assert core.tmn_deliver(s, H, n, 3, local, _native.TM_ROUTE_AGGRE if local else 0) == TM_OK
        assert core.fake_deliver_count() - c0 == 1 and core.fake_set_reruns(s) == 0
        exp, exp_dl, exp_gs, exp_go = expected(core, topics, 3, local)
        got, dl, groups = results(core, s, 3)
        assert got == exp and dl == (0, exp_dl) and groups == (0, exp_gs, exp_go)
        assert 1 < len(exp_gs) < len(exp_dl), "subscribers with several deliveries"
    assert core.tmn_deliver(s, H, n, 3, 3, 0) == TM_EINVAL                           # local_dest >= n_dests
    assert results(core, s, -1)[1:] == ((TM_EINVAL, []), (TM_EINVAL, [], []))
    assert core.tmn_deliver(s, H, n, 0, 0, 0) == TM_EINVAL
    # a plain tmn_dispatch on the same set: deliveries, no groups; then grouped again
    assert core.tmn_dispatch(s, H, n, 3, 1, 0) == TM_OK
    got, dl, groups = results(core, s, 3)
    assert dl[0] == 0 and groups[0] == TM_EINVAL
    assert core.tmn_deliver(s, H, n, 3, 1, 0) == TM_OK and results(core, s, 3)[2][0] == 0
    core.tmn_give(pool, s)
    a0, f0 = core.fake_count(0), core.fake_count(1)
    core.fake_pool_free(pool)
    # blob, offs, vals, err, rdoff, rtopic, dhead, dtopic, dvalue, dsub, ghead, gsub, goff
    assert core.fake_count(1) - f0 >= 13
    assert core.fake_count(0) == a0 == core.fake_count(1), "buffers released with the set"


@pytest.mark.parametrize("kind", ["cap", "dcap", "gcap", "all"])
def test_ecap_reruns_once_per_kind(core, kind):
    """ONE rerun with room for out_dest_offsets[n_dests + 1] entries, out_head[1] deliveries and
    out_ghead[0] groups; only what did not fit grows (the groups with the deliveries: a group per
    delivery, since deliveries that did not fit hide groups)"""
    topics = [b"abcdefg", b"hijklmn"] if kind in ("dcap", "gcap") else [b"x" * 3000, b"y" * 200]
    mult = {"cap": 1, "dcap": 200, "gcap": 200, "all": 2}[kind]
    n_dests, local = {"cap": (15, 2), "dcap": (1, 0), "gcap": (1, 0), "all": (4, 2)}[kind]
    core.fake_dispatch_mult(mult)
    core.fake_deliver_mod(13 if kind == "cap" else 0)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    assert pack(core, s, topics) == TM_OK
    before = 0
    if kind == "gcap":   # a plain dispatch grows the delivery buffers first: only the groups are short then
        assert core.tmn_dispatch(s, H, 2, n_dests, local, 0) == TM_OK
        before = core.fake_set_reruns(s)
        assert before == 1
    c0 = core.fake_deliver_count()
    assert core.tmn_deliver(s, H, 2, n_dests, local, 0) == TM_OK
    assert core.fake_deliver_count() - c0 == 2 and core.fake_set_reruns(s) - before == 1
    exp, exp_dl, exp_gs, exp_go = expected(core, topics, n_dests, local, mult)
    total, T, G = sum(map(len, exp)), len(exp_dl), len(exp_gs)
    cap0, cap1 = core.fake_deliver_cap(c0), core.fake_deliver_cap(c0 + 1)
    dcap0, dcap1 = core.fake_deliver_dcap(c0), core.fake_deliver_dcap(c0 + 1)
    gcap0, gcap1 = core.fake_deliver_gcap(c0), core.fake_deliver_gcap(c0 + 1)
    assert (cap0 < total) == (kind in ("cap", "all")) and (dcap0 < T) == (kind in ("dcap", "all"))
    assert (gcap0 < G) == (kind != "cap")
    assert cap1 >= total and dcap1 >= T and gcap1 >= G
    assert (cap1 == cap0) == (kind in ("dcap", "gcap")) and (dcap1 == dcap0) == (kind in ("cap", "gcap"))
    assert (gcap1 == gcap0) == (kind == "cap")
    assert core.fake_set_route_cap(s) >= 4 * total and core.fake_set_delivery_cap(s) >= 4 * T
    assert core.fake_set_group_cap(s) >= 4 * G
    got, dl, groups = results(core, s, n_dests)
    assert got == exp and dl == (0, exp_dl) and groups == (0, exp_gs, exp_go)
    c0 = core.fake_deliver_count()
    assert core.tmn_deliver(s, H, 2, n_dests, local, 0) == TM_OK
    assert core.fake_deliver_count() - c0 == 1 and core.fake_set_reruns(s) - before == 1   # sticky sizes: no rerun
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
    assert core.fake_count(0) == core.fake_count(1)
    core.fake_dispatch_mult(1)
    core.fake_deliver_mod(13)


def test_device_failure_is_a_device_error(core):
    core.fake_dispatch_mult(1)
    core.fake_deliver_mod(13)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    for topics in ([b"ab", b"!x", b"cd"], [b"ab", b"~x"]):                          # err flag 4; TM_EDEVICE
        assert pack(core, s, topics) == TM_OK
        assert core.tmn_deliver(s, H, len(topics), 2, 0, 0) == TM_EDEVICE
        b, e = C.c_uint64(), C.c_uint64()
        assert core.tmn_route_dest(s, 0, C.byref(b), C.byref(e)) == TM_EINVAL       # no result to slice
        assert results(core, s, -1)[1:] == ((TM_EINVAL, []), (TM_EINVAL, [], []))
    topics = [b"abcdefgh", b"+x"]
    assert pack(core, s, topics) == TM_OK
    assert core.tmn_deliver(s, H, 2, 2, 1, 0) == TM_OK
    exp, exp_dl, exp_gs, exp_go = expected(core, topics, 2, 1)
    got, dl, groups = results(core, s, 2)
    assert got == exp and dl == (0, exp_dl) and groups == (0, exp_gs, exp_go)
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
    assert core.fake_count(0) == core.fake_count(1)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler (gcc) to build the NIF deliver check")
    exe = tmp_path / "nif_deliver_check"
    b = subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}",
                        "-o", str(exe)] + [str(s) for s in SOURCES] +
                       [str(ROOT / "tests" / "native" / "nif_deliver_check.c")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok"
