"""tm_publish_batch32 without a device: the export, the ABI minor, the debug
keys, every argument check that needs no GPU, and the NIF core's share half
(c_src/tmatch_nif_share.c) against the stand-in libtmatch
(tests/native/fake_tmatch.c + fake_tmatch_route.c + fake_tmatch_dispatch.c +
fake_tmatch_share.c): slices, picks and deliveries, key words NULL or given
(and living in the set), one rerun per kind of TM_ECAP -- from the entries the
stand-in's state moves once, from the deliveries alone twice, as the header
says -- err 4 -> TM_EDEVICE, buffers released with the set.

The same cases, with tmn_give and the pool's destruction, run once more in a
stand-alone C program (tests/native/nif_share_check.c) built with
-fsanitize=address,undefined and started as a subprocess; nothing sanitised is
loaded into Python.
"""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest

from emqx_amd import _native

ROOT = Path(__file__).resolve().parent.parent
TM_OK, TM_EINVAL, TM_EDEVICE, TM_ECAP = 0, -1, -3, -4
NONE = 0xFFFFFFFF
SOURCES = [ROOT / "c_src" / "tmatch_nif_core.c", ROOT / "c_src" / "tmatch_nif_route.c",
           ROOT / "c_src" / "tmatch_nif_dispatch.c", ROOT / "c_src" / "tmatch_nif_share.c",
           ROOT / "tests" / "native" / "fake_tmatch.c", ROOT / "tests" / "native" / "fake_tmatch_route.c",
           ROOT / "tests" / "native" / "fake_tmatch_dispatch.c", ROOT / "tests" / "native" / "fake_tmatch_share.c"]


def test_export_abi_minor_and_debug_keys():
    lib = _native.load_library()
    assert "tm_publish_batch32" in _native.EXPORTS and hasattr(lib, "tm_publish_batch32")
    v = lib.tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 19
    assert (_native.TM_DEBUG_PUBLISH_ONE, _native.TM_DEBUG_PUBLISH_GRID) == (35, 36)
    header = (ROOT / "include" / "tmatch.h").read_text()
    for name, key in (("TM_DEBUG_PUBLISH_ONE", 35), ("TM_DEBUG_PUBLISH_GRID", 36)):
        assert f"{name} = {key}" in header
    assert "int tm_publish_batch32(" in header
    assert hasattr(_native.Index, "publish_batch32")
    from emqx_amd.topic_index import Tab
    assert hasattr(Tab, "publish_kids32")


def test_null_handle_is_einval():
    lib = _native.load_library()
    offs = (C.c_uint32 * 2)(0, 1)
    doff = (C.c_uint32 * 3)()
    head = (C.c_uint64 * 2)()
    err = (C.c_uint8 * 1)()
    assert lib.tm_publish_batch32(None, 1, b"a" * 16, offs, 1, 0, _native.TM_ROUTE_AGGRE, doff, None, None, 0, head, None,
                                  None, None, 0, None, None, 0, None, err) == TM_EINVAL


def test_the_wrapper_refuses_wrong_buffers_before_any_call():
    """Index.publish_batch32's own checks raise before the library (or a device) is touched"""
    import numpy as np
    ix = _native.Index.__new__(_native.Index)                    # (no handle: nothing below reaches the library)
    u32, u8, u64 = (lambda k: np.zeros(k, np.uint32)), (lambda k: np.zeros(k, np.uint8)), (lambda k: np.zeros(k, np.uint64))
    blob, offs = u8(16), np.array([0, 1], np.uint32)
    good = lambda: (u32(3), u32(8), u32(8), u8(1), u64(2), u32(8), u32(8), u32(8))
    with pytest.raises(ValueError):                              # u64 topic offsets
        ix.publish_batch32(blob, offs.astype(np.uint64), 1, 0, good(), u32(8))
    with pytest.raises(ValueError):                              # a member array of the wrong type
        ix.publish_batch32(blob, offs, 1, 0, good(), u64(8))
    with pytest.raises(ValueError):                              # a key array shorter than the batch
        ix.publish_batch32(blob, np.array([0, 1, 2], np.uint32), 1, 0, good()[:3] + (u8(2),) + good()[4:], u32(8),
                           key_clientid=u32(1))
    with pytest.raises(ValueError):                              # cap beyond the member array
        ix.publish_batch32(blob, offs, 1, 0, good(), u32(4), cap=8)


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("nifshare") / "libnifshare.so"
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
    lib.tmn_match.argtypes = [vp, vp, u32, u32]
    lib.tmn_dispatch.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_publish.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_share_keys.argtypes = [vp, vp, u32, vp, vp]
    lib.tmn_route_dest.argtypes = [vp, u32, p64, p64]
    lib.tmn_deliveries.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), C.POINTER(p32), p64]
    lib.tmn_picks.argtypes = [vp, C.POINTER(p32), p64]
    for f in (lib.fake_set_vals, lib.fake_set_route_topics):
        f.argtypes, f.restype = [vp], p32
    for f in (lib.fake_set_reruns, lib.fake_set_delivery_cap, lib.fake_set_route_cap, lib.fake_set_member_cap):
        f.argtypes, f.restype = [vp], u64
    lib.fake_publish_count.restype = lib.fake_share_moves.restype = C.c_long
    for f in (lib.fake_publish_cap, lib.fake_publish_dcap):
        f.argtypes, f.restype = [C.c_long], u64
    lib.fake_publish_keys.argtypes = [C.c_long]
    lib.fake_set_keys_in_set.argtypes = [vp, C.c_long]
    lib.fake_share_member.argtypes, lib.fake_share_member.restype = [u32, u32, u32, u32, C.c_long], u32
    lib.fake_dispatch_mult.argtypes = [u32]
    yield lib
    lib.fake_dispatch_mult(1)


H = C.c_void_p(1)


def pack(lib, s, topics):
    arr = (C.c_char_p * len(topics))(*topics)
    lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
    return lib.tmn_pack(s, H, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))


def set_keys(lib, s, n, kc, kt):
    a = None if kc is None else (C.c_uint32 * n)(*kc)
    b = None if kt is None else (C.c_uint32 * n)(*kt)
    return lib.tmn_share_keys(s, H, n, a, b)


def results(lib, s, n_dests):
    """-> (slices [(topic, value, member)] per destination, (rc, deliveries), rc of tmn_picks)"""
    vals, tops = lib.fake_set_vals(s), lib.fake_set_route_topics(s)
    m, cnt = C.POINTER(C.c_uint32)(), C.c_uint64(99)
    prc = lib.tmn_picks(s, C.byref(m), C.byref(cnt))
    out, seen = [], 0
    for d in range(n_dests + 1):
        b, e = C.c_uint64(), C.c_uint64()
        assert lib.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
        out.append([(tops[k], vals[k], m[k]) for k in range(b.value, e.value)])
        seen += e.value - b.value
    assert seen == cnt.value, "the picks are aligned with the entry slices"
    t, v, ds = (C.POINTER(C.c_uint32)() for _ in range(3))
    dc = C.c_uint64(99)
    rc = lib.tmn_deliveries(s, C.byref(t), C.byref(v), C.byref(ds), C.byref(dc))
    return out, (rc, [(t[k], v[k], ds[k]) for k in range(dc.value)]), prc


def expected(lib, topics, n_dests, local, kc, kt, seed, mult=1):
    """the fakes' rules: value 1000 i + k per byte, bucket v % (n_dests + 1); ((v % 1000) % 7) * mult
    subscribers; no pick for v % 5 == 0, else fake_share_member with the state of the call that stands"""
    moves = lib.fake_share_moves() - 1
    out = [[] for _ in range(n_dests + 1)]
    for i, t in enumerate(topics):
        if t[:1] == b"+":
            continue
        for k in range(len(t)):
            v = 1000 * i + k
            m = NONE if v % 5 == 0 else lib.fake_share_member(v, kc[i] if kc else 0, kt[i] if kt else 0, seed, moves)
            out[v % (n_dests + 1)].append((i, v, m))
    dl = [(i, v, v * 16 + r) for i, v, _ in out[local] for r in range((v % 1000) % 7 * mult)]
    return out, dl


def test_slices_picks_deliveries_and_key_words(core):
    core.fake_dispatch_mult(1)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    topics = [b"abcde", b"+x", b"", b"xyz", b"0123456789"]
    n = len(topics)
    assert pack(core, s, topics) == TM_OK
    m, cnt = C.POINTER(C.c_uint32)(), C.c_uint64(7)
    assert core.tmn_picks(s, C.byref(m), C.byref(cnt)) == TM_EINVAL and cnt.value == 0      # nothing published yet
    kc5, kt5 = [11, 22, 33, 44, 55], [5, 4, 3, 2, 1]
    for local, seed, kc, kt, mask in ((1, 9, None, None, 0), (0, 3, kc5, kt5, 3), (2, 3, None, kt5, 2), (2, 4, kc5, None, 1),
                                      (1, 1, None, None, 0)):
        assert set_keys(core, s, n, kc, kt) == TM_OK
        c0, m0 = core.fake_publish_count(), core.fake_share_moves()
        assert core.tmn_publish(s, H, n, 3, local, seed) == TM_OK
        assert core.fake_publish_count() - c0 == 1 and core.fake_share_moves() - m0 == 1 and core.fake_set_reruns(s) == 0
        assert core.fake_publish_keys(c0) == mask and core.fake_set_keys_in_set(s, c0), "the key words live in the set"
        exp, exp_dl = expected(core, topics, 3, local, kc, kt, seed)
        got, dl, prc = results(core, s, 3)
        assert prc == 0 and got == exp and dl == (0, exp_dl) and len(exp_dl) > 5
        members = [m for sl in got for _, _, m in sl]
        assert NONE in members and len(set(members)) > 10
    assert set_keys(core, s, n, kc5, None) == TM_OK
    assert core.tmn_publish(s, H, n - 1, 3, 1, 0) == TM_EINVAL             # keys set for another n
    assert set_keys(core, s, n, None, None) == TM_OK
    assert core.tmn_publish(s, H, n, 3, 3, 0) == TM_EINVAL                 # local_dest >= n_dests
    assert core.tmn_picks(s, C.byref(m), C.byref(cnt)) == TM_EINVAL and cnt.value == 0
    assert core.tmn_publish(s, H, n, 0, 0, 0) == TM_EINVAL
    # a plain tmn_dispatch on the same set: deliveries, no picks; and matches/3 (tmn_match) for the packed batch
    assert core.tmn_publish(s, H, n, 3, 1, 0) == TM_OK and core.tmn_picks(s, C.byref(m), C.byref(cnt)) == 0
    assert core.tmn_dispatch(s, H, n, 3, 1, _native.TM_ROUTE_AGGRE) == TM_OK
    assert core.tmn_picks(s, C.byref(m), C.byref(cnt)) == TM_EINVAL
    assert core.tmn_match(s, H, n, 0) == TM_OK
    core.tmn_give(pool, s)
    a0, f0 = core.fake_count(0), core.fake_count(1)
    core.fake_pool_free(pool)
    # blob, offs, hit, vals, err, rdoff, rtopic, dhead, dtopic, dvalue, dsub, skc, skt, smember
    assert core.fake_count(1) - f0 >= 14
    assert core.fake_count(0) == a0 == core.fake_count(1), "buffers released with the set"


@pytest.mark.parametrize("kind", ["cap", "dcap", "both"])
def test_ecap_reruns_once_and_says_how_often_the_state_moved(core, kind):
    """ONE rerun with room for out_dest_offsets[n_dests + 1] entries (and members) and out_head[1]
    deliveries.  From the entries the first call picked nothing: the state moves once.  From the
    deliveries alone the first call's picks stood: the rerun picks again, the state has moved twice."""
    topics = [b"abcdefg", b"hijklmn"] if kind == "dcap" else [b"x" * 3000, b"y" * 200]
    mult = {"cap": 1, "dcap": 2000, "both": 40}[kind]
    n_dests, local = (1, 0) if kind == "dcap" else (4, 2)
    core.fake_dispatch_mult(mult)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    assert pack(core, s, topics) == TM_OK
    assert set_keys(core, s, 2, [7, 8], None) == TM_OK
    c0, m0 = core.fake_publish_count(), core.fake_share_moves()
    assert core.tmn_publish(s, H, 2, n_dests, local, 5) == TM_OK
    assert core.fake_publish_count() - c0 == 2 and core.fake_set_reruns(s) == 1
    assert core.fake_share_moves() - m0 == (2 if kind == "dcap" else 1)
    exp, exp_dl = expected(core, topics, n_dests, local, [7, 8], None, 5, mult)
    total, T = sum(map(len, exp)), len(exp_dl)
    cap0, cap1 = core.fake_publish_cap(c0), core.fake_publish_cap(c0 + 1)
    dcap0, dcap1 = core.fake_publish_dcap(c0), core.fake_publish_dcap(c0 + 1)
    assert (cap0 < total) == (kind != "dcap") and (dcap0 < T) == (kind != "cap")
    assert cap1 >= total and dcap1 >= T
    assert (cap1 == cap0) == (kind == "dcap") and (dcap1 == dcap0) == (kind == "cap")   # only what did not fit grew
    assert core.fake_set_route_cap(s) >= 4 * total and core.fake_set_delivery_cap(s) >= 4 * T
    assert core.fake_set_member_cap(s) >= 4 * total
    got, dl, prc = results(core, s, n_dests)
    assert prc == 0 and got == exp and dl == (0, exp_dl)
    c0, m0 = core.fake_publish_count(), core.fake_share_moves()
    assert core.tmn_publish(s, H, 2, n_dests, local, 5) == TM_OK
    assert core.fake_publish_count() - c0 == 1 and core.fake_set_reruns(s) == 1   # sticky sizes: no rerun
    assert core.fake_share_moves() - m0 == 1
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
    assert core.fake_count(0) == core.fake_count(1)
    core.fake_dispatch_mult(1)


def test_device_failure_is_a_device_error(core):
    core.fake_dispatch_mult(1)
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    m, cnt = C.POINTER(C.c_uint32)(), C.c_uint64(7)
    for topics in ([b"ab", b"!x", b"cd"], [b"ab", b"~x"]):
        assert pack(core, s, topics) == TM_OK
        assert core.tmn_publish(s, H, len(topics), 2, 0, 0) == TM_EDEVICE
        b, e = C.c_uint64(), C.c_uint64()
        assert core.tmn_route_dest(s, 0, C.byref(b), C.byref(e)) == TM_EINVAL   # no result to slice
        assert core.tmn_picks(s, C.byref(m), C.byref(cnt)) == TM_EINVAL and cnt.value == 0
    topics = [b"abcdefgh", b"+x"]
    assert pack(core, s, topics) == TM_OK
    assert core.tmn_publish(s, H, 2, 2, 1, 0) == TM_OK
    exp, exp_dl = expected(core, topics, 2, 1, None, None, 0)
    got, dl, prc = results(core, s, 2)
    assert prc == 0 and got == exp and dl == (0, exp_dl)
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
    assert core.fake_count(0) == core.fake_count(1)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler (gcc) to build the NIF share check")
    exe = tmp_path / "nif_share_check"
    b = subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}",
                        "-o", str(exe)] + [str(s) for s in SOURCES] +
                       [str(ROOT / "tests" / "native" / "nif_share_check.c")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok"
