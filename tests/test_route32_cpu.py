"""tm_route_batch32 without a device: the export, the ABI minor, the argument
check that needs no GPU, and the NIF core's route half
(c_src/tmatch_nif_route.c) against the stand-in libtmatch
(tests/native/fake_tmatch.c + fake_tmatch_route.c): the capacity rerun sized
from the bucket offsets, the per-destination slices, err 4 -> TM_EDEVICE."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

from emqx_amd import _native

ROOT = Path(__file__).resolve().parent.parent
TM_OK, TM_EINVAL, TM_EDEVICE, TM_ECAP = 0, -1, -3, -4


def test_export_and_abi_minor():
    lib = _native.load_library()
    assert "tm_route_batch32" in _native.EXPORTS and hasattr(lib, "tm_route_batch32")
    v = lib.tm_abi_version()
    assert v >> 16 == 1 and (v & 0xFFFF) >= 13
    assert (_native.TM_DEBUG_ROUTE_ONE, _native.TM_DEBUG_ROUTE_GRID) == (26, 27)


def test_null_handle_is_einval():
    lib = _native.load_library()
    offs = (C.c_uint32 * 2)(0, 1)
    doff = (C.c_uint32 * 3)()
    err = (C.c_uint8 * 1)()
    assert lib.tm_route_batch32(None, 1, b"a" * 16, offs, 1, doff, None, None, 0, err) == TM_EINVAL


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("nifroute") / "libnifroute.so"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out),
                    str(ROOT / "c_src" / "tmatch_nif_core.c"), str(ROOT / "c_src" / "tmatch_nif_route.c"),
                    str(ROOT / "tests" / "native" / "fake_tmatch.c"),
                    str(ROOT / "tests" / "native" / "fake_tmatch_route.c")], check=True)
    lib = C.CDLL(str(out))
    vp = C.c_void_p
    lib.fake_pool_new.restype = vp
    lib.fake_pool_free.argtypes = [vp]
    lib.fake_count.restype = C.c_long
    lib.tmn_take.restype = vp
    lib.tmn_take.argtypes = [vp]
    lib.tmn_give.argtypes = [vp, vp]
    lib.tmn_pack.argtypes = [vp, vp, C.c_uint32, vp, vp]
    lib.tmn_route.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    lib.tmn_route_dest.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fake_set_vals.argtypes = [vp]
    lib.fake_set_vals.restype = C.POINTER(C.c_uint32)
    lib.fake_set_route_topics.argtypes = [vp]
    lib.fake_set_route_topics.restype = C.POINTER(C.c_uint32)
    lib.fake_set_route_cap.argtypes = [vp]
    lib.fake_set_route_cap.restype = C.c_uint64
    lib.fake_set_reruns.argtypes = [vp]
    lib.fake_set_reruns.restype = C.c_uint64
    lib.fake_route_count.restype = C.c_long
    lib.fake_route_cap.argtypes = [C.c_long]
    lib.fake_route_cap.restype = C.c_uint64
    return lib


H = C.c_void_p(1)


def pack(lib, s, topics):
    arr = (C.c_char_p * len(topics))(*topics)
    lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
    return lib.tmn_pack(s, H, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))


def slices(lib, s, n_dests):
    """-> [[(topic, value)] per bucket 0 .. n_dests] through tmn_route_dest"""
    vals, tops = lib.fake_set_vals(s), lib.fake_set_route_topics(s)
    out = []
    for d in range(n_dests + 1):
        b, e = C.c_uint64(), C.c_uint64()
        assert lib.tmn_route_dest(s, d, C.byref(b), C.byref(e)) == 0
        out.append([(tops[k], vals[k]) for k in range(b.value, e.value)])
    return out


def expected(topics, n_dests):
    out = [[] for _ in range(n_dests + 1)]
    for i, t in enumerate(topics):
        if t[:1] == b"+":
            continue
        for k in range(len(t)):
            out[(1000 * i + k) % (n_dests + 1)].append((i, 1000 * i + k))
    return out


def test_route_slices_per_destination(core):
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    topics = [b"abcde", b"+x", b"", b"xyz"]
    assert pack(core, s, topics) == TM_OK
    assert core.tmn_route(s, H, len(topics), 3) == TM_OK
    got = slices(core, s, 3)
    assert got == expected(topics, 3) and sum(map(len, got)) == 8
    b, e = C.c_uint64(7), C.c_uint64(7)
    assert core.tmn_route_dest(s, 5, C.byref(b), C.byref(e)) == TM_EINVAL and (b.value, e.value) == (0, 0)
    assert core.tmn_route(s, H, len(topics), 0) == TM_EINVAL
    # the same set still serves matches/3 (tmn_match) for the packed batch
    core.tmn_match.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    assert core.tmn_match(s, H, len(topics), 0) == TM_OK
    core.tmn_give(pool, s)
    f0 = core.fake_count(1)
    core.fake_pool_free(pool)
    assert core.fake_count(1) - f0 >= 7   # blob, offs, hit, vals, err, rdoff, rtopic


def test_ecap_reruns_once_sized_from_the_offsets(core):
    """More entries than the first guess (TMN_IDS_PER_TOPIC per topic + 1024):
    one rerun with room for out_dest_offsets[n_dests + 1] entries, and the
    grown buffers stay with the set."""
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    topics = [b"x" * 3000, b"y" * 200]
    total = 3200
    assert pack(core, s, topics) == TM_OK
    c0 = core.fake_route_count()
    assert core.tmn_route(s, H, 2, 4) == TM_OK
    assert core.fake_route_count() - c0 == 2 and core.fake_set_reruns(s) == 1
    assert core.fake_route_cap(c0) < total <= core.fake_route_cap(c0 + 1)
    assert core.fake_set_route_cap(s) >= 4 * total
    assert slices(core, s, 4) == expected(topics, 4)
    c0 = core.fake_route_count()
    assert core.tmn_route(s, H, 2, 4) == TM_OK
    assert core.fake_route_count() - c0 == 1 and core.fake_set_reruns(s) == 1   # sticky size: no rerun
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)


def test_device_failure_is_a_device_error(core):
    pool = core.fake_pool_new()
    s = core.tmn_take(pool)
    for topics in ([b"ab", b"!x", b"cd"], [b"ab", b"~x"]):
        assert pack(core, s, topics) == TM_OK
        assert core.tmn_route(s, H, len(topics), 2) == TM_EDEVICE
        b, e = C.c_uint64(), C.c_uint64()
        assert core.tmn_route_dest(s, 0, C.byref(b), C.byref(e)) == TM_EINVAL   # no result to slice
    assert pack(core, s, [b"ab", b"+x"]) == TM_OK
    assert core.tmn_route(s, H, 2, 2) == TM_OK
    assert slices(core, s, 2) == expected([b"ab", b"+x"], 2)
    core.tmn_give(pool, s)
    core.fake_pool_free(pool)
