"""TEST INFRASTRUCTURE shared by tests/test_gpu_nif_chain.py and
tests/test_gpu_nif_match.py: the seven ERTS-free units of c_src/ and
tests/native/nif_chain_shim.c linked against the real emqx_amd/libtmatch.so,
and one caller's buffer set read back through the units' own readers
(tmn_route_dest, tmn_deliveries, tmn_picks, tmn_groups, tmn_direct, tmn_row,
tmn_first_row) into numpy arrays."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from emqx_amd import _native

ROOT = Path(__file__).resolve().parent.parent
UNITS = ("core", "route", "aggre", "dispatch", "share", "deliver", "publish_deliver")
ENTRIES, DELIVERIES, GROUPS, VALUES = 0, 1, 2, 3   # shim_cap's kinds
EINVAL = _native.TM_EINVAL


def load(tmp_dir):
    out = Path(tmp_dir) / "libnifchain.so"
    libdir = ROOT / "emqx_amd"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'c_src'}", "-o", str(out)]
                   + [str(ROOT / "c_src" / f"tmatch_nif_{u}.c") for u in UNITS]
                   + [str(ROOT / "tests" / "native" / "nif_chain_shim.c"),
                      f"-L{libdir}", "-l:libtmatch.so", f"-Wl,-rpath,{libdir}"], check=True)
    _native.load_library()
    lib = C.CDLL(str(out))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    p32, p64 = C.POINTER(u32), C.POINTER(u64)
    lib.shim_pool_new.restype = vp
    lib.shim_pool_new.argtypes = [vp, u32]
    lib.shim_pool_free.argtypes = [vp]
    lib.shim_pool_count.argtypes = [vp]
    lib.tmn_take.restype = vp
    lib.tmn_take.argtypes = [vp]
    lib.tmn_give.argtypes = [vp, vp]
    lib.tmn_pack.argtypes = [vp, vp, u32, vp, vp]
    lib.tmn_share_keys.argtypes = [vp, vp, u32, vp, vp]
    for f in (lib.tmn_route, lib.tmn_route_aggre, lib.tmn_match):
        f.argtypes = [vp, vp, u32, u32]
    lib.tmn_first.argtypes = [vp, vp, u32]
    for f in (lib.tmn_dispatch, lib.tmn_publish, lib.tmn_deliver, lib.tmn_publish_deliver):
        f.argtypes = [vp, vp, u32, u32, u32, u32]
    lib.tmn_route_dest.argtypes = [vp, u32, p64, p64]
    lib.tmn_row.argtypes = [vp, u32, u32, u32, p64, p64]
    lib.tmn_first_row.argtypes = [vp, u32, p32]
    lib.tmn_deliveries.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), C.POINTER(p32), p64]
    lib.tmn_groups.argtypes = [vp, C.POINTER(p32), C.POINTER(p32), p64]
    lib.tmn_picks.argtypes = [vp, C.POINTER(p32), p64]
    for f in (lib.shim_vals, lib.shim_route_topics):
        f.argtypes, f.restype = [vp], p32
    lib.shim_err.argtypes, lib.shim_err.restype = [vp], C.POINTER(C.c_uint8)
    for f in (lib.shim_direct, lib.shim_reruns):
        f.argtypes, f.restype = [vp], u64
    for f in (lib.shim_in_flags, lib.shim_input_flags, lib.shim_dispatched):
        f.argtypes, f.restype = [vp], u32
    lib.shim_ids_per_topic.restype = u32
    lib.shim_cap.argtypes, lib.shim_cap.restype = [vp, C.c_int], u64
    lib.shim_first_cap.argtypes, lib.shim_first_cap.restype = [vp, u64], u64
    return lib


def _arr(ptr, k, dtype=np.uint32):
    return np.ctypeslib.as_array(ptr, shape=(k,)).astype(dtype) if k else np.zeros(0, dtype)


class Caller:
    """one caller: a pool of its own on the index (or a set from a shared pool), one buffer set"""

    def __init__(self, lib, ix, in_flags=_native.TM_ALLOC_VRAM, pool=None):
        self.lib, self.ix, self.h = lib, ix, ix._h
        self.own = pool is None
        self.pool = lib.shim_pool_new(self.h, in_flags) if pool is None else pool
        self.s = lib.tmn_take(self.pool)
        assert self.s

    def close(self):
        self.lib.tmn_give(self.pool, self.s)
        if self.own:
            self.lib.shim_pool_free(self.pool)

    # ---- the calls
    def pack(self, topics):
        arr = (C.c_char_p * len(topics))(*topics)
        lens = (C.c_uint64 * len(topics))(*[len(t) for t in topics])
        return self.lib.tmn_pack(self.s, self.h, len(topics), C.cast(arr, C.c_void_p), C.cast(lens, C.c_void_p))

    def keys(self, n, kc, kt):
        a = None if kc is None else np.ascontiguousarray(kc[:n], np.uint32)
        b = None if kt is None else np.ascontiguousarray(kt[:n], np.uint32)
        return self.lib.tmn_share_keys(self.s, self.h, n, _native._ptr(a), _native._ptr(b))

    def route(self, n, n_dests, aggre=False):
        return (self.lib.tmn_route_aggre if aggre else self.lib.tmn_route)(self.s, self.h, n, n_dests)

    def dispatch(self, n, n_dests, local, flags=0):
        return self.lib.tmn_dispatch(self.s, self.h, n, n_dests, local, flags)

    def publish(self, n, n_dests, local, seed):
        return self.lib.tmn_publish(self.s, self.h, n, n_dests, local, seed)

    def deliver(self, n, n_dests, local, flags=0):
        return self.lib.tmn_deliver(self.s, self.h, n, n_dests, local, flags)

    def publish_deliver(self, n, n_dests, local, seed):
        return self.lib.tmn_publish_deliver(self.s, self.h, n, n_dests, local, seed)

    def match(self, n, order):
        return self.lib.tmn_match(self.s, self.h, n, order)

    def first(self, n):
        return self.lib.tmn_first(self.s, self.h, n)

    # ---- the set's words
    reruns = property(lambda self: self.lib.shim_reruns(self.s))
    direct = property(lambda self: self.lib.shim_direct(self.s))
    dispatched = property(lambda self: self.lib.shim_dispatched(self.s))
    in_flags = property(lambda self: self.lib.shim_in_flags(self.s))
    input_flags = property(lambda self: self.lib.shim_input_flags(self.s))

    def cap(self, what):
        return self.lib.shim_cap(self.s, what)

    # ---- the readers
    def slices(self, n, n_dests):
        """every tmn_route_dest slice, 0 .. n_dests -> (rc, bucket offsets u64[n_dests + 2], topic, values, err[:n]);
        the slices must tile [0, total) in order"""
        doff = np.zeros(n_dests + 2, np.uint64)
        for d in range(n_dests + 1):
            b, e = C.c_uint64(7), C.c_uint64(7)
            rc = self.lib.tmn_route_dest(self.s, d, C.byref(b), C.byref(e))
            if rc:
                assert (b.value, e.value) == (0, 0), "a refused slice is empty"
                return rc, None, None, None, None
            assert b.value == int(doff[d]) and e.value >= b.value, "the slices tile the entries"
            doff[d + 1] = e.value
        b, e = C.c_uint64(7), C.c_uint64(7)
        assert self.lib.tmn_route_dest(self.s, n_dests + 1, C.byref(b), C.byref(e)) == EINVAL and b.value == e.value == 0
        total = int(doff[-1])
        return 0, doff, _arr(self.lib.shim_route_topics(self.s), total), _arr(self.lib.shim_vals(self.s), total), \
            _arr(self.lib.shim_err(self.s), n, np.uint8)

    def deliveries(self):
        t, v, s = (C.POINTER(C.c_uint32)() for _ in range(3))
        cnt = C.c_uint64(99)
        rc = self.lib.tmn_deliveries(self.s, C.byref(t), C.byref(v), C.byref(s), C.byref(cnt))
        if rc:
            assert cnt.value == 0 and not t and not v and not s, "a refused read hands out nothing"
            return rc, None, None, None
        assert t and v and s, "a read that succeeded handed out no arrays"
        return 0, _arr(t, cnt.value), _arr(v, cnt.value), _arr(s, cnt.value)

    def picks(self):
        m, cnt = C.POINTER(C.c_uint32)(), C.c_uint64(99)
        rc = self.lib.tmn_picks(self.s, C.byref(m), C.byref(cnt))
        if rc:
            assert cnt.value == 0 and not m, "a refused read hands out nothing"
            return rc, None
        assert m, "a read that succeeded handed out no array"
        return 0, _arr(m, cnt.value)

    def groups(self):
        gs, go, cnt = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64(99)
        rc = self.lib.tmn_groups(self.s, C.byref(gs), C.byref(go), C.byref(cnt))
        if rc:
            assert cnt.value == 0 and not gs and not go, "a refused read hands out nothing"
            return rc, None, None
        assert gs and go, "a read that succeeded handed out no arrays"
        return 0, _arr(gs, cnt.value), _arr(go, cnt.value + 1).astype(np.uint64)

    def rows(self, n, order):
        """every tmn_row, 0 .. n - 1 -> (flags u8[n], counts i64[n], the rows' values one after the other)"""
        flags, lo, hi = np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
        b, e = C.c_uint64(), C.c_uint64()
        row, s, pb, pe = self.lib.tmn_row, self.s, C.byref(b), C.byref(e)
        for i in range(n):
            flags[i] = row(s, n, order, i, pb, pe)
            lo[i], hi[i] = b.value, e.value
        cnt = hi - lo
        assert (cnt >= 0).all() and (cnt[flags != 0] == 0).all(), "a flagged topic has no values"
        top = int(hi.max()) if n else 0
        assert 4 * top <= 4 * self.cap(VALUES), "a row ends past the value buffer"
        vals = _arr(self.lib.shim_vals(self.s), top)
        at = np.repeat(lo - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(int(cnt.sum())) if n else cnt
        return flags, cnt, vals[at]

    def firsts(self, n):
        """every tmn_first_row -> (found u8[n], value u32[n])"""
        found, val = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        v = C.c_uint32()
        row, s, pv = self.lib.tmn_first_row, self.s, C.byref(v)
        for i in range(n):
            found[i] = row(s, i, pv)
            val[i] = v.value
        return found, val
