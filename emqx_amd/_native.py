"""ctypes binding of ``libtmatch.so`` (the C ABI in ``include/tmatch.h``).

This is the only way the Python host layer reaches the match path.  There is
no fallback: if the library is missing or no GPU is visible, calls raise
:class:`NativeUnavailable` (the product path never routes through a CPU
implementation).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from .build import LIB_TMATCH

TM_OK, TM_EINVAL, TM_ENOMEM, TM_EDEVICE, TM_ECAP = 0, -1, -2, -3, -4
TM_OP_DELETE, TM_OP_INSERT = 0, 1
TM_KEY_BINARY, TM_KEY_WORDS, TM_KEY_EMPTY_LIST, TM_KEY_ESCAPED = 0, 1, 2, 4
TM_ORDER_TRAVERSAL, TM_ORDER_SORTED, TM_ORDER_UNIQUE = 0, 1, 2

# every symbol include/tmatch.h declares (tests check the export table)
EXPORTS = ("tm_create", "tm_destroy", "tm_apply_deltas", "tm_sync", "tm_match_batch",
           "tm_match_batch_dev", "tm_first_batch", "tm_stats", "tm_profile_enable", "tm_profile_read",
           "tm_last_error", "tm_abi_version", "tm_merge_shards", "tm_host_alloc", "tm_host_free",
           "tm_stream_release", "tm_match_batch_ex", "tm_match_batch_dev_ex", "tm_sort_segments",
           "tm_matches_filter", "tm_apply_deltas_ex", "tm_read_begin", "tm_read_end", "tm_epoch",
           "tm_create_replicas", "tm_replica_stats", "tm_debug_set", "tm_debug_get", "tm_match_batch32_ex",
           "tm_match_batch32_dev", "tm_matches_filter_ex", "tm_host_alloc_ex", "tm_commit",
           "tm_match_batch32_pairs", "tm_match_batch_dev_pairs", "tm_set_dests", "tm_fanout_dev", "tm_route_batch",
           "tm_fanout_dev_pairs", "tm_route_batch32", "tm_set_route_filters", "tm_aggre_dev", "tm_route_batch_ex",
           "tm_route_batch32_ex", "tm_set_subscribers", "tm_dispatch_dev", "tm_dispatch_batch",
           "tm_dispatch_batch32", "tm_set_share_slots", "tm_set_share_members", "tm_share_state_set",
           "tm_share_state_get", "tm_share_pick_dev", "tm_publish_batch", "tm_publish_batch32",
           "tm_group_subs_dev", "tm_deliver_batch", "tm_deliver_batch32", "tm_set_member_subs",
           "tm_group_picks_dev", "tm_publish_deliver_batch", "tm_publish_deliver_batch32",
           "tm_retained_create", "tm_retained_destroy", "tm_retained_put", "tm_retained_delete", "tm_retained_get",
           "tm_retained_match", "tm_retained_expire", "tm_retained_compact", "tm_retained_stats",
           "tm_retained_last_error", "tm_retained_match_page", "tm_retained_pin", "tm_retained_unpin")
TM_ALLOC_VRAM = 1
TM_ROUTE_AGGRE = 1          # tm_route_batch_ex / tm_route_batch32_ex: aggre/1 applied to the buckets
NO_FILTER = 0xFFFFFFFF      # tm_set_route_filters: no filter known (equal to nothing)
# shared-subscription pick (include/tmatch.h): no slot / no pick, a state never set, the strategy bytes
TM_SHARE_NONE = TM_SHARE_UNDEF = 0xFFFFFFFF
(TM_SHARE_RANDOM, TM_SHARE_ROUND_ROBIN, TM_SHARE_ROUND_ROBIN_PER_GROUP, TM_SHARE_STICKY, TM_SHARE_LOCAL,
 TM_SHARE_HASH_CLIENTID, TM_SHARE_HASH_TOPIC) = range(7)
TM_DEBUG_LB_SPINS, TM_DEBUG_LB_FAIL_BLOCK, TM_DEBUG_LB_LAUNCHES, TM_DEBUG_PHASES = 1, 2, 3, 4
TM_DEBUG_FAILED_BATCHES, TM_DEBUG_RETRIED_BATCHES = 5, 6
TM_DEBUG_PATH_PHASES, TM_DEBUG_PATH_SMALL, TM_DEBUG_PATH_LANE = 7, 8, 9
TM_DEBUG_SMALL_KERNEL = 10
SMALL_AUTO, SMALL_WAVE, SMALL_WAVE8 = 0, 1, 3   # (2: round 5's lane kernel, removed)
TM_DEBUG_COMBINE, TM_DEBUG_COMBINED_LAUNCHES, TM_DEBUG_COMBINED_BATCHES = 12, 13, 14
TM_DEBUG_WIDE_NODES, TM_DEBUG_DENSE_WIDE = 15, 16
TM_DEBUG_CMB_GATHER, TM_DEBUG_CMB_LAND = 17, 18
TM_DEBUG_COMMITS, TM_DEBUG_COMMIT_WAITS, TM_DEBUG_COMMIT_FORCED = 19, 20, 21
TM_DEBUG_SMALL_TICKET = 22
TM_DEBUG_CMB_SPIN = 23
TM_DEBUG_PATCH_ZC = 24
TM_DEBUG_FANOUT_GRID = 25   # (get only) one-wave blocks of a fan-out pass
TM_DEBUG_ROUTE_ONE, TM_DEBUG_ROUTE_GRID = 26, 27   # (get only) route_batch32 calls per fan-out path
# (get only) the node annexed to a vocab-hint slot (depth << 32 | children; all ones: none); hints that disagree (0)
TM_DEBUG_ANNEX0, TM_DEBUG_ANNEX1, TM_DEBUG_HINT_AUDIT = 28, 29, 30
TM_DEBUG_SUB_COMPACTIONS = 31   # (get only) rewrites of tm_set_subscribers' pool
TM_DEBUG_DISPATCH_ONE, TM_DEBUG_DISPATCH_GRID = 32, 33   # (get only) dispatch_batch32 calls per finishing leg
TM_DEBUG_DP1_MAX = 34   # deliveries the one-launch dispatch kernel expands itself (clamped to DP1_DELIVERIES)
DP1_DELIVERIES = 32768
TM_DEBUG_PUBLISH_ONE, TM_DEBUG_PUBLISH_GRID = 35, 36   # (get only) publish_batch32 calls per picking leg
# (get only) keys a block of group_subs_dev ranks per pass at a time; the digit passes its calls ran / skipped
TM_DEBUG_GROUP_TILE, TM_DEBUG_GROUP_PASSES_RUN, TM_DEBUG_GROUP_PASSES_SKIPPED = 37, 38, 39
TM_DEBUG_GROUP_GRID = 40    # (get only) the blocks of group_subs_dev's fixed grid
TM_DEBUG_DELIVER_ONE, TM_DEBUG_DELIVER_GRID = 41, 42   # (get only) deliver_batch32 calls per grouping leg
TM_DEBUG_GS1_MAX = 43       # deliveries the one-workgroup grouping takes itself (clamped to GS1_DELIVERIES)
TM_DEBUG_GP1_MAX = 44       # merged deliveries (T + K) the one-workgroup merge takes itself (clamped to GP1_DELIVERIES)
# (get only) publish_deliver_batch32 calls per ending: one workgroup / the grid kernels or the staged path
TM_DEBUG_PUBLISH_DELIVER_ONE, TM_DEBUG_PUBLISH_DELIVER_GRID = 45, 46
GS1_DELIVERIES = 16384
GP1_DELIVERIES = 8192        # (emqx_amd/csrc/tm_dev.h) merged deliveries, T + K, of tm_publish_deliver_batch32's one workgroup
MAX_DESTS = 65536           # tm_fanout_dev / tm_route_batch: n_dests is 1 .. MAX_DESTS
# the retained-message store (emqx_amd/csrc/tm_retain.h): levels kept in columns, rows a block scans
RT_COLS, RT_TILE = 8, 256
RT_PUT_REPLACED, RT_PUT_NEW, RT_PUT_INVALID = 0, 1, 2   # tm_retained_put's out_code
# match cursors (tm_retained_match_page): open, the end, and out_err's "cursor of another epoch"
TM_RET_CURSOR_BEGIN, TM_RET_CURSOR_DONE, TM_RET_ESTALE = 0, 0xFFFFFFFFFFFFFFFF, 3


class NativeUnavailable(RuntimeError):
    pass


class TmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"tmatch error {code}: {msg}")
        self.code = code


class DeviceError(TmError):
    """TM_EDEVICE: the GPU failed the call (e.g. a batch whose look-back wait
    expired twice, include/tmatch.h err flag 4).  Never a client error: the
    reference raises badarg only for a '+'/'#' topic level
    (emqx_trie_search.erl:374-375)."""


class tm_options(C.Structure):
    _fields_ = [("device", C.c_int32), ("copies", C.c_uint32), ("hint_keys", C.c_uint64)]


class tm_stats_t(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_keys", "n_wild_keys", "n_exact_keys", "n_dead_keys",
                                          "n_nodes", "n_edges", "n_words", "device_bytes",
                                          "uploads", "patch_bytes")]


class tm_retained_opts(C.Structure):
    _fields_ = [("initial_rows", C.c_uint32), ("tail_max", C.c_uint32)]


class tm_retained_stats_t(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("live_rows", "base_rows", "tail_rows", "dead_rows", "words", "compactions",
                                          "growths", "match_launches", "no_launch_filters", "device_bytes",
                                          "rt_cols", "rt_tile")]


_lib = None


def load_library(path: Path | None = None):
    """Load libtmatch.so (does not touch the GPU)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    import os
    # TM_LIB: an experimental build of the same library (emqx_amd.build.build_variant)
    p = Path(path) if path else Path(os.environ.get("TM_LIB", LIB_TMATCH))
    if not p.exists():
        raise NativeUnavailable(f"{p} is not built (run emqx_amd.build.build_all())")
    lib = C.CDLL(str(p))
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    sig = {
        "tm_create": (i32, [C.POINTER(tm_options), C.POINTER(vp)]),
        "tm_destroy": (i32, [vp]),
        "tm_apply_deltas": (i32, [vp, u64, vp, vp, vp, vp, vp]),
        "tm_sync": (i32, [vp, vp]),
        "tm_match_batch": (i32, [vp, u64, vp, vp, vp, vp, u64, vp]),
        "tm_match_batch_dev": (i32, [vp, u64, vp, vp, vp, vp, u64, vp, vp]),
        "tm_first_batch": (i32, [vp, u64, vp, vp, vp, vp]),
        "tm_matches_filter": (i32, [vp, u64, vp, vp, vp, vp, u64, vp]),
        "tm_matches_filter_ex": (i32, [vp, u64, vp, vp, vp, vp, vp, u64, vp]),
        "tm_stats": (i32, [vp, C.POINTER(tm_stats_t)]),
        "tm_profile_enable": (i32, [vp, i32]),
        "tm_profile_read": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64), i32]),
        "tm_last_error": (C.c_char_p, [vp]),
        "tm_abi_version": (u32, []),
        "tm_merge_shards": (i32, [u32, u64, vp, vp, u64, vp, vp, u64, vp]),
        "tm_host_alloc": (i32, [vp, u64, C.POINTER(vp)]),
        "tm_host_free": (i32, [vp, vp]),
        "tm_host_alloc_ex": (i32, [vp, u64, u32, C.POINTER(vp)]),
        "tm_stream_release": (i32, [vp, vp]),
        "tm_match_batch_ex": (i32, [vp, u64, vp, vp, vp, vp, u64, vp, u32, vp]),
        "tm_match_batch_dev_ex": (i32, [vp, u64, vp, vp, vp, vp, u64, vp, u32, vp, vp]),
        "tm_match_batch_dev_pairs": (i32, [vp, u64, vp, vp, vp, vp, u64, vp, vp]),
        "tm_sort_segments": (i32, [vp, u64, vp, vp, u64, u32, vp, vp]),
        "tm_apply_deltas_ex": (i32, [vp, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]),
        "tm_commit": (i32, [vp, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]),
        "tm_read_begin": (i32, [vp, C.POINTER(u64)]),
        "tm_read_end": (i32, [vp, u64]),
        "tm_epoch": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "tm_create_replicas": (i32, [C.POINTER(tm_options), C.POINTER(C.c_int32), u32, C.POINTER(vp)]),
        "tm_replica_stats": (i32, [vp, u32, C.POINTER(u64), C.POINTER(C.c_int32)]),
        "tm_match_batch32_ex": (i32, [vp, u64, vp, vp, vp, vp, u64, vp, u32, vp]),
        "tm_match_batch32_dev": (i32, [vp, u64, vp, vp, vp, vp, u64, vp, vp]),
        "tm_match_batch32_pairs": (i32, [vp, u64, vp, vp, vp, vp, u64, vp]),
        "tm_set_dests": (i32, [vp, u64, vp, vp]),
        "tm_fanout_dev": (i32, [vp, u64, vp, vp, u64, vp, u64, u32, vp, vp, vp, vp]),
        "tm_fanout_dev_pairs": (i32, [vp, u64, vp, vp, u64, vp, u64, u32, vp, vp, vp, vp]),
        "tm_route_batch": (i32, [vp, u64, vp, vp, u32, vp, vp, vp, u64, vp]),
        "tm_route_batch32": (i32, [vp, u64, vp, vp, u32, vp, vp, vp, u64, vp]),
        "tm_set_route_filters": (i32, [vp, u64, vp, vp]),
        "tm_aggre_dev": (i32, [vp, u32, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp]),
        "tm_route_batch_ex": (i32, [vp, u64, vp, vp, u32, vp, vp, vp, u64, vp, u32]),
        "tm_route_batch32_ex": (i32, [vp, u64, vp, vp, u32, vp, vp, vp, u64, vp, u32]),
        "tm_set_subscribers": (i32, [vp, u64, vp, vp, vp]),
        "tm_dispatch_dev": (i32, [vp, u32, vp, u32, vp, vp, u64, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, vp]),
        "tm_dispatch_batch": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp]),
        "tm_dispatch_batch32": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp]),
        "tm_set_share_slots": (i32, [vp, u64, vp, vp]),
        "tm_set_share_members": (i32, [vp, u64, vp, vp, vp, vp, vp]),
        "tm_share_state_set": (i32, [vp, u64, vp, vp]),
        "tm_share_state_get": (i32, [vp, u32, u64, vp, vp]),
        "tm_share_pick_dev": (i32, [vp, u32, vp, vp, vp, u64, vp, vp, u64, u32, vp, u64, vp, u64, vp, u64, vp, vp, vp, vp]),
        "tm_publish_batch": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, u32, vp,
                                   vp]),
        "tm_publish_batch32": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, u32, vp,
                                     vp]),
        "tm_group_subs_dev": (i32, [vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp]),
        "tm_deliver_batch32": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, u64,
                                     vp]),
        "tm_deliver_batch": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, u64,
                                   vp]),
        "tm_set_member_subs": (i32, [vp, u64, vp, vp]),
        "tm_group_picks_dev": (i32, [vp, vp, vp, vp, vp, u64, u32, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp, u64, vp, vp, vp,
                                     vp, u64, vp]),
        "tm_publish_deliver_batch": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, u32,
                                           vp, vp, vp, vp, u64, vp]),
        "tm_publish_deliver_batch32": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, u32,
                                             vp, vp, vp, vp, u64, vp]),
        "tm_retained_create": (i32, [i32, C.POINTER(tm_retained_opts), C.POINTER(vp)]),
        "tm_retained_destroy": (i32, [vp]),
        "tm_retained_put": (i32, [vp, u64, vp, vp, vp, vp, vp]),
        "tm_retained_delete": (i32, [vp, u64, vp, vp, vp]),
        "tm_retained_get": (i32, [vp, u64, vp, vp, u64, vp, vp]),
        "tm_retained_match": (i32, [vp, u64, vp, vp, u64, vp, vp, u64, vp]),
        "tm_retained_expire": (i32, [vp, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(i32)]),
        "tm_retained_compact": (i32, [vp]),
        "tm_retained_stats": (i32, [vp, C.POINTER(tm_retained_stats_t)]),
        "tm_retained_last_error": (C.c_char_p, [vp]),
        "tm_retained_match_page": (i32, [vp, u64, vp, vp, u64, vp, u32, u64, vp, vp, u64, vp, vp]),
        "tm_retained_pin": (i32, [vp]),
        "tm_retained_unpin": (i32, [vp]),
        "tm_debug_set": (i32, [vp, u32, u64]),
        "tm_debug_get": (i32, [vp, u32, C.POINTER(u64)]),
    }
    for name, (res, args) in sig.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            if p == LIB_TMATCH:
                raise
            continue   # (an older TM_LIB study build: newer entry points absent)
        f.restype, f.argtypes = res, args
    if path is None:
        _lib = lib
    return lib


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _gpu_present() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # pragma: no cover
        return False


def merge_shards(world: int, n: int, d_shard_hit: int, d_shard_vals: int, stride: int, d_out_hit: int,
                 d_out_vals: int, cap: int, stream: int | None = None):
    """tm_merge_shards on device pointers (filter-sharded mode)."""
    if not _gpu_present():
        raise NativeUnavailable("no HIP device visible: the shard merge runs on the GPU only")
    lib = load_library()
    rc = lib.tm_merge_shards(world, n, d_shard_hit, d_shard_vals, stride, d_out_hit, d_out_vals, cap, stream)
    if rc != TM_OK:
        raise TmError(rc, lib.tm_last_error(None).decode())


def pack_strings(items) -> tuple[np.ndarray, np.ndarray]:
    """bytes-likes -> (uint8 blob, uint64 offsets[n+1])."""
    items = [bytes(x) for x in items]
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        offs[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    blob = np.frombuffer(b"".join(items) + b"\0" * 16, dtype=np.uint8)
    return blob, offs


class Index:
    """Owning handle of one device-resident topic index (tm_index*)."""

    def __init__(self, device: int = -1, hint_keys: int = 0, devices=None, copies: int = 1):
        """devices: a list of HIP devices -> one host image with a replica on
        each (tm_create_replicas); otherwise one device.  copies: copies of the
        tables per device (tm_options.copies: deltas never wait for batches in
        flight on another copy)."""
        if not _gpu_present():
            raise NativeUnavailable("no HIP device visible: the topic index runs on the GPU only")
        self._lib = load_library()
        opts = tm_options(device, copies, hint_keys)
        h = C.c_void_p()
        if devices is not None:
            devs = (C.c_int32 * len(devices))(*devices)
            rc = self._lib.tm_create_replicas(C.byref(opts), devs, len(devices), C.byref(h))
        else:
            rc = self._lib.tm_create(C.byref(opts), C.byref(h))
        if rc != TM_OK:
            raise TmError(rc, self._lib.tm_last_error(None).decode())
        self._h = h

    def _check(self, rc):
        if rc != TM_OK:
            cls = DeviceError if rc == TM_EDEVICE else TmError
            raise cls(rc, self._lib.tm_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._pinned = []   # tm_destroy frees the tm_host_alloc buffers
            self._lib.tm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- deltas
    def apply(self, ops: np.ndarray, blob: np.ndarray, offs: np.ndarray, values: np.ndarray,
              flags: np.ndarray | None = None, commit: bool = False):
        """tm_apply_deltas_ex, or (commit) tm_commit: published on a table copy no
        batch is reading, so no batch waits for the patch.  -> the delta epoch."""
        ops = np.ascontiguousarray(ops, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        values = np.ascontiguousarray(values, dtype=np.uint32)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        if flags is not None:
            flags = np.ascontiguousarray(flags, dtype=np.uint8)
        e = C.c_uint64()
        fn = self._lib.tm_commit if commit else self._lib.tm_apply_deltas_ex
        self._check(fn(self._h, len(ops), _ptr(ops), _ptr(blob), _ptr(offs), _ptr(values), _ptr(flags), C.byref(e)))
        return e.value

    # ---- reader epochs (include/tmatch.h "Reader epochs")
    def read_begin(self) -> int:
        t = C.c_uint64()
        self._check(self._lib.tm_read_begin(self._h, C.byref(t)))
        return t.value

    def read_end(self, ticket: int):
        self._check(self._lib.tm_read_end(self._h, ticket))

    def epoch(self) -> tuple[int, int]:
        """-> (current epoch, safe epoch: the oldest running reader's, or current)."""
        cur, safe = C.c_uint64(), C.c_uint64()
        self._check(self._lib.tm_epoch(self._h, C.byref(cur), C.byref(safe)))
        return cur.value, safe.value

    def sync(self, stream: int | None = None):
        self._check(self._lib.tm_sync(self._h, stream))

    # ---- pinned host buffers (tm_host_alloc)
    def host_array(self, n: int, dtype, vram: bool = False) -> np.ndarray:
        """A numpy array in pinned host memory mapped into the device.  Batches
        whose buffers (topics 16-byte aligned, offsets, outputs) all come from
        here run in place, without staging copies (include/tmatch.h).  Valid
        until host_free() or close().  vram: device memory mapped into the host
        (TM_ALLOC_VRAM) for a batch's inputs -- write it, never read it back
        (each host read is an uncached PCIe round trip)."""
        dtype = np.dtype(dtype)
        nbytes = max(int(n), 1) * dtype.itemsize
        p = C.c_void_p()
        self._check(self._lib.tm_host_alloc_ex(self._h, nbytes, TM_ALLOC_VRAM if vram else 0, C.byref(p)))
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype, count=max(int(n), 1))
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p.value)
        return a

    def host_free(self, a: np.ndarray):
        addr = a.__array_interface__["data"][0]
        self._check(self._lib.tm_host_free(self._h, C.c_void_p(addr)))
        self._pinned.remove(addr)

    # ---- matching (host buffers)
    def match_batch(self, blob: np.ndarray, offs: np.ndarray, cap: int | None = None, out=None,
                    order: int = TM_ORDER_TRAVERSAL, unique_counts: np.ndarray | None = None):
        """-> (hit_offsets u64[n+1], values u32[total], err u8[n]), each topic's
        values in `order` (traversal by default; TM_ORDER_SORTED ascending;
        TM_ORDER_UNIQUE ascending distinct values first, padded with
        0xFFFFFFFF, the distinct count per topic in `unique_counts`).

        `out` = (hit u64[>= n+1], values u32[cap], err u8[>= n]): caller-owned
        buffers reused across batches (what a NIF keeps per scheduler); the
        results are views into them.  Without it fresh arrays are allocated."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        if unique_counts is not None and (len(unique_counts) < n or unique_counts.dtype != np.uint32):
            raise ValueError("match_batch: unique_counts too small or not uint32")
        uc = _ptr(unique_counts)
        if out is not None:
            hit, vals, err = out
            if len(hit) < n + 1 or len(err) < n or hit.dtype != np.uint64 or vals.dtype != np.uint32 \
                    or err.dtype != np.uint8:
                raise ValueError("match_batch: out buffers too small or of the wrong dtype")
            rc = self._lib.tm_match_batch_ex(self._h, n, _ptr(blob), _ptr(offs), _ptr(hit), _ptr(vals), len(vals),
                                             _ptr(err), order, uc)
            self._check(rc)
            return hit[: n + 1], vals[: int(hit[n])], err[:n]
        hit = np.zeros(n + 1, dtype=np.uint64)
        err = np.zeros(max(n, 1), dtype=np.uint8)
        if cap is None:
            cap = max(4 * n, 1024)
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint32)
            rc = self._lib.tm_match_batch_ex(self._h, n, _ptr(blob), _ptr(offs), _ptr(hit), _ptr(out), cap, _ptr(err),
                                             order, uc)
            if rc == TM_ECAP:
                cap = int(hit[n])
                continue
            self._check(rc)
            return hit, out[: int(hit[n])], err[:n]

    def match_batch32(self, blob: np.ndarray, offs: np.ndarray, out, order: int = TM_ORDER_TRAVERSAL,
                      unique_counts: np.ndarray | None = None):
        """tm_match_batch32_ex: u32 topic offsets in, u32 hit offsets out.
        out = (hit u32[>= n+1], values u32[cap], err u8[>= n]); in place when
        every buffer comes from host_array() (a NIF's pooled buffers).  Raises
        TmError(TM_ECAP) when the values do not fit (hit offsets valid)."""
        n = len(offs) - 1
        hit, vals, err = out
        if offs.dtype != np.uint32 or hit.dtype != np.uint32 or len(hit) < n + 1 or len(err) < n:
            raise ValueError("match_batch32: u32 offsets and large enough outputs expected")
        self._check(self._lib.tm_match_batch32_ex(self._h, n, _ptr(blob), _ptr(offs), _ptr(hit), _ptr(vals), len(vals),
                                                  _ptr(err), order, _ptr(unique_counts)))
        return hit[: n + 1], vals[: int(hit[n])], err[:n]

    def match_batch32_pairs(self, blob: np.ndarray, offs: np.ndarray, out):
        """tm_match_batch32_pairs: u32 topic offsets in; out = (pairs u32[>= 2n+1],
        values u32[cap], err u8[>= n]) -> (pairs[:2n+1], values, err[:n]);
        topic i's values are values[pairs[2i] : pairs[2i] + pairs[2i+1]]
        (disjoint spans, not in topic order).  In place, through the combiner,
        when every buffer comes from host_array()."""
        n = len(offs) - 1
        pairs, vals, err = out
        if offs.dtype != np.uint32 or pairs.dtype != np.uint32 or len(pairs) < 2 * n + 1 or len(err) < n:
            raise ValueError("match_batch32_pairs: u32 offsets and large enough outputs expected")
        self._check(self._lib.tm_match_batch32_pairs(self._h, n, _ptr(blob), _ptr(offs), _ptr(pairs), _ptr(vals),
                                                     len(vals), _ptr(err)))
        return pairs[: 2 * n + 1], vals, err[:n]

    def match_batch32_dev(self, n: int, d_blob: int, d_offs: int, d_hit: int, d_out: int, cap: int, d_err: int,
                          stream: int | None = None):
        self._check(self._lib.tm_match_batch32_dev(self._h, n, d_blob, d_offs, d_hit, d_out, cap, d_err, stream))

    def first_batch(self, blob: np.ndarray, offs: np.ndarray):
        """-> (value u32[n], found u8[n]: 1 hit, 0 none, 2 badarg, 3 > 65536 levels)."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        val = np.zeros(max(n, 1), dtype=np.uint32)
        found = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._lib.tm_first_batch(self._h, n, _ptr(blob), _ptr(offs), _ptr(val), _ptr(found)))
        return val[:n], found[:n]

    def matches_filter_batch(self, blob: np.ndarray, offs: np.ndarray, flags: np.ndarray | None = None):
        """matches_filter/3 for n subscription filters on the device (tm_matches_filter_ex;
        flags: TM_KEY_ESCAPED per filter given as an escaped word list, or None):
        -> (hit_offsets u64[n+1], values u32 in traversal order, err u8[n])."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        if flags is not None:
            flags = np.ascontiguousarray(flags, dtype=np.uint8)
        hit = np.zeros(n + 1, dtype=np.uint64)
        err = np.zeros(max(n, 1), dtype=np.uint8)
        cap = 1024
        while True:
            out = np.zeros(max(cap, 1), dtype=np.uint32)
            rc = self._lib.tm_matches_filter_ex(self._h, n, _ptr(blob), _ptr(offs), _ptr(flags), _ptr(hit), _ptr(out),
                                                cap, _ptr(err))
            if rc == TM_ECAP and int(hit[n]) > cap:
                cap = int(hit[n])
                continue
            self._check(rc)
            return hit, out[: int(hit[n])], err[:n]

    # ---- matching (device buffers, e.g. torch tensors' data_ptr())
    def match_batch_dev(self, n: int, d_blob: int, d_offs: int, d_hit: int, d_out: int, cap: int, d_err: int,
                        stream: int | None = None, order: int = TM_ORDER_TRAVERSAL, d_unique: int | None = None):
        self._check(self._lib.tm_match_batch_dev_ex(self._h, n, d_blob, d_offs, d_hit, d_out, cap, d_err, order,
                                                    d_unique, stream))

    def match_batch_dev_pairs(self, n: int, d_blob: int, d_offs: int, d_pairs: int, d_out: int, cap: int, d_err: int,
                              stream: int | None = None):
        """tm_match_batch_dev_pairs: per-topic (first position, count) u32 pairs, d_pairs[2 n] = total."""
        self._check(self._lib.tm_match_batch_dev_pairs(self._h, n, d_blob, d_offs, d_pairs, d_out, cap, d_err, stream))

    def sort_segments(self, n: int, d_hit: int, d_vals: int, cap: int, order: int = TM_ORDER_SORTED,
                      d_unique: int | None = None, stream: int | None = None):
        """tm_sort_segments: sort each of n CSR segments on the device in place."""
        self._check(self._lib.tm_sort_segments(self._h, n, d_hit, d_vals, cap, order, d_unique, stream))

    # ---- route fan-out (include/tmatch.h "Route fan-out")
    def set_dests(self, values, dests):
        """tm_set_dests: dests[i] becomes the destination id of values[i] (u32 each)."""
        values = np.ascontiguousarray(values, dtype=np.uint32)
        dests = np.ascontiguousarray(dests, dtype=np.uint32)
        if len(values) != len(dests):
            raise ValueError("set_dests: one destination per value")
        self._check(self._lib.tm_set_dests(self._h, len(values), _ptr(values), _ptr(dests)))

    def fanout_dev(self, n: int, d_hit: int, d_vals: int, cap: int, n_dests: int, d_dest_offs: int, d_out_topic: int,
                   d_out_value: int, d_dest_of: int | None = None, dest_len: int = 0, stream: int | None = None):
        """tm_fanout_dev on device pointers: the CSR (d_hit u64[n+1], d_vals)
        stably partitioned by destination into d_out_topic / d_out_value, bucket
        b at [d_dest_offs[b], d_dest_offs[b+1]) (u64[n_dests+2]; bucket n_dests:
        unrouted).  d_dest_of None: the table of set_dests."""
        self._check(self._lib.tm_fanout_dev(self._h, n, d_hit, d_vals, cap, d_dest_of, dest_len, n_dests, d_dest_offs,
                                            d_out_topic, d_out_value, stream))

    def fanout_dev_pairs(self, n: int, d_pairs: int, d_vals: int, cap: int, n_dests: int, d_dest_offs: int,
                         d_out_topic: int, d_out_value: int, d_dest_of: int | None = None, dest_len: int = 0,
                         stream: int | None = None):
        """tm_fanout_dev_pairs on device pointers: fanout_dev for a batch given as
        per-topic (first position, count) u32 pairs (d_pairs 8-byte aligned,
        [0, 2 n) read; match_batch_dev_pairs / match_batch32_pairs write them):
        the same outputs as fanout_dev on the CSR the spans stand for."""
        self._check(self._lib.tm_fanout_dev_pairs(self._h, n, d_pairs, d_vals, cap, d_dest_of, dest_len, n_dests,
                                                  d_dest_offs, d_out_topic, d_out_value, stream))

    def set_route_filters(self, values, filter_ids):
        """tm_set_route_filters: filter_ids[i] becomes the filter id (the To) of the
        route values[i] names (u32 each; NO_FILTER: none known)."""
        values = np.ascontiguousarray(values, dtype=np.uint32)
        filter_ids = np.ascontiguousarray(filter_ids, dtype=np.uint32)
        if len(values) != len(filter_ids):
            raise ValueError("set_route_filters: one filter id per value")
        self._check(self._lib.tm_set_route_filters(self._h, len(values), _ptr(values), _ptr(filter_ids)))

    def aggre_dev(self, n_dests: int, d_dest_offs: int, d_topic: int, d_value: int, cap: int, d_out_dest_offs: int,
                  d_out_topic: int, d_out_value: int, d_filter_of: int | None = None, filter_len: int = 0,
                  stream: int | None = None):
        """tm_aggre_dev on device pointers: a fan-out's output (d_dest_offs
        u64[n_dests+2], d_topic, d_value) without the entries whose predecessor
        in the same routed bucket has the same topic and the same filter, into
        d_out_* (which must not overlap the inputs); d_out_dest_offs
        u64[n_dests+2], the kept total last.  d_filter_of None: the table of
        set_route_filters."""
        self._check(self._lib.tm_aggre_dev(self._h, n_dests, d_dest_offs, d_topic, d_value, cap, d_filter_of, filter_len,
                                           d_out_dest_offs, d_out_topic, d_out_value, stream))

    @staticmethod
    def _out32(name, offs, n_dests, out, member=None, keys=(), cap=None, dcap=None):
        """The checks of a 32-bit call's caller-owned buffers, before the library
        is touched.  out: route_batch32's four arrays or dispatch_batch32's
        eight; member: publish_batch32's; keys: its key arrays (None: absent).
        -> (cap, dcap), by default all of the entry / the delivery arrays."""
        n = len(offs) - 1
        doff, err, head = out[0], out[3], out[4:5]
        entries = tuple(out[1:3]) + (() if member is None else (member,))
        deliveries = tuple(out[5:])
        if offs.dtype != np.uint32 or doff.dtype != np.uint32 or err.dtype != np.uint8 \
                or any(h.dtype != np.uint64 or len(h) < 2 for h in head) \
                or any(a.dtype != np.uint32 for a in entries + deliveries) or len(doff) < n_dests + 2 or len(err) < n:
            raise ValueError(f"{name}: u32 offsets and large enough outputs of the right dtype expected")
        if any(k is not None and (k.dtype != np.uint32 or len(k) < n) for k in keys):
            raise ValueError(f"{name}: one u32 key word per topic")
        room, droom = min(map(len, entries)), min(map(len, deliveries), default=0)
        cap, dcap = room if cap is None else cap, droom if dcap is None else dcap
        if cap > room or dcap > droom:
            raise ValueError(f"{name}: cap / dcap exceeds the output arrays")
        return cap, dcap

    def route_batch(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, cap: int | None = None,
                    aggre: bool = False):
        """tm_route_batch -> (dest_offsets u64[n_dests+2], topic u32[total],
        values u32[total], err u8[n]): destination b's (topic index, value)
        pairs are [dest_offsets[b], dest_offsets[b+1]), in topic order and
        traversal order inside a topic; bucket n_dests holds the values
        without a destination.  A cap that proves too small is retried once,
        sized from the returned bucket sizes.  aggre: TM_ROUTE_AGGRE -- the
        buckets after aggre/1 (set_route_filters), the kept total last."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        doff = np.zeros(n_dests + 2, dtype=np.uint64)
        err = np.zeros(max(n, 1), dtype=np.uint8)
        if cap is None:
            cap = max(4 * n, 1024)
        while True:
            topic = np.empty(max(cap, 1), dtype=np.uint32)
            vals = np.empty(max(cap, 1), dtype=np.uint32)
            rc = self._lib.tm_route_batch_ex(self._h, n, _ptr(blob), _ptr(offs), n_dests, _ptr(doff), _ptr(topic),
                                             _ptr(vals), cap, _ptr(err), TM_ROUTE_AGGRE if aggre else 0)
            if rc == TM_ECAP and int(doff[-1]) > cap:
                cap = int(doff[-1])
                continue
            self._check(rc)
            total = int(doff[-1])
            return doff, topic[:total], vals[:total], err[:n]

    def route_batch32(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, out, cap: int | None = None,
                      aggre: bool = False):
        """tm_route_batch32: route_batch with u32 topic offsets in and u32 bucket
        offsets out.  out = (dest_offsets u32[>= n_dests+2], topic u32[cap],
        values u32[cap], err u8[>= n]) -> (dest_offsets[:n_dests+2],
        topic[:total], values[:total], err[:n]) as views; in place (no staging,
        one fan-out launch) when every array comes from host_array() and the
        batch is a micro-batch (include/tmatch.h).  cap: use only that many
        entries of topic / values (default: all).  Raises TmError(TM_ECAP) when
        the entries do not fit (the offsets are valid: the total is the last).
        aggre: TM_ROUTE_AGGRE -- the buckets after aggre/1; TM_ECAP then when
        the entries BEFORE aggregation do not fit (the offsets are those sizes)."""
        n = len(offs) - 1
        doff, topic, vals, err = out
        cap, _ = self._out32("route_batch32", offs, n_dests, out, cap=cap)
        self._check(self._lib.tm_route_batch32_ex(self._h, n, _ptr(blob), _ptr(offs), n_dests, _ptr(doff), _ptr(topic),
                                                  _ptr(vals), cap, _ptr(err), TM_ROUTE_AGGRE if aggre else 0))
        total = int(doff[n_dests + 1])
        return doff[: n_dests + 2], topic[:total], vals[:total], err[:n]

    # ---- local dispatch (include/tmatch.h "Local dispatch on the device")
    def set_subscribers(self, values, lists):
        """tm_set_subscribers: lists[i] (u32 subscriber ids, in dispatch order)
        becomes the local subscriber list of route value values[i]."""
        values = np.ascontiguousarray(values, dtype=np.uint32)
        if len(values) != len(lists):
            raise ValueError("set_subscribers: one list per value")
        offs = np.zeros(len(values) + 1, dtype=np.uint64)
        if len(values):
            offs[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
        subs = np.zeros(max(int(offs[-1]), 1), dtype=np.uint32)
        for i, x in enumerate(lists):
            subs[int(offs[i]):int(offs[i + 1])] = np.asarray(x, dtype=np.uint32)
        self._check(self._lib.tm_set_subscribers(self._h, len(values), _ptr(values), _ptr(offs), _ptr(subs)))

    def dispatch_dev(self, n_dests: int, d_dest_offs: int, bucket: int, d_topic: int, d_value: int, cap: int,
                     d_out_head: int, d_out_topic: int, d_out_value: int, d_out_sub: int, out_cap: int,
                     d_out_offsets: int | None = None, d_sub_span: int | None = None, span_len: int = 0,
                     d_sub_pool: int | None = None, pool_len: int = 0, stream: int | None = None):
        """tm_dispatch_dev on device pointers: bucket `bucket` of a fan-out's or
        an aggre pass's output expanded to one (topic, value, subscriber)
        delivery per subscriber of each entry's value; d_out_head u64[2] = (the
        bucket's entries M, the deliveries T), the first min(T, out_cap) of them
        written; d_out_offsets (optional) u64[M + 1].  d_sub_span None: the
        table of set_subscribers."""
        self._check(self._lib.tm_dispatch_dev(self._h, n_dests, d_dest_offs, bucket, d_topic, d_value, cap, d_sub_span,
                                              span_len, d_sub_pool, pool_len, d_out_head, d_out_offsets, d_out_topic,
                                              d_out_value, d_out_sub, out_cap, stream))

    def dispatch_batch(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int, cap: int | None = None,
                       dcap: int | None = None, aggre: bool = False):
        """tm_dispatch_batch -> (route_batch's (dest_offsets, topic, values, err),
        (dtopic u32[T], dvalue u32[T], dsub u32[T])): the route buckets and the
        deliveries of bucket local_dest with the table of set_subscribers, in
        entry order and list order.  A cap that proves too small is retried,
        sized from what the call returned."""
        route, deliveries, _ = self._dispatch_loop(blob, offs, n_dests, local_dest, cap, dcap,
                                                   TM_ROUTE_AGGRE if aggre else 0)
        return route, deliveries

    def group_subs_dev(self, d_head: int, d_topic: int, d_value: int, d_sub: int, cap: int, d_out_ghead: int,
                       d_out_gsub: int, d_out_goff: int, gcap: int, d_out_topic: int, d_out_value: int, d_out_sub: int,
                       d_out_perm: int | None = None, stream: int | None = None):
        """tm_group_subs_dev on device pointers: the first min(d_head[1], cap)
        deliveries a dispatch wrote, stably sorted by subscriber into d_out_topic
        / d_out_value / d_out_sub (d_out_perm: the input positions); d_out_ghead
        u64[2] = (groups G, deliveries W), the first min(G, gcap) subscribers in
        d_out_gsub, their offsets and the last one's end in d_out_goff
        u64[gcap + 1]."""
        self._check(self._lib.tm_group_subs_dev(self._h, d_head, d_topic, d_value, d_sub, cap, d_out_ghead, d_out_gsub,
                                                d_out_goff, gcap, d_out_topic, d_out_value, d_out_sub, d_out_perm,
                                                stream))

    def deliver_batch(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int, cap: int | None = None,
                      dcap: int | None = None, gcap: int | None = None, aggre: bool = False):
        """tm_deliver_batch -> (route_batch's tuple, (dtopic, dvalue, dsub) u32[T]
        GROUPED by subscriber -- ascending ids, each subscriber's deliveries in
        dispatch_batch's order -- and (gsub u32[G], goff u64[G + 1]): subscriber
        gsub[g] owns the deliveries [goff[g], goff[g + 1]).  A cap that proves
        too small is retried, sized from what the call returned."""
        return self._deliver_loop(blob, offs, n_dests, local_dest, cap, dcap, TM_ROUTE_AGGRE if aggre else 0,
                                  1024 if gcap is None else gcap)

    def _dispatch_loop(self, blob, offs, n_dests, local_dest, cap, dcap, flags, pick=None):
        """dispatch_batch's and publish_batch's loop: allocate, call, grow what
        was short from what the call returned.  pick: (key_clientid, key_topic,
        seed) -- tm_publish_batch, else tm_dispatch_batch.
        -> (route tuple, deliveries, member or None)."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        doff = np.zeros(n_dests + 2, dtype=np.uint64)
        head = np.zeros(2, dtype=np.uint64)
        err = np.zeros(max(n, 1), dtype=np.uint8)
        if cap is None:
            cap = max(4 * n, 1024)
        if dcap is None:
            dcap = max(4 * n, 1024)
        for _ in range(4):
            topic, vals = (np.empty(max(cap, 1), dtype=np.uint32) for _ in range(2))
            member = None if pick is None else np.empty(max(cap, 1), dtype=np.uint32)
            dt, dv, ds = (np.empty(max(dcap, 1), dtype=np.uint32) for _ in range(3))
            args = (self._h, n, _ptr(blob), _ptr(offs), n_dests, local_dest, flags, _ptr(doff), _ptr(topic), _ptr(vals),
                    cap, _ptr(head), _ptr(dt), _ptr(dv), _ptr(ds), dcap)
            if pick is None:
                rc = self._lib.tm_dispatch_batch(*args, _ptr(err))
            else:
                rc = self._lib.tm_publish_batch(*args, _ptr(pick[0]), _ptr(pick[1]), pick[2], _ptr(member), _ptr(err))
            total, T = int(doff[-1]), int(head[1])
            if rc == TM_ECAP and pick is not None and total <= cap:
                # publish, dcap alone: the picks stand (the state has moved); only the dispatch is fetched again
                _, (dt, dv, ds), _ = self._dispatch_loop(blob, offs, n_dests, local_dest, cap, T, flags)
            elif rc == TM_ECAP and (total > cap or T > dcap):
                # (a publish made no pick: the state has not moved)
                cap, dcap = max(cap, total), max(dcap, T)
                continue
            else:
                self._check(rc)
            return (doff, topic[:total], vals[:total], err[:n]), (dt[:T], dv[:T], ds[:T]), \
                None if member is None else member[:total]
        raise TmError(TM_ECAP, f"{'dispatch_batch' if pick is None else 'publish_batch'}: the totals kept growing")

    def _deliver_loop(self, blob, offs, n_dests, local_dest, cap, dcap, flags, gcap):
        """_dispatch_loop's shape for tm_deliver_batch, with gcap as a third size
        -> (route tuple, grouped deliveries, (gsub, goff))."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        doff = np.zeros(n_dests + 2, dtype=np.uint64)
        head, ghead = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        err = np.zeros(max(n, 1), dtype=np.uint8)
        if cap is None:
            cap = max(4 * n, 1024)
        if dcap is None:
            dcap = max(4 * n, 1024)
        for _ in range(4):
            topic, vals = (np.empty(max(cap, 1), dtype=np.uint32) for _ in range(2))
            dt, dv, ds = (np.empty(max(dcap, 1), dtype=np.uint32) for _ in range(3))
            gsub, goff = np.empty(max(gcap, 1), dtype=np.uint32), np.zeros(gcap + 1, dtype=np.uint64)
            rc = self._lib.tm_deliver_batch(self._h, n, _ptr(blob), _ptr(offs), n_dests, local_dest, flags, _ptr(doff),
                                            _ptr(topic), _ptr(vals), cap, _ptr(head), _ptr(dt), _ptr(dv), _ptr(ds), dcap,
                                            _ptr(ghead), _ptr(gsub), _ptr(goff), gcap, _ptr(err))
            total, T, G = int(doff[-1]), int(head[1]), int(ghead[0])
            if rc == TM_ECAP and (total > cap or T > dcap or G > gcap):
                # (G counts the groups of the deliveries that fitted: at most T of them in the end)
                cap, dcap, gcap = max(cap, total), max(dcap, T), max(gcap, G if T <= dcap else min(T, max(4 * G, 1024)))
                continue
            self._check(rc)
            return (doff, topic[:total], vals[:total], err[:n]), (dt[:T], dv[:T], ds[:T]), (gsub[:G], goff[:G + 1])
        raise TmError(TM_ECAP, "deliver_batch: the totals kept growing")

    def dispatch_batch32(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int, out,
                         cap: int | None = None, dcap: int | None = None, aggre: bool = False):
        """tm_dispatch_batch32: dispatch_batch with u32 topic offsets in and u32
        bucket offsets out.  out = (dest_offsets u32[>= n_dests+2], topic
        u32[cap], values u32[cap], err u8[>= n], head u64[2], dtopic u32[dcap],
        dvalue u32[dcap], dsub u32[dcap]) -> ((dest_offsets[:n_dests+2],
        topic[:total], values[:total], err[:n]), (dtopic[:T], dvalue[:T],
        dsub[:T])) as views; in place (no staging, one synchronisation) when
        every array comes from host_array() and the batch is a micro-batch
        (include/tmatch.h).  cap / dcap: use only that many entries /
        deliveries of the arrays (default: all).  Raises TmError(TM_ECAP) when
        something does not fit: dest_offsets[n_dests+1] (before aggregation
        under aggre) and head[1] size the retry."""
        n = len(offs) - 1
        doff, topic, vals, err, head, dt, dv, ds = out
        cap, dcap = self._out32("dispatch_batch32", offs, n_dests, out, cap=cap, dcap=dcap)
        self._check(self._lib.tm_dispatch_batch32(self._h, n, _ptr(blob), _ptr(offs), n_dests, local_dest,
                                                  TM_ROUTE_AGGRE if aggre else 0, _ptr(doff), _ptr(topic), _ptr(vals),
                                                  cap, _ptr(head), _ptr(dt), _ptr(dv), _ptr(ds), dcap, _ptr(err)))
        total, T = int(doff[n_dests + 1]), int(head[1])
        return (doff[: n_dests + 2], topic[:total], vals[:total], err[:n]), (dt[:T], dv[:T], ds[:T])

    def deliver_batch32(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int, out,
                        cap: int | None = None, dcap: int | None = None, gcap: int | None = None, aggre: bool = False):
        """tm_deliver_batch32: deliver_batch with u32 topic offsets in and u32
        bucket and group offsets out.  out = dispatch_batch32's eight arrays,
        then (ghead u64[2], gsub u32[gcap], goff u32[gcap + 1]) ->
        (dispatch_batch32's two tuples, the deliveries GROUPED by subscriber,
        (gsub[:G], goff[:G + 1])) as views; in place (no staging, one
        synchronisation) when every array comes from host_array() and the batch
        is a micro-batch (include/tmatch.h).  gcap: use only that many groups
        of gsub / goff (default: all that both hold).  Raises TmError(TM_ECAP)
        when something does not fit: dest_offsets[n_dests+1], head[1] and
        ghead[0] size the retry."""
        n = len(offs) - 1
        if len(out) != 11:
            raise ValueError("deliver_batch32: out is dispatch_batch32's eight arrays, then ghead, gsub and goff")
        doff, topic, vals, err, head, dt, dv, ds, ghead, gsub, goff = out
        cap, dcap = self._out32("deliver_batch32", offs, n_dests, out[:8], cap=cap, dcap=dcap)
        if ghead.dtype != np.uint64 or len(ghead) < 2 or gsub.dtype != np.uint32 or goff.dtype != np.uint32 or len(goff) < 1:
            raise ValueError("deliver_batch32: ghead u64[2], gsub u32[gcap] and goff u32[gcap + 1] expected")
        groom = min(len(gsub), len(goff) - 1)
        gcap = groom if gcap is None else gcap
        if gcap < 0 or gcap > groom:
            raise ValueError("deliver_batch32: gcap exceeds the group arrays")
        self._check(self._lib.tm_deliver_batch32(self._h, n, _ptr(blob), _ptr(offs), n_dests, local_dest,
                                                 TM_ROUTE_AGGRE if aggre else 0, _ptr(doff), _ptr(topic), _ptr(vals), cap,
                                                 _ptr(head), _ptr(dt), _ptr(dv), _ptr(ds), dcap, _ptr(ghead), _ptr(gsub),
                                                 _ptr(goff), gcap, _ptr(err)))
        total, T, G = int(doff[n_dests + 1]), int(head[1]), int(ghead[0])
        return (doff[: n_dests + 2], topic[:total], vals[:total], err[:n]), (dt[:T], dv[:T], ds[:T]), \
            (gsub[:G], goff[: G + 1])

    # ---- shared-subscription pick (include/tmatch.h "Shared-subscription pick on the device")
    def set_share_slots(self, values, slots):
        """tm_set_share_slots: route value values[i] belongs to slot slots[i] (the
        caller's dense id of a {Group, To} pair; TM_SHARE_NONE: none)."""
        values = np.ascontiguousarray(values, dtype=np.uint32)
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        if len(values) != len(slots):
            raise ValueError("set_share_slots: one slot per value")
        self._check(self._lib.tm_set_share_slots(self._h, len(values), _ptr(values), _ptr(slots)))

    def set_share_members(self, slots, lists, n_local, meta):
        """tm_set_share_members: lists[i] (u32 member ids in subscribers/2's order,
        the n_local[i] local ones first) becomes slot slots[i]'s member list,
        meta[i] = strategy | init_strategy << 8.  Never touches a slot's state."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        n_local = np.ascontiguousarray(n_local, dtype=np.uint32)
        meta = np.ascontiguousarray(meta, dtype=np.uint32)
        if not len(slots) == len(lists) == len(n_local) == len(meta):
            raise ValueError("set_share_members: one list, n_local and meta per slot")
        offs = np.zeros(len(slots) + 1, dtype=np.uint64)
        if len(slots):
            offs[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
        mem = np.zeros(max(int(offs[-1]), 1), dtype=np.uint32)
        for i, x in enumerate(lists):
            mem[int(offs[i]):int(offs[i + 1])] = np.asarray(x, dtype=np.uint32)
        self._check(self._lib.tm_set_share_members(self._h, len(slots), _ptr(slots), _ptr(offs), _ptr(mem), _ptr(n_local),
                                                   _ptr(meta)))

    def share_state_set(self, slots, states):
        """tm_share_state_set: the slots' state words, on every device entry."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        states = np.ascontiguousarray(states, dtype=np.uint32)
        if len(slots) != len(states):
            raise ValueError("share_state_set: one state per slot")
        self._check(self._lib.tm_share_state_set(self._h, len(slots), _ptr(slots), _ptr(states)))

    def share_state_get(self, slots, dev: int = 0) -> np.ndarray:
        """tm_share_state_get: the slots' state words on device entry `dev`, after
        every pick queued there so far (TM_SHARE_UNDEF: never set)."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros(max(len(slots), 1), dtype=np.uint32)
        self._check(self._lib.tm_share_state_get(self._h, dev, len(slots), _ptr(slots), _ptr(out)))
        return out[:len(slots)]

    def share_pick_dev(self, n_dests: int, d_dest_offs: int, d_topic: int, d_value: int, cap: int, d_out_head: int,
                       d_out_member: int, d_key_clientid: int | None = None, d_key_topic: int | None = None,
                       n_topics: int = 0, seed: int = 0, d_slot_of: int | None = None, slot_of_len: int = 0,
                       d_slot_rec: int | None = None, n_slots: int = 0, d_pool: int | None = None, pool_len: int = 0,
                       d_state: int | None = None, stream: int | None = None):
        """tm_share_pick_dev on device pointers: one member (or TM_SHARE_NONE) per
        entry of an aggre pass's output into d_out_member, d_out_head u64[2] =
        (entries with a slot, entries with a pick); the slots' state words
        advance once.  d_slot_of None: the tables of set_share_slots /
        set_share_members and the index's own state."""
        self._check(self._lib.tm_share_pick_dev(self._h, n_dests, d_dest_offs, d_topic, d_value, cap, d_key_clientid,
                                                d_key_topic, n_topics, seed, d_slot_of, slot_of_len, d_slot_rec, n_slots,
                                                d_pool, pool_len, d_state, d_out_head, d_out_member, stream))

    def publish_batch(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int, cap: int | None = None,
                      dcap: int | None = None, key_clientid=None, key_topic=None, seed: int = 0):
        """tm_publish_batch -> (dispatch_batch's two tuples under aggre, member
        u32[K]): member[q] is the shared-subscription pick of kept entry q
        (TM_SHARE_NONE: none).  A cap that proves too small is retried, sized
        from what the call returned; the state moves only in the call that
        stands, unless dcap alone was short (the picks of that call stand, the
        retry picks again)."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        kc = None if key_clientid is None else np.ascontiguousarray(key_clientid, dtype=np.uint32)
        kt = None if key_topic is None else np.ascontiguousarray(key_topic, dtype=np.uint32)
        if any(k is not None and len(k) < n for k in (kc, kt)):
            raise ValueError("publish_batch: one key word per topic")
        return self._dispatch_loop(blob, offs, n_dests, local_dest, cap, dcap, TM_ROUTE_AGGRE, pick=(kc, kt, seed))

    # ---- picks grouped with the deliveries (include/tmatch.h, ABI minor 22)
    def set_member_subs(self, members, sub_ids):
        """tm_set_member_subs: sub_ids[i] becomes the local subscriber id of share
        member members[i] (u32 each; TM_SHARE_NONE: not a connection of this node)."""
        members = np.ascontiguousarray(members, dtype=np.uint32)
        sub_ids = np.ascontiguousarray(sub_ids, dtype=np.uint32)
        if len(members) != len(sub_ids):
            raise ValueError("set_member_subs: one subscriber id per member")
        self._check(self._lib.tm_set_member_subs(self._h, len(members), _ptr(members), _ptr(sub_ids)))

    def group_picks_dev(self, d_head: int, d_topic: int, d_value: int, d_sub: int, cap: int, n_dests: int,
                        d_dest_offs: int, d_etopic: int, d_evalue: int, d_member: int, ecap: int, d_out_ghead: int,
                        d_out_gsub: int, d_out_goff: int, gcap: int, d_out_topic: int, d_out_value: int, d_out_sub: int,
                        out_cap: int, d_out_src: int | None = None, d_sub_of: int | None = None, sub_of_len: int = 0,
                        stream: int | None = None):
        """tm_group_picks_dev on device pointers: the first min(d_head[1], cap)
        deliveries a dispatch wrote and the local picks (d_sub_of[d_member[q]] !=
        TM_SHARE_NONE) among the first min(d_dest_offs[n_dests + 1], ecap)
        aggregated entries, merged by message and stably sorted by subscriber
        into d_out_topic / d_out_value / d_out_sub (d_out_src: a delivery's
        position, or W + a pick's rank); d_out_ghead u64[2] = (groups G, merged
        deliveries N), groups as group_subs_dev.  d_sub_of None: the table of
        set_member_subs."""
        self._check(self._lib.tm_group_picks_dev(self._h, d_head, d_topic, d_value, d_sub, cap, n_dests, d_dest_offs,
                                                 d_etopic, d_evalue, d_member, ecap, d_sub_of, sub_of_len, d_out_ghead,
                                                 d_out_gsub, d_out_goff, gcap, d_out_topic, d_out_value, d_out_sub,
                                                 d_out_src, out_cap, stream))

    def publish_deliver_batch(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int,
                              cap: int | None = None, dcap: int | None = None, gcap: int | None = None,
                              key_clientid=None, key_topic=None, seed: int = 0):
        """tm_publish_deliver_batch -> (route tuple, (dtopic, dvalue, dsub) u32[N]
        -- the direct deliveries and the local picks merged and GROUPED by
        subscriber --, member u32[K], (gsub u32[G], goff u64[G + 1]), T the
        direct deliveries' number).  cap and dcap are sized from a first try:
        a call that returns TM_ECAP for either made no pick and moved no state,
        and is repeated once.  A gcap that proves too small is NOT retried (the
        picks of that call stand): the groups are read off the sorted dsub."""
        n = len(offs) - 1
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        kc = None if key_clientid is None else np.ascontiguousarray(key_clientid, dtype=np.uint32)
        kt = None if key_topic is None else np.ascontiguousarray(key_topic, dtype=np.uint32)
        if any(k is not None and len(k) < n for k in (kc, kt)):
            raise ValueError("publish_deliver_batch: one key word per topic")
        doff = np.zeros(n_dests + 2, dtype=np.uint64)
        head, ghead = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        err = np.zeros(max(n, 1), dtype=np.uint8)
        cap = max(4 * n, 1024) if cap is None else cap
        dcap = max(8 * n, 2048) if dcap is None else dcap
        gcap = 1024 if gcap is None else gcap
        for attempt in range(3):
            topic, vals, member = (np.empty(max(cap, 1), dtype=np.uint32) for _ in range(3))
            dt, dv, ds = (np.empty(max(dcap, 1), dtype=np.uint32) for _ in range(3))
            gsub, goff = np.empty(max(gcap, 1), dtype=np.uint32), np.zeros(gcap + 1, dtype=np.uint64)
            rc = self._lib.tm_publish_deliver_batch(self._h, n, _ptr(blob), _ptr(offs), n_dests, local_dest, TM_ROUTE_AGGRE,
                                                    _ptr(doff), _ptr(topic), _ptr(vals), cap, _ptr(head), _ptr(dt),
                                                    _ptr(dv), _ptr(ds), dcap, _ptr(kc), _ptr(kt), seed, _ptr(member),
                                                    _ptr(ghead), _ptr(gsub), _ptr(goff), gcap, _ptr(err))
            total, T = int(doff[-1]), int(head[1])
            if rc == TM_ECAP and (total > cap or T + total > dcap):
                # no pick was made and no state moved: sized from what came back (under total > cap the
                # un-aggregated total, an upper bound of K)
                cap, dcap = max(cap, total), max(dcap, T + total)
                continue
            G, N = int(ghead[0]), int(ghead[1])
            if rc == TM_ECAP and G > gcap:
                # the picks stand and the grouped arrays are complete: the groups from the sorted subscribers
                s = ds[:N]
                starts = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1]))) if N else np.zeros(0, np.int64)
                gsub, goff = s[starts].copy(), np.concatenate((starts, [N])).astype(np.uint64)
            else:
                self._check(rc)
                gsub, goff = gsub[:G], goff[:G + 1]
            return (doff, topic[:total], vals[:total], err[:n]), (dt[:N], dv[:N], ds[:N]), member[:total], \
                (gsub, goff), T
        raise TmError(TM_ECAP, "publish_deliver_batch: the totals kept growing")

    def publish_batch32(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int, out, member,
                        key_clientid=None, key_topic=None, seed: int = 0, cap: int | None = None,
                        dcap: int | None = None):
        """tm_publish_batch32: publish_batch with u32 topic offsets in and u32
        bucket offsets out, over caller-owned buffers.  out: dispatch_batch32's
        eight arrays; member u32[>= cap]; key_clientid / key_topic: u32[>= n] or
        None -> (dispatch_batch32's two tuples under aggre, member[:K]) as
        views.  In place (no staging, one synchronisation) when every array
        comes from host_array() and the batch is a micro-batch
        (include/tmatch.h).  Raises TmError(TM_ECAP) when something does not
        fit: from cap (dest_offsets[n_dests+1] > cap) no pick was made and no
        state moved; from dcap alone (head[1] > dcap) the picks stand."""
        n = len(offs) - 1
        doff, topic, vals, err, head, dt, dv, ds = out
        cap, dcap = self._out32("publish_batch32", offs, n_dests, out, member, (key_clientid, key_topic), cap, dcap)
        self._check(self._lib.tm_publish_batch32(self._h, n, _ptr(blob), _ptr(offs), n_dests, local_dest, TM_ROUTE_AGGRE,
                                                 _ptr(doff), _ptr(topic), _ptr(vals), cap, _ptr(head), _ptr(dt), _ptr(dv),
                                                 _ptr(ds), dcap, _ptr(key_clientid), _ptr(key_topic), seed, _ptr(member),
                                                 _ptr(err)))
        total, T = int(doff[n_dests + 1]), int(head[1])
        return (doff[: n_dests + 2], topic[:total], vals[:total], err[:n]), (dt[:T], dv[:T], ds[:T]), member[:total]

    def publish_deliver_batch32(self, blob: np.ndarray, offs: np.ndarray, n_dests: int, local_dest: int, out, member,
                                key_clientid=None, key_topic=None, seed: int = 0, cap: int | None = None,
                                dcap: int | None = None, gcap: int | None = None):
        """tm_publish_deliver_batch32: publish_deliver_batch with u32 topic offsets
        in and u32 bucket and group offsets out, over caller-owned buffers.
        out: deliver_batch32's eleven arrays; member u32[>= cap]; key_clientid /
        key_topic: u32[>= n] or None -> (the route tuple, (dtopic, dvalue,
        dsub)[:N] -- the direct deliveries and the local picks merged and
        GROUPED by subscriber --, member[:K], (gsub[:G], goff[:G + 1]), T) as
        views.  In place (no staging, one synchronisation) when every array
        comes from host_array() and the batch is a micro-batch
        (include/tmatch.h).  Raises TmError(TM_ECAP) when cap or dcap is short
        (dest_offsets[n_dests+1] > cap or head[1] + dest_offsets[n_dests+1] >
        dcap): no pick was made and no state moved, the same sizes size the
        retry.  A gcap that proves too small raises nothing: the picks of the
        call stand, the grouped arrays are complete, and the group bounds are
        read off the sorted dsub (fresh arrays instead of views)."""
        n = len(offs) - 1
        if len(out) != 11:
            raise ValueError("publish_deliver_batch32: out is dispatch_batch32's eight arrays, then ghead, gsub and goff")
        doff, topic, vals, err, head, dt, dv, ds, ghead, gsub, goff = out
        cap, dcap = self._out32("publish_deliver_batch32", offs, n_dests, out[:8], member, (key_clientid, key_topic), cap,
                                dcap)
        if ghead.dtype != np.uint64 or len(ghead) < 2 or gsub.dtype != np.uint32 or goff.dtype != np.uint32 or len(goff) < 1:
            raise ValueError("publish_deliver_batch32: ghead u64[2], gsub u32[gcap] and goff u32[gcap + 1] expected")
        groom = min(len(gsub), len(goff) - 1)
        gcap = groom if gcap is None else gcap
        if gcap < 0 or gcap > groom:
            raise ValueError("publish_deliver_batch32: gcap exceeds the group arrays")
        rc = self._lib.tm_publish_deliver_batch32(self._h, n, _ptr(blob), _ptr(offs), n_dests, local_dest, TM_ROUTE_AGGRE,
                                                  _ptr(doff), _ptr(topic), _ptr(vals), cap, _ptr(head), _ptr(dt), _ptr(dv),
                                                  _ptr(ds), dcap, _ptr(key_clientid), _ptr(key_topic), seed, _ptr(member),
                                                  _ptr(ghead), _ptr(gsub), _ptr(goff), gcap, _ptr(err))
        if rc not in (TM_OK, TM_ECAP):
            self._check(rc)
        total, T = int(doff[n_dests + 1]), int(head[1])
        G, N = int(ghead[0]), int(ghead[1])
        if rc == TM_ECAP and not (total <= cap and T + total <= dcap and G > gcap):
            self._check(rc)   # cap or dcap: nothing moved
        if rc == TM_ECAP:
            # the picks stand and the grouped arrays are complete: the groups from the sorted subscribers
            s = ds[:N]
            starts = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1]))) if N else np.zeros(0, np.int64)
            groups = (s[starts].copy(), np.concatenate((starts, [N])).astype(np.uint32))
        else:
            groups = (gsub[:G], goff[: G + 1])
        return (doff[: n_dests + 2], topic[:total], vals[:total], err[:n]), (dt[:N], dv[:N], ds[:N]), member[:total], \
            groups, T

    def release_stream(self, stream: int | None):
        """Drop the batch scratch the library keeps for `stream`."""
        self._check(self._lib.tm_stream_release(self._h, stream))

    def profile(self, enable: bool = True):
        self._check(self._lib.tm_profile_enable(self._h, int(enable)))

    def profile_read(self, reset: bool = True):
        """-> (walk kernel ms, whole batch ms, batches) accumulated on the device."""
        w, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self._check(self._lib.tm_profile_read(self._h, C.byref(w), C.byref(b), C.byref(n), int(reset)))
        return w.value, b.value, n.value

    def replica_stats(self, r: int) -> tuple[int, int]:
        """-> (host-API batches replica r served, its device)."""
        b, d = C.c_uint64(), C.c_int32()
        self._check(self._lib.tm_replica_stats(self._h, r, C.byref(b), C.byref(d)))
        return b.value, d.value

    def debug_set(self, key: int, value: int):
        """tm_debug_set (test hooks, include/tmatch.h)."""
        self._check(self._lib.tm_debug_set(self._h, key, value))

    def debug_get(self, key: int) -> int:
        v = C.c_uint64()
        self._check(self._lib.tm_debug_get(self._h, key, C.byref(v)))
        return v.value

    def stats(self) -> dict:
        s = tm_stats_t()
        self._check(self._lib.tm_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in tm_stats_t._fields_}


class Retained:
    """Owning handle of one device-resident retained-message store (tm_retained*,
    include/tmatch.h "The retained-message store"): stored topic names with a
    caller-chosen u32 value and an expiry each, looked up by subscription
    filters (emqx_retainer_mnesia:match_messages/3) on the GPU."""

    def __init__(self, device: int = -1, initial_rows: int = 0, tail_max: int = 0):
        if not _gpu_present():
            raise NativeUnavailable("no HIP device visible: the retained store runs on the GPU only")
        self._lib = load_library()
        opts = tm_retained_opts(initial_rows, tail_max)
        h = C.c_void_p()
        rc = self._lib.tm_retained_create(device, C.byref(opts), C.byref(h))
        if rc != TM_OK:
            raise TmError(rc, self._lib.tm_retained_last_error(None).decode())
        self._h = h

    def _check(self, rc):
        if rc != TM_OK:
            cls = DeviceError if rc == TM_EDEVICE else TmError
            raise cls(rc, self._lib.tm_retained_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tm_retained_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def put(self, topics, values, expiry_ms=None) -> np.ndarray:
        """store_retained for a batch -> codes (0 replaced, 1 new, 2 invalid topic: nothing stored)"""
        blob, offs = pack_strings(topics)
        return self.put_packed(blob, offs, values, expiry_ms)

    def put_packed(self, blob, offs, values, expiry_ms=None) -> np.ndarray:
        """put() over topics already packed (pack_strings' form)"""
        n = len(offs) - 1
        blob, offs = np.ascontiguousarray(blob, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint64)
        values = np.ascontiguousarray(values, dtype=np.uint32)
        exp = None if expiry_ms is None else np.ascontiguousarray(expiry_ms, dtype=np.uint64)
        if len(values) != n or (exp is not None and len(exp) != n):
            raise ValueError("a value (and an expiry) per topic")
        code = np.zeros(n, np.uint8)
        self._check(self._lib.tm_retained_put(self._h, n, _ptr(blob), _ptr(offs), _ptr(values), _ptr(exp), _ptr(code)))
        return code

    def delete(self, topics) -> np.ndarray:
        """delete_message for exact topics -> found flags"""
        blob, offs = pack_strings(topics)
        found = np.zeros(len(offs) - 1, np.uint8)
        self._check(self._lib.tm_retained_delete(self._h, len(found), _ptr(blob), _ptr(offs), _ptr(found)))
        return found.astype(bool)

    def get(self, topics, now_ms: int = 0):
        """read_message (expiry == 0 or expiry >= now_ms) -> (values, found flags)"""
        blob, offs = pack_strings(topics)
        n = len(offs) - 1
        vals, found = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._check(self._lib.tm_retained_get(self._h, n, _ptr(blob), _ptr(offs), now_ms, _ptr(vals), _ptr(found)))
        return vals, found.astype(bool)

    def match_packed(self, blob, offs, now_ms: int = 0):
        """tm_retained_match over packed filters -> (offsets[n + 1], values, err[n]); sizes, then fills"""
        n = len(offs) - 1
        hit = np.zeros(n + 1, np.uint64)
        err = np.zeros(n, np.uint8)
        rc = self._lib.tm_retained_match(self._h, n, _ptr(blob), _ptr(offs), now_ms, _ptr(hit), None, 0, _ptr(err))
        if rc == TM_ECAP:
            vals = np.zeros(int(hit[n]), np.uint32)
            rc = self._lib.tm_retained_match(self._h, n, _ptr(blob), _ptr(offs), now_ms, _ptr(hit), _ptr(vals), len(vals),
                                             _ptr(err))
        else:
            vals = np.zeros(0, np.uint32)
        self._check(rc)
        return hit, vals, err

    def match(self, filters, now_ms: int = 0):
        """match_messages for a batch of filters (expiry == 0 or expiry > now_ms) -> one array of values per filter,
        in no particular order; an invalid filter ('#' not last) gives an empty one"""
        blob, offs = pack_strings(filters)
        hit, vals, _ = self.match_packed(blob, offs, now_ms)
        return [vals[int(hit[i]):int(hit[i + 1])] for i in range(len(offs) - 1)]

    def match_page_packed(self, blob, offs, now_ms: int = 0, cursors=None, limit: int = 1000, scan_rows: int = 0):
        """tm_retained_match_page over packed filters -> (offsets[n + 1], values, cursors[n], err[n]): one buffer of
        n * limit values, one call"""
        n = len(offs) - 1
        if limit < 1:
            raise ValueError("a page takes at least one value")
        cur = None if cursors is None else np.ascontiguousarray(cursors, dtype=np.uint64)
        if cur is not None and len(cur) != n:
            raise ValueError("a cursor per filter")
        hit = np.zeros(n + 1, np.uint64)
        vals = np.empty(n * limit, np.uint32)
        out_cur = np.zeros(n, np.uint64)
        err = np.zeros(n, np.uint8)
        self._check(self._lib.tm_retained_match_page(self._h, n, _ptr(blob), _ptr(offs), now_ms, _ptr(cur), limit, scan_rows,
                                                     _ptr(hit), _ptr(vals), len(vals), _ptr(out_cur), _ptr(err)))
        return hit, vals[: int(hit[n])], out_cur, err

    def match_page(self, filters, now_ms: int = 0, cursors=None, limit: int = 1000, scan_rows: int = 0):
        """One page of match_messages/3 for each filter (emqx_retainer_mnesia.erl:288-304): at most `limit` values
        each, in scan order, from its cursor on (None: all from the start) -> (lists, cursors, err).  A cursor of
        TM_RET_CURSOR_DONE is the end; err[i] == TM_RET_ESTALE: the store compacted since the cursor was handed out
        (pin() prevents that), start again; scan_rows bounds the rows a filter examines in this call (a short page
        with a live cursor is then legal)."""
        blob, offs = pack_strings(filters)
        hit, vals, cur, err = self.match_page_packed(blob, offs, now_ms, cursors, limit, scan_rows)
        return [vals[int(hit[i]):int(hit[i + 1])] for i in range(len(offs) - 1)], cur, err

    def pin(self):
        """a holder of open cursors more: the store does not compact until every holder has unpinned"""
        self._check(self._lib.tm_retained_pin(self._h))

    def unpin(self):
        """... and one fewer; the last one compacts if a compaction is due or the tail is past tail_max"""
        self._check(self._lib.tm_retained_unpin(self._h))

    def expire(self, deadline_ms: int, limit: int = 0):
        """clear_expired -> (complete, values of the rows deleted)"""
        st = self.stats()
        out = np.zeros(max(int(limit) if limit else st["live_rows"], 1), np.uint32)
        n, complete = C.c_uint64(), C.c_int()
        self._check(self._lib.tm_retained_expire(self._h, deadline_ms, limit, _ptr(out), len(out), C.byref(n),
                                                 C.byref(complete)))
        return bool(complete.value), out[: n.value]

    def compact(self):
        self._check(self._lib.tm_retained_compact(self._h))

    def stats(self) -> dict:
        st = tm_retained_stats_t()
        self._check(self._lib.tm_retained_stats(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}
