"""The numpy definition of tm_group_subs_dev in include/tmatch.h, shared by
tests/test_gpu_group.py, tests/test_gpu_deliver_batch.py (the yardstick) and
tests/test_group_cpu.py (which checks the yardstick itself against a plain
dict-of-lists grouping)."""
import numpy as np


def group_ref(head, topic, value, sub, cap, gcap):
    """-> (ghead [G, W], out_topic, out_value, out_sub, out_perm: W each,
    out_gsub: the first Gw = min(G, gcap), out_goff: Gw + 1 u64)"""
    W = min(int(head[1]), cap)
    s = np.asarray(sub, np.uint32)[:W]
    p = np.argsort(s, kind="stable").astype(np.uint32)
    gs, cnt = np.unique(s, return_counts=True)
    G = len(gs)
    Gw = min(G, gcap)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    return ([G, W], np.asarray(topic, np.uint32)[:W][p], np.asarray(value, np.uint32)[:W][p], s[p], p,
            gs[:Gw].astype(np.uint32), off[:Gw + 1])


def group_by_dict(topic, value, sub):
    """the same grouping with no sort at all: {sub: [(position, topic, value)]} in input order"""
    d = {}
    for i, (t, v, s) in enumerate(zip(topic, value, sub)):
        d.setdefault(int(s), []).append((i, int(t), int(v)))
    return d
