"""The numpy definition of tm_group_picks_dev in include/tmatch.h, shared by
tests/test_gpu_group_picks.py, tests/test_gpu_publish_deliver_batch.py (the
yardstick) and tests/test_publish_deliver_cpu.py (which checks the yardstick
itself against a plain dict-of-lists construction)."""
import numpy as np

NONE = 0xFFFFFFFF


def group_picks_ref(head, topic, value, sub, cap, n_dests, doff, etopic, evalue, member, ecap, sub_of, out_cap, gcap):
    """-> (ghead [G, N], out_topic, out_value, out_sub, out_src: the first
    min(N, out_cap) each, out_gsub: the first Gw = min(G, gcap), out_goff: Gw +
    1 u64, W, P)"""
    W = min(int(head[1]), cap)
    E = min(int(doff[n_dests + 1]), ecap)
    sub_of = np.asarray(sub_of, np.uint32)
    m = np.asarray(member, np.uint32)[:E]
    ls = np.full(E, NONE, np.uint32)
    ok = m < len(sub_of)
    ls[ok] = sub_of[m[ok]]
    pq = np.nonzero(ls != NONE)[0]
    P = len(pq)
    N = W + P
    t = np.concatenate([np.asarray(topic, np.uint32)[:W], np.asarray(etopic, np.uint32)[:E][pq]])
    v = np.concatenate([np.asarray(value, np.uint32)[:W], np.asarray(evalue, np.uint32)[:E][pq]])
    s = np.concatenate([np.asarray(sub, np.uint32)[:W], ls[pq]])
    p = np.lexsort((t, s)).astype(np.uint32)   # by subscriber, then message, then place: stable
    keep = min(N, out_cap)
    gs, cnt = np.unique(s, return_counts=True)
    G = len(gs)
    Gw = min(G, gcap)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    return ([G, N], t[p][:keep], v[p][:keep], s[p][:keep], p[:keep], gs[:Gw].astype(np.uint32), off[:Gw + 1], W, P)


def group_picks_by_dict(topic, value, sub, etopic, evalue, local_sub):
    """the same lists with no sort over the whole: {sub: [(src, topic, value)]},
    a subscriber's direct deliveries (src = position) and its picks (src = W +
    rank among the local picks; local_sub[q] NONE: not one) gathered message by
    message, the directs of a message first"""
    W = len(sub)
    per = {}   # sub -> {message: ([direct], [pick])}
    for i, (t, v, s) in enumerate(zip(topic, value, sub)):
        per.setdefault(int(s), {}).setdefault(int(t), ([], []))[0].append((i, int(t), int(v)))
    r = 0
    for q, ls in enumerate(local_sub):
        if int(ls) == NONE:
            continue
        per.setdefault(int(ls), {}).setdefault(int(etopic[q]), ([], []))[1].append((W + r, int(etopic[q]), int(evalue[q])))
        r += 1
    return {s: [x for msg in sorted(m) for x in m[msg][0] + m[msg][1]] for s, m in per.items()}
