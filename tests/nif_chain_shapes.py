"""The small indexes of tests/test_gpu_nif_chain.py as plain tables, and their
totals computed WITHOUT a device: the oracle (oracle/pyoracle.py) gives each
topic's values in traversal order, numpy applies the destination table, the
header's aggre/1 rule and the subscriber table.  The GPU test asserts these
totals against a fresh set's first capacities before it runs a batch, and
tests/test_nif_chain_shapes_cpu.py does the same with no GPU at all, so a shape
that would not force the rerun it is meant to force fails here first.

Every shape is nv filters of one kind ('#' unless said otherwise), value v on
destination v % 3 (none when v % 11 == 5: the bucket past the last), the local
node is destination 0.  Each value is its own filter id, except that v + 3
shares v's when v % 12 == 1 -- two REMOTE entries next to each other in bucket
1, so aggre/1 drops one per topic and K < total.  The first `sub_values` local
values have `subs_per` subscribers of their own (ids 1000 v + r).  Every odd
value has a shared-subscription slot of 1 to 5 members, strategy slot % 7; a
third of the members are connections of this node and subscribe directly as
well, a third are local connections with ids of their own, a third remote.
"""
import numpy as np

from pyoracle import Oracle

NONE = 0xFFFFFFFF
HASH_TOPIC, HASH_CLIENTID, ROUND_ROBIN_PER_GROUP = 6, 5, 2

# nv: values; sub_values: local values that have subscribers (None: all); subs_per: subscribers each
SHAPES = {
    "thin": dict(nv=200, sub_values=50, subs_per=1),        # 20 topics: total 4,000, T 1,000
    "thick": dict(nv=200, sub_values=None, subs_per=2),     # 20 topics: total 4,000, T 2,440
    "deliveries": dict(nv=60, sub_values=None, subs_per=11),   # 20 topics: total 1,200, T 4,180
    "wide": dict(nv=30, sub_values=None, subs_per=300),     # 2,700 distinct subscribers: G = T per topic
    "tiny": dict(nv=6, sub_values=None, subs_per=2, flt=b"a/+"),
    "threads": dict(nv=9, sub_values=None, subs_per=3, threads=True),
}


class FatTables:
    def __init__(self, nv, sub_values, subs_per, flt=b"#", threads=False):
        self.nv, self.flt, self.n_dests, self.local = nv, flt, 3, 0
        v = np.arange(nv, dtype=np.uint32)
        self.dest_of = np.where(v % 11 == 5, NONE, v % 3).astype(np.uint32)
        self.filt_of = v.copy()
        pair = v[(v % 12 == 1) & (v + 3 < nv)]
        self.filt_of[pair + 3] = pair
        local = [int(x) for x in v[self.dest_of == self.local]]
        self.subs = {x: [1000 * x + r for r in range(subs_per)] for x in local[:sub_values]}
        direct = [s for x in self.subs for s in self.subs[x]]
        self.slot_values = [int(x) for x in v[v % 2 == 1]]
        ns = len(self.slot_values)
        self.members = [[8 * s + j for j in range(1 + s % 5)] for s in range(ns)]
        self.meta = [s % 7 | HASH_TOPIC << 8 for s in range(ns)]
        if threads:   # slot 0: round_robin_per_group over five remote members; the others pick by a hash, statelessly
            self.members[0] = [900 + j for j in range(5)]
            self.members[1:] = [[8 * s + j for j in range(3)] for s in range(1, ns)]
            self.meta = [ROUND_ROBIN_PER_GROUP] + [(HASH_CLIENTID, HASH_TOPIC)[s % 2] for s in range(1, ns)]
        self.n_local = [min(len(m), s % 3) for s, m in enumerate(self.members)]
        top = max(max(m) for m in self.members) + 1
        self.sub_of = np.full(top, NONE, np.uint32)
        for m in range(min(top, 8 * ns)):
            if m % 3 == 0:
                self.sub_of[m] = direct[(7 * m) % len(direct)] if direct else 700_000 + m
            elif m % 3 == 1:
                self.sub_of[m] = 800_000 + m


def plan(tab, topics):
    """-> {total: entries before aggre/1, K: after, T: the local bucket's deliveries, G: its distinct subscribers}"""
    o = Oracle()
    for v in range(tab.nv):
        o.insert(tab.flt, v)
    o.prepare()
    total = K = T = 0
    seen = set()
    for t in topics:
        m = o.matches(t)
        if m is None:
            continue
        m = np.asarray(m, np.uint32)
        total += len(m)
        bucket = np.minimum(tab.dest_of[m], tab.n_dests)
        for d in range(tab.n_dests + 1):
            mine = m[bucket == d]
            f = tab.filt_of[mine]
            keep = np.ones(len(mine), bool)
            if d < tab.n_dests and len(mine) > 1:
                keep[1:] = f[1:] != f[:-1]      # (adjacent entries of one topic with one filter id: the first stays)
            K += int(keep.sum())
            if d == tab.local:
                for x in mine[keep].tolist():
                    T += len(tab.subs.get(x, ()))
                    seen.update(tab.subs.get(x, ()))
    return dict(n=len(topics), total=total, K=K, T=T, G=len(seen))


ONE_WORKGROUP = "total <= 16384 and T + K <= 8192"   # the in-place endings' bounds (emqx_amd/csrc/tm_dev.h)
# case -> (shape, topics, what must hold between the totals and a fresh set's first capacities: `cap` words of
# entries / deliveries / groups, `pd_dcap` words of tmn_publish_deliver's deliveries)
CASES = {
    "publish-entries": ("thick", 20, ("total > cap", "T <= cap", "K < total", "K <= 16384")),
    "publish-deliveries": ("deliveries", 20, ("total <= cap", "T > cap")),
    "pd-entries": ("thin", 20, ("total > cap", "T + K <= pd_dcap", "K < total", ONE_WORKGROUP)),
    "pd-deliveries": ("deliveries", 20, ("total <= cap", "T + K > pd_dcap", "T <= pd_dcap", ONE_WORKGROUP)),
    "pd-both": ("thick", 20, ("total > cap", "T + K > pd_dcap", "K < total", ONE_WORKGROUP)),
    "deliver-entries": ("thin", 20, ("total > cap", "T <= cap", "G <= cap")),
    "deliver-deliveries": ("wide", 2, ("total <= cap", "T > cap", "G > cap")),
    "deliver-groups": ("wide", 1, ("total <= cap", "G > cap")),
    "deliver-groups-dispatch-before": ("wide", 2, ("total <= cap", "T > cap")),
}


def topics_of(n):
    return [b"t/%d" % i for i in range(n)]


def check_case(case, ids_per_topic, first_cap):
    """the case's totals (plan) with the first capacities -- first_cap(words): what a fresh buffer asked to hold
    `words` words ends up with -- and every condition of the case asserted -> the figures"""
    shape, n, conds = CASES[case]
    p = plan(FatTables(**SHAPES[shape]), topics_of(n))
    want = ids_per_topic * n + 1024
    p.update(cap=first_cap(want), pd_dcap=first_cap(2 * want))
    for cond in conds:
        assert eval(cond, {}, dict(p)), f"{case}: the shape does not land where it was meant to: not {cond} with {p}"
    return p
