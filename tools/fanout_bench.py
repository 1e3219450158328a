#!/usr/bin/env python3
"""Route fan-out: tm_fanout_dev against what a user would write with torch.

Builds a C3-style index (emqx_amd.workload, --filters keys), matches ONE batch
of --batch topics with tm_match_batch_dev, and then regroups that CSR by
destination two ways on the same GPU:

  hip    tm_fanout_dev (emqx_amd/csrc/tm_fanout.hip)
  torch  torch.sort(dest_of[values], stable=True); topic =
         repeat_interleave(arange(n), counts); the two gathers by the sort's
         permutation; the bucket offsets by bincount + cumsum (every value
         of the batch has a destination, so this shortest form is exact)

for 16 destinations (one pass) and 4,096 (two passes).  Both results are
compared first (they must be identical), then timed with HIP events: a
warm-up, then --reps repetitions, the two interleaved; median and spread
(min, p10, p90, max) per path.  Bytes are the algorithm's, per entry and pass:
4 read (value) + 4 gathered (dest_of) + 8 written (topic, value), plus the
n + 1 offsets read and the n_dests + 2 written.  One JSON line per destination
count on stdout.

--form csr|pairs|both (default csr: the lines above, unchanged).  pairs / both
add, per destination count, the same batch matched with
tm_match_batch_dev_pairs (its cap sized in an untimed pass: the CSR's total +
4096 x the most hits of one topic, the extent checked against it) and

  fanout_call  tm_fanout_dev on the CSR against tm_fanout_dev_pairs on the
               pairs, outputs compared first (they must be identical)
  pipeline     match + fan-out on one stream: tm_match_batch_dev +
               tm_fanout_dev against tm_match_batch_dev_pairs +
               tm_fanout_dev_pairs

timed the same way (the two forms alternating), and one synthetic line with
no index (synthetic_skew): the same number of entries over the same number of
topics once spread evenly and once with 64 topics holding half of them, both
calls on each -- what skew costs.  --form pairs leaves the torch line out.

--small: the NIF's micro-batches instead (nothing of the above runs): the same
index with 16 destinations set through tm_set_dests, batches of 64, 1,024,
4,096 and 16,384 topics in host_array buffers, timed host to host
(perf_counter around the call: 20 warm-up and 200 timed repetitions, the legs
interleaved), one JSON line per batch size with three legs:

  route_batch      (a) tm_route_batch, the staged product path
  match32_pairs    (b) tm_match_batch32_pairs alone: the match with no fan-out
  route_batch32    (c) tm_route_batch32, in place

(a)'s and (c)'s outputs are compared first (they must be identical); the line
also says which fan-out (c) took (TM_DEBUG_ROUTE_ONE / _GRID).

--group: deliveries grouped by subscriber (nothing of the first part runs, no
index): 1M synthetic deliveries whose subscriber ids come from 1,000 and from
1M pids, uniform and skewed (one pid holding half); tm_group_subs_dev against
the torch composition on the same device tensors -- torch.sort(stable=True),
unique_consecutive with counts, cumsum, the two gathers -- outputs compared
first (identical), then interleaved under HIP events; one JSON line per input
with the digit passes the call ran and skipped.  --small --group: the --small
index with a subscriber table of dense ids and one fan-in consumer;
tm_deliver_batch beside tm_dispatch_batch, host to host and interleaved, at 64
/ 1,024 / 4,096 topics (--sizes), tm_deliver_batch's outputs checked against
tm_dispatch_batch's grouped on the host; the grouping's added time is
deliver_minus_dispatch_ms.  Beside them the in-place forms on tm_host_alloc
buffers, tm_dispatch_batch32 and tm_deliver_batch32 (outputs checked against
tm_deliver_batch's; grouped_by says whether the one-workgroup grouping
finished it): deliver32_minus_dispatch32_ms is what the grouping adds there.
With a library from before tm_deliver_batch the dispatch legs run alone, from
before tm_deliver_batch32 all but that one.

--aggre: aggre/1 on the device (nothing of the first part runs).  The batch is
matched as pairs and fanned out with tm_fanout_dev_pairs over a destination
table that puts a share p of the values on destination 0 (the local node) and
the rest uniformly on the others, so that a topic's hits meet in one bucket;
then tm_aggre_dev is timed against the torch composition a user would write on
the same arrays (shifted compares, a boolean-mask index, bincount + cumsum over
the kept entries' buckets), outputs compared first (identical), for two inputs:
none_dropped -- p = 0.55 and filter_of[v] = v (every value its own filter) --
and quarter -- filter_of built from the fanned-out arrays: the neighbours of one
topic inside one bucket are the pairs that can be dropped; the distinct value
pairs among them, in a seeded random order, are given equal ids (the ids of a
prefix of that order, merged transitively), and the prefix is found by
bisection so that the dropped share, counted with the torch composition before
anything is timed, comes closest to a quarter.  p = 0.55 is kept when that gets
within 3 points of a quarter; else p = 0.75 and p = 1 are tried and the closest
input is taken (with many destinations a topic's hits seldom meet in a bucket
unless most values are local).  The line says which p was taken, how many
pairs were merged and what was dropped.  The call's median stands beside
tm_fanout_dev_pairs' on the same entries, timed the same way.  With --small: a fourth leg, tm_route_batch32_ex with
TM_ROUTE_AGGRE (the index's filter table: one id per distinct filter), its
outputs compared with the numpy definition applied to (c)'s.

--dispatch: local dispatch on the device (nothing of the first part runs).  The
batch is matched as pairs and fanned out over 16 uniform destinations with
tm_fanout_dev_pairs; bucket 0 (the local node) is then expanded with
tm_dispatch_dev over two explicit subscriber tables -- uniform: 1 to 4
subscribers per value; skewed: the same, plus 0.1 % of the values with 10,000
-- against the torch composition on the same device arrays (gather the spans,
cumsum, repeat_interleave, three gathers), outputs compared first (identical).
tm_fanout_dev_pairs and tm_aggre_dev (filter_of[v] = v) are timed on the same
entries in the same run.  One JSON line per table: both medians and spreads,
deliveries/s, the algorithmic bytes (12 written + 4 read per delivery, 8 + 8 +
12 per entry) per second, and the last line the skewed table's time per
delivery over the uniform one's.  With --small: the NIF's call instead, host to
host as above, per batch size and per table (uniform / skewed, installed with
tm_set_subscribers; --subs LO HI changes the uniform range), four legs
interleaved:

  dispatch_batch32       tm_dispatch_batch32, in place (--dp1-max N sets
                         TM_DEBUG_DP1_MAX for it: the deliveries the one-launch
                         kernel expands itself)
  dispatch_batch32_grid  the same call with TM_DEBUG_DP1_MAX 0: the route
                         outputs in one launch, the deliveries by the grid
                         kernels -- the other side of the crossover
  dispatch_batch         tm_dispatch_batch on the same topics, the staged path
  route_batch32          tm_route_batch32_ex alone: what dispatch adds

Outputs are compared before anything is timed (identical); the line says which
leg finished each call (TM_DEBUG_DISPATCH_ONE / _GRID).  --aggre passes
TM_ROUTE_AGGRE to every leg.  Under TM_LIB naming a library without
tm_dispatch_batch32 only the last two legs run (the yardstick of an A/B).

--share: the shared-subscription pick (nothing of the first part runs).  The
batch is matched as pairs, fanned out over 16 uniform destinations and
aggregated (filter_of[v] = v); the first four destinations are shared groups,
their values spread over 1,000 and over 1M slots, every slot round_robin with
2 to 8 members.  tm_share_pick_dev on the aggregated arrays is timed against
the torch composition on the same arrays -- a stable sort by slot, a segmented
arange (cummax of the run heads), the gathers and the scatter back; the
groups' buckets come first, so their bound is handed over as a host integer;
it does not advance the state words, one pass less than the kernels -- outputs
compared first (identical).  One JSON line per slot count.  With --small:
tm_publish_batch beside tm_dispatch_batch (both with TM_ROUTE_AGGRE), host to
host as above, per batch size; destinations 1 to 4 are groups, one slot per
value; the figure is publish_minus_dispatch_ms.  Two more legs, interleaved
with those two, run the in-place forms on tm_host_alloc buffers:
tm_publish_batch32 and tm_dispatch_batch32 (publish_batch32, dispatch_batch32,
publish32_minus_dispatch32_ms: what the pick adds in place;
publish_over_publish32; picked_by: the one-launch kernel, or the grid pick /
the staged path); the route outputs, the head and which entries have a pick
are compared with tm_publish_batch's first.  Under TM_LIB naming a library
without tm_publish_batch only tm_dispatch_batch runs (the yardstick of an A/B);
--dispatch-leg-only times this library the same way, the other side of that A/B.

--group --share: the picks grouped with the deliveries (no index): 1M synthetic
deliveries (100,000 pids, 250,000 messages) and 1M aggregated entries of which
0 / 65,536 / 1M carry a member that is a local subscriber; tm_group_picks_dev
against (a) the torch composition on the same tensors -- the local picks
compacted, cat, a stable sort by message and one by subscriber,
unique_consecutive, gathers -- outputs compared first (identical), and (b)
tm_group_subs_dev on the deliveries alone: the floor, so the line with no local
pick shows what the merge's front end costs over it; the three interleaved
under HIP events.  --small --group --share: the --small index with --small
--share's groups (member ids below 200,000, half of them local subscribers
through tm_set_member_subs); tm_publish_deliver_batch beside tm_publish_batch
and tm_deliver_batch, host to host and interleaved, at 64 / 1,024 / 4,096
topics (--sizes); its grouped arrays are checked against the definition applied
to tm_publish_batch's deliveries and its own entries and picks; pair_p50_ms is
the two calls' sum, merged_over_pair the new call over it.  The in-place legs run
beside them on tm_host_alloc buffers: tm_publish_batch32, tm_deliver_batch32 and
tm_publish_deliver_batch32, whose outputs and state words are compared with the
staged call's from the same start state first (--no-pd32-leg leaves the last one
out, so that a library from before it, given through TM_LIB, runs the same
rounds); staged_over_in_place is the staged call's p50 over the new leg's,
merged32_minus_publish32_ms what the merge adds over tm_publish_batch32.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from emqx_amd import _native, workload as wl   # noqa: E402


def torch_fanout(torch, hit, vals, total, n, dest_of, n_dests):
    """(every value of the batch has a destination below n_dests here, so the
    composition needs no unrouted bucket: its shortest form)"""
    b = dest_of[vals[:total]]   # (values are non-negative int32: indexed as they are, no cast pass)
    _, perm = torch.sort(b, stable=True)
    counts = hit[1:] - hit[:-1]
    topic = torch.repeat_interleave(torch.arange(n, device=vals.device, dtype=torch.int32), counts, output_size=total)
    offs = torch.zeros(n_dests + 2, dtype=torch.int64, device=vals.device)
    offs[1:] = torch.cumsum(torch.bincount(b, minlength=n_dests + 1), 0)
    return offs, topic[perm], vals[:total][perm]


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "p10_ms": round(float(a[len(a) // 10]), 4), "p90_ms": round(float(a[(len(a) * 9) // 10]), 4),
            "max_ms": round(float(a[-1]), 4)}


def timed_pair(torch, fa, fb, warmup, reps):
    """fa and fb alternating, HIP events around each -> (ms of fa, ms of fb)"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(reps):
        ev[0].record()
        fa()
        ev[1].record()
        fb()
        ev[2].record()
        torch.cuda.synchronize()
        ta.append(ev[0].elapsed_time(ev[1]))
        tb.append(ev[1].elapsed_time(ev[2]))
    return ta, tb


def both_forms(torch, ix, a, s, n, d_blob, d_offs, d_hit, d_vals, cap, d_err, total, most, n_dests, dest_of, nvals, fs_len):
    """the fanout_call and pipeline lines of one destination count"""
    dev = d_vals.device
    cap_p = total + 4096 * most
    d_pairs = torch.zeros(2 * n + 2, dtype=torch.int32, device=dev)
    d_pv = torch.zeros(cap_p, dtype=torch.int32, device=dev)
    outs = [(torch.zeros(n_dests + 2, dtype=torch.int64, device=dev), torch.zeros(total, dtype=torch.int32, device=dev),
             torch.zeros(total, dtype=torch.int32, device=dev)) for _ in range(2)]

    def m_csr():
        ix.match_batch_dev(n, d_blob.data_ptr(), d_offs.data_ptr(), d_hit.data_ptr(), d_vals.data_ptr(), cap,
                           d_err.data_ptr(), s)

    def m_pairs():
        ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_pv.data_ptr(), cap_p,
                                 d_err.data_ptr(), s)

    def f_csr():
        o = outs[0]
        ix.fanout_dev(n, d_hit.data_ptr(), d_vals.data_ptr(), total, n_dests, o[0].data_ptr(), o[1].data_ptr(),
                      o[2].data_ptr(), dest_of.data_ptr(), nvals, s)

    def f_pairs():
        o = outs[1]
        ix.fanout_dev_pairs(n, d_pairs.data_ptr(), d_pv.data_ptr(), cap_p, n_dests, o[0].data_ptr(), o[1].data_ptr(),
                            o[2].data_ptr(), dest_of.data_ptr(), nvals, s)

    m_pairs()
    torch.cuda.synchronize()
    assert int(d_pairs[2 * n]) & 0xFFFFFFFF == total and int(d_pairs[2 * n + 1]) & 0xFFFFFFFF <= cap_p, \
        "pairs: total differs or values dropped"
    f_csr()
    f_pairs()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*outs)), f"n_dests {n_dests}: the two forms' outputs differ"
    passes = 1 if n_dests + 1 <= 256 else 2
    base = {"tool": "fanout_bench", "filters": fs_len, "topics": n, "entries": total, "n_dests": n_dests,
            "passes": passes, "reps": a.reps, "pairs_cap": cap_p}
    tc, tp = timed_pair(torch, f_csr, f_pairs, a.warmup, a.reps)
    c, q = stats(tc), stats(tp)
    print(json.dumps({**base, "kind": "fanout_call", "csr": c, "pairs": q,
                      "pairs_over_csr": round(q["median_ms"] / c["median_ms"], 3), "identical": True}), flush=True)
    tc, tp = timed_pair(torch, lambda: (m_csr(), f_csr()), lambda: (m_pairs(), f_pairs()), a.warmup, a.reps)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*outs)), f"n_dests {n_dests}: the two pipelines' outputs differ"
    c, q = stats(tc), stats(tp)
    print(json.dumps({**base, "kind": "pipeline", "csr": c, "pairs": q,
                      "pairs_over_csr": round(q["median_ms"] / c["median_ms"], 3),
                      "csr_topics_per_s": round(n / (c["median_ms"] * 1e-3), 1),
                      "pairs_topics_per_s": round(n / (q["median_ms"] * 1e-3), 1), "identical": True}), flush=True)


def synthetic_skew(torch, ix, a, s, n, total, n_dests=16):
    """no index: `total` entries over n topics, spread evenly / 64 topics holding half of them; both calls on each"""
    dev = torch.device("cuda")
    rng = np.random.default_rng(11)
    nvals = 1 << 20
    dest_of = torch.from_numpy(rng.integers(0, n_dests, nvals, dtype=np.int64).astype(np.int32)).to(dev)
    res = {}
    for name in ("even", "skewed"):
        lens = np.full(n, total // n, np.int64)
        lens[: total - int(lens.sum())] += 1
        if name == "skewed":
            lens = np.full(n, (total // 2) // n, np.int64)
            heavy = np.arange(64) * (n // 64)
            lens[heavy] += (total - int(lens.sum())) // 64
            lens[0] += total - int(lens.sum())
        hit = np.zeros(n + 1, np.int64)
        hit[1:] = np.cumsum(lens)
        vals = rng.integers(0, nvals, total, dtype=np.int64).astype(np.int32)
        d_hit = torch.from_numpy(hit).to(dev)
        d_vals = torch.from_numpy(vals).to(dev)
        d_pairs = torch.from_numpy(np.stack([hit[:-1], lens], axis=1).astype(np.uint32).view(np.int32).reshape(-1)).to(dev)
        outs = [(torch.zeros(n_dests + 2, dtype=torch.int64, device=dev), torch.zeros(total, dtype=torch.int32, device=dev),
                 torch.zeros(total, dtype=torch.int32, device=dev)) for _ in range(2)]

        def f_csr():
            o = outs[0]
            ix.fanout_dev(n, d_hit.data_ptr(), d_vals.data_ptr(), total, n_dests, o[0].data_ptr(), o[1].data_ptr(),
                          o[2].data_ptr(), dest_of.data_ptr(), nvals, s)

        def f_pairs():
            o = outs[1]
            ix.fanout_dev_pairs(n, d_pairs.data_ptr(), d_vals.data_ptr(), total, n_dests, o[0].data_ptr(), o[1].data_ptr(),
                                o[2].data_ptr(), dest_of.data_ptr(), nvals, s)

        f_csr()
        f_pairs()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(*outs)), f"synthetic {name}: the two forms' outputs differ"
        tc, tp = timed_pair(torch, f_csr, f_pairs, a.warmup, a.reps)
        res[name] = {"most_hits": int(lens.max()), "csr": stats(tc), "pairs": stats(tp)}
    print(json.dumps({"tool": "fanout_bench", "kind": "synthetic_skew", "topics": n, "entries": total, "n_dests": n_dests,
                      "reps": a.reps, **res,
                      "skew_cost_csr": round(res["skewed"]["csr"]["median_ms"] / res["even"]["csr"]["median_ms"], 3),
                      "skew_cost_pairs": round(res["skewed"]["pairs"]["median_ms"] / res["even"]["pairs"]["median_ms"], 3)}),
          flush=True)


def torch_aggre(torch, doff, t, v, E, fof, dest_of, n_dests):
    """the composition a user would write on a fan-out's output (every value routed)"""
    t, v = t[:E], v[:E]
    f = fof[v]
    keep = torch.ones(E, dtype=torch.bool, device=v.device)
    keep[1:] = ~((t[1:] == t[:-1]) & (f[1:] == f[:-1]) & (f[1:] != -1))
    heads = doff[:n_dests + 1]
    keep[heads[heads < E]] = True
    out_t, out_v = t[keep], v[keep]
    offs = torch.zeros(n_dests + 2, dtype=torch.int64, device=v.device)
    offs[1:] = torch.cumsum(torch.bincount(dest_of[out_v], minlength=n_dests + 1), 0)
    return offs, out_t, out_v


def merged_ids(nvals, pa, pb):
    """filter ids with pa[i] and pb[i] equal for every i, transitively: the smallest value of each group"""
    lab = np.arange(nvals, dtype=np.int64)
    while len(pa):
        new = lab.copy()
        m = np.minimum(lab[pa], lab[pb])
        np.minimum.at(new, pa, m)
        np.minimum.at(new, pb, m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def quarter_table(torch, fo, total, n_dests, nvals, dest_of, want=0.25, seed=11):
    """filter_of from a fan-out's output (see the docstring) -> (pairs merged, dropped share, filter_of)"""
    t, v = fo[1][:total], fo[2][:total]
    head = torch.zeros(total, dtype=torch.bool, device=v.device)
    heads = fo[0][:n_dests + 1]
    head[heads[heads < total]] = True
    cand = (t[1:] == t[:-1]) & ~head[1:]
    va, vb = v[:-1][cand].cpu().numpy().astype(np.int64), v[1:][cand].cpu().numpy().astype(np.int64)
    keys, cnt = np.unique(np.minimum(va, vb) * nvals + np.maximum(va, vb), return_counts=True)
    # rare pairs first (a seeded random order among equals): the share then grows in small steps
    # until the few pairs of popular filters, which are worth whole points each, come in
    keys = keys[np.lexsort((np.random.default_rng(seed).random(len(keys)), cnt))]
    if os.environ.get("FANOUT_BENCH_VERBOSE"):
        top = np.sort(cnt)[::-1][:8]
        print(f"quarter_table: {len(va)} candidate neighbours of {total} entries, {len(keys)} distinct pairs, "
              f"most frequent {top.tolist()}", file=sys.stderr, flush=True)
    pa, pb = keys // nvals, keys % nvals

    def dropped(k):
        fof = torch.from_numpy(merged_ids(nvals, pa[:k], pb[:k]).astype(np.int32)).to(v.device)
        kept = len(torch_aggre(torch, fo[0], fo[1], fo[2], total, fof, dest_of, n_dests)[1])
        return 1 - kept / total, fof

    lo, hi = 0, len(keys)   # the share grows with the prefix: bisect for the first prefix at or above `want`
    while lo < hi:
        mid = (lo + hi) // 2
        if dropped(mid)[0] < want:
            lo = mid + 1
        else:
            hi = mid
    cands = [(abs(dropped(k)[0] - want), k) for k in {max(lo - 1, 0), lo}]
    k = min(cands)[1]
    frac, fof = dropped(k)
    return k, frac, fof


def aggre_legs(torch, ix, a, s, n, d_blob, d_offs, d_err, total, most, nvals, fs_len):
    """--aggre: tm_aggre_dev against the torch composition, and beside tm_fanout_dev_pairs"""
    dev = d_blob.device
    cap_p = total + 4096 * most
    d_pairs = torch.zeros(2 * n + 2, dtype=torch.int32, device=dev)
    d_pv = torch.zeros(cap_p, dtype=torch.int32, device=dev)
    ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_pv.data_ptr(), cap_p,
                             d_err.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(d_pairs[2 * n]) & 0xFFFFFFFF == total and int(d_pairs[2 * n + 1]) & 0xFFFFFFFF <= cap_p
    rng = np.random.default_rng(7)
    u, spread = rng.random(nvals), rng.integers(0, 1 << 30, nvals)
    for n_dests in a.dests:
        fo = (torch.zeros(n_dests + 2, dtype=torch.int64, device=dev), torch.zeros(total, dtype=torch.int32, device=dev),
              torch.zeros(total, dtype=torch.int32, device=dev))
        out = (torch.zeros(n_dests + 2, dtype=torch.int64, device=dev), torch.zeros(total, dtype=torch.int32, device=dev),
               torch.zeros(total, dtype=torch.int32, device=dev))
        dest_of = torch.zeros(nvals, dtype=torch.int32, device=dev)

        def fanout():
            ix.fanout_dev_pairs(n, d_pairs.data_ptr(), d_pv.data_ptr(), cap_p, n_dests, fo[0].data_ptr(), fo[1].data_ptr(),
                                fo[2].data_ptr(), dest_of.data_ptr(), nvals, s)

        def table(p):
            dest_of.copy_(torch.from_numpy(np.where(u < p, 0, spread % n_dests).astype(np.int32)))

        best = None   # (distance from a quarter, p, pairs merged, filter_of)
        for p in (0.55, 0.75, 1.0):
            table(p)
            fanout()
            torch.cuda.synchronize()
            k, frac, fof = quarter_table(torch, fo, total, n_dests, nvals, dest_of)
            if best is None or abs(frac - 0.25) < best[0]:
                best = (abs(frac - 0.25), p, k, fof)
            if best[0] <= 0.03:
                break
        inputs = {"none_dropped": (0.55, torch.arange(nvals, dtype=torch.int32, device=dev), "v"),
                  "quarter": (best[1], best[3], f"{best[2]} neighbouring value pairs merged")}
        for name, (p_local, fof, how) in inputs.items():
            table(p_local)
            fanout()
            torch.cuda.synchronize()
            assert int(fo[0][n_dests + 1]) == total

            def hip():
                ix.aggre_dev(n_dests, fo[0].data_ptr(), fo[1].data_ptr(), fo[2].data_ptr(), total, out[0].data_ptr(),
                             out[1].data_ptr(), out[2].data_ptr(), fof.data_ptr(), nvals, s)

            def tor():
                return torch_aggre(torch, fo[0], fo[1], fo[2], total, fof, dest_of, n_dests)

            hip()
            r = tor()
            torch.cuda.synchronize()
            K = int(out[0][n_dests + 1])
            assert K == len(r[1]) and torch.equal(out[0], r[0]) and torch.equal(out[1][:K], r[1]) and \
                torch.equal(out[2][:K], r[2]), f"n_dests {n_dests} {name}: the two paths differ"
            del r
            th, tt = timed_pair(torch, hip, tor, a.warmup, a.reps)
            th2, tf = timed_pair(torch, hip, fanout, a.warmup, a.reps)
            h, t, h2, f = stats(th), stats(tt), stats(th2), stats(tf)
            nbytes = 12 * total + 8 * K + 12 * ((total + 63) // 64) + 16 * (n_dests + 2)
            print(json.dumps({"tool": "fanout_bench", "kind": "aggre", "filters": fs_len, "topics": n, "entries": total,
                              "n_dests": n_dests, "input": name, "local_share": p_local, "filter_of": how, "kept": K,
                              "dropped_fraction": round(1 - K / total, 4), "reps": a.reps, "hip": h, "torch": t,
                              "torch_over_hip": round(t["median_ms"] / h["median_ms"], 2),
                              "hip_beside_fanout": h2, "fanout_dev_pairs": f,
                              "aggre_over_fanout": round(h2["median_ms"] / f["median_ms"], 3),
                              "algorithmic_bytes": nbytes,
                              "hip_algorithmic_GBps": round(nbytes / (h["median_ms"] * 1e-3) / 1e9, 1),
                              "identical": True}), flush=True)
            assert h["p90_ms"] < t["p10_ms"], f"n_dests {n_dests} {name}: tm_aggre_dev is not clearly below the torch composition"


def dispatch_legs(torch, ix, a, s, n, d_blob, d_offs, d_err, total, most, nvals, fs_len, n_dests=16):
    """--dispatch: tm_dispatch_dev on the local bucket against the torch composition"""
    dev = d_blob.device
    cap_p = total + 4096 * most
    d_pairs = torch.zeros(2 * n + 2, dtype=torch.int32, device=dev)
    d_pv = torch.zeros(cap_p, dtype=torch.int32, device=dev)
    ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_pv.data_ptr(), cap_p,
                             d_err.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(d_pairs[2 * n]) & 0xFFFFFFFF == total and int(d_pairs[2 * n + 1]) & 0xFFFFFFFF <= cap_p
    rng = np.random.default_rng(7)
    dest_of = torch.from_numpy(rng.integers(0, n_dests, nvals, dtype=np.int64).astype(np.int32)).to(dev)
    fof = torch.arange(nvals, dtype=torch.int32, device=dev)
    fo, ag = ((torch.zeros(n_dests + 2, dtype=torch.int64, device=dev), torch.zeros(total, dtype=torch.int32, device=dev),
               torch.zeros(total, dtype=torch.int32, device=dev)) for _ in range(2))

    def fanout():
        ix.fanout_dev_pairs(n, d_pairs.data_ptr(), d_pv.data_ptr(), cap_p, n_dests, fo[0].data_ptr(), fo[1].data_ptr(),
                            fo[2].data_ptr(), dest_of.data_ptr(), nvals, s)

    def aggre():
        ix.aggre_dev(n_dests, fo[0].data_ptr(), fo[1].data_ptr(), fo[2].data_ptr(), total, ag[0].data_ptr(),
                     ag[1].data_ptr(), ag[2].data_ptr(), fof.data_ptr(), nvals, s)

    fanout()
    torch.cuda.synchronize()
    q0, q1 = int(fo[0][0]), int(fo[0][1])
    M = q1 - q0
    tf, ta = timed_pair(torch, fanout, aggre, a.warmup, a.reps)
    beside = {"fanout_dev_pairs": stats(tf), "aggre_dev": stats(ta)}
    per_delivery = {}
    for name in ("uniform", "skewed"):
        cnt = rng.integers(1, 5, nvals)
        if name == "skewed":
            cnt[rng.choice(nvals, max(nvals // 1000, 1), replace=False)] = 10_000
        pos = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        pool_len = int(cnt.sum())
        assert pool_len < 1 << 31
        span = torch.from_numpy(np.stack([pos, cnt], axis=1).astype(np.int32).reshape(-1)).to(dev)
        pool = torch.from_numpy(rng.integers(0, 1 << 31, pool_len, dtype=np.int64).astype(np.int32)).to(dev)
        span2 = span.view(nvals, 2)
        T = int(span2[fo[2][q0:q1].long(), 1].sum())
        head = torch.zeros(2, dtype=torch.int64, device=dev)
        out = tuple(torch.zeros(T, dtype=torch.int32, device=dev) for _ in range(3))

        def hip():
            ix.dispatch_dev(n_dests, fo[0].data_ptr(), 0, fo[1].data_ptr(), fo[2].data_ptr(), total, head.data_ptr(),
                            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), T, d_sub_span=span.data_ptr(),
                            span_len=nvals, d_sub_pool=pool.data_ptr(), pool_len=pool_len, stream=s)

        def tor():
            # (the bucket's bounds and T as host integers: no synchronisation inside the composition)
            t, v = fo[1][q0:q1], fo[2][q0:q1]
            sp = span2[v.long()]
            c = sp[:, 1].long()
            first = torch.cumsum(c, 0) - c
            src = torch.repeat_interleave(torch.arange(M, device=dev), c, output_size=T)
            at = sp[:, 0].long()[src] + (torch.arange(T, device=dev) - first[src])
            return t[src], v[src], pool[at]

        hip()
        r = tor()
        torch.cuda.synchronize()
        assert head.tolist() == [M, T] and all(torch.equal(x, y) for x, y in zip(out, r)), f"{name}: the two paths differ"
        del r
        th, tt = timed_pair(torch, hip, tor, a.warmup, a.reps)
        h, t = stats(th), stats(tt)
        nbytes = 16 * T + 28 * M
        per_delivery[name] = h["median_ms"] * 1e6 / T   # ns
        print(json.dumps({"tool": "fanout_bench", "kind": "dispatch", "filters": fs_len, "topics": n, "entries": total,
                          "n_dests": n_dests, "lists": name, "bucket_entries": M, "deliveries": T,
                          "longest_list": int(cnt.max()), "pool_words": pool_len, "reps": a.reps, "hip": h, "torch": t,
                          "torch_over_hip": round(t["median_ms"] / h["median_ms"], 2),
                          "hip_deliveries_per_s": round(T / (h["median_ms"] * 1e-3), 1),
                          "algorithmic_bytes": nbytes,
                          "hip_algorithmic_GBps": round(nbytes / (h["median_ms"] * 1e-3) / 1e9, 1),
                          "hip_ns_per_delivery": round(per_delivery[name], 4), **beside, "identical": True}), flush=True)
    print(json.dumps({"tool": "fanout_bench", "kind": "dispatch_skew",
                      "skewed_over_uniform_per_delivery": round(per_delivery["skewed"] / per_delivery["uniform"], 3)}),
          flush=True)


def share_legs(torch, ix, a, s, n, d_blob, d_offs, d_err, total, most, nvals, fs_len, n_dests=16, n_groups=4):
    """--share: tm_share_pick_dev on the batch's aggregated arrays against the torch composition (a stable
    argsort by slot, a segmented arange, gathers; its bounds handed over as host integers).  The first
    n_groups of the n_dests destinations are shared groups, every slot round_robin (the reference's
    default) with 2-8 members; the composition leaves the state words alone -- one pass less than the kernels."""
    dev = d_blob.device
    cap_p = total + 4096 * most
    d_pairs = torch.zeros(2 * n + 2, dtype=torch.int32, device=dev)
    d_pv = torch.zeros(cap_p, dtype=torch.int32, device=dev)
    ix.match_batch_dev_pairs(n, d_blob.data_ptr(), d_offs.data_ptr(), d_pairs.data_ptr(), d_pv.data_ptr(), cap_p,
                             d_err.data_ptr(), s)
    rng = np.random.default_rng(7)
    dest_np = rng.integers(0, n_dests, nvals, dtype=np.int64)
    dest_of = torch.from_numpy(dest_np.astype(np.int32)).to(dev)
    fof = torch.arange(nvals, dtype=torch.int32, device=dev)
    fo, ag = ((torch.zeros(n_dests + 2, dtype=torch.int64, device=dev), torch.zeros(total, dtype=torch.int32, device=dev),
               torch.zeros(total, dtype=torch.int32, device=dev)) for _ in range(2))
    ix.fanout_dev_pairs(n, d_pairs.data_ptr(), d_pv.data_ptr(), cap_p, n_dests, fo[0].data_ptr(), fo[1].data_ptr(),
                        fo[2].data_ptr(), dest_of.data_ptr(), nvals, s)
    ix.aggre_dev(n_dests, fo[0].data_ptr(), fo[1].data_ptr(), fo[2].data_ptr(), total, ag[0].data_ptr(),
                 ag[1].data_ptr(), ag[2].data_ptr(), fof.data_ptr(), nvals, s)
    torch.cuda.synchronize()
    E, Q = int(ag[0][n_dests + 1]), int(ag[0][n_groups])   # the groups' buckets come first: [0, Q) are the active entries
    for n_slots in (1000, 1_000_000):
        slot_np = np.where(dest_np < n_groups, rng.integers(0, n_slots, nvals), -1)
        slot_of = torch.from_numpy(slot_np.astype(np.int32)).to(dev)
        cnt = rng.integers(2, 9, n_slots)
        pos = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        pool_len = int(cnt.sum())
        rec = torch.from_numpy(np.stack([pos, cnt, np.zeros(n_slots, np.int64), np.full(n_slots, _native.TM_SHARE_ROUND_ROBIN)],
                                        axis=1).astype(np.int32).reshape(-1)).to(dev)
        rec4 = rec.view(n_slots, 4)
        pool = torch.from_numpy(rng.integers(0, 1 << 31, pool_len, dtype=np.int64).astype(np.int32)).to(dev)
        state0 = torch.from_numpy(rng.integers(0, 8, n_slots, dtype=np.int64).astype(np.int32)).to(dev)
        state = state0.clone()
        head = torch.zeros(2, dtype=torch.int64, device=dev)
        out = torch.full((E,), -1, dtype=torch.int32, device=dev)

        def hip():
            ix.share_pick_dev(n_dests, ag[0].data_ptr(), ag[1].data_ptr(), ag[2].data_ptr(), total, head.data_ptr(),
                              out.data_ptr(), n_topics=n, d_slot_of=slot_of.data_ptr(), slot_of_len=nvals,
                              d_slot_rec=rec.data_ptr(), n_slots=n_slots, d_pool=pool.data_ptr(), pool_len=pool_len,
                              d_state=state.data_ptr(), stream=s)

        def tor():
            sl = slot_of[ag[2][:Q].long()].long()
            ss, order = torch.sort(sl, stable=True)
            ar = torch.arange(Q, device=dev)
            first = torch.ones(Q, dtype=torch.bool, device=dev)
            first[1:] = ss[1:] != ss[:-1]
            start = torch.cummax(torch.where(first, ar, torch.zeros_like(ar)), 0).values
            r = rec4[ss]
            c = r[:, 1].long()
            idx = (state0[ss].long() + 1 + (ar - start)) % c
            res = torch.full((E,), -1, dtype=torch.int32, device=dev)
            res[order] = pool[r[:, 0].long() + idx]
            return res

        hip()
        r = tor()
        torch.cuda.synchronize()
        assert head.tolist() == [Q, Q] and torch.equal(out, r), f"n_slots {n_slots}: the two paths differ"
        del r
        th, tt = timed_pair(torch, hip, tor, a.warmup, a.reps)
        h, t = stats(th), stats(tt)
        print(json.dumps({"tool": "fanout_bench", "kind": "share", "filters": fs_len, "topics": n, "entries": E,
                          "n_dests": n_dests, "groups": n_groups, "active_entries": Q, "n_slots": n_slots,
                          "digit_passes": (max(n_slots - 1, 0).bit_length() + 8) // 9, "members": [2, 8],
                          "strategy": "round_robin", "warmup": a.warmup, "reps": a.reps, "hip": h, "torch": t,
                          "torch_over_hip": round(t["median_ms"] / h["median_ms"], 2),
                          "hip_ns_per_active_entry": round(h["median_ms"] * 1e6 / max(Q, 1), 4), "identical": True}),
              flush=True)


def small_share(a, ix, fs_len, nvals, sizes, n_dests, warmup, reps, local=0, n_groups=4):
    """--small --share: tm_publish_batch host to host beside tm_dispatch_batch (both under TM_ROUTE_AGGRE);
    destinations 1 .. n_groups are shared groups, one slot per value, round_robin, 2-8 members"""
    import time
    P = _native._ptr
    lib, h = ix._lib, ix._h
    has = hasattr(lib, "tm_publish_batch") and not a.dispatch_leg_only
    has32 = has and hasattr(lib, "tm_publish_batch32")
    rng = np.random.default_rng(7)
    cnt = rng.integers(a.subs[0], a.subs[1] + 1, nvals)
    loffs = np.zeros(nvals + 1, np.uint64)
    loffs[1:] = np.cumsum(cnt)
    subs = rng.integers(0, 1 << 31, int(loffs[-1]), dtype=np.int64).astype(np.uint32)
    vals = np.arange(nvals, dtype=np.uint32)
    assert lib.tm_set_subscribers(h, nvals, P(vals), P(loffs), P(subs)) == 0
    if has:
        dest = np.random.default_rng(7).integers(0, n_dests, nvals)   # (small_batches' destination table)
        grp = np.nonzero((dest >= 1) & (dest <= n_groups))[0].astype(np.uint32)
        ix.set_share_slots(grp, np.arange(len(grp), dtype=np.uint32))
        mc = rng.integers(2, 9, len(grp))
        moffs = np.zeros(len(grp) + 1, np.uint64)
        moffs[1:] = np.cumsum(mc)
        mem = rng.integers(0, 1 << 31, int(moffs[-1]), dtype=np.int64).astype(np.uint32)
        zero, meta = np.zeros(len(grp), np.uint32), np.full(len(grp), _native.TM_SHARE_ROUND_ROBIN, np.uint32)
        assert lib.tm_set_share_members(h, len(grp), P(np.arange(len(grp), dtype=np.uint32)), P(moffs), P(mem), P(zero),
                                        P(meta)) == 0
    for n in sizes:
        tp = wl.topics(3, a.filters, n)
        blob, offs = np.ascontiguousarray(tp.blob), np.ascontiguousarray(tp.offs, dtype=np.uint64)
        cap = 16 * n + 1024
        d64, head, err = np.zeros(n_dests + 2, np.uint64), np.zeros(2, np.uint64), np.zeros(n, np.uint8)
        rc = lib.tm_dispatch_batch(h, n, P(blob), P(offs), n_dests, local, 1, P(d64), None, None, 0, P(head), None, None,
                                   None, 0, P(err))
        assert rc in (0, _native.TM_ECAP)
        dcap = int(head[1]) + 1024
        t_, v_, m_ = (np.zeros(cap, np.uint32) for _ in range(3))
        dd = tuple(np.zeros(dcap, np.uint32) for _ in range(3))
        kc = rng.integers(0, 1 << 32, n, dtype=np.uint32)

        def leg_d():
            return lib.tm_dispatch_batch(h, n, P(blob), P(offs), n_dests, local, 1, P(d64), P(t_), P(v_), cap, P(head),
                                         P(dd[0]), P(dd[1]), P(dd[2]), dcap, P(err))

        def leg_p():
            return lib.tm_publish_batch(h, n, P(blob), P(offs), n_dests, local, 1, P(d64), P(t_), P(v_), cap, P(head),
                                        P(dd[0]), P(dd[1]), P(dd[2]), dcap, P(kc), P(kc), 1, P(m_), P(err))

        legs = [("dispatch_batch", leg_d)] + ([("publish_batch", leg_p)] if has else [])
        pinned, took = [], None
        if has32:
            # the in-place forms on tm_host_alloc buffers: tm_publish_batch32 and, to show what the pick adds, tm_dispatch_batch32
            def pin(k, dt):
                pinned.append(ix.host_array(k, dt))
                return pinned[-1]
            nb = int(offs[-1])
            b32, o32, e32 = pin(nb + 16, np.uint8), pin(n + 1, np.uint32), pin(n, np.uint8)
            b32[:nb], o32[:] = blob[:nb], offs.astype(np.uint32)
            d32, h32 = pin(n_dests + 2, np.uint32), pin(2, np.uint64)
            t32, v32, m32 = (pin(cap, np.uint32) for _ in range(3))
            dd32 = tuple(pin(dcap, np.uint32) for _ in range(3))
            k32 = pin(n, np.uint32)
            k32[:] = kc

            def leg_p32():
                return lib.tm_publish_batch32(h, n, P(b32), P(o32), n_dests, local, 1, P(d32), P(t32), P(v32), cap, P(h32),
                                              P(dd32[0]), P(dd32[1]), P(dd32[2]), dcap, P(k32), P(k32), 1, P(m32), P(e32))

            def leg_d32():
                return lib.tm_dispatch_batch32(h, n, P(b32), P(o32), n_dests, local, 1, P(d32), P(t32), P(v32), cap,
                                               P(h32), P(dd32[0]), P(dd32[1]), P(dd32[2]), dcap, P(e32))

            ONE = _native.TM_DEBUG_PUBLISH_ONE
            c0 = ix.debug_get(ONE)
            assert leg_p() == 0 and leg_p32() == 0
            took = "one_launch" if ix.debug_get(ONE) > c0 else "grid_or_staged"
            K32 = int(d32[n_dests + 1])
            assert np.array_equal(d64, d32.astype(np.uint64)) and np.array_equal(t_[:K32], t32[:K32]) and \
                np.array_equal(v_[:K32], v32[:K32]) and h32.tolist() == head.tolist() and \
                np.array_equal(m_[:K32] == 0xFFFFFFFF, m32[:K32] == 0xFFFFFFFF), \
                f"n {n}: tm_publish_batch and tm_publish_batch32 differ"
            legs += [("publish_batch32", leg_p32), ("dispatch_batch32", leg_d32)]
        ms = {k: [] for k, _ in legs}
        for r in range(warmup + reps):
            for k, f in legs:
                t0 = time.perf_counter_ns()
                assert f() == 0
                t1 = time.perf_counter_ns()
                if r >= warmup:
                    ms[k].append((t1 - t0) * 1e-6)
        st = {k: dict(stats(v), p50_ms=round(float(np.median(v)), 4)) for k, v in ms.items()}
        K = int(d64[n_dests + 1])
        line = {"tool": "fanout_bench", "kind": "small_share", "filters": fs_len, "topics": n, "kept_entries": K,
                "n_dests": n_dests, "groups": n_groups, "deliveries": int(head[1]), "warmup": warmup, "reps": reps, **st}
        if has:
            line["picks"] = int((m_[:K] != 0xFFFFFFFF).sum())
            line["publish_minus_dispatch_ms"] = round(st["publish_batch"]["p50_ms"] - st["dispatch_batch"]["p50_ms"], 4)
        if has32:
            line["picked_by"] = took
            line["publish32_minus_dispatch32_ms"] = round(st["publish_batch32"]["p50_ms"] -
                                                          st["dispatch_batch32"]["p50_ms"], 4)
            line["publish_over_publish32"] = round(st["publish_batch"]["p50_ms"] / st["publish_batch32"]["p50_ms"], 2)
        print(json.dumps(line), flush=True)
        for x in pinned:
            ix.host_free(x)


def _np_aggre(doff, t, v, fof, n_dests):
    """include/tmatch.h's numpy definition on a whole fan-out"""
    doff = doff.astype(np.int64)
    E = int(doff[n_dests + 1])
    f = fof[v[:E]]
    keep = np.ones(E, bool)
    if E > 1:
        keep[1:] = ~((t[1:E] == t[:E - 1]) & (f[1:] == f[:-1]) & (f[1:] != 0xFFFFFFFF))
    heads = doff[:n_dests + 1]
    keep[heads[heads < E]] = True
    keep[min(int(doff[n_dests]), E):] = True
    before = np.concatenate([[0], np.cumsum(keep)])
    return before[np.minimum(doff, E)], t[:E][keep], v[:E][keep]


def small_batches(a, sizes=(64, 1024, 4096, 16384), n_dests=16, warmup=20, reps=200):
    """--small: host-to-host latency of a micro-batch's route fan-out, three legs interleaved"""
    import time
    fs = wl.filters(3, a.filters)
    ix = _native.Index(hint_keys=len(fs))
    rng = np.random.default_rng(7)
    nvals = int(fs.vals.max()) + 1
    ix.set_dests(np.arange(nvals, dtype=np.uint32), rng.integers(0, n_dests, nvals).astype(np.uint32))
    fof = None
    if a.aggre or a.share:   # one id per distinct filter, in order of first sight
        ids: dict = {}
        raw = fs.blob.tobytes()
        fof = np.full(nvals, 0xFFFFFFFF, np.uint32)
        for k in range(len(fs)):
            fof[int(fs.vals[k])] = ids.setdefault(raw[int(fs.offs[k]):int(fs.offs[k + 1])], len(ids))
        ix.set_route_filters(np.arange(nvals, dtype=np.uint32), fof)
    ix.apply(np.ones(len(fs), np.uint8), fs.blob, fs.offs, fs.vals)
    ix.sync(None)
    P = _native._ptr
    lib, h = ix._lib, ix._h
    if a.group and a.share:
        small_group_share(a, ix, len(fs), nvals, sizes if a.sizes else (64, 1024, 4096), n_dests, warmup, reps)
        return
    if a.group:
        small_group(a, ix, len(fs), nvals, sizes if a.sizes else (64, 1024, 4096), n_dests, warmup, reps)
        return
    if a.share:
        small_share(a, ix, len(fs), nvals, sizes, n_dests, warmup, reps)
        return
    if a.dispatch:
        small_dispatch(a, ix, len(fs), nvals, sizes, n_dests, warmup, reps)
        return
    for n in sizes:
        tp = wl.topics(3, a.filters, n)
        assert len(tp) == n
        nb = int(tp.offs[-1])
        cap = 16 * n + 1024
        blob, offs32 = ix.host_array(nb + 16, np.uint8), ix.host_array(n + 1, np.uint32)
        blob[:nb] = tp.blob[:nb]
        offs32[:] = tp.offs.astype(np.uint32)
        offs64 = ix.host_array(n + 1, np.uint64)
        offs64[:] = tp.offs
        err = ix.host_array(n, np.uint8)
        pairs, pvals = ix.host_array(2 * n + 1, np.uint32), ix.host_array(cap, np.uint32)
        o32 = (ix.host_array(n_dests + 2, np.uint32), ix.host_array(cap, np.uint32), ix.host_array(cap, np.uint32))
        o64 = (ix.host_array(n_dests + 2, np.uint64), ix.host_array(cap, np.uint32), ix.host_array(cap, np.uint32))

        def leg_a():
            return lib.tm_route_batch(h, n, P(blob), P(offs64), n_dests, P(o64[0]), P(o64[1]), P(o64[2]), cap, P(err))

        def leg_b():
            return lib.tm_match_batch32_pairs(h, n, P(blob), P(offs32), P(pairs), P(pvals), cap, P(err))

        def leg_c():
            return lib.tm_route_batch32(h, n, P(blob), P(offs32), n_dests, P(o32[0]), P(o32[1]), P(o32[2]), cap, P(err))

        one0, grid0 = ix.debug_get(_native.TM_DEBUG_ROUTE_ONE), ix.debug_get(_native.TM_DEBUG_ROUTE_GRID)
        assert leg_a() == 0 and leg_c() == 0 and leg_b() == 0, "a leg failed (or cap too small)"
        path = "one_launch" if ix.debug_get(_native.TM_DEBUG_ROUTE_ONE) > one0 else "grid"
        assert ix.debug_get(_native.TM_DEBUG_ROUTE_ONE) + ix.debug_get(_native.TM_DEBUG_ROUTE_GRID) == one0 + grid0 + 1
        total = int(o64[0][n_dests + 1])
        assert total == int(pairs[2 * n]) and np.array_equal(o64[0], o32[0].astype(np.uint64)) and \
            np.array_equal(o64[1][:total], o32[1][:total]) and np.array_equal(o64[2][:total], o32[2][:total]), \
            f"n {n}: tm_route_batch and tm_route_batch32 differ"
        legs = (leg_a, leg_b, leg_c)
        extra = {}
        if a.aggre:
            o32a = (ix.host_array(n_dests + 2, np.uint32), ix.host_array(cap, np.uint32), ix.host_array(cap, np.uint32))

            def leg_d():
                return lib.tm_route_batch32_ex(h, n, P(blob), P(offs32), n_dests, P(o32a[0]), P(o32a[1]), P(o32a[2]), cap,
                                               P(err), _native.TM_ROUTE_AGGRE)

            assert leg_d() == 0
            e_off, e_t, e_v = _np_aggre(o32[0], o32[1], o32[2], fof, n_dests)
            K = int(e_off[-1])
            assert np.array_equal(o32a[0].astype(np.int64), e_off) and np.array_equal(o32a[1][:K], e_t) and \
                np.array_equal(o32a[2][:K], e_v), f"n {n}: the aggregated call differs from the definition"
            legs = (leg_a, leg_b, leg_c, leg_d)
            extra = {"kept": K}
        ms = tuple([] for _ in legs)
        for r in range(warmup + reps):
            for k, f in enumerate(legs):
                t0 = time.perf_counter_ns()
                f()
                t1 = time.perf_counter_ns()
                if r >= warmup:
                    ms[k].append((t1 - t0) * 1e-6)
        sa, sb, sc = stats(ms[0]), stats(ms[1]), stats(ms[2])
        if a.aggre:
            sd = stats(ms[3])
            sd["p50_ms"], sd["p99_ms"] = sd["median_ms"], round(float(np.percentile(ms[3], 99)), 4)
            sc = dict(sc, p99_ms=round(float(np.percentile(ms[2], 99)), 4))
            extra.update({"route_batch32_aggre": sd, "d_minus_c_ms": round(sd["median_ms"] - sc["median_ms"], 4)})
            for x in o32a:
                ix.host_free(x)
        print(json.dumps({"tool": "fanout_bench", "kind": "small", "filters": len(fs), "topics": n, "entries": total,
                          "n_dests": n_dests, "warmup": warmup, "reps": reps, "route32_fanout": path,
                          "route_batch": sa, "match32_pairs": sb, "route_batch32": sc,
                          "c_minus_b_ms": round(sc["median_ms"] - sb["median_ms"], 4),
                          "a_minus_c_ms": round(sa["median_ms"] - sc["median_ms"], 4), "identical": True, **extra}),
              flush=True)
        for x in (blob, offs32, offs64, err, pairs, pvals, *o32, *o64):
            ix.host_free(x)


def small_dispatch(a, ix, fs_len, nvals, sizes, n_dests, warmup, reps, local=0):
    """--small --dispatch: host-to-host latency of a micro-batch's route fan-out plus local dispatch"""
    import time
    P = _native._ptr
    lib, h = ix._lib, ix._h
    has32 = hasattr(lib, "tm_dispatch_batch32")
    flags = _native.TM_ROUTE_AGGRE if a.aggre else 0
    ONE, GRID, DP1 = _native.TM_DEBUG_DISPATCH_ONE, _native.TM_DEBUG_DISPATCH_GRID, _native.TM_DEBUG_DP1_MAX
    dp1 = a.dp1_max if a.dp1_max is not None else _native.DP1_DELIVERIES
    rng = np.random.default_rng(7)
    for name in ("uniform", "skewed"):
        cnt = rng.integers(a.subs[0], a.subs[1] + 1, nvals)
        if name == "skewed":
            cnt[rng.choice(nvals, max(nvals // 1000, 1), replace=False)] = 10_000
        loffs = np.zeros(nvals + 1, np.uint64)
        loffs[1:] = np.cumsum(cnt)
        subs = rng.integers(0, 1 << 31, int(loffs[-1]), dtype=np.int64).astype(np.uint32)
        vals = np.arange(nvals, dtype=np.uint32)
        assert lib.tm_set_subscribers(h, nvals, P(vals), P(loffs), P(subs)) == 0
        for n in sizes:
            tp = wl.topics(3, a.filters, n)
            nb = int(tp.offs[-1])
            blob, offs32, offs64 = ix.host_array(nb + 16, np.uint8), ix.host_array(n + 1, np.uint32), \
                ix.host_array(n + 1, np.uint64)
            blob[:nb] = tp.blob[:nb]
            offs32[:], offs64[:] = tp.offs.astype(np.uint32), tp.offs
            err = ix.host_array(n, np.uint8)
            cap = 16 * n + 1024
            # the sizes first (TM_ECAP with full offsets and the exact head), then buffers that fit
            d64, head = ix.host_array(n_dests + 2, np.uint64), ix.host_array(2, np.uint64)
            rc = lib.tm_dispatch_batch(h, n, P(blob), P(offs64), n_dests, local, flags, P(d64), None, None, 0, P(head),
                                       None, None, None, 0, P(err))
            assert rc in (0, _native.TM_ECAP)
            M, T = int(head[0]), int(head[1])
            dcap = T + 1024
            ra, rb, rc_ = ((ix.host_array(cap, np.uint32), ix.host_array(cap, np.uint32)) for _ in range(3))
            da, db = (tuple(ix.host_array(dcap, np.uint32) for _ in range(3)) for _ in range(2))
            d32, r32, head32 = ix.host_array(n_dests + 2, np.uint32), ix.host_array(n_dests + 2, np.uint32), \
                ix.host_array(2, np.uint64)

            def leg_x():
                return lib.tm_dispatch_batch32(h, n, P(blob), P(offs32), n_dests, local, flags, P(d32), P(ra[0]),
                                               P(ra[1]), cap, P(head32), P(da[0]), P(da[1]), P(da[2]), dcap, P(err))

            def leg_y():
                return lib.tm_dispatch_batch(h, n, P(blob), P(offs64), n_dests, local, flags, P(d64), P(rb[0]), P(rb[1]),
                                             cap, P(head), P(db[0]), P(db[1]), P(db[2]), dcap, P(err))

            def leg_z():
                return lib.tm_route_batch32_ex(h, n, P(blob), P(offs32), n_dests, P(r32), P(rc_[0]), P(rc_[1]), cap,
                                               P(err), flags)

            assert leg_y() == 0 and leg_z() == 0, "a leg failed (or cap too small)"
            total = int(d64[n_dests + 1])
            took = {}
            if has32:
                for key, bound in (("dispatch_batch32", dp1), ("dispatch_batch32_grid", 0)):
                    ix.debug_set(DP1, bound)
                    for x in (*ra, *da):
                        x[:] = 0xC0FFEE11
                    c0 = (ix.debug_get(ONE), ix.debug_get(GRID))
                    assert leg_x() == 0
                    took[key] = "one_launch" if ix.debug_get(ONE) > c0[0] else "grid"
                    assert ix.debug_get(ONE) + ix.debug_get(GRID) == sum(c0) + 1
                    assert head32.tolist() == [M, T] == head.tolist() and np.array_equal(d64, d32.astype(np.uint64)) and \
                        all(np.array_equal(x[:total], y[:total]) for x, y in zip(ra, rb)) and \
                        all(np.array_equal(x[:T], y[:T]) for x, y in zip(da, db)) and \
                        all((x[total:] == 0xC0FFEE11).all() for x in ra) and \
                        all((x[T:] == 0xC0FFEE11).all() for x in da), \
                        f"n {n}: tm_dispatch_batch and tm_dispatch_batch32 ({key}) differ"
            legs = [("dispatch_batch", leg_y, None), ("route_batch32", leg_z, None)]
            if has32:
                legs = [("dispatch_batch32", leg_x, dp1), ("dispatch_batch32_grid", leg_x, 0)] + legs
            ms = {k: [] for k, _, _ in legs}
            for r in range(warmup + reps):
                for k, f, bound in legs:
                    if bound is not None:
                        ix.debug_set(DP1, bound)
                    t0 = time.perf_counter_ns()
                    f()
                    t1 = time.perf_counter_ns()
                    if r >= warmup:
                        ms[k].append((t1 - t0) * 1e-6)
            if has32:
                ix.debug_set(DP1, dp1)
            st = {k: dict(stats(v), p50_ms=round(float(np.median(v)), 4)) for k, v in ms.items()}
            line = {"tool": "fanout_bench", "kind": "small_dispatch", "filters": fs_len, "topics": n, "entries": total,
                    "n_dests": n_dests, "lists": name, "subs": list(a.subs), "aggre": bool(a.aggre), "bucket_entries": M,
                    "deliveries": T, "dp1_max": dp1 if has32 else None, "warmup": warmup, "reps": reps, "finished_by": took,
                    **st, "dispatch_minus_route32_ms": round(st["dispatch_batch"]["p50_ms"] - st["route_batch32"]["p50_ms"], 4),
                    "identical": True if has32 else None}
            if has32:
                line["batch32_minus_route32_ms"] = round(st["dispatch_batch32"]["p50_ms"] - st["route_batch32"]["p50_ms"], 4)
                line["batch_over_batch32"] = round(st["dispatch_batch"]["p50_ms"] / st["dispatch_batch32"]["p50_ms"], 2)
            print(json.dumps(line), flush=True)
            for x in (blob, offs32, offs64, err, d64, head, d32, r32, head32, *ra, *rb, *rc_, *da, *db):
                ix.host_free(x)


def torch_group(torch, t, v, s):
    """the grouping as a torch composition on the same device tensors (ids below 2^31: int32 order is u32 order)"""
    ss, perm = torch.sort(s, stable=True)
    gs, cnt = torch.unique_consecutive(ss, return_counts=True)
    goff = torch.zeros(len(gs) + 1, dtype=torch.int64, device=s.device)
    goff[1:] = torch.cumsum(cnt, 0)
    return t[perm], v[perm], ss, gs, goff


def group_legs(torch, a, T=1_000_000):
    """--group: tm_group_subs_dev against the torch composition (stable sort, unique_consecutive, gathers),
    interleaved, on T synthetic deliveries whose subscribers come from 1,000 / 1M pids, uniform / one pid holding half"""
    dev = torch.device("cuda")
    ix = _native.Index()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    RUN, SKIP = _native.TM_DEBUG_GROUP_PASSES_RUN, _native.TM_DEBUG_GROUP_PASSES_SKIPPED
    for pids in (1_000, 1_000_000):
        for shape in ("uniform", "skewed"):
            sub = rng.integers(0, pids, T, dtype=np.int64)
            if shape == "skewed":
                sub[rng.random(T) < 0.5] = pids // 3
            d_s = torch.from_numpy(sub.astype(np.int32)).to(dev)
            d_t = torch.from_numpy(np.sort(rng.integers(0, T // 4, T)).astype(np.int32)).to(dev)
            d_v = torch.from_numpy(rng.integers(0, 1 << 20, T).astype(np.int32)).to(dev)
            d_head = torch.tensor([T, T], dtype=torch.int64, device=dev)
            o_t, o_v, o_s = (torch.zeros(T, dtype=torch.int32, device=dev) for _ in range(3))
            o_gsub = torch.zeros(T, dtype=torch.int32, device=dev)
            o_goff = torch.zeros(T + 1, dtype=torch.int64, device=dev)
            o_ghead = torch.zeros(2, dtype=torch.int64, device=dev)

            def hip():
                ix.group_subs_dev(d_head.data_ptr(), d_t.data_ptr(), d_v.data_ptr(), d_s.data_ptr(), T, o_ghead.data_ptr(),
                                  o_gsub.data_ptr(), o_goff.data_ptr(), T, o_t.data_ptr(), o_v.data_ptr(), o_s.data_ptr(),
                                  stream=s)

            def tor():
                return torch_group(torch, d_t, d_v, d_s)

            torch.cuda.synchronize()
            p0 = (ix.debug_get(RUN), ix.debug_get(SKIP))
            hip()
            r_t, r_v, r_s, r_gs, r_goff = tor()
            torch.cuda.synchronize()
            passes = (ix.debug_get(RUN) - p0[0], ix.debug_get(SKIP) - p0[1])
            G = int(o_ghead[0])
            assert G == len(r_gs) and int(o_ghead[1]) == T and torch.equal(o_t, r_t) and torch.equal(o_v, r_v) and \
                torch.equal(o_s, r_s) and torch.equal(o_gsub[:G], r_gs) and torch.equal(o_goff[:G + 1], r_goff), \
                f"{pids} pids, {shape}: the two paths differ"
            del r_t, r_v, r_s, r_gs, r_goff
            t_hip, t_tor = timed_pair(torch, hip, tor, a.warmup, a.reps)
            h, t = stats(t_hip), stats(t_tor)
            nbytes = T * (4 + passes[0] * 20 + 8 + 28)   # pre, per pass run hist + scatter, heads, emit
            print(json.dumps({"tool": "fanout_bench", "kind": "group", "deliveries": T, "pids": pids, "shape": shape,
                              "groups": G, "passes_run": passes[0], "passes_skipped": passes[1], "reps": a.reps,
                              "hip": h, "torch": t, "torch_over_hip": round(t["median_ms"] / h["median_ms"], 2),
                              "algorithmic_bytes": nbytes,
                              "hip_algorithmic_GBps": round(nbytes / (h["median_ms"] * 1e-3) / 1e9, 1),
                              "identical": True}), flush=True)


def torch_group_picks(torch, t, v, s, et, ev, member, sub_of):
    """the merge and the grouping as a torch composition on the same device tensors (ids below 2^31): the local
    picks compacted, cat, two stable sorts (by message, then by subscriber), unique_consecutive, gathers"""
    ok = (member >= 0) & (member < len(sub_of))
    ls = torch.where(ok, sub_of[member.clamp(0, len(sub_of) - 1).long()], torch.full_like(member, -1))
    pq = torch.nonzero(ls != -1).squeeze(1)
    ct, cv, cs = torch.cat([t, et[pq]]), torch.cat([v, ev[pq]]), torch.cat([s, ls[pq]])
    _, p1 = torch.sort(ct, stable=True)
    ss, p2 = torch.sort(cs[p1], stable=True)
    perm = p1[p2]
    gs, cnt = torch.unique_consecutive(ss, return_counts=True)
    goff = torch.zeros(len(gs) + 1, dtype=torch.int64, device=s.device)
    goff[1:] = torch.cumsum(cnt, 0)
    return ct[perm], cv[perm], ss, gs, goff


def group_share_legs(torch, a, T=1_000_000, E=1_000_000):
    """--group --share: tm_group_picks_dev at T deliveries with P = 0 / 64k / 1M local picks among E entries, against
    (a) the torch composition and (b) tm_group_subs_dev on the same deliveries alone (the floor: what the parent offers
    without the picks), the three interleaved"""
    dev = torch.device("cuda")
    ix = _native.Index()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    pids, n_msgs, n_members, n_dests = 100_000, T // 4, 200_000, 4
    d_s = torch.from_numpy(rng.integers(0, pids, T).astype(np.int32)).to(dev)
    d_t = torch.from_numpy(np.sort(rng.integers(0, n_msgs, T)).astype(np.int32)).to(dev)
    d_v = torch.from_numpy(rng.integers(0, 1 << 20, T).astype(np.int32)).to(dev)
    d_head = torch.tensor([T, T], dtype=torch.int64, device=dev)
    cuts = np.sort(rng.integers(0, E + 1, n_dests))
    doff = np.concatenate([[0], cuts, [E]]).astype(np.int64)
    et = np.concatenate([np.sort(rng.integers(0, n_msgs, int(doff[b + 1] - doff[b]))) for b in range(n_dests + 1)])
    d_doff = torch.from_numpy(doff).to(dev)
    d_et = torch.from_numpy(et.astype(np.int32)).to(dev)
    d_ev = torch.from_numpy(rng.integers(0, 1 << 20, E).astype(np.int32)).to(dev)
    sub_of = np.full(n_members, -1, np.int32)
    sub_of[:n_members // 2] = rng.integers(0, pids, n_members // 2)       # the lower half of the members is local
    d_sub_of = torch.from_numpy(sub_of).to(dev)
    C = T + E
    o_t, o_v, o_s = (torch.zeros(C, dtype=torch.int32, device=dev) for _ in range(3))
    o_gsub = torch.zeros(C, dtype=torch.int32, device=dev)
    o_goff = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    o_ghead = torch.zeros(2, dtype=torch.int64, device=dev)
    f_t, f_v, f_s, f_gsub = (torch.zeros(T, dtype=torch.int32, device=dev) for _ in range(4))
    f_goff = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    f_ghead = torch.zeros(2, dtype=torch.int64, device=dev)
    for want in (0, 65_536, E):
        member = rng.integers(n_members // 2, n_members, E)              # remote
        member[rng.random(E) < 0.2] = -1                                  # no pick
        member[rng.permutation(E)[:want]] = rng.integers(0, n_members // 2, want)
        d_m = torch.from_numpy(member.astype(np.int32)).to(dev)

        def hip():
            ix.group_picks_dev(d_head.data_ptr(), d_t.data_ptr(), d_v.data_ptr(), d_s.data_ptr(), T, n_dests,
                               d_doff.data_ptr(), d_et.data_ptr(), d_ev.data_ptr(), d_m.data_ptr(), E, o_ghead.data_ptr(),
                               o_gsub.data_ptr(), o_goff.data_ptr(), C, o_t.data_ptr(), o_v.data_ptr(), o_s.data_ptr(), C,
                               d_sub_of=d_sub_of.data_ptr(), sub_of_len=n_members, stream=s)

        def tor():
            return torch_group_picks(torch, d_t, d_v, d_s, d_et, d_ev, d_m, d_sub_of)

        def floor():
            ix.group_subs_dev(d_head.data_ptr(), d_t.data_ptr(), d_v.data_ptr(), d_s.data_ptr(), T, f_ghead.data_ptr(),
                              f_gsub.data_ptr(), f_goff.data_ptr(), T, f_t.data_ptr(), f_v.data_ptr(), f_s.data_ptr(),
                              stream=s)

        hip()
        r_t, r_v, r_s, r_gs, r_goff = tor()
        floor()
        torch.cuda.synchronize()
        G, N = int(o_ghead[0]), int(o_ghead[1])
        assert N == T + want == len(r_t) and G == len(r_gs) and torch.equal(o_t[:N], r_t) and torch.equal(o_s[:N], r_s) and \
            torch.equal(o_v[:N], r_v) and torch.equal(o_gsub[:G], r_gs) and torch.equal(o_goff[:G + 1], r_goff), \
            f"P {want}: the two paths differ"
        if want == 0:
            assert torch.equal(o_t[:T], f_t) and torch.equal(o_v[:T], f_v) and torch.equal(o_s[:T], f_s)
        del r_t, r_v, r_s, r_gs, r_goff
        for _ in range(a.warmup):
            hip(), tor(), floor()
        torch.cuda.synchronize()
        ms = ([], [], [])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for _ in range(a.reps):   # interleaved: hip, torch, floor, hip, ...
            ev[0].record()
            hip()
            ev[1].record()
            tor()
            ev[2].record()
            floor()
            ev[3].record()
            torch.cuda.synchronize()
            for k in range(3):
                ms[k].append(ev[k].elapsed_time(ev[k + 1]))
        h, t, f = stats(ms[0]), stats(ms[1]), stats(ms[2])
        print(json.dumps({"tool": "fanout_bench", "kind": "group_share", "deliveries": T, "entries": E, "local_picks": want,
                          "merged": N, "groups": G, "pids": pids, "messages": n_msgs, "reps": a.reps,
                          "group_picks": h, "torch": t, "group_subs_floor": f,
                          "torch_over_hip": round(t["median_ms"] / h["median_ms"], 2),
                          "hip_over_floor": round(h["median_ms"] / f["median_ms"], 2),
                          "hip_minus_floor_ms": round(h["median_ms"] - f["median_ms"], 4), "identical": True}), flush=True)


def small_group_share(a, ix, fs_len, nvals, sizes, n_dests, warmup, reps, local=0, n_groups=4):
    """--small --group --share: tm_publish_deliver_batch host to host beside tm_publish_batch followed by
    tm_deliver_batch (what gives the same lists without it, minus the host merge), all under TM_ROUTE_AGGRE,
    interleaved; small_share's groups with members below 200,000, half of them local subscribers"""
    import time
    P = _native._ptr
    lib, h = ix._lib, ix._h
    rng = np.random.default_rng(7)
    cnt = rng.integers(a.subs[0], a.subs[1] + 1, nvals)
    loffs = np.zeros(nvals + 1, np.uint64)
    loffs[1:] = np.cumsum(cnt)
    n_pids, n_members = 100_000, 200_000
    subs = rng.integers(0, n_pids, int(loffs[-1]), dtype=np.int64).astype(np.uint32)
    assert lib.tm_set_subscribers(h, nvals, P(np.arange(nvals, dtype=np.uint32)), P(loffs), P(subs)) == 0
    dest = np.random.default_rng(7).integers(0, n_dests, nvals)   # (small_batches' destination table)
    grp = np.nonzero((dest >= 1) & (dest <= n_groups))[0].astype(np.uint32)
    ix.set_share_slots(grp, np.arange(len(grp), dtype=np.uint32))
    mc = rng.integers(2, 9, len(grp))
    moffs = np.zeros(len(grp) + 1, np.uint64)
    moffs[1:] = np.cumsum(mc)
    mem = rng.integers(0, n_members, int(moffs[-1]), dtype=np.int64).astype(np.uint32)
    zero, meta = np.zeros(len(grp), np.uint32), np.full(len(grp), _native.TM_SHARE_ROUND_ROBIN, np.uint32)
    assert lib.tm_set_share_members(h, len(grp), P(np.arange(len(grp), dtype=np.uint32)), P(moffs), P(mem), P(zero),
                                    P(meta)) == 0
    sub_of = np.where(rng.random(n_members) < 0.5, rng.integers(0, n_pids, n_members), 0xFFFFFFFF).astype(np.uint32)
    ix.set_member_subs(np.arange(n_members, dtype=np.uint32), sub_of)
    for n in sizes:
        tp = wl.topics(3, a.filters, n)
        blob, offs = np.ascontiguousarray(tp.blob), np.ascontiguousarray(tp.offs, dtype=np.uint64)
        cap = 16 * n + 1024
        d64, head, ghead, err = np.zeros(n_dests + 2, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint64), \
            np.zeros(n, np.uint8)
        rc = lib.tm_dispatch_batch(h, n, P(blob), P(offs), n_dests, local, 1, P(d64), None, None, 0, P(head), None, None,
                                   None, 0, P(err))
        assert rc in (0, _native.TM_ECAP)
        T = int(head[1])
        dcap = T + cap
        t_, v_, m_ = (np.zeros(cap, np.uint32) for _ in range(3))
        t2, v2, m2 = (np.zeros(cap, np.uint32) for _ in range(3))
        dd, dg, dm = (tuple(np.zeros(dcap, np.uint32) for _ in range(3)) for _ in range(3))
        gsub, goff = np.zeros(dcap, np.uint32), np.zeros(dcap + 1, np.uint64)
        kc = rng.integers(0, 1 << 32, n, dtype=np.uint32)

        def leg_p():
            return lib.tm_publish_batch(h, n, P(blob), P(offs), n_dests, local, 1, P(d64), P(t_), P(v_), cap, P(head),
                                        P(dd[0]), P(dd[1]), P(dd[2]), dcap, P(kc), P(kc), 1, P(m_), P(err))

        def leg_g():
            return lib.tm_deliver_batch(h, n, P(blob), P(offs), n_dests, local, 1, P(d64), P(t_), P(v_), cap, P(head),
                                        P(dg[0]), P(dg[1]), P(dg[2]), dcap, P(ghead), P(gsub), P(goff), dcap, P(err))

        def leg_m():
            return lib.tm_publish_deliver_batch(h, n, P(blob), P(offs), n_dests, local, 1, P(d64), P(t2), P(v2), cap, P(head),
                                                P(dm[0]), P(dm[1]), P(dm[2]), dcap, P(kc), P(kc), 1, P(m2), P(ghead), P(gsub),
                                                P(goff), dcap, P(err))

        # the merged call against the definition over its own entries and picks and the dispatch's deliveries
        assert leg_p() == 0 and leg_m() == 0
        K, N, G = int(d64[n_dests + 1]), int(ghead[1]), int(ghead[0])
        ls = np.where(m2[:K] < n_members, sub_of[np.minimum(m2[:K], n_members - 1)], 0xFFFFFFFF)
        pq = np.nonzero(ls != 0xFFFFFFFF)[0]
        ct, cv, cs = (np.concatenate([x[:T], y[pq]]) for x, y in ((dd[0], t2[:K]), (dd[1], v2[:K]), (dd[2], ls)))
        perm = np.lexsort((ct, cs))
        assert N == T + len(pq) and np.array_equal(dm[0][:N], ct[perm]) and np.array_equal(dm[1][:N], cv[perm]) and \
            np.array_equal(dm[2][:N], cs[perm]) and np.array_equal(gsub[:G], np.unique(cs)), \
            f"n {n}: tm_publish_deliver_batch differs from the definition"
        legs = [("publish_batch", leg_p), ("deliver_batch", leg_g), ("publish_deliver_batch", leg_m)]
        # the in-place forms on tm_host_alloc buffers: tm_publish_batch32, tm_deliver_batch32 and, merged and
        # grouped, tm_publish_deliver_batch32 (a library from before it, or --no-pd32-leg: the first two alone)
        pinned, took = [], None
        has_pd32 = hasattr(lib, "tm_publish_deliver_batch32") and not a.no_pd32_leg
        if hasattr(lib, "tm_publish_batch32") and hasattr(lib, "tm_deliver_batch32"):
            def pin(k, dt):
                pinned.append(ix.host_array(k, dt))
                return pinned[-1]
            nb = int(offs[-1])
            b32, o32, e32, k32 = pin(nb + 16, np.uint8), pin(n + 1, np.uint32), pin(n, np.uint8), pin(n, np.uint32)
            b32[:nb], o32[:], k32[:] = blob[:nb], offs.astype(np.uint32), kc
            d32, h32, gh32 = pin(n_dests + 2, np.uint32), pin(2, np.uint64), pin(2, np.uint64)
            t32, v32, m32 = (pin(cap, np.uint32) for _ in range(3))
            dd32 = tuple(pin(dcap, np.uint32) for _ in range(3))
            gs32, go32 = pin(dcap, np.uint32), pin(dcap + 1, np.uint32)

            def leg_p32():
                return lib.tm_publish_batch32(h, n, P(b32), P(o32), n_dests, local, 1, P(d32), P(t32), P(v32), cap, P(h32),
                                              P(dd32[0]), P(dd32[1]), P(dd32[2]), dcap, P(k32), P(k32), 1, P(m32), P(e32))

            def leg_g32():
                return lib.tm_deliver_batch32(h, n, P(b32), P(o32), n_dests, local, 1, P(d32), P(t32), P(v32), cap, P(h32),
                                              P(dd32[0]), P(dd32[1]), P(dd32[2]), dcap, P(gh32), P(gs32), P(go32), dcap,
                                              P(e32))

            def leg_m32():
                return lib.tm_publish_deliver_batch32(h, n, P(b32), P(o32), n_dests, local, 1, P(d32), P(t32), P(v32), cap,
                                                      P(h32), P(dd32[0]), P(dd32[1]), P(dd32[2]), dcap, P(k32), P(k32), 1,
                                                      P(m32), P(gh32), P(gs32), P(go32), dcap, P(e32))

            assert leg_p32() == 0 and leg_g32() == 0, "an in-place leg failed"
            legs += [("publish_batch32", leg_p32), ("deliver_batch32", leg_g32)]
            if has_pd32:
                # outputs equal first: both from the same start state of the slots
                slots = np.arange(len(grp), dtype=np.uint32)
                start = ix.share_state_get(slots)
                assert leg_m() == 0
                after = ix.share_state_get(slots)
                ix.share_state_set(slots, start)
                ONE = _native.TM_DEBUG_PUBLISH_DELIVER_ONE
                c0 = ix.debug_get(ONE)
                assert leg_m32() == 0
                took = "one_workgroup" if ix.debug_get(ONE) > c0 else "grid_or_staged"
                K2, N2, G2 = int(d64[n_dests + 1]), int(ghead[1]), int(ghead[0])
                assert gh32.tolist() == ghead.tolist() and h32.tolist() == head.tolist() and \
                    np.array_equal(d32[: n_dests + 2].astype(np.uint64), d64) and np.array_equal(m32[:K2], m2[:K2]) and \
                    np.array_equal(t32[:K2], t2[:K2]) and np.array_equal(v32[:K2], v2[:K2]) and \
                    all(np.array_equal(x[:N2], y[:N2]) for x, y in zip(dd32, dm)) and \
                    np.array_equal(gs32[:G2], gsub[:G2]) and np.array_equal(go32[:G2 + 1].astype(np.uint64), goff[:G2 + 1]) and \
                    np.array_equal(ix.share_state_get(slots), after), \
                    f"n {n}: tm_publish_deliver_batch32 differs from tm_publish_deliver_batch"
                legs.append(("publish_deliver_batch32", leg_m32))
        ms = {k: [] for k, _ in legs}
        for r in range(warmup + reps):
            for k, f in legs:
                t0 = time.perf_counter_ns()
                assert f() == 0
                t1 = time.perf_counter_ns()
                if r >= warmup:
                    ms[k].append((t1 - t0) * 1e-6)
        st = {k: dict(stats(v), p50_ms=round(float(np.median(v)), 4), p99_ms=round(float(np.percentile(v, 99)), 4))
              for k, v in ms.items()}
        pair = st["publish_batch"]["p50_ms"] + st["deliver_batch"]["p50_ms"]
        line = {"tool": "fanout_bench", "kind": "small_group_share", "filters": fs_len, "topics": n,
                "kept_entries": K, "n_dests": n_dests, "groups_shared": n_groups, "deliveries": T,
                "local_picks": len(pq), "merged": N, "subscribers": G, "warmup": warmup, "reps": reps, **st,
                "pair_p50_ms": round(pair, 4),
                "merged_over_pair": round(st["publish_deliver_batch"]["p50_ms"] / pair, 3),
                "merged_minus_publish_ms": round(st["publish_deliver_batch"]["p50_ms"] - st["publish_batch"]["p50_ms"], 4),
                "identical": True}
        if took is not None:
            line["merged32_by"] = took
            line["staged_over_in_place"] = round(st["publish_deliver_batch"]["p50_ms"] /
                                                 st["publish_deliver_batch32"]["p50_ms"], 2)
            line["merged32_minus_publish32_ms"] = round(st["publish_deliver_batch32"]["p50_ms"] -
                                                        st["publish_batch32"]["p50_ms"], 4)
        print(json.dumps(line), flush=True)
        for x in pinned:
            ix.host_free(x)


def small_group(a, ix, fs_len, nvals, sizes, n_dests, warmup, reps, local=0):
    """--small --group: tm_deliver_batch beside tm_dispatch_batch, host to host, interleaved"""
    import time
    P = _native._ptr
    lib, h = ix._lib, ix._h
    has = hasattr(lib, "tm_deliver_batch")   # (a library from before it: the dispatch leg alone)
    flags = _native.TM_ROUTE_AGGRE if a.aggre else 0
    rng = np.random.default_rng(7)
    cnt = rng.integers(a.subs[0], a.subs[1] + 1, nvals)
    loffs = np.zeros(nvals + 1, np.uint64)
    loffs[1:] = np.cumsum(cnt)
    subs = rng.integers(0, 100_000, int(loffs[-1]), dtype=np.int64).astype(np.uint32)   # interned, dense pids
    subs[rng.random(len(subs)) < 0.3] = 7                                              # and one fan-in consumer
    assert lib.tm_set_subscribers(h, nvals, P(np.arange(nvals, dtype=np.uint32)), P(loffs), P(subs)) == 0
    for n in sizes:
        tp = wl.topics(3, a.filters, n)
        nb = int(tp.offs[-1])
        blob, offs64 = ix.host_array(nb + 16, np.uint8), ix.host_array(n + 1, np.uint64)
        blob[:nb] = tp.blob[:nb]
        offs64[:] = tp.offs
        err = np.zeros(n, np.uint8)
        cap = 16 * n + 1024
        d64, head, ghead = (np.zeros(k, np.uint64) for k in (n_dests + 2, 2, 2))
        rc = lib.tm_dispatch_batch(h, n, P(blob), P(offs64), n_dests, local, flags, P(d64), None, None, 0, P(head),
                                   None, None, None, 0, P(err))
        assert rc in (0, _native.TM_ECAP)
        T = int(head[1])
        dcap = T + 1024
        ra, rb = ((np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)) for _ in range(2))
        da, db = (tuple(np.zeros(dcap, np.uint32) for _ in range(3)) for _ in range(2))
        gsub, goff = np.zeros(dcap, np.uint32), np.zeros(dcap + 1, np.uint64)

        def leg_d():
            return lib.tm_dispatch_batch(h, n, P(blob), P(offs64), n_dests, local, flags, P(d64), P(ra[0]), P(ra[1]), cap,
                                         P(head), P(da[0]), P(da[1]), P(da[2]), dcap, P(err))

        def leg_g():
            return lib.tm_deliver_batch(h, n, P(blob), P(offs64), n_dests, local, flags, P(d64), P(rb[0]), P(rb[1]), cap,
                                        P(head), P(db[0]), P(db[1]), P(db[2]), dcap, P(ghead), P(gsub), P(goff), dcap, P(err))

        assert leg_d() == 0, "the dispatch leg failed (or cap too small)"
        legs = [("dispatch_batch", leg_d)]
        G = None
        if has:
            assert leg_g() == 0
            G = int(ghead[0])
            p = np.argsort(da[2][:T], kind="stable")
            gs, c = np.unique(da[2][:T], return_counts=True)
            assert int(ghead[1]) == T and all(np.array_equal(x[:T][p], y[:T]) for x, y in zip(da, db)) and \
                np.array_equal(gsub[:G], gs) and np.array_equal(goff[:G + 1], np.concatenate([[0], np.cumsum(c)])), \
                f"n {n}: tm_deliver_batch differs from tm_dispatch_batch grouped on the host"
            legs.append(("deliver_batch", leg_g))
        pinned, took = [], None
        has_d32 = hasattr(lib, "tm_dispatch_batch32")
        has_g32 = hasattr(lib, "tm_deliver_batch32") and not a.no_deliver32_leg
        if has_d32:
            # the in-place forms on tm_host_alloc buffers: tm_dispatch_batch32 and, grouped, tm_deliver_batch32
            def pin(k, dt):
                pinned.append(ix.host_array(k, dt))
                return pinned[-1]
            b32, o32, e32 = pin(nb + 16, np.uint8), pin(n + 1, np.uint32), pin(n, np.uint8)
            b32[:nb], o32[:] = blob[:nb], offs64.astype(np.uint32)
            d32, h32, gh32 = pin(n_dests + 2, np.uint32), pin(2, np.uint64), pin(2, np.uint64)
            t32, v32 = (pin(cap, np.uint32) for _ in range(2))
            dd32 = tuple(pin(dcap, np.uint32) for _ in range(3))
            gs32, go32 = pin(dcap, np.uint32), pin(dcap + 1, np.uint32)

            def leg_d32():
                return lib.tm_dispatch_batch32(h, n, P(b32), P(o32), n_dests, local, flags, P(d32), P(t32), P(v32), cap,
                                               P(h32), P(dd32[0]), P(dd32[1]), P(dd32[2]), dcap, P(e32))

            def leg_g32():
                return lib.tm_deliver_batch32(h, n, P(b32), P(o32), n_dests, local, flags, P(d32), P(t32), P(v32), cap,
                                              P(h32), P(dd32[0]), P(dd32[1]), P(dd32[2]), dcap, P(gh32), P(gs32), P(go32),
                                              dcap, P(e32))

            assert leg_d32() == 0, "the in-place dispatch leg failed"
            legs.append(("dispatch_batch32", leg_d32))
            if has_g32:
                ONE = _native.TM_DEBUG_DELIVER_ONE
                c0 = ix.debug_get(ONE)
                assert leg_g() == 0 and leg_g32() == 0
                took = "one_workgroup" if ix.debug_get(ONE) > c0 else "grid_or_staged"
                assert gh32.tolist() == ghead.tolist() and h32.tolist() == head.tolist() and \
                    all(np.array_equal(x[:T], y[:T]) for x, y in zip(dd32, db)) and np.array_equal(gs32[:G], gsub[:G]) and \
                    np.array_equal(go32[:G + 1].astype(np.uint64), goff[:G + 1]), \
                    f"n {n}: tm_deliver_batch32 differs from tm_deliver_batch"
                legs.append(("deliver_batch32", leg_g32))
        ms = {k: [] for k, _ in legs}
        for r in range(warmup + reps):
            for k, f in legs:
                t0 = time.perf_counter_ns()
                f()
                t1 = time.perf_counter_ns()
                if r >= warmup:
                    ms[k].append((t1 - t0) * 1e-6)
        st = {k: dict(stats(v), p50_ms=round(float(np.median(v)), 4), p99_ms=round(float(np.percentile(v, 99)), 4))
              for k, v in ms.items()}
        line = {"tool": "fanout_bench", "kind": "small_group", "filters": fs_len, "topics": n, "entries": int(d64[n_dests + 1]),
                "n_dests": n_dests, "subs": list(a.subs), "aggre": bool(a.aggre), "deliveries": T, "groups": G,
                "warmup": warmup, "reps": reps, **st, "identical": True if has else None}
        if has:
            line["deliver_minus_dispatch_ms"] = round(st["deliver_batch"]["p50_ms"] - st["dispatch_batch"]["p50_ms"], 4)
        if took is not None:
            line["grouped_by"] = took
            line["deliver32_minus_dispatch32_ms"] = round(st["deliver_batch32"]["p50_ms"] -
                                                          st["dispatch_batch32"]["p50_ms"], 4)
            line["deliver_over_deliver32"] = round(st["deliver_batch"]["p50_ms"] / st["deliver_batch32"]["p50_ms"], 2)
        print(json.dumps(line), flush=True)
        for x in [blob, offs64] + pinned:
            ix.host_free(x)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--filters", type=int, default=1_000_000)
    p.add_argument("--batch", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--dests", type=int, nargs="+", default=[16, 4096])
    p.add_argument("--form", choices=["csr", "pairs", "both"], default="csr")
    p.add_argument("--small", action="store_true", help="the NIF's micro-batches, host to host (see above)")
    p.add_argument("--aggre", action="store_true", help="aggre/1 on the device (see above); with --small: a fourth leg")
    p.add_argument("--dispatch", action="store_true", help="local dispatch on the device (see above)")
    p.add_argument("--share", action="store_true",
                   help="the shared-subscription pick: tm_share_pick_dev vs the torch composition; with --small: "
                        "tm_publish_batch beside tm_dispatch_batch, host to host")
    p.add_argument("--group", action="store_true",
                   help="deliveries grouped by subscriber: tm_group_subs_dev vs the torch composition at 1M deliveries; "
                        "with --small: tm_deliver_batch beside tm_dispatch_batch, host to host; with --share: "
                        "tm_group_picks_dev vs the torch composition and the tm_group_subs_dev floor; with --small "
                        "--share: tm_publish_deliver_batch beside tm_publish_batch followed by tm_deliver_batch")
    p.add_argument("--dispatch-leg-only", action="store_true",
                   help="--small --share: time tm_dispatch_batch alone, as a library without tm_publish_batch is timed")
    p.add_argument("--no-deliver32-leg", action="store_true",
                   help="--small --group: leave the tm_deliver_batch32 leg out, as a library without it is timed")
    p.add_argument("--no-pd32-leg", action="store_true",
                   help="--small --group --share: leave the tm_publish_deliver_batch32 leg out, as a library without it "
                        "is timed (the two in-place legs beside it stay)")
    p.add_argument("--sizes", type=int, nargs="+", default=None, help="--small: the batch sizes")
    p.add_argument("--dp1-max", type=int, default=None,
                   help="--small --dispatch: TM_DEBUG_DP1_MAX for the dispatch_batch32 leg (default: the compiled bound)")
    p.add_argument("--subs", type=int, nargs=2, default=[1, 4], metavar=("LO", "HI"),
                   help="--small --dispatch: subscribers per value of the uniform table")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fanout_bench: no HIP device (this measurement has no CPU form)")
    if a.small:
        small_batches(a, **({"sizes": tuple(a.sizes)} if a.sizes else {}))
        return
    if a.group:
        (group_share_legs if a.share else group_legs)(torch, a)
        return
    dev = torch.device("cuda")
    fs = wl.filters(3, a.filters)
    ix = _native.Index(hint_keys=len(fs))
    ix.apply(np.ones(len(fs), np.uint8), fs.blob, fs.offs, fs.vals)
    s = torch.cuda.current_stream().cuda_stream
    ix.sync(s)
    tp = wl.topics(3, a.filters, a.batch)
    n = len(tp)
    d_blob = torch.from_numpy(tp.blob).to(dev)
    d_offs = torch.from_numpy(tp.offs.view(np.int64)).to(dev)
    cap = 16 * n
    d_hit = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_vals = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_err = torch.zeros(n, dtype=torch.uint8, device=dev)
    ix.match_batch_dev(n, d_blob.data_ptr(), d_offs.data_ptr(), d_hit.data_ptr(), d_vals.data_ptr(), cap,
                       d_err.data_ptr(), s)
    torch.cuda.synchronize()
    total = int(d_hit[n])
    assert 0 < total <= cap, f"hit total {total} against cap {cap}"
    nvals = int(fs.vals.max()) + 1
    assert int(d_vals[:total].max()) < nvals and int(d_vals[:total].min()) >= 0
    most = int((d_hit[1:] - d_hit[:-1]).max())
    if a.share:
        share_legs(torch, ix, a, s, n, d_blob, d_offs, d_err, total, most, nvals, len(fs))
        return
    if a.dispatch:
        dispatch_legs(torch, ix, a, s, n, d_blob, d_offs, d_err, total, most, nvals, len(fs))
        return
    if a.aggre:
        aggre_legs(torch, ix, a, s, n, d_blob, d_offs, d_err, total, most, nvals, len(fs))
        return
    rng = np.random.default_rng(7)
    for n_dests in a.dests:
        # every value routed, the destinations uniform: a cluster's nodes / a deployment's groups
        dest_of = torch.from_numpy(rng.integers(0, n_dests, nvals, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)
        if a.form != "csr":
            both_forms(torch, ix, a, s, n, d_blob, d_offs, d_hit, d_vals, cap, d_err, total, most, n_dests, dest_of, nvals,
                       len(fs))
            if a.form == "pairs":
                continue
        o_offs = torch.zeros(n_dests + 2, dtype=torch.int64, device=dev)
        o_topic = torch.zeros(total, dtype=torch.int32, device=dev)
        o_value = torch.zeros(total, dtype=torch.int32, device=dev)

        def hip():
            ix.fanout_dev(n, d_hit.data_ptr(), d_vals.data_ptr(), total, n_dests, o_offs.data_ptr(), o_topic.data_ptr(),
                          o_value.data_ptr(), dest_of.data_ptr(), nvals, s)

        def tor():
            return torch_fanout(torch, d_hit, d_vals, total, n, dest_of, n_dests)

        hip()
        r_offs, r_topic, r_value = tor()
        torch.cuda.synchronize()
        assert torch.equal(o_offs, r_offs) and torch.equal(o_topic, r_topic) and torch.equal(o_value, r_value), \
            f"n_dests {n_dests}: the two paths differ"
        del r_offs, r_topic, r_value
        for _ in range(a.warmup):
            hip()
            tor()
        torch.cuda.synchronize()
        t_hip, t_tor = [], []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for _ in range(a.reps):   # interleaved: hip, torch, hip, torch, ...
            ev[0].record()
            hip()
            ev[1].record()
            tor()
            ev[2].record()
            torch.cuda.synchronize()
            t_hip.append(ev[0].elapsed_time(ev[1]))
            t_tor.append(ev[1].elapsed_time(ev[2]))
        passes = 1 if n_dests + 1 <= 256 else 2
        nbytes = passes * 16 * total + 8 * (n + 1) + 8 * (n_dests + 2)
        h, t = stats(t_hip), stats(t_tor)
        print(json.dumps({"tool": "fanout_bench", "filters": len(fs), "topics": n, "entries": total,
                          "hits_per_topic": round(total / n, 3), "n_dests": n_dests, "passes": passes, "reps": a.reps,
                          "hip": h, "torch": t, "torch_over_hip": round(t["median_ms"] / h["median_ms"], 2),
                          "algorithmic_bytes": nbytes,
                          "hip_algorithmic_GBps": round(nbytes / (h["median_ms"] * 1e-3) / 1e9, 1),
                          "identical": True}), flush=True)
        assert h["median_ms"] < t["median_ms"], f"n_dests {n_dests}: the HIP path is not faster than the torch composition"
    if a.form != "csr":
        synthetic_skew(torch, ix, a, s, n, total)


if __name__ == "__main__":
    main()
