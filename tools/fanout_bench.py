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
"""
import argparse
import json
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--filters", type=int, default=1_000_000)
    p.add_argument("--batch", type=int, default=1_000_000)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--dests", type=int, nargs="+", default=[16, 4096])
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fanout_bench: no HIP device (this measurement has no CPU form)")
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
    rng = np.random.default_rng(7)
    for n_dests in a.dests:
        # every value routed, the destinations uniform: a cluster's nodes / a deployment's groups
        dest_of = torch.from_numpy(rng.integers(0, n_dests, nvals, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)
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


if __name__ == "__main__":
    main()
