#!/usr/bin/env python3
"""Retained-message lookup: the device store against the torch composition.

    python tools/retain_bench.py --rows 1000000 [--out profiles/retain/bench_1m.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/retain_bench.py --rows 1000000 --trace full_scan:64 [--page 1000]
    python tools/retain_bench.py --rows 1000000 --page 1000 [--scan-rows N] [--out profiles/retain/page_1m.jsonl]

Store: `--rows` distinct topics of the C3 workload's topic stream (seeded;
the stream repeats a few topics, so it is drawn until the store holds that
many), every tenth with an expiry in the future, compacted into the base.

Filter classes, made from stored topics: exact; narrow (the first two levels
and '#'); plus_leaf (prefix/+/leaf: the last level but one replaced by '+');
full_scan (every level but the last replaced by '+': no prefix, every row is
tested); hash ('#').  Batches of 1, 64 and 1,024 filters; a leg whose result
would pass --max-hits values is reported as not measured.

Per leg: the host-to-host p50 of tm_retained_match (sizing call and filling
call together, as a caller without a buffer pays) over a window of at least
--window seconds after warm-up; then the store and the torch composition on
the same column tensors alternately, --repeats times each; their outputs are
compared as sorted lists per filter.  The store counts as faster only when its
slowest repeat beats the composition's fastest.

The composition, per filter: (nlev == k or nlev >= k) & live & the '$' mask &
the expiry mask & a conjunction of == over the literal levels' columns, then
nonzero and a gather of the values.

--page LIMIT measures match cursors instead (tm_retained_match_page): the first
page of LIMIT values per filter for the classes hash and full_scan at batches
of 1, 64 and 1,024, one call with one buffer of batch * LIMIT values, against
tm_retained_match of the same filters (sizing and filling call) in the same
run, alternating, --repeats times each.  For hash x 1,024 the full list cannot
be held (1.0e9 values), so that leg is compared against the full match of the
batch of 64 and says so.  Every page is checked against the full list: its
length is min(LIMIT, the list's length) and its values are among the list's,
without a duplicate.  Then one leg of '#' with LIMIT = 65,536 page by page to
the end against the single full match, the drain's values compared as a sorted
list.  "Faster" only where the slower side's fastest repeat is slower than the
other's slowest.

Kernel times are not taken here: --trace CLASS:BATCH runs that leg alone (no
composition), for a rocprofv3 --kernel-trace --stats run of its own.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from emqx_amd import _native, workload  # noqa: E402

NOW = 1_000_000
CLASSES = ("exact", "narrow", "plus_leaf", "full_scan", "hash")
BATCHES = (1, 64, 1024)
HBM_TBS = 8.0   # MI355X peak HBM bandwidth


def build_store(rows: int, seed: int, tail_max: int):
    """-> (store, topics list in value order, expiry array, seconds to load, seconds to compact)"""
    s = _native.Retained(initial_rows=rows + rows // 8 + 1024, tail_max=tail_max)
    topics, first, t_put = [], 0, 0.0
    while len(topics) < rows:
        want = rows - len(topics)
        chunk = workload.topics(3, 1_000_000, want + want // 16 + 1024, first=first, seed=seed)
        first += len(chunk)
        # a row's value is its topic's index in `topics`: the stream's repeats are dropped here
        seen = set(topics)
        keep = []
        for t in chunk.items():
            if t not in seen and len(topics) + len(keep) < rows:
                seen.add(t)
                keep.append(t)
        vals = np.arange(len(topics), len(topics) + len(keep), dtype=np.uint32)
        exp = np.where(vals % 10 == 3, NOW + 1 + vals.astype(np.uint64), 0).astype(np.uint64)
        t0 = time.perf_counter()
        code = s.put(keep, vals, exp)
        t_put += time.perf_counter() - t0
        assert (code == 1).all()
        topics += keep
    t0 = time.perf_counter()
    s.compact()
    t_compact = time.perf_counter() - t0
    vals = np.arange(rows, dtype=np.uint64)
    expiry = np.where(vals % 10 == 3, NOW + 1 + vals, 0).astype(np.uint64)
    return s, topics, expiry, t_put, t_compact


def make_filters(topics, cls: str, n: int, r: np.random.Generator):
    out = []
    while len(out) < n:
        lv = topics[int(r.integers(len(topics)))].split(b"/")
        if cls == "exact":
            out.append(b"/".join(lv))
        elif cls == "narrow" and len(lv) >= 3:
            out.append(b"/".join(lv[:2]) + b"/#")
        elif cls == "plus_leaf" and len(lv) >= 3:
            out.append(b"/".join(lv[:-2] + [b"+", lv[-1]]))
        elif cls == "full_scan" and len(lv) >= 2:
            out.append(b"/".join([b"+"] * (len(lv) - 1) + [lv[-1]]))
        elif cls == "hash":
            out.append(b"#")
    return out


class Columns:
    """the same rows as torch tensors on the device, ids from a dictionary of our own"""

    def __init__(self, topics, expiry):
        import torch
        self.torch = torch
        self.ids = {}
        n = len(topics)
        cols = np.full((_native.RT_COLS, n), 0xFFFFFFFF, np.int64)
        nlev = np.zeros(n, np.int32)
        dollar = np.zeros(n, bool)
        for i, t in enumerate(topics):
            lv = t.split(b"/")
            assert len(lv) <= _native.RT_COLS, "the composition covers the column levels"
            nlev[i] = len(lv)
            dollar[i] = t[:1] == b"$"
            for l, w in enumerate(lv):
                cols[l, i] = self.ids.setdefault(w, len(self.ids))
        dev = torch.device("cuda")
        self.cols = [torch.from_numpy(cols[l].astype(np.int32)).to(dev) for l in range(_native.RT_COLS)]
        self.nlev = torch.from_numpy(nlev).to(dev)
        self.not_dollar = torch.from_numpy(~dollar).to(dev)
        self.expiry = torch.from_numpy(expiry.astype(np.int64)).to(dev)
        self.values = torch.arange(n, dtype=torch.int32, device=dev)

    def match(self, filters, now):
        torch = self.torch
        visible = (self.expiry == 0) | (self.expiry > now)
        out = []
        for f in filters:
            lv = f.split(b"/")
            hash_ = lv[-1] == b"#"
            if hash_:
                lv = lv[:-1]
            ids = [None if w == b"+" else self.ids.get(w, -2) for w in lv]
            mask = (self.nlev >= len(lv)) if hash_ else (self.nlev == len(lv))
            mask = mask & visible
            if (hash_ and not lv) or (lv and lv[0] == b"+"):
                mask = mask & self.not_dollar
            for l, w in enumerate(ids):
                if w is not None:
                    mask = mask & (self.cols[l] == w)
            out.append(self.values[mask.nonzero().squeeze(1)])
        torch.cuda.synchronize()
        return out


def scan_bytes(cls, filters, rows, hits, expiry_share):
    """the bytes a full scan must read, per pass: meta and the literal levels' columns for every row of every
    filter, expiry only for the rows that pass every other test and carry one -- here the hits (no stored expiry
    has passed at NOW), of which `expiry_share` are flagged"""
    if cls not in ("full_scan", "hash"):
        return None
    total = 8 * expiry_share * hits
    for f in filters:
        lit = sum(w not in (b"+", b"#") for w in f.split(b"/"))
        total += rows * (4 + 4 * lit)
    return round(total)


def run_leg(s, cols, topics, cls, batch, args, r):
    filters = make_filters(topics, cls, batch, r)
    blob, offs = _native.pack_strings(filters)
    hit, vals, _ = s.match_packed(blob, offs, NOW)          # warm-up, and the size of the result
    total = int(hit[-1])
    leg = {"class": cls, "batch": batch, "rows": len(topics), "hits": total}
    if total > args.max_hits:
        leg["status"] = "not measured: %d values in the result" % total
        return leg
    for _ in range(2):
        s.match_packed(blob, offs, NOW)
    times, t_end = [], time.perf_counter() + args.window
    while time.perf_counter() < t_end or len(times) < 5:
        t0 = time.perf_counter()
        s.match_packed(blob, offs, NOW)
        times.append(time.perf_counter() - t0)
    leg["store_p50_us"] = round(float(np.median(times)) * 1e6, 1)
    leg["store_calls"] = len(times)
    leg["scan_bytes_per_pass"] = scan_bytes(cls, filters, len(topics), total, 0.1)
    if cols is not None:
        ref = cols.match(filters, NOW)                           # warm-up
        st, tt = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            hit, vals, _ = s.match_packed(blob, offs, NOW)
            st.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ref = cols.match(filters, NOW)
            tt.append(time.perf_counter() - t0)
        for i in range(batch):
            got = np.sort(vals[int(hit[i]):int(hit[i + 1])])
            want = np.sort(ref[i].cpu().numpy().astype(np.uint32))
            assert np.array_equal(got, want), (cls, batch, i, filters[i], len(got), len(want))
        leg["store_us"] = [round(x * 1e6, 1) for x in st]
        leg["torch_us"] = [round(x * 1e6, 1) for x in tt]
        leg["store_faster"] = max(st) < min(tt)
        leg["torch_faster"] = max(tt) < min(st)
        leg["ratio_p50"] = round(float(np.median(tt) / np.median(st)), 2)
        leg["outputs_equal"] = True
    return leg


def _timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def _verdict(leg, page_t, full_t):
    leg["page_us"] = [round(x * 1e6, 1) for x in page_t]
    leg["full_us"] = [round(x * 1e6, 1) for x in full_t]
    leg["page_faster"] = max(page_t) < min(full_t)
    leg["full_faster"] = max(full_t) < min(page_t)
    leg["ratio_p50"] = round(float(np.median(full_t) / np.median(page_t)), 2)


def page_leg(s, topics, cls, batch, args, r):
    """the first page of args.page values per filter against the whole lists of the same filters"""
    filters = make_filters(topics, cls, batch, r)
    blob, offs = _native.pack_strings(filters)
    full_batch = batch
    leg = {"mode": "first_page", "class": cls, "batch": batch, "limit": args.page, "scan_rows": args.scan_rows,
           "rows": len(topics)}
    if cls == "hash" and batch > 64:   # 1.0e9 values: the full list cannot be held
        full_batch = 64
        leg["comparator"] = "tm_retained_match of a batch of 64 '#': the full list of %d cannot be held" % batch
    fblob, foffs = _native.pack_strings(filters[:full_batch])
    page = lambda: s.match_page_packed(blob, offs, NOW, None, args.page, args.scan_rows)
    full = lambda: s.match_packed(fblob, foffs, NOW)
    st0 = s.stats()["match_launches"]
    hit, vals, cur, err = page()                                 # warm-up, and the check
    leg["device_calls_per_lookup"] = s.stats()["match_launches"] - st0
    fhit, fvals, _ = full()
    assert not err.any()
    for i in range(full_batch):
        got, whole = vals[int(hit[i]):int(hit[i + 1])], fvals[int(fhit[i]):int(fhit[i + 1])]
        if not args.scan_rows:
            assert len(got) == min(args.page, len(whole)), (cls, batch, i, len(got), len(whole))
            assert (int(cur[i]) == _native.TM_RET_CURSOR_DONE) == (len(got) < args.page)
        assert len(np.unique(got)) == len(got) and np.isin(got, whole).all(), (cls, batch, i)
    leg["page_values"], leg["full_values"] = int(hit[-1]), int(fhit[-1])
    leg["live_cursors"] = int((cur != np.uint64(_native.TM_RET_CURSOR_DONE)).sum())
    times, t_end = [], time.perf_counter() + args.window
    while time.perf_counter() < t_end or len(times) < 5:
        times.append(_timed(page)[0])
    leg["page_p50_us"], leg["page_calls"] = round(float(np.median(times)) * 1e6, 1), len(times)
    pt, ft = [], []
    for _ in range(args.repeats):
        pt.append(_timed(page)[0])
        ft.append(_timed(full)[0])
    _verdict(leg, pt, ft)
    leg["outputs_checked"] = True
    return leg


def drain_leg(s, args):
    """'#' page by page to the end with LIMIT = 65,536 against the single full match"""
    limit = 65_536
    blob, offs = _native.pack_strings([b"#"])

    def drain():
        parts, cur, calls = [], None, 0
        while cur is None or int(cur[0]) != _native.TM_RET_CURSOR_DONE:
            hit, vals, cur, _ = s.match_page_packed(blob, offs, NOW, cur, limit, args.scan_rows)
            parts.append(vals)
            calls += 1
        return np.concatenate(parts), calls
    full = lambda: s.match_packed(blob, offs, NOW)
    (got, calls), (fhit, fvals, _) = drain(), full()
    assert np.array_equal(np.sort(got), np.sort(fvals)), (len(got), len(fvals))
    leg = {"mode": "full_drain", "class": "hash", "batch": 1, "limit": limit, "scan_rows": args.scan_rows,
           "values": int(len(got)), "calls_per_drain": calls, "outputs_equal": True}
    dt, ft = [], []
    for _ in range(args.repeats):
        dt.append(_timed(drain)[0])
        ft.append(_timed(full)[0])
    _verdict(leg, dt, ft)
    return leg


def tail_cost(s, topics, args, r, emit):
    """what a tail of T rows costs every filter, against what one compaction costs"""
    filters = make_filters(topics, "exact", 64, r)
    blob, offs = _native.pack_strings(filters)

    def p50():
        for _ in range(3):
            s.match_packed(blob, offs, NOW)
        ts = []
        for _ in range(50):
            t0 = time.perf_counter()
            s.match_packed(blob, offs, NOW)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e6
    base = p50()
    added = 0
    for T in (4096, 65536):                                     # each tail is timed, then merged: one compaction each
        extra = [b"tail/%d/%d" % (T, i) for i in range(T)]
        s.put(extra, np.arange(T, dtype=np.uint32) + 0x40000000 + added, None)
        added += T
        emit({"tail_rows": s.stats()["tail_rows"], "exact_batch64_p50_us": round(p50(), 1), "no_tail_p50_us": round(base, 1)})
        t0 = time.perf_counter()
        s.compact()
        emit({"compaction_s": round(time.perf_counter() - t0, 4), "rows": s.stats()["base_rows"], "merged_tail_rows": T})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0x52455442)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-hits", type=int, default=80_000_000)
    ap.add_argument("--trace", default=None, help="CLASS:BATCH -- that leg alone, 20 calls, no composition")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--page", type=int, nargs="?", const=1000, default=None, metavar="LIMIT",
                    help="match cursors: the first page of LIMIT values (default 1000) against the full match")
    ap.add_argument("--scan-rows", type=int, default=0, help="with --page: rows a filter examines per call (0: no bound)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    r = np.random.default_rng(args.seed)
    s, topics, expiry, t_put, t_compact = build_store(args.rows, args.seed, tail_max=args.rows + 70_000)
    st = s.stats()
    emit({"store": st, "distinct_topics": len(set(topics)), "load_s": round(t_put, 2), "first_compaction_s": round(t_compact, 2)})
    if args.trace:
        cls, batch = args.trace.split(":")
        filters = make_filters(topics, cls, int(batch), r)
        blob, offs = _native.pack_strings(filters)
        for _ in range(22):
            if args.page is not None:                            # (with --page: that leg's first page alone)
                hit = s.match_page_packed(blob, offs, NOW, None, args.page, args.scan_rows)[0]
            else:
                hit, _, _ = s.match_packed(blob, offs, NOW)
        emit({"trace": args.trace, "calls": 22, "hits": int(hit[-1]),
              "scan_bytes_per_pass": scan_bytes(cls, filters, len(topics), int(hit[-1]), 0.1)})
    elif args.page is not None:
        for cls in ("hash", "full_scan"):
            for batch in BATCHES:
                emit(page_leg(s, topics, cls, batch, args, r))
        emit(drain_leg(s, args))
    else:
        cols = None if args.no_torch else Columns(topics, expiry)
        for cls in CLASSES:
            for batch in BATCHES:
                emit(run_leg(s, cols, topics, cls, batch, args, r))
        tail_cost(s, topics, args, r, emit)
    s.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(d) + "\n" for d in lines))


if __name__ == "__main__":
    main()
