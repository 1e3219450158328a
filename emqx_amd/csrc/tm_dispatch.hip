// tm_dispatch.hip -- emqx_broker:dispatch/2 on the local node's bucket of the
// route fan-out, for gfx950.
//
// do_publish/1 is route(aggre(match_routes(Topic)), Delivery); for a route on
// the local node do_route2/2 calls emqx_broker:dispatch/2, and do_dispatch2/2
// (apps/emqx/src/emqx_broker.erl:726-760) looks (message, To) up in the
// ?SUBSCRIBER bag and sends {deliver, To, Msg} to every pid, shard rows
// expanded where they stand.  On the device that is a segmented expansion: the
// M entries of one bucket of the fan-out's (or the aggre pass's) output, each
// with the subscriber list of its value -- span[2 v] words into pool,
// span[2 v + 1] of them -- become T = sum(cnt) deliveries (topic, value,
// subscriber) in entry order and list order.
//
// List lengths are very skewed (one subscriber mostly, 10^5 for a broadcast
// filter), so the output, not the input, is what the blocks share out.  The
// fan-out's fixed grid, FO_GRID one-wave blocks, no block waits for another;
// four launches:
//   k_dp_count    block k owns the entries [k * chunk, (k + 1) * chunk) of
//                 [0, M), chunk = ceil(M / FO_GRID) rounded up to 64: values
//                 loaded coalesced, the span's 8 bytes gathered, a span that
//                 does not lie inside the pool counted as empty; the counts go
//                 to scratch, the chunk's 64-bit sum to tot[k];
//   k_dp_scan     the exclusive scan of the FO_GRID sums; head = [M, T];
//   k_dp_offsets  block k wave-scans its chunk's counts from its base into
//                 off[], off[M] = T;
//   k_dp_expand   block k owns the output positions [k * ochunk, (k + 1) *
//                 ochunk) of [0, W), W = min(T, out_cap), ochunk = ceil(W /
//                 FO_GRID) rounded up to 64.  The entry of a position is the
//                 last j with off[j] <= p: the fan-out's 64-ary search at the
//                 chunk's start, then its LDS window of the next 64 offsets per
//                 step (tm_dev.h fo_topic_at, fo_step_topics).  Lane p writes
//                 (topic[j], value[j], pool[pos_j + p - off[j]]): consecutive
//                 lanes inside one list read consecutive pool words, and a
//                 10^5-subscriber list is spread over many blocks.
// Bytes per entry: 4 read + 8 gathered (count), 4 written + 4 read + 8 written
// (counts, offsets); per delivery: 12 written + 4 read (pool) and, per run of
// one entry's deliveries inside a step, 8 + 8 + 8 gathered (offset, topic and
// value, span).
#include <hip/hip_runtime.h>

#include "tm_dev.h"

namespace tmx {

namespace {

constexpr int DP_UNROLL = 4;   // steps whose loads a counting block issues together
static_assert(FO_GRID % 256 == 0, "k_dp_scan: 256 threads share the sums evenly");

// the bucket's entries: [q0, q0 + M) of the input arrays
__device__ __forceinline__ void dp_bucket(const uint64_t *doff, uint32_t n_dests, uint32_t bucket, uint64_t cap,
                                          uint64_t &q0, uint64_t &M) {
    const uint64_t total = doff[n_dests + 1], E = total < cap ? total : cap;
    const uint64_t a = doff[bucket], b = doff[bucket + 1];
    q0 = a < E ? a : E;
    const uint64_t q1 = b < E ? b : E;
    M = q1 > q0 ? q1 - q0 : 0;
}

// the positions block `blk` owns: [c0, c1) of [0, N)
__device__ __forceinline__ void dp_chunk(uint64_t N, uint32_t blk, uint64_t &c0, uint64_t &c1) {
    const uint64_t chunk = ((N + FO_GRID - 1) / FO_GRID + 63) & ~63ull;
    c0 = (uint64_t)blk * chunk;
    c1 = c0 + chunk < N ? c0 + chunk : N;
    if (c0 > c1) c0 = c1;
}

__device__ __forceinline__ uint64_t dp_incl_scan64(uint64_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    return x;
}

// value v's list: its count, 0 when v has no span or the span does not lie
// inside the pool (the sum in 64 bits: pos + cnt may pass 2^32)
__device__ __forceinline__ uint32_t dp_count(uint32_t v, const uint2 *span, uint64_t span_len, uint64_t pool_len) {
    if (v >= span_len) return 0u;
    const uint2 sp = span[v];
    return (uint64_t)sp.x + sp.y > pool_len ? 0u : sp.y;
}

__global__ __launch_bounds__(64) void k_dp_count(const uint64_t *doff, uint32_t n_dests, uint32_t bucket, uint64_t cap,
                                                 const uint32_t *in_v, const uint2 *span, uint64_t span_len,
                                                 uint64_t pool_len, uint32_t *cnt, uint64_t *tot) {
    const uint32_t lane = threadIdx.x;
    uint64_t q0, M, c0, c1;
    dp_bucket(doff, n_dests, bucket, cap, q0, M);
    dp_chunk(M, blockIdx.x, c0, c1);
    uint64_t sum = 0;
    for (uint64_t p0 = c0; p0 < c1; p0 += 64 * DP_UNROLL) {
        uint32_t v[DP_UNROLL], c[DP_UNROLL];
#pragma unroll
        for (int k = 0; k < DP_UNROLL; k++) {
            const uint64_t p = p0 + (uint64_t)k * 64 + lane;
            v[k] = p < c1 ? in_v[q0 + p] : 0u;
        }
#pragma unroll
        for (int k = 0; k < DP_UNROLL; k++) {
            const uint64_t p = p0 + (uint64_t)k * 64 + lane;
            c[k] = p < c1 ? dp_count(v[k], span, span_len, pool_len) : 0u;
        }
#pragma unroll
        for (int k = 0; k < DP_UNROLL; k++) {
            const uint64_t p = p0 + (uint64_t)k * 64 + lane;
            if (p < c1) cnt[p] = c[k];
            sum += c[k];
        }
    }
    const uint64_t inc = dp_incl_scan64(sum, lane);
    if (lane == 63) tot[blockIdx.x] = inc;   // (every block, every run: nothing of an earlier run survives)
}

// the FO_GRID chunk sums -> their exclusive scan in place, T into tot[FO_GRID]; head = [M, T]
__global__ __launch_bounds__(256) void k_dp_scan(const uint64_t *doff, uint32_t n_dests, uint32_t bucket, uint64_t cap,
                                                 uint64_t *tot, uint64_t *head) {
    constexpr int PER = FO_GRID / 256;
    __shared__ uint64_t s_w[4];
    uint64_t *row = tot + threadIdx.x * PER;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t x[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { x[k] = row[k]; sum += x[k]; }
    const uint64_t inc = dp_incl_scan64(sum, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint64_t base = inc - sum;
    for (uint32_t q = 0; q < wv; q++) base += s_w[q];
#pragma unroll
    for (int k = 0; k < PER; k++) { row[k] = base; base += x[k]; }
    if (threadIdx.x == 255) {
        uint64_t q0, M;
        dp_bucket(doff, n_dests, bucket, cap, q0, M);
        tot[FO_GRID] = base;
        head[0] = M;
        head[1] = base;
    }
}

__global__ __launch_bounds__(64) void k_dp_offsets(const uint64_t *doff, uint32_t n_dests, uint32_t bucket, uint64_t cap,
                                                   const uint32_t *cnt, const uint64_t *tot, uint64_t *off) {
    const uint32_t lane = threadIdx.x;
    uint64_t q0, M, c0, c1;
    dp_bucket(doff, n_dests, bucket, cap, q0, M);
    dp_chunk(M, blockIdx.x, c0, c1);
    uint64_t base = tot[blockIdx.x];
    for (uint64_t p0 = c0; p0 < c1; p0 += 64) {
        const uint64_t p = p0 + lane;
        const uint64_t c = p < c1 ? cnt[p] : 0u;
        const uint64_t inc = dp_incl_scan64(c, lane);
        if (p < c1) off[p] = base + inc - c;
        base += __shfl(inc, 63, 64);
    }
    if (blockIdx.x == 0 && lane == 0) off[M] = tot[FO_GRID];
}

__global__ __launch_bounds__(64) void k_dp_expand(const uint64_t *doff, uint32_t n_dests, uint32_t bucket, uint64_t cap,
                                                  const uint32_t *in_t, const uint32_t *in_v, const uint2 *span,
                                                  uint64_t span_len, const uint32_t *pool, uint64_t pool_len,
                                                  const uint64_t *off, const uint64_t *tot, uint32_t *out_t,
                                                  uint32_t *out_v, uint32_t *out_s, uint64_t out_cap) {
    __shared__ uint64_t s_win[64];
    const uint32_t lane = threadIdx.x;
    uint64_t q0, M, c0, c1;
    dp_bucket(doff, n_dests, bucket, cap, q0, M);
    const uint64_t T = tot[FO_GRID], W = T < out_cap ? T : out_cap;
    dp_chunk(W, blockIdx.x, c0, c1);
    uint64_t jcur = 0;   // off[jcur] <= the step's first position
    if (c0 < c1) jcur = fo_topic_at(off, M, c0, 0, lane);
    for (uint64_t p0 = c0; p0 < c1; p0 += 64) {
        const uint64_t p = p0 + lane;
        const bool ok = p < c1;
        const uint32_t j = fo_step_topics(off, M, p0, c1, ok, jcur, s_win, lane);
        if (ok && j < M) {   // (j < M always: p < T = off[M])
            const uint32_t t = in_t[q0 + j], v = in_v[q0 + j];
            uint32_t sub = 0;
            if (v < span_len) {   // (always, and the word lies inside the pool: k_dp_count counted this list)
                const uint64_t at = (uint64_t)span[v].x + (p - off[j]);
                if (at < pool_len) sub = pool[at];
            }
            out_t[p] = t;
            out_v[p] = v;
            out_s[p] = sub;
        }
    }
}

// ---- a micro-batch (tm_dispatch_batch32): ONE workgroup of FO1_BLOCK threads
// finishes what k_fo_one (and under TM_ROUTE_AGGRE k_ag_one) left in the
// lane's scratch -- u32 offsets, topics, values, the status words -- and
// writes every output of the caller, which may be mapped host memory: the
// device never reads those buffers.
//   1. the route outputs: the n_dests + 2 final bucket offsets, one thread
//      each, and the first min(E, cap) entries, consecutive threads to
//      consecutive slots.  Under aggre with more un-aggregated entries than
//      cap the caller has no room for the fan-out (TM_ECAP): the fan-out's
//      offsets and no entry, as tm_route_batch_ex; the dispatch below still
//      runs on the aggregated arrays, as tm_dispatch_batch's does.
//   2. the local bucket's M entries: wave w owns [w * C, (w + 1) * C), C =
//      ceil(M / 16) rounded up to 64; values loaded coalesced, the span's 8
//      bytes gathered, dp_count's rule; the list's pool position goes to
//      s_pos, the wave's running 64-bit scan of the counts (low words) to
//      s_off, the wave totals to LDS; after the barrier every wave adds its
//      base to its own part.  head = [M, T].
//   3. T > dp1_max: DP1_TOO_LARGE in the status word, nothing expanded (the
//      host queues the grid kernels on the same arrays).  Else the W = min(T,
//      dcap) output positions are shared out over the waves in 64-aligned
//      chunks; a wave finds its first entry by binary search of s_off and
//      steps on from there: a lane searches the 64 offsets after the step's
//      first entry, and all of them up to M only when its entry lies beyond
//      (a run of more than 64 empty entries).  Lane p writes (topic[j],
//      value[j], pool[s_pos[j] + p - s_off[j]]): the three loads of a step
//      depend on LDS alone, DP1_UNROLL steps' loads are in flight together.
// Bytes per entry: 8 read + 8 written (route copy), 4 read + 8 gathered
// (count), 8 of LDS; per delivery: 12 written + 4 read (pool) + 8 gathered
// (topic, value).  128 KiB + 144 B of static LDS, no scratch.
constexpr uint32_t DP1_WAVES = FO1_BLOCK / 64;
constexpr uint32_t DP1_STEPS = FO1_ENTRIES / FO1_BLOCK;   // 64-entry steps of a wave's counting, at most
constexpr int DP1_UNROLL = 4;
static_assert(FO1_MAX_DESTS + 2 <= FO1_BLOCK, "k_dp_one: one thread per offset");
static_assert(DP1_DELIVERIES < 0xFFFFFFFFull, "k_dp_one: 32-bit delivery offsets in LDS");

// the last j of [lo, hi) with off[j] <= p (off[lo] <= p < off[hi])
__device__ __forceinline__ uint32_t dp1_search(const uint32_t *off, uint32_t lo, uint32_t hi, uint32_t p) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(FO1_BLOCK) void k_dp_one(
    const uint32_t *st_in, const uint32_t *fo_doff, const uint32_t *fo_t, const uint32_t *fo_v, const uint32_t *ag_doff,
    const uint32_t *ag_t, const uint32_t *ag_v, uint32_t n_dests, uint32_t bucket, const uint2 *span, uint64_t span_len,
    const uint32_t *pool, uint64_t pool_len, uint32_t *out_doff, uint32_t *out_t, uint32_t *out_v, uint64_t cap,
    uint64_t *out_head, uint32_t *out_dt, uint32_t *out_dv, uint32_t *out_ds, uint64_t dcap, uint64_t dp1_max,
    uint32_t *st_out) {
    __shared__ uint32_t s_off[FO1_ENTRIES + 1];
    __shared__ uint32_t s_pos[FO1_ENTRIES];
    __shared__ uint64_t s_wt[DP1_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t state = st_in[FO1_ST_STATE], total = st_in[FO1_ST_TOTAL];
    if (state != FO1_DONE || n_dests > FO1_MAX_DESTS || bucket > n_dests) {   // (block-uniform)
        if (tid == 0) {
            st_out[DP1_ST_T_LO] = 0; st_out[DP1_ST_T_HI] = 0;
            st_out[FO1_ST_TOTAL] = total; st_out[FO1_ST_STATE] = state == FO1_DONE ? FO1_TOO_LARGE : state;
        }
        return;
    }
    // 1. the route outputs
    uint32_t Ef = fo_doff[n_dests + 1];
    if (Ef > FO1_ENTRIES) Ef = FO1_ENTRIES;   // (never: k_fo_one completed)
    const bool aggre = ag_doff != nullptr;
    const bool room = Ef <= cap;
    const uint32_t *doff = aggre ? ag_doff : fo_doff, *in_t = aggre ? ag_t : fo_t, *in_v = aggre ? ag_v : fo_v;
    uint32_t E = doff[n_dests + 1];   // the entries the dispatch reads
    if (E > Ef) E = Ef;               // (never: aggre keeps a subset)
    if (tid <= n_dests + 1) out_doff[tid] = aggre && !room ? fo_doff[tid] : doff[tid];
    const uint32_t keep = aggre ? (room ? E : 0u) : (room ? E : (uint32_t)cap);
    for (uint32_t i = tid; i < keep; i += FO1_BLOCK) {
        out_t[i] = in_t[i];
        out_v[i] = in_v[i];
    }
    // 2. the local bucket's counts and their scan
    const uint32_t a = doff[bucket], b = doff[bucket + 1];
    const uint32_t q0 = a < E ? a : E, q1 = b < E ? b : E, M = q1 > q0 ? q1 - q0 : 0;
    in_t += q0;
    in_v += q0;
    const uint32_t C = ((M + DP1_WAVES - 1) / DP1_WAVES + 63) & ~63u;   // (<= 64 * DP1_STEPS)
    const uint32_t c0 = wv * C < M ? wv * C : M, c1 = c0 + C < M ? c0 + C : M;
    uint64_t run = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < DP1_STEPS; k++) {
        if (k * 64 >= C) break;   // (block-uniform)
        const uint32_t p = c0 + k * 64 + lane;
        uint32_t cnt = 0, pos = 0;
        if (p < c1) {
            const uint32_t v = in_v[p];
            if (v < span_len) {
                const uint2 sp = span[v];
                pos = sp.x;
                cnt = (uint64_t)sp.x + sp.y > pool_len ? 0u : sp.y;
            }
        }
        const uint64_t inc = dp_incl_scan64(cnt, lane);
        if (p < c1) {
            s_off[p] = (uint32_t)(run + inc - cnt);
            s_pos[p] = pos;
        }
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) s_wt[wv] = run;
    __syncthreads();
    uint64_t base = 0, T = 0;
    for (uint32_t q = 0; q < DP1_WAVES; q++) {
        if (q < wv) base += s_wt[q];
        T += s_wt[q];
    }
    if (tid == 0) {
        out_head[0] = M;
        out_head[1] = T;
        st_out[DP1_ST_T_LO] = (uint32_t)T;
        st_out[DP1_ST_T_HI] = (uint32_t)(T >> 32);
    }
    if (T > dp1_max || T > DP1_DELIVERIES) {   // (block-uniform)
        if (tid == 0) { st_out[FO1_ST_TOTAL] = total; st_out[FO1_ST_STATE] = DP1_TOO_LARGE; }
        return;
    }
    for (uint32_t p = c0 + lane; p < c1; p += 64) s_off[p] += (uint32_t)base;   // (its own wave's part)
    if (tid == 0) s_off[M] = (uint32_t)T;
    __syncthreads();
    // 3. the expansion
    const uint32_t W = T < dcap ? (uint32_t)T : (uint32_t)dcap;
    const uint32_t D = ((W + DP1_WAVES - 1) / DP1_WAVES + 63) & ~63u;
    const uint32_t d0 = wv * D < W ? wv * D : W, d1 = d0 + D < W ? d0 + D : W;
    uint32_t jcur = 0;   // s_off[jcur] <= the step's first position
    if (d0 < d1) jcur = dp1_search(s_off, 0, M, d0);   // (d0 < W <= T = s_off[M])
    for (uint32_t p0 = d0; p0 < d1; p0 += 64 * DP1_UNROLL) {
        uint32_t j[DP1_UNROLL], at[DP1_UNROLL], t[DP1_UNROLL], v[DP1_UNROLL], sub[DP1_UNROLL];
#pragma unroll
        for (int k = 0; k < DP1_UNROLL; k++) {
            const uint32_t p = p0 + k * 64 + lane;
            j[k] = jcur;
            at[k] = 0;
            if (p < d1) {
                const uint32_t w1 = jcur + 64 < M ? jcur + 64 : M;
                j[k] = s_off[w1] > p ? dp1_search(s_off, jcur, w1, p) : dp1_search(s_off, w1, M, p);
                at[k] = s_pos[j[k]] + (p - s_off[j[k]]);
            }
            jcur = __shfl(j[k], 63, 64);   // (a lane past d1 keeps jcur: no step follows it)
        }
#pragma unroll
        for (int k = 0; k < DP1_UNROLL; k++) {
            const uint32_t p = p0 + k * 64 + lane;
            t[k] = v[k] = sub[k] = 0;
            if (p < d1) {
                t[k] = in_t[j[k]];
                v[k] = in_v[j[k]];
                if (at[k] < pool_len) sub[k] = pool[at[k]];   // (always: the list was counted as inside the pool)
            }
        }
#pragma unroll
        for (int k = 0; k < DP1_UNROLL; k++) {
            const uint32_t p = p0 + k * 64 + lane;
            if (p < d1) {
                out_dt[p] = t[k];
                out_dv[p] = v[k];
                out_ds[p] = sub[k];
            }
        }
    }
    if (tid == 0) { st_out[FO1_ST_TOTAL] = total; st_out[FO1_ST_STATE] = FO1_DONE; }
}

}  // namespace

hipError_t launch_dispatch_one(const uint32_t *status_in, const uint32_t *fo_offsets, const uint32_t *fo_topic,
                               const uint32_t *fo_value, const uint32_t *ag_offsets, const uint32_t *ag_topic,
                               const uint32_t *ag_value, uint32_t n_dests, uint32_t bucket, const uint32_t *span,
                               uint64_t span_len, const uint32_t *pool, uint64_t pool_len, uint32_t *out_dest_offsets,
                               uint32_t *out_topic, uint32_t *out_value, uint64_t cap, uint64_t *out_head,
                               uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub, uint64_t dcap,
                               uint64_t dp1_max, uint32_t *status, hipStream_t s) {
    if (!n_dests || n_dests > FO1_MAX_DESTS || bucket > n_dests || ((uintptr_t)span & 7) || ((uintptr_t)out_head & 7))
        return hipErrorInvalidValue;
    if (!span) span_len = 0;
    if (!pool) pool_len = 0;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (dcap > 0xFFFFFFFFull) dcap = 0xFFFFFFFFull;
    hipLaunchKernelGGL(k_dp_one, dim3(1), dim3(FO1_BLOCK), 0, s, status_in, fo_offsets, fo_topic, fo_value, ag_offsets,
                       ag_topic, ag_value, n_dests, bucket, reinterpret_cast<const uint2 *>(span), span_len, pool, pool_len,
                       out_dest_offsets, out_topic, out_value, cap, out_head, out_dtopic, out_dvalue, out_dsub, dcap,
                       dp1_max, status);
    return hipGetLastError();
}

hipError_t launch_dispatch(const FanoutScratch &fs, uint32_t n_dests, const uint64_t *dest_offsets, uint32_t bucket,
                           const uint32_t *in_topic, const uint32_t *in_value, uint64_t cap, const uint32_t *span,
                           uint64_t span_len, const uint32_t *pool, uint64_t pool_len, uint64_t *head,
                           uint64_t *out_offsets, uint32_t *out_topic, uint32_t *out_value, uint32_t *out_sub,
                           uint64_t out_cap, hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS || bucket > n_dests || ((uintptr_t)span & 7)) return hipErrorInvalidValue;
    if (!span) span_len = 0;
    if (!pool) pool_len = 0;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (out_cap > 0xFFFFFFFFull) out_cap = 0xFFFFFFFFull;
    if (!fs.dp_cnt || !fs.dp_tot || cap > fs.dp_cap) return hipErrorInvalidValue;
    if (!out_offsets) {
        if (!fs.dp_off || cap > fs.dp_off_cap) return hipErrorInvalidValue;
        out_offsets = fs.dp_off;
    }
    const uint2 *sp = reinterpret_cast<const uint2 *>(span);
    const dim3 g(FO_GRID), b(64);
    hipLaunchKernelGGL(k_dp_count, g, b, 0, s, dest_offsets, n_dests, bucket, cap, in_value, sp, span_len, pool_len,
                       fs.dp_cnt, fs.dp_tot);
    hipLaunchKernelGGL(k_dp_scan, dim3(1), dim3(256), 0, s, dest_offsets, n_dests, bucket, cap, fs.dp_tot, head);
    hipLaunchKernelGGL(k_dp_offsets, g, b, 0, s, dest_offsets, n_dests, bucket, cap, fs.dp_cnt, fs.dp_tot, out_offsets);
    hipLaunchKernelGGL(k_dp_expand, g, b, 0, s, dest_offsets, n_dests, bucket, cap, in_topic, in_value, sp, span_len, pool,
                       pool_len, out_offsets, fs.dp_tot, out_topic, out_value, out_sub, out_cap);
    return hipGetLastError();
}

}  // namespace tmx
