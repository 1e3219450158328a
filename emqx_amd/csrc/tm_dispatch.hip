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

}  // namespace

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
