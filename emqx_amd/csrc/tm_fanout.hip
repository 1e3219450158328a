// tm_fanout.hip -- route fan-out on the device: a batch's topic-major hit lists
// (the CSR tm_match_batch_dev writes) regrouped by the destination of each
// value, for gfx950.
//
// emqx_broker:do_publish/1 is route(aggre(match_routes(Topic)), Delivery)
// (apps/emqx/src/emqx_broker.erl:293-298): every hit is a route {To, Dest} and
// do_route2/2 (:401-406) dispatches it locally, forwards it to
// get_dest_node(Dest) (emqx_router.erl:580-585) or hands it to a shared group.
// A batched broker wants, per destination, the (message, route) pairs that go
// there: one forward per node per micro-batch.  That is a stable partition of
// the flat (topic, value) list by bucket = dest_of[value]; bucket n_dests takes
// every value without a destination (v >= dest_len, dest_of[v] >= n_dests), so
// nothing is dropped.  The result equals numpy.argsort(bucket, kind="stable")
// applied to (topic, value).
//
// The total is known only on the device and the call is asynchronous, so the
// grid is fixed: FO_GRID one-wave blocks, block k owns the positions
// [k * chunk, (k + 1) * chunk) with chunk = ceil(E / FO_GRID) rounded up to 64,
// E = min(hit[n], cap), and goes through them in order.  One LSD pass over a
// digit of `bits` bits is three launches:
//   k_fo_hist     the block's digit histogram (LDS atomics), written bin-major
//                 into tab[bin * FO_GRID + block] -- every block writes every
//                 bin, so nothing of an earlier, larger run survives;
//   k_fo_scan     one block per bin: the exclusive scan of its row in place,
//                 the row's total into tot[bin];
//   k_fo_scatter  base[bin] = (scan of tot)[bin] + tab[bin][block] into LDS,
//                 then 64 entries a step: the lanes with an equal digit find
//                 each other with one ballot per digit bit (peer mask), a
//                 lane's slot is base[digit] + the peers below it, and the
//                 highest peer adds the group's size to base[digit].  Stable
//                 because blocks, steps and lanes are all in position order.
// One pass (digit = the bucket) when n_dests + 1 <= 256 -- clusters have tens
// of nodes --, else two: the low ceil(w / 2) bits of the w-bit bucket ids
// first, into the stream's scratch as (topic, value, bucket) triples, then the
// high bits from there into the outputs.  A first pass finds an entry's topic
// from the offsets: a 64-ary search by the wave at the chunk's start, then per
// step a window of the next 64 offsets in LDS that each lane searches; lanes
// whose topic lies beyond the window (a run of more than 64 empty topics)
// search again from the first of them.
//
// Bucket b's entries end up at [dest_offsets[b], dest_offsets[b + 1]);
// dest_offsets[n_dests + 1] = E.  One pass: the scan of tot is that array.
// Two passes: k_fo_bounds finds each bucket's first position in the output by
// binary search (the output is sorted by bucket).
// Bytes per entry and pass: 4 read twice (histogram, scatter) + 4 gathered
// twice (dest_of) + 8 written -- (topic, value); a first of two passes writes
// 12 and the second reads 4 + 12.
//
// The pairs form (tm_match_batch_dev_pairs' spans; launch_fanout_pairs): two
// launches scan the spans' effective counts into the offsets of the CSR they
// stand for, k_fo_resolve writes that CSR's entries as triples with the first
// digit's histogram, and the scan / scatter kernels above run on the triples
// (SRC 1) -- 8 B read (pair) + 8 written (offset) per topic, and per entry 4
// gathered (value) + 4 (dest_of) + 12 written more than a CSR pass.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tm_dev.h"

namespace tmx {

namespace {

static_assert(FO_GRID % 256 == 0, "k_fo_scan: 256 threads share a row evenly");
constexpr int FO_HIST_UNROLL = 4;   // steps whose loads a histogram block issues together

__device__ __forceinline__ uint32_t fo_bucket(uint32_t v, const uint32_t *dest_of, uint64_t dest_len,
                                              uint32_t n_dests) {
    uint32_t b = n_dests;
    if (v < dest_len) {
        const uint32_t d = dest_of[v];
        if (d < n_dests) b = d;
    }
    return b;
}

// the positions block `blk` owns: [c0, c1) of [0, E)
__device__ __forceinline__ void fo_chunk(const uint64_t *hit, uint64_t n, uint64_t cap, uint32_t blk, uint64_t &c0,
                                         uint64_t &c1, uint64_t &E) {
    const uint64_t total = hit[n];
    E = total < cap ? total : cap;
    const uint64_t chunk = ((E + FO_GRID - 1) / FO_GRID + 63) & ~63ull;
    c0 = (uint64_t)blk * chunk;
    c1 = c0 + chunk < E ? c0 + chunk : E;
    if (c0 > c1) c0 = c1;
}

// (fo_topic_at and fo_step_topics, the search for the topic of a position: tm_dev.h,
// shared with tm_dispatch.hip)

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    return x;
}

// SRC 0: the digit's source is the CSR's values (bucket = dest_of[value]);
// SRC 1: the buckets a first pass stored
template <int SRC>
__global__ __launch_bounds__(64) void k_fo_hist(const uint64_t *hit, uint64_t n, uint64_t cap, const uint32_t *in,
                                                const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests,
                                                uint32_t shift, uint32_t bits, uint32_t *tab) {
    __shared__ uint32_t s_h[FO_BINS];
    const uint32_t lane = threadIdx.x, nb = 1u << bits, mask = nb - 1;
    for (uint32_t i = lane; i < nb; i += 64) s_h[i] = 0;
    __syncthreads();
    uint64_t c0, c1, E;
    fo_chunk(hit, n, cap, blockIdx.x, c0, c1, E);
    for (uint64_t p0 = c0; p0 < c1; p0 += 64 * FO_HIST_UNROLL) {
        uint32_t x[FO_HIST_UNROLL];
#pragma unroll
        for (int k = 0; k < FO_HIST_UNROLL; k++) {
            const uint64_t p = p0 + (uint64_t)k * 64 + lane;
            x[k] = p < c1 ? in[p] : 0u;
        }
#pragma unroll
        for (int k = 0; k < FO_HIST_UNROLL; k++) {
            const uint64_t p = p0 + (uint64_t)k * 64 + lane;
            if (p < c1) {
                const uint32_t b = SRC == 0 ? fo_bucket(x[k], dest_of, dest_len, n_dests) : x[k];
                atomicAdd(&s_h[(b >> shift) & mask], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < nb; i += 64) tab[(uint64_t)i * FO_GRID + blockIdx.x] = s_h[i];
}

// one block per bin: its row of FO_GRID block counts -> exclusive scan in place, the total into tot[bin]
__global__ __launch_bounds__(256) void k_fo_scan(uint32_t *tab, uint32_t *tot) {
    constexpr int PER = FO_GRID / 256;
    __shared__ uint32_t s_w[4];
    uint32_t *row = tab + (uint64_t)blockIdx.x * FO_GRID + threadIdx.x * PER;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { x[k] = row[k]; sum += x[k]; }
    const uint32_t inc = wave_incl_scan(sum, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = inc - sum;
    for (uint32_t q = 0; q < wv; q++) base += s_w[q];
#pragma unroll
    for (int k = 0; k < PER; k++) { row[k] = base; base += x[k]; }
    if (threadIdx.x == 255) tot[blockIdx.x] = base;
}

// SRC 0: entries from the CSR (topic from the offsets, bucket from dest_of);
// SRC 1: the triples a first pass stored.  LAST: (topic, value) into the
// outputs; else the triple into the scratch for the next pass.
template <int SRC, bool LAST>
__global__ __launch_bounds__(64) void k_fo_scatter(const uint64_t *hit, uint64_t n, uint64_t cap, const uint32_t *in_v,
                                                   const uint32_t *in_t, const uint32_t *in_b, const uint32_t *dest_of,
                                                   uint64_t dest_len, uint32_t n_dests, uint32_t shift, uint32_t bits,
                                                   const uint32_t *tab, const uint32_t *tot, uint32_t *out_t,
                                                   uint32_t *out_v, uint32_t *out_b, uint64_t *dest_offsets) {
    __shared__ uint32_t s_base[FO_BINS];
    __shared__ uint64_t s_win[64];
    const uint32_t lane = threadIdx.x, nb = 1u << bits, mask = nb - 1;
    // every block scans the bins' totals itself (at most 8 rounds of one wave)
    const bool offs_out = dest_offsets && blockIdx.x == 0;   // (one pass: the buckets are the bins)
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < nb; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t x = i < nb ? tot[i] : 0u;
        const uint32_t inc = wave_incl_scan(x, lane);
        const uint32_t exc = carry + inc - x;
        if (i < nb) {
            s_base[i] = exc + tab[(uint64_t)i * FO_GRID + blockIdx.x];
            if (offs_out && i <= n_dests + 1) dest_offsets[i] = exc;
        }
        carry += __shfl(inc, 63, 64);
    }
    if (offs_out && n_dests + 1 == nb && lane == 0) dest_offsets[nb] = carry;
    __syncthreads();
    uint64_t c0, c1, E;
    fo_chunk(hit, n, cap, blockIdx.x, c0, c1, E);
    uint64_t tcur = 0;   // hit[tcur] <= the step's first position
    if (SRC == 0 && c0 < c1) tcur = fo_topic_at(hit, n, c0, 0, lane);
    for (uint64_t p0 = c0; p0 < c1; p0 += 64) {
        const uint64_t p = p0 + lane;
        const bool ok = p < c1;
        uint32_t v = 0, b = 0, t = 0;
        if (SRC == 0) {
            if (ok) {
                v = in_v[p];
                b = fo_bucket(v, dest_of, dest_len, n_dests);
            }
            t = fo_step_topics(hit, n, p0, c1, ok, tcur, s_win, lane);
        } else if (ok) {
            v = in_v[p];
            t = in_t[p];
            b = in_b[p];
        }
        const uint32_t d = (b >> shift) & mask;
        // the lanes of this step with my digit
        uint64_t peers = __ballot(ok);
        for (uint32_t k = 0; k < bits; k++) {
            const bool bit = (d >> k) & 1u;
            const uint64_t m = __ballot(ok && bit);
            peers &= bit ? m : ~m;
        }
        uint32_t dst = 0;
        if (ok) dst = s_base[d] + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        __syncthreads();
        if (ok && (peers >> lane) == 1ull) s_base[d] += (uint32_t)__popcll(peers);
        __syncthreads();
        // (dst < E whenever the histogram saw what this kernel sees; the test
        // keeps a caller who rewrites an input in between inside the outputs)
        if (ok && dst < E) {
            out_t[dst] = t;
            out_v[dst] = v;
            if (!LAST) out_b[dst] = b;
        }
    }
}

// two passes: dest_offsets[b] = the first output position whose bucket is >= b
__global__ __launch_bounds__(256) void k_fo_bounds(const uint64_t *hit, uint64_t n, uint64_t cap, const uint32_t *out_v,
                                                   const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests,
                                                   uint64_t *dest_offsets) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_dests + 1) return;
    const uint64_t total = hit[n], E = total < cap ? total : cap;
    uint64_t lo = 0, hi = E;
    if (b > n_dests) lo = E;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (fo_bucket(out_v[mid], dest_of, dest_len, n_dests) < b) lo = mid + 1;
        else hi = mid;
    }
    dest_offsets[b] = lo;
}

// ---- the pairs form (tm_fanout_dev_pairs): per-topic (first position, count)
// spans of `values`, disjoint but in any order, with gaps, and cut by cap.
// Topic t contributes eff_t = min(cnt_t, cap - pos_t) entries (0 for pos_t >=
// cap); voff = the exclusive scan of eff (64-bit sums) is the CSR the spans
// stand for, and entry p of it is values[pos_t + (p - voff[t])] for the last
// t with voff[t] <= p.  k_fo_resolve turns the entries below E = min(voff[n],
// cap) into (topic, value, bucket) triples in position order, with the first
// digit's histogram, and the SRC 1 kernels above take it from there.

__device__ __forceinline__ uint32_t fp_eff(uint2 pr, uint64_t cap) {   // (cap <= 2^32 - 1)
    if (pr.x >= cap) return 0u;
    const uint64_t room = cap - pr.x;
    return pr.y < room ? pr.y : (uint32_t)room;
}

__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    return x;
}

// the block's four waves' inclusive totals in s_w -> their sum (256 threads)
__device__ __forceinline__ uint64_t fp_block_total(const uint64_t *s_w) { return s_w[0] + s_w[1] + s_w[2] + s_w[3]; }

// The scan is tile sums, then every block scans the sums below its own tile
// itself and adds them back: no block waits for another.  Block k owns the
// topics [k * tile, (k + 1) * tile); at most FP_TILES blocks.
__global__ __launch_bounds__(256) void k_fp_sums(const uint2 *pairs, uint64_t n, uint64_t cap, uint64_t tile,
                                                 uint64_t *sums) {
    __shared__ uint64_t s_w[4];
    const uint64_t t0 = (uint64_t)blockIdx.x * tile, t1 = t0 + tile < n ? t0 + tile : n;
    uint64_t sum = 0;
    for (uint64_t t = t0 + threadIdx.x; t < t1; t += 256) sum += fp_eff(pairs[t], cap);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t inc = wave_incl_scan64(sum, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = fp_block_total(s_w);
}

__global__ __launch_bounds__(256) void k_fp_offsets(const uint2 *pairs, uint64_t n, uint64_t cap, uint64_t tile,
                                                    const uint64_t *sums, uint64_t *voff) {
    __shared__ uint64_t s_w[4];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t x = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 256) x += sums[k];
    uint64_t inc = wave_incl_scan64(x, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint64_t base = fp_block_total(s_w);   // the entries of the topics below t0
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * tile, t1 = t0 + tile < n ? t0 + tile : n;
    for (uint64_t r = t0; r < t1; r += 256) {
        const uint64_t t = r + threadIdx.x;
        const uint64_t e = t < t1 ? fp_eff(pairs[t], cap) : 0u;
        inc = wave_incl_scan64(e, lane);
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        uint64_t exc = base + inc - e;
        for (uint32_t q = 0; q < wv; q++) exc += s_w[q];
        if (t < t1) voff[t] = exc;
        base += fp_block_total(s_w);
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) voff[n] = base;   // (the last tile is never empty, or n == 0)
}

// Block k's chunk of [0, E), as in the passes above: each entry's topic from
// voff (the search of a first CSR pass), its value through the topic's pair,
// the triple to position p of out_t / out_v / out_b, and the block's histogram
// of the digit's low `bits` bits into tab -- k_fo_hist<1> on out_b would
// count the same.
__global__ __launch_bounds__(64) void k_fo_resolve(const uint64_t *voff, uint64_t n, uint64_t cap, const uint2 *pairs,
                                                   const uint32_t *values, const uint32_t *dest_of, uint64_t dest_len,
                                                   uint32_t n_dests, uint32_t bits, uint32_t *tab, uint32_t *out_t,
                                                   uint32_t *out_v, uint32_t *out_b) {
    __shared__ uint32_t s_h[FO_BINS];
    __shared__ uint64_t s_win[64];
    const uint32_t lane = threadIdx.x, nb = 1u << bits, mask = nb - 1;
    for (uint32_t i = lane; i < nb; i += 64) s_h[i] = 0;
    __syncthreads();
    uint64_t c0, c1, E;
    fo_chunk(voff, n, cap, blockIdx.x, c0, c1, E);
    uint64_t tcur = 0;
    if (c0 < c1) tcur = fo_topic_at(voff, n, c0, 0, lane);
    for (uint64_t p0 = c0; p0 < c1; p0 += 64) {
        const uint64_t p = p0 + lane;
        const bool ok = p < c1;
        const uint32_t t = fo_step_topics(voff, n, p0, c1, ok, tcur, s_win, lane);
        if (ok) {
            uint32_t v = 0;
            if (t < n) {   // (always: p < voff[n])
                const uint64_t at = (uint64_t)pairs[t].x + (p - voff[t]);
                if (at < cap) v = values[at];   // (always: p - voff[t] < eff_t <= cap - pos_t)
            }
            const uint32_t b = fo_bucket(v, dest_of, dest_len, n_dests);
            out_t[p] = t;
            out_v[p] = v;
            out_b[p] = b;
            atomicAdd(&s_h[b & mask], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < nb; i += 64) tab[(uint64_t)i * FO_GRID + blockIdx.x] = s_h[i];
}

// ---- a micro-batch in one launch (tm_route_batch32): ONE workgroup of
// FO1_BLOCK threads does the whole pairs-form fan-out of up to FO1_TOPICS
// topics and FO1_ENTRIES entries, so no block waits for another and nothing
// passes through global scratch:
//   1. the scan of eff_t (FO1_TPT topics a thread) into s_voff, each non-empty
//      topic's head (its index) marked at its first position; a batch whose
//      spans hold more than FO1_ENTRIES entries ends here with FO1_TOO_LARGE;
//   2. wave w owns the positions [w * C, (w + 1) * C) of [0, E), C = ceil(E /
//      16) rounded up to 64: per entry the topic (the last head at or before
//      it: a wave max-scan), the value through the topic's pair and the
//      bucket, kept in registers (FO1_STEPS entries a lane) and counted into
//      the wave's own 256-bin row (fo1_partition: steps 2 to 4);
//   3. per bin the exclusive scan over the waves, then over the bins: the
//      bucket offsets (written out) and every wave's running bases;
//   4. k_fo_scatter's peer-mask step per wave into the LDS image of the two
//      output arrays -- stable because waves, steps and lanes are in position
//      order; only waves synchronise, each on its own row;
//   5. the image's first min(E, cap) entries to the outputs, coalesced: mapped
//      host memory takes whole lines instead of 4-byte scattered stores.
constexpr uint32_t FO1_WAVES = FO1_BLOCK / 64;
constexpr uint32_t FO1_STEPS = FO1_ENTRIES / FO1_BLOCK;   // 64-entry steps of a wave, at most
constexpr uint32_t FO1_TPT = FO1_TOPICS / FO1_BLOCK;      // topics per thread of the scan
constexpr uint32_t FO1_BINS = FO1_MAX_DESTS + 1;
static_assert(FO1_ENTRIES % FO1_BLOCK == 0 && FO1_TOPICS % FO1_BLOCK == 0, "k_fo_one: whole steps");
static_assert(FO1_TOPICS <= 65536, "k_fo_one: topics are staged as 16 bits");
static_assert(FO1_BINS == 256 && FO1_BINS <= FO1_BLOCK, "k_fo_one: one thread per bin, four waves of them");

__device__ __forceinline__ void fo_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Steps 2 to 4 of k_fo_one for waves of at most S 64-entry steps.  Each
// sub-step runs over all S steps before the next begins, so a lane's S loads
// of each level (pair, value, destination) are in flight together: three
// memory latencies a wave, not three a step.
template <uint32_t S>
__device__ __forceinline__ void fo1_partition(const uint2 *pairs, uint32_t n, const uint32_t *values, uint64_t vcap,
                                              const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests,
                                              uint32_t bits, uint32_t *dest_offsets, uint32_t E, uint32_t C,
                                              const uint32_t *s_voff, uint32_t *s_h, uint32_t *s_bw, uint32_t *s_ov,
                                              uint16_t *s_ot) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t c0 = wv * C < E ? wv * C : E, c1 = c0 + C < E ? c0 + C : E;
    uint32_t *my_h = s_h + wv * FO1_BINS;
    // 2. the wave's entries into registers, counted per bucket
    uint32_t rt[S], rv[S], rb[S];   // topic, then its span's first position / the value, bucket
    // The topic of the chunk's first position: the last t of [0, n) with
    // s_voff[t] <= c0 (s_voff[0] = 0), 13 branch-free probes, the same in every
    // lane.  From there the heads in s_ot (the topic at the first position of
    // every non-empty topic, zero elsewhere) carry it forward: a position's
    // topic is the last head at or before it, a running maximum since the heads
    // ascend -- one wave scan a step instead of a search per entry.
    uint32_t carry = 0;
    for (uint32_t st = FO1_TOPICS / 2; st; st >>= 1) {
        const uint32_t m = carry + st;
        if (m < n && s_voff[m] <= c0) carry = m;
    }
#pragma unroll
    for (uint32_t k = 0; k < S; k++) {
        const uint32_t p = c0 + k * 64 + lane;
        uint32_t x = p < c1 ? s_ot[p] : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= (uint32_t)d && y > x) x = y;
        }
        if (carry > x) x = carry;
        carry = __shfl(x, 63, 64);
        rt[k] = x;
    }
#pragma unroll
    for (uint32_t k = 0; k < S; k++) {
        const bool ok = c0 + k * 64 + lane < c1;
        rv[k] = ok ? pairs[rt[k]].x : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < S; k++) {
        const uint32_t p = c0 + k * 64 + lane;
        const uint64_t at = (uint64_t)rv[k] + (p - s_voff[rt[k]]);
        rv[k] = p < c1 && at < vcap ? values[at] : 0u;   // (at < vcap always: p - voff[t] < eff_t <= vcap - pos_t)
    }
#pragma unroll
    for (uint32_t k = 0; k < S; k++) {
        const bool ok = c0 + k * 64 + lane < c1;
        rb[k] = ok ? fo_bucket(rv[k], dest_of, dest_len, n_dests) : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < S; k++)
        if (c0 + k * 64 + lane < c1) atomicAdd(&my_h[rb[k]], 1u);
    __syncthreads();
    // 3. bin b: its counts' exclusive scan over the waves, then over the bins
    uint32_t tot = 0;
    if (tid < FO1_BINS)
        for (uint32_t q = 0; q < FO1_WAVES; q++) {
            const uint32_t x = s_h[q * FO1_BINS + tid];
            s_h[q * FO1_BINS + tid] = tot;
            tot += x;
        }
    const uint32_t binc = wave_incl_scan(tot, lane);
    if (tid < FO1_BINS && lane == 63) s_bw[wv] = binc;
    __syncthreads();
    if (tid < FO1_BINS) {
        uint32_t exc = binc - tot;
        for (uint32_t q = 0; q < wv; q++) exc += s_bw[q];
        for (uint32_t q = 0; q < FO1_WAVES; q++) s_h[q * FO1_BINS + tid] += exc;
        if (tid <= n_dests) dest_offsets[tid] = exc;
    }
    if (tid == 0) dest_offsets[n_dests + 1] = E;
    __syncthreads();
    // 4. the stable scatter, into the outputs' image
#pragma unroll
    for (uint32_t k = 0; k < S; k++) {
        if (k * 64 >= C) break;   // (block-uniform)
        const bool ok = c0 + k * 64 + lane < c1;
        const uint32_t d = rb[k];
        uint64_t peers = __ballot(ok);
        for (uint32_t q = 0; q < bits; q++) {
            const bool bit = (d >> q) & 1u;
            const uint64_t m = __ballot(ok && bit);
            peers &= bit ? m : ~m;
        }
        uint32_t dst = 0;
        if (ok) dst = my_h[d] + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        fo_wave_sync();
        if (ok && (peers >> lane) == 1ull) my_h[d] += (uint32_t)__popcll(peers);
        fo_wave_sync();
        if (ok && dst < E) {   // (always, as in k_fo_scatter)
            s_ov[dst] = rv[k];
            s_ot[dst] = (uint16_t)rt[k];
        }
    }
}

__global__ __launch_bounds__(FO1_BLOCK) void k_fo_one(const uint2 *pairs, uint64_t n, const uint32_t *values,
                                                      uint64_t vcap, const uint32_t *dest_of, uint64_t dest_len,
                                                      uint32_t n_dests, uint32_t bits, uint32_t *dest_offsets,
                                                      uint32_t *out_t, uint32_t *out_v, uint64_t cap,
                                                      uint32_t *status) {
    __shared__ uint32_t s_voff[FO1_TOPICS + 1];
    __shared__ uint32_t s_h[FO1_WAVES * FO1_BINS];
    __shared__ uint32_t s_ov[FO1_ENTRIES];
    __shared__ __attribute__((aligned(4))) uint16_t s_ot[FO1_ENTRIES];   // the topics' heads, then the image
    __shared__ uint64_t s_w[FO1_WAVES];
    __shared__ uint32_t s_bw[FO1_BINS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t total = n ? reinterpret_cast<const uint32_t *>(pairs)[2 * n] : 0u;
    if (n > FO1_TOPICS || n_dests > FO1_MAX_DESTS) {
        if (tid == 0) { status[FO1_ST_TOTAL] = total; status[FO1_ST_STATE] = FO1_TOO_LARGE; }
        return;
    }
    // 1. the virtual CSR's offsets
    uint32_t e[FO1_TPT];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < FO1_TPT; k++) {
        const uint32_t t = tid * FO1_TPT + k;
        e[k] = t < n ? fp_eff(pairs[t], vcap) : 0u;
        sum += e[k];
    }
    const uint64_t inc = wave_incl_scan64(sum, lane);
    if (lane == 63) s_w[wv] = inc;
    for (uint32_t i = tid; i < FO1_WAVES * FO1_BINS; i += FO1_BLOCK) s_h[i] = 0;
    for (uint32_t i = tid; i < FO1_ENTRIES / 2; i += FO1_BLOCK) reinterpret_cast<uint32_t *>(s_ot)[i] = 0;
    __syncthreads();
    uint64_t base = inc - sum, Ev = 0;
    for (uint32_t q = 0; q < FO1_WAVES; q++) {
        if (q < wv) base += s_w[q];
        Ev += s_w[q];
    }
    if (Ev > FO1_ENTRIES) {   // (block-uniform)
        if (tid == 0) { status[FO1_ST_TOTAL] = total; status[FO1_ST_STATE] = FO1_TOO_LARGE; }
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < FO1_TPT; k++) {   // (every offset <= Ev <= FO1_ENTRIES from here)
        const uint32_t t = tid * FO1_TPT + k;
        if (t < n) s_voff[t] = (uint32_t)base;
        if (e[k]) s_ot[base] = (uint16_t)t;   // the topic's head (base + e[k] <= Ev: inside the image)
        base += e[k];
    }
    if (tid == 0) s_voff[n] = (uint32_t)Ev;
    const uint32_t E = Ev < vcap ? (uint32_t)Ev : (uint32_t)vcap;
    __syncthreads();
    // 2.-4. with the wave's steps as a compile-time bound: a micro-batch of a
    // few hundred entries pays for one step, not FO1_STEPS
    const uint32_t C = ((E + FO1_WAVES - 1) / FO1_WAVES + 63) & ~63u;   // (<= 64 * FO1_STEPS)
#define FO1_PARTITION(S)                                                                                         \
    fo1_partition<S>(pairs, (uint32_t)n, values, vcap, dest_of, dest_len, n_dests, bits, dest_offsets, E, C, s_voff, \
                     s_h, s_bw, s_ov, s_ot)
    if (C <= 64) FO1_PARTITION(1);
    else if (C <= 256) FO1_PARTITION(4);
    else FO1_PARTITION(FO1_STEPS);
#undef FO1_PARTITION
    __syncthreads();
    // 5. what the caller has room for
    const uint32_t keep = E < cap ? E : (uint32_t)cap;
    for (uint32_t i = tid; i < keep; i += FO1_BLOCK) {
        out_v[i] = s_ov[i];
        out_t[i] = s_ot[i];
    }
    if (tid == 0) { status[FO1_ST_TOTAL] = total; status[FO1_ST_STATE] = FO1_DONE; }
}

}  // namespace

hipError_t launch_fanout_one(uint64_t n, const uint32_t *pairs, const uint32_t *values, uint64_t vcap,
                             const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests, uint32_t *dest_offsets,
                             uint32_t *out_topic, uint32_t *out_value, uint64_t cap, uint32_t *status, hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS || n >= 0xFFFFFFFFull || ((uintptr_t)pairs & 7)) return hipErrorInvalidValue;
    if (!dest_of) dest_len = 0;
    if (vcap > 0xFFFFFFFFull) vcap = 0xFFFFFFFFull;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    uint32_t w = 1;   // bits of the largest bucket id, n_dests
    while ((n_dests >> w) != 0) w++;
    hipLaunchKernelGGL(k_fo_one, dim3(1), dim3(FO1_BLOCK), 0, s, reinterpret_cast<const uint2 *>(pairs), n, values, vcap,
                       dest_of, dest_len, n_dests, w, dest_offsets, out_topic, out_value, cap, status);
    return hipGetLastError();
}

bool fanout_two_pass(uint32_t n_dests) { return n_dests + 1 > 256; }

hipError_t launch_fanout(const FanoutScratch &fs, uint64_t n, const uint64_t *hit, const uint32_t *values,
                         uint64_t cap, const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests,
                         uint64_t *dest_offsets, uint32_t *out_topic, uint32_t *out_value, hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS) return hipErrorInvalidValue;
    if (!dest_of) dest_len = 0;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    uint32_t w = 1;   // bits of the largest bucket id, n_dests
    while ((n_dests >> w) != 0) w++;
    const dim3 g(FO_GRID), b(64);
    if (!fanout_two_pass(n_dests)) {
        hipLaunchKernelGGL(k_fo_hist<0>, g, b, 0, s, hit, n, cap, values, dest_of, dest_len, n_dests, 0u, w, fs.tab);
        hipLaunchKernelGGL(k_fo_scan, dim3(1u << w), dim3(256), 0, s, fs.tab, fs.tot);
        hipLaunchKernelGGL((k_fo_scatter<0, true>), g, b, 0, s, hit, n, cap, values, (const uint32_t *)nullptr,
                           (const uint32_t *)nullptr, dest_of, dest_len, n_dests, 0u, w, fs.tab, fs.tot, out_topic,
                           out_value, (uint32_t *)nullptr, dest_offsets);
        return hipGetLastError();
    }
    if (cap > fs.cap) return hipErrorInvalidValue;   // (the triples of the first pass)
    const uint32_t lo = (w + 1) / 2, hi = w - lo;
    hipLaunchKernelGGL(k_fo_hist<0>, g, b, 0, s, hit, n, cap, values, dest_of, dest_len, n_dests, 0u, lo, fs.tab);
    hipLaunchKernelGGL(k_fo_scan, dim3(1u << lo), dim3(256), 0, s, fs.tab, fs.tot);
    hipLaunchKernelGGL((k_fo_scatter<0, false>), g, b, 0, s, hit, n, cap, values, (const uint32_t *)nullptr,
                       (const uint32_t *)nullptr, dest_of, dest_len, n_dests, 0u, lo, fs.tab, fs.tot, fs.t, fs.v, fs.b,
                       (uint64_t *)nullptr);
    hipLaunchKernelGGL(k_fo_hist<1>, g, b, 0, s, hit, n, cap, fs.b, dest_of, dest_len, n_dests, lo, hi, fs.tab);
    hipLaunchKernelGGL(k_fo_scan, dim3(1u << hi), dim3(256), 0, s, fs.tab, fs.tot);
    hipLaunchKernelGGL((k_fo_scatter<1, true>), g, b, 0, s, hit, n, cap, fs.v, fs.t, fs.b, dest_of, dest_len, n_dests, lo,
                       hi, fs.tab, fs.tot, out_topic, out_value, (uint32_t *)nullptr, (uint64_t *)nullptr);
    hipLaunchKernelGGL(k_fo_bounds, dim3((n_dests + 2 + 255) / 256), dim3(256), 0, s, hit, n, cap, out_value, dest_of,
                       dest_len, n_dests, dest_offsets);
    return hipGetLastError();
}

hipError_t launch_fanout_pairs(const FanoutScratch &fs, uint64_t n, const uint32_t *pairs, const uint32_t *values,
                               uint64_t cap, const uint32_t *dest_of, uint64_t dest_len, uint32_t n_dests,
                               uint64_t *dest_offsets, uint32_t *out_topic, uint32_t *out_value, hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS) return hipErrorInvalidValue;
    if (!dest_of) dest_len = 0;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    const bool two = fanout_two_pass(n_dests);
    if (cap > fs.cap || n + 1 > fs.voff_cap || (two && !fs.b2)) return hipErrorInvalidValue;
    uint32_t w = 1;
    while ((n_dests >> w) != 0) w++;
    // the topics' tiles: at most FP_TILES of them, a multiple of the block each
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>((n + FP_TILES - 1) / FP_TILES, 1), FP_TILES);
    const uint64_t tile = std::max<uint64_t>(((n + want - 1) / want + 255) / 256 * 256, 256);
    const uint32_t tiles = (uint32_t)std::max<uint64_t>((n + tile - 1) / tile, 1);
    const uint2 *pr = reinterpret_cast<const uint2 *>(pairs);
    hipLaunchKernelGGL(k_fp_sums, dim3(tiles), dim3(256), 0, s, pr, n, cap, tile, fs.sums);
    hipLaunchKernelGGL(k_fp_offsets, dim3(tiles), dim3(256), 0, s, pr, n, cap, tile, fs.sums, fs.voff);
    const uint64_t *hit = fs.voff;
    const dim3 g(FO_GRID), b(64);
    if (!two) {
        hipLaunchKernelGGL(k_fo_resolve, g, b, 0, s, hit, n, cap, pr, values, dest_of, dest_len, n_dests, w, fs.tab, fs.t,
                           fs.v, fs.b);
        hipLaunchKernelGGL(k_fo_scan, dim3(1u << w), dim3(256), 0, s, fs.tab, fs.tot);
        hipLaunchKernelGGL((k_fo_scatter<1, true>), g, b, 0, s, hit, n, cap, fs.v, fs.t, fs.b, dest_of, dest_len, n_dests,
                           0u, w, fs.tab, fs.tot, out_topic, out_value, (uint32_t *)nullptr, dest_offsets);
        return hipGetLastError();
    }
    // two passes: the resolved entries wait in the outputs (positions below E
    // only) and fs.b2, the first pass moves them into the triples
    const uint32_t lo = (w + 1) / 2, hi = w - lo;
    hipLaunchKernelGGL(k_fo_resolve, g, b, 0, s, hit, n, cap, pr, values, dest_of, dest_len, n_dests, lo, fs.tab,
                       out_topic, out_value, fs.b2);
    hipLaunchKernelGGL(k_fo_scan, dim3(1u << lo), dim3(256), 0, s, fs.tab, fs.tot);
    hipLaunchKernelGGL((k_fo_scatter<1, false>), g, b, 0, s, hit, n, cap, out_value, out_topic, fs.b2, dest_of, dest_len,
                       n_dests, 0u, lo, fs.tab, fs.tot, fs.t, fs.v, fs.b, (uint64_t *)nullptr);
    hipLaunchKernelGGL(k_fo_hist<1>, g, b, 0, s, hit, n, cap, fs.b, dest_of, dest_len, n_dests, lo, hi, fs.tab);
    hipLaunchKernelGGL(k_fo_scan, dim3(1u << hi), dim3(256), 0, s, fs.tab, fs.tot);
    hipLaunchKernelGGL((k_fo_scatter<1, true>), g, b, 0, s, hit, n, cap, fs.v, fs.t, fs.b, dest_of, dest_len, n_dests, lo,
                       hi, fs.tab, fs.tot, out_topic, out_value, (uint32_t *)nullptr, (uint64_t *)nullptr);
    hipLaunchKernelGGL(k_fo_bounds, dim3((n_dests + 2 + 255) / 256), dim3(256), 0, s, hit, n, cap, out_value, dest_of,
                       dest_len, n_dests, dest_offsets);
    return hipGetLastError();
}

}  // namespace tmx
