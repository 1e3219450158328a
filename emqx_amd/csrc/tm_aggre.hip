// tm_aggre.hip -- emqx_broker:aggre/1 on the fan-out's output, for gfx950.
//
// do_publish/1 is route(aggre(match_routes(Topic)), Delivery)
// (apps/emqx/src/emqx_broker.erl:293-298).  aggre/1 (:408-424) reduces
// {To, {Group, Node}} to {To, Group} and lists:usort's the list: a shared group
// with members on k nodes -- k routes of one filter -- gets a message once.
// The fan-out (tm_fanout.hip) is a stable partition of a batch whose topics
// list their keys in ascending term order, the keys of one filter contiguous;
// so inside one destination bucket the entries of one topic that share a
// filter are adjacent, and the usort is "drop an entry whose predecessor in
// the same bucket has the same topic and the same filter":
//   entry q < E = min(dest_offsets[n_dests + 1], cap) is dropped iff it is not
//   a bucket's first position, lies below the unrouted bucket n_dests,
//   topic[q] == topic[q - 1] and f(value[q]) == f(value[q - 1]) != NONE, with
//   f(v) = filter_of[v] for v < filter_len, else NONE.
// A segmented stable compaction over the fan-out's fixed grid: FO_GRID one-wave
// blocks, block k owns [k * chunk, (k + 1) * chunk) of [0, E), chunk = ceil(E /
// FO_GRID) rounded up to 64.  Five launches, no block waits for another:
//   k_ag_flag     topic and value loaded coalesced, filter_of gathered, the
//                 predecessor by a __shfl_up (lane 0: the step before, or one
//                 load at the chunk's start); the step's __ballot is word
//                 p / 64 of the bitmap, the block's kept count goes to cnt;
//   k_ag_heads    one thread per bucket: its first position is kept whatever
//                 the flags say (atomicOr; whoever sets the bit counts it);
//   k_ag_scan     the exclusive scan of the FO_GRID counts, the total K last;
//   k_ag_move     slot = the block's base + the kept lanes below; every step's
//                 base is left in pre[p / 64];
//   k_ag_offsets  out_dest_offsets[b] = pre + popcount at min(dest_offsets[b], E).
// Bytes per entry: 8 read + 4 gathered (flag), 8 read + 8 written for a kept
// entry (move), 12 per 64 entries of bitmap and bases.
//
// k_ag_one: the same rule for a micro-batch (tm_route_batch32_ex), ONE
// workgroup from the one-launch fan-out's results in HBM into the caller's
// buffers.
#include <hip/hip_runtime.h>

#include "tm_dev.h"

namespace tmx {

namespace {

constexpr int AG_UNROLL = 4;   // steps whose loads a block issues together
constexpr uint32_t AG_NONE = 0xFFFFFFFFu;
static_assert(FO_GRID % 256 == 0, "k_ag_scan: 256 threads share the counts evenly");

__device__ __forceinline__ uint32_t ag_filter(uint32_t v, const uint32_t *filter_of, uint64_t filter_len) {
    return v < filter_len ? filter_of[v] : AG_NONE;
}

__device__ __forceinline__ uint64_t ag_total(const uint64_t *doff, uint32_t n_dests, uint64_t cap) {
    const uint64_t total = doff[n_dests + 1];
    return total < cap ? total : cap;
}

__device__ __forceinline__ uint64_t ag_chunk_size(uint64_t E) { return ((E + FO_GRID - 1) / FO_GRID + 63) & ~63ull; }

// the positions block `blk` owns: [c0, c1) of [0, E)
__device__ __forceinline__ void ag_chunk(uint64_t E, uint32_t blk, uint64_t &c0, uint64_t &c1) {
    const uint64_t chunk = ag_chunk_size(E);
    c0 = (uint64_t)blk * chunk;
    c1 = c0 + chunk < E ? c0 + chunk : E;
    if (c0 > c1) c0 = c1;
}

__global__ __launch_bounds__(64) void k_ag_flag(const uint64_t *doff, uint32_t n_dests, uint64_t cap,
                                                const uint32_t *in_t, const uint32_t *in_v, const uint32_t *filter_of,
                                                uint64_t filter_len, uint64_t *bits, uint32_t *cnt) {
    const uint32_t lane = threadIdx.x;
    const uint64_t E = ag_total(doff, n_dests, cap);
    uint64_t c0, c1;
    ag_chunk(E, blockIdx.x, c0, c1);
    const uint64_t u0 = doff[n_dests], U = u0 < E ? u0 : E;   // the unrouted bucket: copied whole
    // the predecessor of the step's first entry (the same in every lane)
    uint32_t pt = 0, pf = AG_NONE;
    if (c0 < c1 && c0 > 0) {
        pt = in_t[c0 - 1];
        pf = ag_filter(in_v[c0 - 1], filter_of, filter_len);
    }
    uint32_t kept = 0;
    for (uint64_t p0 = c0; p0 < c1; p0 += 64 * AG_UNROLL) {
        uint32_t t[AG_UNROLL], f[AG_UNROLL];
#pragma unroll
        for (int k = 0; k < AG_UNROLL; k++) {
            const uint64_t p = p0 + (uint64_t)k * 64 + lane;
            f[k] = p < c1 ? in_v[p] : 0u;
            t[k] = p < c1 ? in_t[p] : 0u;
        }
#pragma unroll
        for (int k = 0; k < AG_UNROLL; k++) {
            const uint64_t p = p0 + (uint64_t)k * 64 + lane;
            f[k] = p < c1 ? ag_filter(f[k], filter_of, filter_len) : AG_NONE;
        }
#pragma unroll
        for (int k = 0; k < AG_UNROLL; k++) {
            const uint64_t q0 = p0 + (uint64_t)k * 64, p = q0 + lane;
            if (q0 >= c1) break;   // (block-uniform)
            uint32_t t1 = __shfl_up(t[k], 1, 64), f1 = __shfl_up(f[k], 1, 64);
            if (lane == 0) { t1 = pt; f1 = pf; }
            const bool same = t[k] == t1 && f[k] == f1 && f[k] != AG_NONE;
            const uint64_t m = __ballot(p < c1 && (!same || p >= U));
            if (lane == 0) bits[q0 >> 6] = m;
            kept += (uint32_t)__popcll(m);
            pt = __shfl(t[k], 63, 64);
            pf = __shfl(f[k], 63, 64);
        }
    }
    if (lane == 0) cnt[blockIdx.x] = kept;   // (every block, every run: nothing of an earlier run survives)
}

__global__ __launch_bounds__(256) void k_ag_heads(const uint64_t *doff, uint32_t n_dests, uint64_t cap, uint64_t *bits,
                                                  uint32_t *cnt) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_dests) return;
    const uint64_t E = ag_total(doff, n_dests, cap), x = doff[b];
    if (x >= E) return;
    const unsigned long long bit = 1ull << (x & 63);
    const unsigned long long old = atomicOr(reinterpret_cast<unsigned long long *>(bits) + (x >> 6), bit);
    if (!(old & bit)) atomicAdd(&cnt[x / ag_chunk_size(E)], 1u);
}

// the FO_GRID block counts -> their exclusive scan in place, the total into cnt[FO_GRID]
__global__ __launch_bounds__(256) void k_ag_scan(uint32_t *cnt) {
    constexpr int PER = FO_GRID / 256;
    __shared__ uint32_t s_w[4];
    uint32_t *row = cnt + threadIdx.x * PER;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { x[k] = row[k]; sum += x[k]; }
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += y;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = inc - sum;
    for (uint32_t q = 0; q < wv; q++) base += s_w[q];
#pragma unroll
    for (int k = 0; k < PER; k++) { row[k] = base; base += x[k]; }
    if (threadIdx.x == 255) cnt[FO_GRID] = base;
}

__global__ __launch_bounds__(64) void k_ag_move(const uint64_t *doff, uint32_t n_dests, uint64_t cap,
                                                const uint32_t *in_t, const uint32_t *in_v, const uint64_t *bits,
                                                const uint32_t *cnt, uint32_t *pre, uint32_t *out_t, uint32_t *out_v) {
    const uint32_t lane = threadIdx.x;
    const uint64_t E = ag_total(doff, n_dests, cap);
    uint64_t c0, c1;
    ag_chunk(E, blockIdx.x, c0, c1);
    uint32_t base = cnt[blockIdx.x];
    for (uint64_t p0 = c0; p0 < c1; p0 += 64 * AG_UNROLL) {
        uint32_t t[AG_UNROLL], v[AG_UNROLL];
        uint64_t m[AG_UNROLL];
#pragma unroll
        for (int k = 0; k < AG_UNROLL; k++) {
            const uint64_t q0 = p0 + (uint64_t)k * 64, p = q0 + lane;
            m[k] = q0 < c1 ? bits[q0 >> 6] : 0ull;
            t[k] = p < c1 ? in_t[p] : 0u;
            v[k] = p < c1 ? in_v[p] : 0u;
        }
#pragma unroll
        for (int k = 0; k < AG_UNROLL; k++) {
            const uint64_t q0 = p0 + (uint64_t)k * 64;
            if (q0 >= c1) break;   // (block-uniform)
            if (lane == 0) pre[q0 >> 6] = base;
            const uint32_t slot = base + (uint32_t)__popcll(m[k] & ((1ull << lane) - 1ull));
            // (slot < K <= E always: the scan counted exactly these bits)
            if (((m[k] >> lane) & 1ull) && slot < E) {
                out_t[slot] = t[k];
                out_v[slot] = v[k];
            }
            base += (uint32_t)__popcll(m[k]);
        }
    }
}

// out_doff[b] = the entries kept before min(doff[b], E); [n_dests + 1] = K
__global__ __launch_bounds__(256) void k_ag_offsets(const uint64_t *doff, uint32_t n_dests, uint64_t cap,
                                                    const uint64_t *bits, const uint32_t *cnt, const uint32_t *pre,
                                                    uint64_t *out_doff) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_dests + 1) return;
    const uint64_t E = ag_total(doff, n_dests, cap), x = doff[b];
    uint64_t r = cnt[FO_GRID];
    if (x < E) r = pre[x >> 6] + (uint32_t)__popcll(bits[x >> 6] & ((1ull << (x & 63)) - 1ull));
    out_doff[b] = r;
}

// ---- a micro-batch (tm_route_batch32_ex): ONE workgroup of FO1_BLOCK threads
// compacts the up to FO1_ENTRIES entries k_fo_one left in the lane's scratch
// (u32 offsets, topics, values, its two status words) into the caller's
// buffers, which may be mapped host memory: a wave's kept entries go to
// consecutive slots, so the stores are whole lines.  Wave w owns the positions
// [w * C, (w + 1) * C), C = ceil(E / 16) rounded up to 64, its entries in
// registers between the flag and the move steps; the bucket heads are a bitmap
// in LDS, the steps' ballots stay there for the new offsets.  E > cap: the
// caller has no room for the fan-out (TM_ECAP), the un-aggregated offsets are
// passed on and no entry is written.  A fan-out that was not completed
// (FO1_TOO_LARGE) is passed on as it is.
constexpr uint32_t AG1_WAVES = FO1_BLOCK / 64;
constexpr uint32_t AG1_STEPS = FO1_ENTRIES / FO1_BLOCK;
static_assert(FO1_MAX_DESTS + 2 <= FO1_BLOCK, "k_ag_one: one thread per offset");

__global__ __launch_bounds__(FO1_BLOCK) void k_ag_one(const uint32_t *st_in, const uint32_t *doff, uint32_t n_dests,
                                                      const uint32_t *in_t, const uint32_t *in_v,
                                                      const uint32_t *filter_of, uint64_t filter_len,
                                                      uint32_t *out_doff, uint32_t *out_t, uint32_t *out_v,
                                                      uint64_t cap, uint32_t *st_out) {
    __shared__ uint32_t s_head[FO1_ENTRIES / 32];
    __shared__ uint64_t s_bal[AG1_WAVES * AG1_STEPS];
    __shared__ uint32_t s_wt[AG1_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t state = st_in[FO1_ST_STATE], total = st_in[FO1_ST_TOTAL];
    if (state != FO1_DONE || n_dests > FO1_MAX_DESTS) {   // (block-uniform)
        if (tid == 0) { st_out[FO1_ST_TOTAL] = total; st_out[FO1_ST_STATE] = state; }
        return;
    }
    uint32_t E = doff[n_dests + 1];
    if (E > FO1_ENTRIES) E = FO1_ENTRIES;   // (never: k_fo_one completed)
    if (E > cap) {
        if (tid <= n_dests + 1) out_doff[tid] = doff[tid];
        if (tid == 0) { st_out[FO1_ST_TOTAL] = total; st_out[FO1_ST_STATE] = FO1_DONE; }
        return;
    }
    for (uint32_t i = tid; i < FO1_ENTRIES / 32; i += FO1_BLOCK) s_head[i] = 0;
    __syncthreads();
    if (tid <= n_dests) {
        const uint32_t x = doff[tid];
        if (x < E) atomicOr(&s_head[x >> 5], 1u << (x & 31));
    }
    const uint32_t u0 = doff[n_dests], U = u0 < E ? u0 : E;
    __syncthreads();
    const uint32_t C = ((E + AG1_WAVES - 1) / AG1_WAVES + 63) & ~63u;   // (<= 64 * AG1_STEPS)
    const uint32_t c0 = wv * C < E ? wv * C : E, c1 = c0 + C < E ? c0 + C : E;
    uint32_t rt[AG1_STEPS], rv[AG1_STEPS], rf[AG1_STEPS];
#pragma unroll
    for (uint32_t k = 0; k < AG1_STEPS; k++) {
        const uint32_t p = c0 + k * 64 + lane;
        rv[k] = p < c1 ? in_v[p] : 0u;
        rt[k] = p < c1 ? in_t[p] : 0u;
    }
    uint32_t pt = 0, pf = AG_NONE;
    if (c0 < c1 && c0 > 0) {
        pt = in_t[c0 - 1];
        pf = ag_filter(in_v[c0 - 1], filter_of, filter_len);
    }
#pragma unroll
    for (uint32_t k = 0; k < AG1_STEPS; k++) {
        const uint32_t p = c0 + k * 64 + lane;
        rf[k] = p < c1 ? ag_filter(rv[k], filter_of, filter_len) : AG_NONE;
    }
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t k = 0; k < AG1_STEPS; k++) {
        if (k * 64 >= C) break;   // (block-uniform)
        const uint32_t p = c0 + k * 64 + lane;
        uint32_t t1 = __shfl_up(rt[k], 1, 64), f1 = __shfl_up(rf[k], 1, 64);
        if (lane == 0) { t1 = pt; f1 = pf; }
        const bool same = rt[k] == t1 && rf[k] == f1 && rf[k] != AG_NONE;
        const bool head = p < c1 && ((s_head[p >> 5] >> (p & 31)) & 1u);
        const uint64_t m = __ballot(p < c1 && (!same || head || p >= U));
        if (lane == 0) s_bal[wv * AG1_STEPS + k] = m;
        kept += (uint32_t)__popcll(m);
        pt = __shfl(rt[k], 63, 64);
        pf = __shfl(rf[k], 63, 64);
    }
    if (lane == 0) s_wt[wv] = kept;
    __syncthreads();
    uint32_t base = 0, K = 0;
    for (uint32_t q = 0; q < AG1_WAVES; q++) {
        if (q < wv) base += s_wt[q];
        K += s_wt[q];
    }
#pragma unroll
    for (uint32_t k = 0; k < AG1_STEPS; k++) {
        if (k * 64 >= C) break;   // (block-uniform)
        const uint64_t m = s_bal[wv * AG1_STEPS + k];
        const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (((m >> lane) & 1ull) && slot < cap) {   // (slot < K <= E <= cap always)
            out_t[slot] = rt[k];
            out_v[slot] = rv[k];
        }
        base += (uint32_t)__popcll(m);
    }
    if (tid <= n_dests + 1) {
        const uint32_t x0 = doff[tid], x = x0 < E ? x0 : E;
        uint32_t r = K;
        if (x < E) {   // (C > 0 then)
            const uint32_t w = x / C, j = (x - w * C) >> 6;
            r = 0;
            for (uint32_t q = 0; q < w; q++) r += s_wt[q];
            for (uint32_t i = 0; i < j; i++) r += (uint32_t)__popcll(s_bal[w * AG1_STEPS + i]);
            r += (uint32_t)__popcll(s_bal[w * AG1_STEPS + j] & ((1ull << (x & 63)) - 1ull));
        }
        out_doff[tid] = r;
    }
    if (tid == 0) { st_out[FO1_ST_TOTAL] = total; st_out[FO1_ST_STATE] = FO1_DONE; }
}

}  // namespace

hipError_t launch_aggre(const FanoutScratch &fs, uint32_t n_dests, const uint64_t *dest_offsets, const uint32_t *in_topic,
                        const uint32_t *in_value, uint64_t cap, const uint32_t *filter_of, uint64_t filter_len,
                        uint64_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_value, hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS) return hipErrorInvalidValue;
    if (!filter_of) filter_len = 0;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (!fs.ag_bits || cap > fs.ag_cap) return hipErrorInvalidValue;   // (a bitmap word per 64 positions below cap)
    const dim3 g(FO_GRID), b(64), gb((n_dests + 2 + 255) / 256), bb(256);
    hipLaunchKernelGGL(k_ag_flag, g, b, 0, s, dest_offsets, n_dests, cap, in_topic, in_value, filter_of, filter_len,
                       fs.ag_bits, fs.ag_cnt);
    hipLaunchKernelGGL(k_ag_heads, gb, bb, 0, s, dest_offsets, n_dests, cap, fs.ag_bits, fs.ag_cnt);
    hipLaunchKernelGGL(k_ag_scan, dim3(1), bb, 0, s, fs.ag_cnt);
    hipLaunchKernelGGL(k_ag_move, g, b, 0, s, dest_offsets, n_dests, cap, in_topic, in_value, fs.ag_bits, fs.ag_cnt,
                       fs.ag_pre, out_topic, out_value);
    hipLaunchKernelGGL(k_ag_offsets, gb, bb, 0, s, dest_offsets, n_dests, cap, fs.ag_bits, fs.ag_cnt, fs.ag_pre,
                       out_dest_offsets);
    return hipGetLastError();
}

hipError_t launch_aggre_one(const uint32_t *status_in, const uint32_t *dest_offsets, uint32_t n_dests,
                            const uint32_t *in_topic, const uint32_t *in_value, const uint32_t *filter_of,
                            uint64_t filter_len, uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_value,
                            uint64_t cap, uint32_t *status, hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS) return hipErrorInvalidValue;
    if (!filter_of) filter_len = 0;
    hipLaunchKernelGGL(k_ag_one, dim3(1), dim3(FO1_BLOCK), 0, s, status_in, dest_offsets, n_dests, in_topic, in_value,
                       filter_of, filter_len, out_dest_offsets, out_topic, out_value, cap, status);
    return hipGetLastError();
}

}  // namespace tmx
