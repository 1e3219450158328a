// tm_retain.hip -- the retained-message store's kernels (gfx950, wave64).
//
// emqx_retainer_mnesia:match_messages/3 is emqx_topic:match/2 of one filter
// over the message table plus the expiry test (emqx_retainer_mnesia.erl:288-304,
// 409-475; emqx_topic.erl:80-116).  Here the table is a column store of level
// ids (tm_retain.h) and a batch of filters is answered by a data-parallel scan:
// the host hands each filter the base range of its literal prefix and the whole
// tail, a block owns one tile of RT_TILE rows of one of those segments and finds
// which by a search over the per-filter tile prefix sums, one lane tests one
// row.  Only the columns of the filter's literal levels past the prefix are
// read, meta always, expiry only where the row is flagged as having one.
// Hits are ranked by ballot and popcount, one atomic per wave; offsets come
// from counts: k_ret_rows<false> counts, k_ret_offsets scans, k_ret_rows<true>
// emits.
#include <hip/hip_runtime.h>

#include "tm_retain.h"
#include "tm_retain_dev.h"   // ret_row_matches, shared with tm_retain_page.hip

namespace tmx {
namespace {

constexpr uint32_t SCAN_THREADS = 256;

template <bool EMIT>
__global__ __launch_bounds__(RT_TILE) void k_ret_rows(RetView v, const RetQ *__restrict__ qs, uint32_t nq,
                                                      const uint32_t *__restrict__ ids, const uint32_t *__restrict__ tile_ps,
                                                      uint32_t tile_base, uint64_t now, uint32_t *__restrict__ counts,
                                                      const uint64_t *__restrict__ offs, uint32_t *__restrict__ cursor,
                                                      uint32_t *__restrict__ out, uint64_t out_cap) {
    // which filter's tile is this block's: the last f with tile_ps[f] <= b (uniform: scalar loads); b is the
    // tile's number in the batch, this launch's first tile plus the block's
    const uint32_t b = tile_base + blockIdx.x;
    uint32_t lo = 0, hi = nq;   // tile_ps[lo] <= b < tile_ps[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tile_ps[mid] <= b) lo = mid; else hi = mid;
    }
    const uint32_t f = lo;
    const RetQ q = qs[f];
    const uint32_t t = b - tile_ps[f];
    uint64_t row, end;
    uint32_t skip;
    if (t < q.base_tiles) {
        row = q.lo + (uint64_t)t * RT_TILE + threadIdx.x;
        end = q.hi;
        skip = q.skip;
    } else {
        row = v.base + (uint64_t)(t - q.base_tiles) * RT_TILE + threadIdx.x;
        end = v.base + v.tail;
        skip = 0;   // the tail is in arrival order: every level is tested
    }
    const bool hit = row < end && ret_row_matches(v, q, ids, skip, row, now);
    const unsigned long long mask = __ballot(hit);
    if (mask == 0) return;
    const uint32_t n = __popcll(mask);
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if constexpr (!EMIT) {
        if (lane == (uint32_t)__ffsll((long long)mask) - 1) atomicAdd(&counts[f], n);
    } else {
        const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1;
        uint32_t first = 0;
        if (lane == leader) first = atomicAdd(&cursor[f], n);
        first = __shfl(first, (int)leader);
        if (hit) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            const uint64_t pos = offs[f] + first + rank;
            if (pos < out_cap) out[pos] = v.value[row];
        }
    }
}

// exclusive sums of counts[0 .. nq) into offs[0 .. nq], cursor zeroed: one block, each thread a contiguous run
__global__ __launch_bounds__(SCAN_THREADS) void k_ret_offsets(const uint32_t *__restrict__ counts, uint32_t nq,
                                                               uint64_t *__restrict__ offs, uint32_t *__restrict__ cursor) {
    __shared__ uint64_t part[SCAN_THREADS];
    const uint32_t per = (nq + SCAN_THREADS - 1) / SCAN_THREADS;
    const uint32_t b = threadIdx.x * per < nq ? threadIdx.x * per : nq;
    const uint32_t e = b + per < nq ? b + per : nq;
    uint64_t sum = 0;
    for (uint32_t i = b; i < e; ++i) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (uint32_t i = 0; i < SCAN_THREADS; ++i) {
            const uint64_t p = part[i];
            part[i] = run;
            run += p;
        }
        offs[nq] = run;
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint32_t i = b; i < e; ++i) {
        offs[i] = run;
        run += counts[i];
        cursor[i] = 0;
    }
}

// the batch's writes: one thread per row written.  An append stores the row's level ids (columns, then
// the overflow run); every write stores value, expiry and, last in program order, meta.
__global__ __launch_bounds__(256) void k_ret_apply(RetView v, const RetOp *__restrict__ ops, uint32_t n_ops,
                                                   const uint32_t *__restrict__ words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ops) return;
    const RetOp op = ops[i];
    if (op.row >= v.stride) return;
    for (uint32_t l = 0; l < op.nwords; ++l) {
        const uint32_t w = words[op.words_off + l];
        if (l < RT_COLS) v.cols[(uint64_t)l * v.stride + op.row] = w;
        else if (op.ovf_off + (l - RT_COLS) < v.ovf_cap) v.ovf[op.ovf_off + (l - RT_COLS)] = w;
    }
    if (op.nwords > RT_COLS) v.ovf_off[op.row] = op.ovf_off;
    v.value[op.row] = op.value;
    v.expiry[op.row] = op.expiry;
    v.meta[op.row] = op.meta;
}

}  // namespace

hipError_t launch_ret_apply(const RetView &v, const RetOp *d_ops, uint32_t n_ops, const uint32_t *d_words, uint64_t,
                            hipStream_t s) {
    if (!n_ops) return hipSuccess;
    hipLaunchKernelGGL(k_ret_apply, dim3((n_ops + 255) / 256), dim3(256), 0, s, v, d_ops, n_ops, d_words);
    return hipGetLastError();
}

hipError_t launch_ret_count(const RetView &v, const RetQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                            uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t *d_counts, hipStream_t s) {
    if (!tiles || !nq) return hipSuccess;
    if (tiles > RT_MAX_LAUNCH_TILES) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_ret_rows<false>, dim3(tiles), dim3(RT_TILE), 0, s, v, d_q, nq, d_ids, d_tile_ps, tile_base, now, d_counts,
                       (const uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint64_t)0);
    return hipGetLastError();
}

hipError_t launch_ret_offsets(const uint32_t *d_counts, uint32_t nq, uint64_t *d_offs, uint32_t *d_cursor, hipStream_t s) {
    hipLaunchKernelGGL(k_ret_offsets, dim3(1), dim3(SCAN_THREADS), 0, s, d_counts, nq, d_offs, d_cursor);
    return hipGetLastError();
}

hipError_t launch_ret_emit(const RetView &v, const RetQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                           uint32_t tile_base, uint32_t tiles, uint64_t now, const uint64_t *d_offs, uint32_t *d_cursor,
                           uint32_t *d_out, uint64_t out_cap, hipStream_t s) {
    if (!tiles || !nq) return hipSuccess;
    if (tiles > RT_MAX_LAUNCH_TILES) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_ret_rows<true>, dim3(tiles), dim3(RT_TILE), 0, s, v, d_q, nq, d_ids, d_tile_ps, tile_base, now,
                       (uint32_t *)nullptr, d_offs, d_cursor, d_out, out_cap);
    return hipGetLastError();
}

}  // namespace tmx
