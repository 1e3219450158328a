// tm_retain_page.hip -- the retained store's paged lookup (gfx950, wave64).
//
// emqx_retainer_mnesia:match_messages/3 with a cursor consumes batch_read_number
// rows of a stream per call (emqx_retainer_mnesia.erl:288-304).  Here a page is
// the first `limit` hits of a filter in scan order (tm_retain_page.h).  As in
// tm_retain.hip a block owns one tile of RT_TILE rows of one segment of one
// filter and finds which through the tile prefix sums; one lane tests one row.
// Hits are placed by rank, not by arrival: k_retp_count stores each tile's hit
// count, k_retp_cut scans one filter's counts up to `limit`, k_retp_emit ranks
// the hits of a tile by ballot plus the waves' prefix from LDS.  No atomic,
// global or LDS; everything left for the host or for a later launch is written
// with ordinary stores.
#include <hip/hip_runtime.h>

#include "tm_retain_page.h"
#include "tm_retain_dev.h"

namespace tmx {
namespace {

constexpr uint32_t WAVES = RT_TILE / 64;

struct TileRows {
    uint32_t f;      // the filter
    uint32_t skip;   // levels known equal
    uint64_t row;    // this lane's row
    uint64_t end;    // its segment's end
};

// which filter's tile is tile b of the batch, and this lane's row in it: the last f with tile_ps[f] <= b
// (uniform: scalar loads)
__device__ __forceinline__ TileRows tile_rows(const RetPQ *__restrict__ qs, uint32_t nq, const uint32_t *__restrict__ tile_ps,
                                              uint32_t b, RetPQ &q) {
    uint32_t lo = 0, hi = nq;   // tile_ps[lo] <= b < tile_ps[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tile_ps[mid] <= b) lo = mid; else hi = mid;
    }
    q = qs[lo];
    const uint32_t t = b - tile_ps[lo];
    TileRows r;
    r.f = lo;
    if (t < q.base_tiles) {
        r.row = q.lo + (uint64_t)t * RT_TILE + threadIdx.x;
        r.end = q.hi;
        r.skip = q.skip;
    } else {
        r.row = q.tail_lo + (uint64_t)(t - q.base_tiles) * RT_TILE + threadIdx.x;
        r.end = q.tail_hi;
        r.skip = 0;   // the tail is in arrival order: every level is tested
    }
    return r;
}

__global__ __launch_bounds__(RT_TILE) void k_retp_count(RetView v, const RetPQ *__restrict__ qs, uint32_t nq,
                                                        const uint32_t *__restrict__ ids, const uint32_t *__restrict__ tile_ps,
                                                        uint32_t tile_base, uint64_t now, uint32_t *__restrict__ tile_cnt) {
    __shared__ uint32_t wave_n[WAVES];
    const uint32_t b = tile_base + blockIdx.x;
    RetPQ q;
    const TileRows r = tile_rows(qs, nq, tile_ps, b, q);
    const bool hit = r.row < r.end && ret_row_matches(v, q, ids, r.skip, r.row, now);
    const unsigned long long mask = __ballot(hit);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t n = 0;
        for (uint32_t w = 0; w < WAVES; ++w) n += wave_n[w];
        tile_cnt[b] = n;
    }
}

// one block per filter: its tiles' counts in chunks of RTP_CHUNK, one tile per thread
__global__ __launch_bounds__(RTP_CHUNK) void k_retp_cut(const uint32_t *__restrict__ tile_ps, const uint32_t *__restrict__ tile_cnt,
                                                        uint32_t limit, uint32_t *__restrict__ tile_excl,
                                                        uint32_t *__restrict__ taken, uint64_t *__restrict__ next_row) {
    __shared__ uint32_t wave_n[RTP_CHUNK / 64];
    const uint32_t f = blockIdx.x;
    const uint32_t first = tile_ps[f], end = tile_ps[f + 1];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t run = 0;   // the hits before this chunk
    uint32_t c = first;
    for (; c < end && run < limit; c += RTP_CHUNK) {   // (end - c may pass 2^31: c never wraps, end < 2^31)
        const uint32_t t = c + threadIdx.x;
        const uint32_t n = t < end ? tile_cnt[t] : 0;
        uint32_t incl = n;   // the inclusive sum over the wave (a tile has at most RT_TILE hits: no overflow)
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_n[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < RTP_CHUNK / 64; ++w) {
            const uint32_t x = wave_n[w];
            if (w < wave) before += x;
            total += x;
        }
        __syncthreads();   // wave_n is written again by the next chunk
        if (t < end) {
            const uint64_t excl = run + before + (incl - n);
            tile_excl[t] = excl < limit ? (uint32_t)excl : limit;
        }
        run += total;
    }
    // the tiles past the cut: nothing to emit
    for (uint64_t t = (uint64_t)c + threadIdx.x; t < end; t += RTP_CHUNK) tile_excl[t] = limit;
    if (threadIdx.x == 0) {
        taken[f] = run < limit ? (uint32_t)run : limit;
        next_row[f] = 0;
    }
}

__global__ __launch_bounds__(RT_TILE) void k_retp_emit(RetView v, const RetPQ *__restrict__ qs, uint32_t nq,
                                                       const uint32_t *__restrict__ ids, const uint32_t *__restrict__ tile_ps,
                                                       uint32_t tile_base, uint64_t now, uint32_t limit,
                                                       const uint32_t *__restrict__ tile_cnt, const uint32_t *__restrict__ tile_excl,
                                                       const uint64_t *__restrict__ offs, uint32_t *__restrict__ out,
                                                       uint64_t out_cap, uint64_t *__restrict__ next_row) {
    __shared__ uint32_t wave_n[WAVES];
    const uint32_t b = tile_base + blockIdx.x;
    const uint32_t excl = tile_excl[b];
    if (excl >= limit || tile_cnt[b] == 0) return;   // (uniform over the block)
    RetPQ q;
    const TileRows r = tile_rows(qs, nq, tile_ps, b, q);
    const bool hit = r.row < r.end && ret_row_matches(v, q, ids, r.skip, r.row, now);
    const unsigned long long mask = __ballot(hit);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_n[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!hit) return;
    uint32_t before = 0;
    for (uint32_t w = 0; w < WAVES; ++w)
        if (w < wave) before += wave_n[w];
    // row order: the waves before this one, then the lanes before this one
    const uint64_t k = (uint64_t)excl + before +
                       __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (k >= limit) return;
    const uint64_t pos = offs[r.f] + k;
    if (pos < out_cap) out[pos] = v.value[r.row];
    if (k == (uint64_t)limit - 1) next_row[r.f] = r.row + 1;
}

}  // namespace

hipError_t launch_retp_count(const RetView &v, const RetPQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                             uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t *d_tile_cnt, hipStream_t s) {
    if (!tiles || !nq) return hipSuccess;
    if (tiles > RT_MAX_LAUNCH_TILES) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_retp_count, dim3(tiles), dim3(RT_TILE), 0, s, v, d_q, nq, d_ids, d_tile_ps, tile_base, now, d_tile_cnt);
    return hipGetLastError();
}

hipError_t launch_retp_cut(const uint32_t *d_tile_ps, uint32_t nq, const uint32_t *d_tile_cnt, uint32_t limit,
                           uint32_t *d_tile_excl, uint32_t *d_taken, uint64_t *d_next_row, hipStream_t s) {
    if (!nq) return hipSuccess;
    hipLaunchKernelGGL(k_retp_cut, dim3(nq), dim3(RTP_CHUNK), 0, s, d_tile_ps, d_tile_cnt, limit, d_tile_excl, d_taken, d_next_row);
    return hipGetLastError();
}

hipError_t launch_retp_emit(const RetView &v, const RetPQ *d_q, uint32_t nq, const uint32_t *d_ids, const uint32_t *d_tile_ps,
                            uint32_t tile_base, uint32_t tiles, uint64_t now, uint32_t limit, const uint32_t *d_tile_cnt,
                            const uint32_t *d_tile_excl, const uint64_t *d_offs, uint32_t *d_out, uint64_t out_cap,
                            uint64_t *d_next_row, hipStream_t s) {
    if (!tiles || !nq) return hipSuccess;
    if (tiles > RT_MAX_LAUNCH_TILES) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_retp_emit, dim3(tiles), dim3(RT_TILE), 0, s, v, d_q, nq, d_ids, d_tile_ps, tile_base, now, limit,
                       d_tile_cnt, d_tile_excl, d_offs, d_out, out_cap, d_next_row);
    return hipGetLastError();
}

}  // namespace tmx
