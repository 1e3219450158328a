// tm_group.hip -- a batch's local deliveries regrouped by subscriber, for gfx950.
//
// do_dispatch2/3 sends SubPid ! {deliver, To, Msg} once per delivery
// (apps/emqx/src/emqx_broker.erl:745-752), and the first thing a connection
// process does is gather its mailbox's delivers back into one list
// (emqx_connection.erl:611-612: [Deliver | emqx_utils:drain_deliver(ActiveN)]).
// A micro-batched broker hands a subscriber its list at once: the W deliveries
// (topic, value, subscriber) a dispatch wrote in message order, stably sorted
// by subscriber, with the G distinct subscribers and their offsets.
//
// The key is an interned pid, any u32, so the fan-out's buckets do not carry
// over: a stable LSD radix sort of (key, position) pairs, 8-bit digits, over a
// fixed grid of GS_GRID blocks of GS_BLOCK threads; block k owns the positions
// [k * chunk, (k + 1) * chunk) of [0, W), chunk = ceil(W / GS_GRID) rounded up
// to GS_TILE.  W = min(head[1], cap) is read on the device by every kernel.
// No block waits for another: every step is a launch of its own.
//   k_gs_pre      the block's histogram of all four digits (LDS, one add per
//                 run of equal digits in a wave), its non-zero counts added
//                 to the digits' bin totals tot[digit][bin] (device atomics:
//                 integer sums, the same whatever the order; dense ids touch
//                 few bins);
//   k_gs_plan     one block: reads the totals and zeroes them for the next
//                 call.  A digit whose W keys all fall in one bin is the
//                 identity: skip[p]; src[p] = where pass p reads (the caller's
//                 array with the positions 0, 1, .. at first, then the two
//                 pair arrays in turn), src[4] = where the sorted pairs end
//                 up; base[p][bin] = the exclusive scan of digit p's totals
//                 (a permutation does not change them: known before any pass
//                 runs).  A dense pid space below 2^16 costs two passes.
//   per pass p that is not skipped (the three kernels of a skipped pass read
//   skip[p] and return; a block whose chunk is empty returns at once):
//   k_gs_hist     the block's histogram of digit p -> tab[bin][block];
//   k_gs_scan     block b: the exclusive scan of bin b's row over the blocks
//                 that own keys, from base[p][b];
//   k_gs_scatter  per tile of GS_TILE keys: a wave finds each key's lanes with
//                 the same digit by 8 ballots (rank inside the wave = the set
//                 lanes below it), the run's first lane stores the run length
//                 in cnt[64-key row][bin]; thread b scans bin b down the 16
//                 rows and carries the block's running offset of its bin;
//                 every key goes to tab[bin][block] + keys of the bin in
//                 earlier tiles + in earlier rows + its rank: stable.
//   k_gs_heads    wave w of block k counts the group heads (a key that
//                 differs from its predecessor) of its quarter of the chunk;
//   k_gs_gscan    one block: the exclusive scan of the GS_GRID * 4 counts;
//                 ghead = [G, W], out_goff[G] = W when G <= gcap;
//   k_gs_emit     the same wave numbers its heads from its base (ballot,
//                 popcount) and writes out_gsub / out_goff below gcap, and
//                 gathers (topic, value) through the position: the payload.
// Bytes per delivery: 4 read (pre), per pass run 4 read (hist) + 8 read + 8
// written (scatter), 8 read (heads: the key and its predecessor), 8 read + 8
// gathered + 12 (16 with out_perm) written (emit).  Scratch: 16 bytes per
// delivery below cap and GS_FIX_WORDS words (1.03 MiB).
#include <hip/hip_runtime.h>

#include "tm_dev.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "tm_group.hip: wave64 ballots and the LDS budget are written for gfx950 only"
#endif

namespace tmx {

namespace {

constexpr uint32_t GS_WAVES = GS_BLOCK / 64;
constexpr uint32_t GS_ROWS = GS_TILE / 64;        // 64-key rows of a tile
constexpr uint32_t GS_PER = GS_ROWS / GS_WAVES;   // rows (keys) a wave (a thread) takes per tile
static_assert(GS_BLOCK == GS_BINS, "thread b of a block owns bin b");
static_assert(GS_TILE % GS_BLOCK == 0 && GS_ROWS % GS_WAVES == 0, "a tile is whole rows per wave");
static_assert(GS_GRID == 1024 && GS_WAVES == 4 && GS_PASSES * GS_BINS == 1024, "k_gs_gscan, k_gs_plan: 1024 threads");
static_assert(GS_GRID == GS_BLOCK * 4 && GS_TAB % 4 == 0, "k_gs_scan: one aligned quad of a row per thread");

struct GsBufs {
    uint32_t *fix, *k[2], *p[2];
};

__device__ __forceinline__ uint64_t gs_w(const uint64_t *head, uint64_t cap) {
    const uint64_t T = head[1];
    return T < cap ? T : cap;
}

// the positions block `blk` owns: [c0, c1) of [0, W); q: a wave's quarter of the chunk
__device__ __forceinline__ void gs_chunk(uint64_t W, uint32_t blk, uint64_t &c0, uint64_t &c1, uint64_t &q) {
    const uint64_t chunk = ((W + GS_GRID - 1) / GS_GRID + GS_TILE - 1) / GS_TILE * GS_TILE;
    q = chunk / GS_WAVES;
    c0 = (uint64_t)blk * chunk;
    if (c0 > W) c0 = W;
    c1 = c0 + chunk < W ? c0 + chunk : W;
}

// the keys and positions pass-source `src` names (positions null: 0, 1, ..)
__device__ __forceinline__ void gs_source(const GsBufs &b, const uint32_t *in_sub, uint32_t src, const uint32_t *&k,
                                          const uint32_t *&p) {
    k = src == GS_IN ? in_sub : b.k[src & 1];
    p = src == GS_IN ? nullptr : b.p[src & 1];
}

// the lanes of the wave (among those with ok) whose 8-bit digit equals this lane's
__device__ __forceinline__ uint64_t gs_match(uint32_t d, bool ok) {
    uint64_t m = __ballot(ok);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__device__ __forceinline__ uint32_t gs_below(uint64_t m, uint32_t lane) {
    return (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

__device__ __forceinline__ uint32_t gs_incl_scan32(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    return x;
}

__global__ __launch_bounds__(GS_BLOCK) void k_gs_pre(const uint64_t *head, uint64_t cap, const uint32_t *in_sub,
                                                     uint32_t *fix) {
    __shared__ uint32_t s_h[GS_PASSES * GS_BINS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t c0, c1, q;
    gs_chunk(gs_w(head, cap), blockIdx.x, c0, c1, q);
    if (c0 >= c1) return;   // (block-uniform)
#pragma unroll
    for (uint32_t p = 0; p < GS_PASSES; p++) s_h[p * GS_BINS + tid] = 0;
    __syncthreads();
    for (uint64_t i0 = c0 + wv * 64; i0 < c1; i0 += GS_BLOCK) {   // (wave-uniform)
        const uint64_t i = i0 + lane;
        const bool ok = i < c1;
        const uint32_t key = ok ? in_sub[i] : 0u;
#pragma unroll
        for (uint32_t p = 0; p < GS_PASSES; p++) {
            const uint32_t d = (key >> (8 * p)) & 255u;
            const uint64_t m = gs_match(d, ok);
            if (ok && gs_below(m, lane) == 0) atomicAdd(&s_h[p * GS_BINS + d], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t p = 0; p < GS_PASSES; p++) {
        const uint32_t c = s_h[p * GS_BINS + tid];
        if (c) atomicAdd(&fix[GS_TOT + p * GS_BINS + tid], c);
    }
}

__global__ __launch_bounds__(1024) void k_gs_plan(const uint64_t *head, uint64_t cap, uint32_t *fix) {
    __shared__ uint32_t s_one[GS_PASSES];
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t W = gs_w(head, cap);
    if (tid < GS_PASSES) s_one[tid] = 0;
    __syncthreads();
    const uint32_t tot = fix[GS_TOT + tid];   // (digit tid / 256, bin tid % 256: four waves a digit)
    fix[GS_TOT + tid] = 0;                    // (the next call on this stream adds to zeroes)
    if (tot == W) s_one[tid / GS_BINS] = 1;   // (W == 0: every bin)
    const uint32_t inc = gs_incl_scan32(tot, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = inc - tot;
    for (uint32_t w = wv & ~3u; w < wv; w++) base += s_w[w];
    fix[GS_BASE + tid] = base;
    if (tid == 0) {
        uint32_t src = GS_IN, run = 0;
        for (uint32_t p = 0; p < GS_PASSES; p++) {
            const uint32_t skip = s_one[p];
            fix[GS_SKIP + p] = skip;
            fix[GS_SRC + p] = src;
            if (!skip) {
                src = src == 0 ? 1u : 0u;   // (GS_IN or pair array 1 -> 0; 0 -> 1)
                run++;
            }
        }
        fix[GS_SRC + GS_PASSES] = src;
        uint64_t *stat = reinterpret_cast<uint64_t *>(fix + GS_STAT);
        stat[0] += run;
        stat[1] += GS_PASSES - run;
    }
}

__global__ __launch_bounds__(GS_BLOCK) void k_gs_hist(const uint64_t *head, uint64_t cap, const uint32_t *in_sub,
                                                      GsBufs bufs, uint32_t pass) {
    __shared__ uint32_t s_h[GS_BINS];
    if (bufs.fix[GS_SKIP + pass]) return;   // (uniform over the grid)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t c0, c1, q;
    gs_chunk(gs_w(head, cap), blockIdx.x, c0, c1, q);
    if (c0 >= c1) return;   // (block-uniform; k_gs_scan reads the columns of blocks that own keys only)
    const uint32_t *kin, *pin;
    gs_source(bufs, in_sub, bufs.fix[GS_SRC + pass], kin, pin);
    s_h[tid] = 0;
    __syncthreads();
    for (uint64_t i0 = c0 + wv * 64; i0 < c1; i0 += GS_BLOCK) {
        const uint64_t i = i0 + lane;
        const bool ok = i < c1;
        const uint32_t d = ((ok ? kin[i] : 0u) >> (8 * pass)) & 255u;
        const uint64_t m = gs_match(d, ok);
        if (ok && gs_below(m, lane) == 0) atomicAdd(&s_h[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    bufs.fix[GS_TAB + tid * GS_GRID + blockIdx.x] = s_h[tid];   // (every word, every pass run: nothing stale)
}

// block b: bin b's row tab[b][0 .. nb) -> its exclusive scan in place from base[pass][b], nb = the
// blocks that own keys (the sums stay below 2^32: W does)
__global__ __launch_bounds__(GS_BLOCK) void k_gs_scan(const uint64_t *head, uint64_t cap, uint32_t *fix, uint32_t pass) {
    __shared__ uint32_t s_w[GS_WAVES];
    if (fix[GS_SKIP + pass]) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, bin = blockIdx.x;
    const uint64_t W = gs_w(head, cap);
    const uint64_t chunk = ((W + GS_GRID - 1) / GS_GRID + GS_TILE - 1) / GS_TILE * GS_TILE;   // (gs_chunk's)
    const uint32_t nb = chunk ? (uint32_t)((W + chunk - 1) / chunk) : 0u;                     // (<= GS_GRID)
    uint4 *quad = reinterpret_cast<uint4 *>(fix + GS_TAB + (uint64_t)bin * GS_GRID) + tid;
    uint4 x = *quad;
    const uint32_t col = 4 * tid;   // (a column at or past nb holds what an older call left: counted as 0)
    if (col + 0 >= nb) x.x = 0;
    if (col + 1 >= nb) x.y = 0;
    if (col + 2 >= nb) x.z = 0;
    if (col + 3 >= nb) x.w = 0;
    const uint32_t sum = x.x + x.y + x.z + x.w;
    const uint32_t inc = gs_incl_scan32(sum, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t run = fix[GS_BASE + pass * GS_BINS + bin] + inc - sum;
    for (uint32_t w = 0; w < wv; w++) run += s_w[w];
    uint4 y;
    y.x = run;
    y.y = y.x + x.x;
    y.z = y.y + x.y;
    y.w = y.z + x.z;
    *quad = y;
}

__global__ __launch_bounds__(GS_BLOCK) void k_gs_scatter(const uint64_t *head, uint64_t cap, const uint32_t *in_sub,
                                                         GsBufs bufs, uint32_t pass) {
    __shared__ uint32_t s_cnt[GS_ROWS][GS_BINS];
    __shared__ uint32_t s_base[GS_BINS];
    if (bufs.fix[GS_SKIP + pass]) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t W = gs_w(head, cap);
    uint64_t c0, c1, q;
    gs_chunk(W, blockIdx.x, c0, c1, q);
    const uint32_t src = bufs.fix[GS_SRC + pass], dst = src == 0 ? 1u : 0u;
    const uint32_t *kin, *pin;
    gs_source(bufs, in_sub, src, kin, pin);
    uint32_t *kout = bufs.k[dst], *pout = bufs.p[dst];
    uint32_t base = bufs.fix[GS_TAB + tid * GS_GRID + blockIdx.x];   // where the block's next key of bin tid goes
    for (uint64_t t0 = c0; t0 < c1; t0 += GS_TILE) {
#pragma unroll
        for (uint32_t r = 0; r < GS_ROWS; r++) s_cnt[r][tid] = 0;
        __syncthreads();
        uint32_t key[GS_PER], pos[GS_PER], rk[GS_PER];
#pragma unroll
        for (uint32_t r = 0; r < GS_PER; r++) {
            const uint32_t row = r * GS_WAVES + wv;
            const uint64_t i = t0 + row * 64 + lane;
            const bool ok = i < c1;
            key[r] = ok ? kin[i] : 0u;
            pos[r] = !ok ? 0u : pin ? pin[i] : (uint32_t)i;
        }
#pragma unroll
        for (uint32_t r = 0; r < GS_PER; r++) {
            const uint32_t row = r * GS_WAVES + wv;
            const bool ok = t0 + row * 64 + lane < c1;
            const uint32_t d = (key[r] >> (8 * pass)) & 255u;
            const uint64_t m = gs_match(d, ok);
            rk[r] = gs_below(m, lane);
            if (ok && rk[r] == 0) s_cnt[row][d] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t run = 0;
#pragma unroll
        for (uint32_t r = 0; r < GS_ROWS; r++) {
            const uint32_t c = s_cnt[r][tid];
            s_cnt[r][tid] = run;
            run += c;
        }
        s_base[tid] = base;
        base += run;
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < GS_PER; r++) {
            const uint32_t row = r * GS_WAVES + wv;
            const bool ok = t0 + row * 64 + lane < c1;
            const uint32_t d = (key[r] >> (8 * pass)) & 255u;
            const uint32_t at = s_base[d] + s_cnt[row][d] + rk[r];
            if (ok && at < W) {   // (at < W always: the bins' counts sum to W)
                kout[at] = key[r];
                pout[at] = pos[r];
            }
        }
        __syncthreads();
    }
}

// is position i (< W) the first of its group
__device__ __forceinline__ bool gs_is_head(const uint32_t *k, uint64_t i, uint32_t key) {
    return i == 0 || k[i - 1] != key;
}

__global__ __launch_bounds__(GS_BLOCK) void k_gs_heads(const uint64_t *head, uint64_t cap, const uint32_t *in_sub,
                                                       GsBufs bufs) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t c0, c1, q;
    gs_chunk(gs_w(head, cap), blockIdx.x, c0, c1, q);
    const uint32_t *k, *p;
    gs_source(bufs, in_sub, bufs.fix[GS_SRC + GS_PASSES], k, p);
    const uint64_t w0 = c0 + wv * q < c1 ? c0 + wv * q : c1, w1 = w0 + q < c1 ? w0 + q : c1;
    uint32_t n = 0;
    for (uint64_t i0 = w0; i0 < w1; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool h = i < w1 && gs_is_head(k, i, k[i]);
        n += (uint32_t)__popcll(__ballot(h));
    }
    if (lane == 0) bufs.fix[GS_GCNT + blockIdx.x * GS_WAVES + wv] = n;
}

__global__ __launch_bounds__(1024) void k_gs_gscan(const uint64_t *head, uint64_t cap, uint32_t *fix, uint64_t *ghead,
                                                   uint64_t *out_goff, uint64_t gcap) {
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint4 *quad = reinterpret_cast<uint4 *>(fix + GS_GCNT) + tid;   // block tid's four waves
    const uint4 x = *quad;
    const uint32_t c = x.x + x.y + x.z + x.w;
    const uint32_t inc = gs_incl_scan32(c, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = inc - c;
    for (uint32_t w = 0; w < wv; w++) base += s_w[w];
    uint4 y;
    y.x = base;
    y.y = y.x + x.x;
    y.z = y.y + x.y;
    y.w = y.z + x.z;
    *quad = y;
    if (tid == 1023) {
        const uint64_t G = (uint64_t)base + c, W = gs_w(head, cap);
        ghead[0] = G;
        ghead[1] = W;
        if (G <= gcap) out_goff[G] = W;
    }
}

__global__ __launch_bounds__(GS_BLOCK) void k_gs_emit(const uint64_t *head, uint64_t cap, const uint32_t *in_topic,
                                                      const uint32_t *in_value, const uint32_t *in_sub, GsBufs bufs,
                                                      uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap,
                                                      uint32_t *out_topic, uint32_t *out_value, uint32_t *out_sub,
                                                      uint32_t *out_perm) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t W = gs_w(head, cap);
    uint64_t c0, c1, q;
    gs_chunk(W, blockIdx.x, c0, c1, q);
    const uint32_t *k, *p;
    gs_source(bufs, in_sub, bufs.fix[GS_SRC + GS_PASSES], k, p);
    const uint64_t w0 = c0 + wv * q < c1 ? c0 + wv * q : c1, w1 = w0 + q < c1 ? w0 + q : c1;
    uint64_t g0 = bufs.fix[GS_GCNT + blockIdx.x * GS_WAVES + wv];   // groups that start before w0
    for (uint64_t i0 = w0; i0 < w1; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool ok = i < w1;
        const uint32_t key = ok ? k[i] : 0u;
        const uint32_t pos = !ok ? 0u : p ? p[i] : (uint32_t)i;
        const bool h = ok && gs_is_head(k, i, key);
        const uint64_t hm = __ballot(h);
        if (h) {
            const uint64_t g = g0 + gs_below(hm, lane);
            if (g < gcap) out_gsub[g] = key;
            if (g <= gcap) out_goff[g] = i;   // (g == gcap < G: where the first group left out starts)
        }
        g0 += (uint32_t)__popcll(hm);
        if (ok && pos < W) {   // (pos < W always)
            out_topic[i] = in_topic[pos];
            out_value[i] = in_value[pos];
            out_sub[i] = key;
            if (out_perm) out_perm[i] = pos;
        }
    }
}

// ---- the shared-subscription picks merged with the deliveries and grouped
// (tm_group_picks_dev).  A connection process receives {deliver, To, Msg} from
// do_dispatch2 and from emqx_shared_sub:dispatch/3 in one mailbox; its list of
// a batch holds both kinds in publish order.  The deliveries come in ascending
// message order, the picks in entry order (bucket by bucket), so the picks are
// merged in by message before the subscriber sort, which is stable:
//   k_gp_count    block k counts the local picks (sub_of[member[q]] != NONE)
//                 among its chunk of the E entries (a ballot and popcount per
//                 wave);
//   k_gp_scan     one block: the exclusive scan of the GS_GRID counts; the
//                 picks' head [0, P] and the merged head [0, N = W + P];
//   k_gp_compact  the block's local picks (topic, value, subscriber) to their
//                 ranks, ascending q: rank = the block's base + the picks of
//                 earlier tiles and waves + the set lanes below;
//   the k_gs_pre / plan / hist / scan / scatter passes above over the P picks'
//   topic indices, head [0, P]: a stable sort by message, a digit all agree on
//   skipped -- a batch of at most 256 messages costs one pass;
//   k_gp_merge    two binary searches on sorted arrays: delivery p goes to p +
//                 the picks with a message < t_p, the pick of sorted rank r to
//                 r + the deliveries with a message <= t_r -- inside one
//                 message the deliveries first, then its picks in ascending q;
//                 writes the merged (topic, value, subscriber, src);
//   the same k_gs_* passes, k_gs_heads and k_gs_gscan over the N merged
//   subscriber ids, head [0, N];
//   k_gp_emit     k_gs_emit with a bound on the positions written (out_cap)
//                 and out_src through the merged src.
// Bytes per entry below E: 8 read twice (member, sub_of), per local pick 8 read
// + 12 written (compact), 4 + per pass 28 (the sort), 16 gathered + 16 written
// and two searches (merge); per delivery 12 read + 16 written and one search
// (merge); per merged delivery the grouping's bytes above, k_gp_emit's 16
// gathered for k_gs_emit's 8.  Scratch: 32 bytes per (cap + ecap), 12 per ecap.
constexpr uint32_t GP_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint64_t gp_e(const uint64_t *doff, uint32_t n_dests, uint64_t ecap) {
    const uint64_t K = doff[(uint64_t)n_dests + 1];
    return K < ecap ? K : ecap;
}

// the entries block `blk` owns: [c0, c1) of [0, E), whole GS_BLOCK tiles
__device__ __forceinline__ void gp_chunk(uint64_t E, uint32_t blk, uint64_t &c0, uint64_t &c1) {
    const uint64_t chunk = ((E + GS_GRID - 1) / GS_GRID + GS_BLOCK - 1) / GS_BLOCK * GS_BLOCK;
    c0 = (uint64_t)blk * chunk;
    if (c0 > E) c0 = E;
    c1 = c0 + chunk < E ? c0 + chunk : E;
}

// the local subscriber entry q's pick goes to (NONE: no pick, or not a connection of this node)
__device__ __forceinline__ uint32_t gp_local(const uint32_t *member, const uint32_t *sub_of, uint64_t sub_of_len,
                                             uint64_t q) {
    const uint32_t m = member[q];
    return m < sub_of_len ? sub_of[m] : GP_NONE;
}

__global__ __launch_bounds__(GS_BLOCK) void k_gp_count(uint32_t n_dests, const uint64_t *doff, uint64_t ecap,
                                                       const uint32_t *member, const uint32_t *sub_of,
                                                       uint64_t sub_of_len, uint32_t *gfix) {
    __shared__ uint32_t s_w[GS_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t c0, c1;
    gp_chunk(gp_e(doff, n_dests, ecap), blockIdx.x, c0, c1);
    uint32_t n = 0;
    for (uint64_t i0 = c0 + wv * 64; i0 < c1; i0 += GS_BLOCK) {   // (wave-uniform)
        const uint64_t i = i0 + lane;
        const bool f = i < c1 && gp_local(member, sub_of, sub_of_len, i) != GP_NONE;
        n += (uint32_t)__popcll(__ballot(f));
    }
    if (lane == 0) s_w[wv] = n;
    __syncthreads();
    if (tid == 0) gfix[GP_CNT + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];   // (every word, every call)
}

__global__ __launch_bounds__(1024) void k_gp_scan(const uint64_t *head, uint64_t cap, uint32_t *gfix) {
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t c = gfix[GP_CNT + tid];
    const uint32_t inc = gs_incl_scan32(c, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = inc - c;
    for (uint32_t w = 0; w < wv; w++) base += s_w[w];
    gfix[GP_CNT + tid] = base;
    if (tid == 1023) {
        const uint64_t P = (uint64_t)base + c;
        uint64_t *ph = reinterpret_cast<uint64_t *>(gfix + GP_PH), *mh = reinterpret_cast<uint64_t *>(gfix + GP_MH);
        ph[0] = 0;
        ph[1] = P;
        mh[0] = 0;
        mh[1] = gs_w(head, cap) + P;
    }
}

__global__ __launch_bounds__(GS_BLOCK) void k_gp_compact(uint32_t n_dests, const uint64_t *doff, uint64_t ecap,
                                                         const uint32_t *e_topic, const uint32_t *e_value,
                                                         const uint32_t *member, const uint32_t *sub_of,
                                                         uint64_t sub_of_len, const uint32_t *gfix, uint32_t *pt,
                                                         uint32_t *pv, uint32_t *ps) {
    __shared__ uint32_t s_w[GS_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t c0, c1;
    gp_chunk(gp_e(doff, n_dests, ecap), blockIdx.x, c0, c1);
    uint64_t base = gfix[GP_CNT + blockIdx.x];
    for (uint64_t t0 = c0; t0 < c1; t0 += GS_BLOCK) {   // (block-uniform)
        const uint64_t i = t0 + tid;
        const uint32_t ls = i < c1 ? gp_local(member, sub_of, sub_of_len, i) : GP_NONE;
        const bool f = ls != GP_NONE;
        const uint64_t m = __ballot(f);
        if (lane == 0) s_w[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint64_t at = base + gs_below(m, lane);
        uint32_t all = 0;
        for (uint32_t w = 0; w < GS_WAVES; w++) {
            if (w < wv) at += s_w[w];
            all += s_w[w];
        }
        if (f && at < ecap) {   // (at < P <= E <= ecap always)
            pt[at] = e_topic[i];
            pv[at] = e_value[i];
            ps[at] = ls;
        }
        base += all;
        __syncthreads();
    }
}

// the keys of k[0 .. n) (ascending) below x / at or below x
__device__ __forceinline__ uint64_t gp_lower(const uint32_t *k, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (k[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t gp_upper(const uint32_t *k, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (k[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(GS_BLOCK) void k_gp_merge(const uint64_t *head, uint64_t cap, const uint32_t *in_topic,
                                                       const uint32_t *in_value, const uint32_t *in_sub, uint64_t ecap,
                                                       GsBufs bufs, const uint32_t *gfix, const uint32_t *pt,
                                                       const uint32_t *pv, const uint32_t *ps, uint32_t *mt, uint32_t *mv,
                                                       uint32_t *ms, uint32_t *msrc) {
    const uint64_t W = gs_w(head, cap);
    uint64_t P = reinterpret_cast<const uint64_t *>(gfix + GP_PH)[1];
    if (P > ecap) P = ecap;   // (never)
    const uint64_t N = W + P;
    const uint32_t *k, *p;   // the picks' topic indices, sorted, and their ranks before the sort
    gs_source(bufs, pt, bufs.fix[GS_SRC + GS_PASSES], k, p);
    for (uint64_t i = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < N; i += (uint64_t)GS_GRID * GS_BLOCK) {
        uint64_t d;
        uint32_t t, v, s, src;
        if (i < W) {
            t = in_topic[i];
            v = in_value[i];
            s = in_sub[i];
            src = (uint32_t)i;
            d = i + gp_lower(k, P, t);
        } else {
            const uint64_t r = i - W;
            uint32_t pos = p ? p[r] : (uint32_t)r;
            if (pos >= P) pos = 0;   // (never: a permutation of [0, P))
            t = k[r];
            v = pv[pos];
            s = ps[pos];
            src = (uint32_t)(W + pos);
            d = r + gp_upper(in_topic, W, t);
        }
        if (d < N) {   // (always)
            mt[d] = t;
            mv[d] = v;
            ms[d] = s;
            msrc[d] = src;
        }
    }
}

// k_gs_emit over the merged arrays (head = [0, N]): only positions below out_cap are written, out_src
// names the input through the merged src
__global__ __launch_bounds__(GS_BLOCK) void k_gp_emit(const uint64_t *head, uint64_t cap, const uint32_t *mt,
                                                      const uint32_t *mv, const uint32_t *ms, const uint32_t *msrc,
                                                      GsBufs bufs, uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap,
                                                      uint32_t *out_topic, uint32_t *out_value, uint32_t *out_sub,
                                                      uint32_t *out_src, uint64_t out_cap) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t N = gs_w(head, cap);
    uint64_t c0, c1, q;
    gs_chunk(N, blockIdx.x, c0, c1, q);
    const uint32_t *k, *p;
    gs_source(bufs, ms, bufs.fix[GS_SRC + GS_PASSES], k, p);
    const uint64_t w0 = c0 + wv * q < c1 ? c0 + wv * q : c1, w1 = w0 + q < c1 ? w0 + q : c1;
    uint64_t g0 = bufs.fix[GS_GCNT + blockIdx.x * GS_WAVES + wv];   // groups that start before w0
    for (uint64_t i0 = w0; i0 < w1; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool ok = i < w1;
        const uint32_t key = ok ? k[i] : 0u;
        const uint32_t pos = !ok ? 0u : p ? p[i] : (uint32_t)i;
        const bool h = ok && gs_is_head(k, i, key);
        const uint64_t hm = __ballot(h);
        if (h) {
            const uint64_t g = g0 + gs_below(hm, lane);
            if (g < gcap) out_gsub[g] = key;
            if (g <= gcap) out_goff[g] = i;   // (g == gcap < G: where the first group left out starts)
        }
        g0 += (uint32_t)__popcll(hm);
        if (ok && pos < N && i < out_cap) {   // (pos < N always)
            out_topic[i] = mt[pos];
            out_value[i] = mv[pos];
            out_sub[i] = key;
            if (out_src) out_src[i] = msrc[pos];
        }
    }
}

// ---- a micro-batch's grouping in ONE workgroup (tm_deliver_batch32), queued
// behind k_dp_one, which under a grouping request writes its deliveries and
// its head to the lane (in_t / in_v / in_s, head) and not to the caller.
//   gate   st_in is the status block k_dp_one itself read (k_fo_one's, under
//          aggre k_ag_one's, in device memory); with FO1_DONE there k_dp_one
//          left head = [M, T], which goes on to the caller's out_head, and
//          expanded the deliveries exactly when T <= dp1_max (the same value
//          both kernels are given, at most GS1_DELIVERIES).  Anything else:
//          GS1_SKIPPED and nothing more, the host takes the grid kernels.
//          The run that queued the kernel may be run again (a value scratch
//          that grew, a look-back retry).  k_sh_one gates itself against that
//          because it moves the slots' state; the grouping moves no state, so
//          a second run would simply write the same outputs again.  (Today a
//          run that is queued again never gets as far as grouping: the lane's
//          first value scratch holds 65,536 values or more, a total above it
//          is more than FO1_ENTRIES entries, so both runs end FO1_TOO_LARGE
//          and the kernel writes GS1_SKIPPED twice; the pairs walk has no
//          look-back to retry.)
//   sort   the W = min(T, dcap) subscriber ids in s_key, their positions as
//          16 bits in s_ix[0]; a block-wide AND and OR of the keys tell which
//          of the four digits every key agrees on (skipped: the grid form's
//          rule, k_gs_plan); per digit left a stable LSD pass between the two
//          index arrays: a row of 256 bins per wave, the rows scanned over the
//          waves and then the bins, and a scatter in which the lanes of a step
//          with the same digit rank themselves by a peer mask.
//          This is k_sh_one's pass (tm_share.hip).  It is a copy, not a shared
//          helper: lifting it would change k_sh_one's code, whose register
//          allocation (and zero scratch) was measured as it stands, and the
//          pass here runs on whole keys and a digit chosen at run time.
//   heads  position p is a head when its key differs from its predecessor's;
//          a ballot and popcount per step, the counts scanned over the waves;
//          head g < gcap gives out_gsub[g], g <= gcap out_goff[g].
//   out    out_ds[p] from LDS, out_dt[p] / out_dv[p] gathered from the lane's
//          arrays through the position; consecutive threads write consecutive
//          words of mapped host memory that is never read.
// status (mapped host memory): GS1_ST_* (tm_dev.h).  LDS: 64 KiB keys + 2 x 32
// KiB indices + 16 KiB bins + 88 B.
constexpr uint32_t GS1_WAVES = FO1_BLOCK / 64;
constexpr uint32_t GS1_STEPS = GS1_DELIVERIES / FO1_BLOCK;   // 64-position steps of a wave, at most
static_assert(GS1_DELIVERIES <= 0x10000u, "k_gs_one: positions are staged as 16 bits");
static_assert(GS1_DELIVERIES % FO1_BLOCK == 0 && GS_BINS <= FO1_BLOCK && GS_BINS % 64 == 0,
              "k_gs_one: whole steps per wave, one thread per bin");

__device__ __forceinline__ void gs1_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(FO1_BLOCK) void k_gs_one(const uint32_t *__restrict__ st_in, const uint64_t *__restrict__ head,
                                                      const uint32_t *__restrict__ in_t, const uint32_t *__restrict__ in_v,
                                                      const uint32_t *__restrict__ in_s, uint64_t dcap, uint64_t dp1_max,
                                                      uint64_t *__restrict__ out_head, uint32_t *__restrict__ out_dt,
                                                      uint32_t *__restrict__ out_dv, uint32_t *__restrict__ out_ds,
                                                      uint64_t *__restrict__ out_ghead, uint32_t *__restrict__ out_gsub,
                                                      uint32_t *__restrict__ out_goff, uint64_t gcap,
                                                      uint32_t *__restrict__ status) {
    __shared__ uint32_t s_key[GS1_DELIVERIES];
    __shared__ __attribute__((aligned(4))) uint16_t s_ix[2][GS1_DELIVERIES];
    __shared__ uint32_t s_h[GS1_WAVES * GS_BINS];
    __shared__ uint32_t s_wt[GS1_WAVES];
    __shared__ uint32_t s_bw[GS_BINS / 64];
    __shared__ uint32_t s_red[2];   // the AND and the OR of the keys
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (st_in[FO1_ST_STATE] != FO1_DONE) {   // (block-uniform) k_dp_one wrote nothing: the head is an older run's
        if (tid == 0) status[GS1_ST_STATE] = GS1_SKIPPED;
        return;
    }
    const uint64_t M = head[0], T = head[1];
    if (tid == 0) {
        out_head[0] = M;
        out_head[1] = T;
    }
    if (T > dp1_max || T > GS1_DELIVERIES) {   // (block-uniform) DP1_TOO_LARGE: no deliveries on the lane
        if (tid == 0) status[GS1_ST_STATE] = GS1_SKIPPED;
        return;
    }
    const uint32_t W = T < dcap ? (uint32_t)T : (uint32_t)dcap;   // (<= GS1_DELIVERIES)
    if (tid == 0) {
        s_red[0] = 0xFFFFFFFFu;
        s_red[1] = 0;
    }
    __syncthreads();
    // ---- the keys and the positions 0, 1, ..
    uint32_t k_and = 0xFFFFFFFFu, k_or = 0;
    for (uint32_t i = tid; i < W; i += FO1_BLOCK) {
        const uint32_t key = in_s[i];
        s_key[i] = key;
        s_ix[0][i] = (uint16_t)i;
        k_and &= key;
        k_or |= key;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        k_and &= __shfl_xor(k_and, d, 64);
        k_or |= __shfl_xor(k_or, d, 64);
    }
    if (lane == 0) {
        atomicAnd(&s_red[0], k_and);
        atomicOr(&s_red[1], k_or);
    }
    __syncthreads();
    const uint32_t diff = W ? s_red[0] ^ s_red[1] : 0u;   // bits on which two keys differ (no key: none)
    // ---- sorted by key.  Wave w owns the positions [w * D, (w + 1) * D) of [0, W)
    const uint32_t D = ((W + GS1_WAVES - 1) / GS1_WAVES + 63) & ~63u;   // (<= 64 * GS1_STEPS)
    const uint32_t d0 = wv * D < W ? wv * D : W, d1 = d0 + D < W ? d0 + D : W;
    uint32_t *my_h = s_h + wv * GS_BINS;
    uint32_t cur = 0, run = 0;
    for (uint32_t pass = 0, shift = 0; pass < GS_PASSES; pass++, shift += 8) {   // (block-uniform)
        if (!((diff >> shift) & (GS_BINS - 1))) continue;                         // every key in one bin: the identity
        run++;
        const uint16_t *src = s_ix[cur];
        uint16_t *dst_ix = s_ix[cur ^ 1];
        for (uint32_t i = tid; i < GS1_WAVES * GS_BINS; i += FO1_BLOCK) s_h[i] = 0;
        __syncthreads();
        for (uint32_t p0 = d0; p0 < d1; p0 += 64) {
            const uint32_t p = p0 + lane;
            if (p < d1) atomicAdd(&my_h[(s_key[src[p]] >> shift) & (GS_BINS - 1)], 1u);
        }
        __syncthreads();
        // bin b: its counts' exclusive scan over the waves, then over the bins
        uint32_t tot = 0;
        if (tid < GS_BINS)
            for (uint32_t q = 0; q < GS1_WAVES; q++) {
                const uint32_t x = s_h[q * GS_BINS + tid];
                s_h[q * GS_BINS + tid] = tot;
                tot += x;
            }
        const uint32_t binc = gs_incl_scan32(tot, lane);
        if (tid < GS_BINS && lane == 63) s_bw[wv] = binc;
        __syncthreads();
        if (tid < GS_BINS) {
            uint32_t exc = binc - tot;
            for (uint32_t q = 0; q < wv; q++) exc += s_bw[q];
            for (uint32_t q = 0; q < GS1_WAVES; q++) s_h[q * GS_BINS + tid] += exc;
        }
        __syncthreads();
        // the stable scatter: waves, steps and lanes are in position order
        for (uint32_t p0 = d0; p0 < d1; p0 += 64) {   // (wave-uniform)
            const uint32_t p = p0 + lane;
            const bool ok = p < d1;
            const uint32_t ix = ok ? src[p] : 0u;
            const uint32_t d = ok ? (s_key[ix] >> shift) & (GS_BINS - 1) : 0u;
            const uint64_t peers = gs_match(d, ok);
            uint32_t dst = 0;
            if (ok) dst = my_h[d] + gs_below(peers, lane);
            gs1_wave_sync();
            if (ok && (peers >> lane) == 1ull) my_h[d] += (uint32_t)__popcll(peers);   // (the run's last lane)
            gs1_wave_sync();
            if (ok && dst < W) dst_ix[dst] = (uint16_t)ix;   // (dst < W always: the histogram saw these keys)
        }
        __syncthreads();
        cur ^= 1;
    }
    // ---- heads.  I: the positions by (key, position)
    const uint16_t *I = s_ix[cur];
    uint32_t n_heads = 0;
    for (uint32_t p0 = d0; p0 < d1; p0 += 64) {   // (wave-uniform)
        const uint32_t p = p0 + lane;
        const bool h = p < d1 && (p == 0 || s_key[I[p - 1]] != s_key[I[p]]);
        n_heads += (uint32_t)__popcll(__ballot(h));
    }
    if (lane == 0) s_wt[wv] = n_heads;
    __syncthreads();
    uint32_t g0 = 0, G = 0;
    for (uint32_t q = 0; q < GS1_WAVES; q++) {
        if (q < wv) g0 += s_wt[q];
        G += s_wt[q];
    }
    // ---- the groups and the payload
#pragma unroll 4
    for (uint32_t k = 0; k < GS1_STEPS; k++) {
        if (k * 64 >= D) break;   // (block-uniform)
        const uint32_t p = d0 + k * 64 + lane;
        const bool ok = p < d1;
        uint32_t pos = ok ? I[p] : 0u;
        if (pos >= W) pos = 0;    // (never: I is a permutation of [0, W))
        const uint32_t key = ok ? s_key[pos] : 0u;
        const bool h = ok && (p == 0 || s_key[I[p - 1]] != key);
        const uint64_t hm = __ballot(h);
        if (h) {
            const uint64_t g = (uint64_t)g0 + gs_below(hm, lane);
            if (g < gcap) out_gsub[g] = key;
            if (g <= gcap) out_goff[g] = p;   // (g == gcap < G: where the first group left out starts)
        }
        g0 += (uint32_t)__popcll(hm);
        if (ok) {
            out_dt[p] = in_t[pos];
            out_dv[p] = in_v[pos];
            out_ds[p] = key;
        }
    }
    if (tid == 0) {
        if (G <= gcap) out_goff[G] = W;
        out_ghead[0] = G;
        out_ghead[1] = W;
        status[GS1_ST_RUN] = run;
        status[GS1_ST_SKIPPED] = GS_PASSES - run;
        status[GS1_ST_G] = G;
        status[GS1_ST_STATE] = GS1_GROUPED;
    }
}

// ---- a micro-batch's picks merged with its deliveries and grouped in ONE
// workgroup (tm_publish_deliver_batch32), queued behind k_dp_one (deliveries
// and head on the lane, as under k_gs_one), k_pd_gate and k_sh_one.
//   k_pd_gate  one wave, one thread at work.  The run that queued the kernels
//          may be run again (a value scratch that grew, a look-back retry) and
//          the pick moves state, so whether the run stands is decided once, on
//          the device, and written to one device word: k_sh_one is given that
//          word as its fail word and k_gp_one reads it, so the pick is made
//          exactly when the merge runs.  Go: k_sh_one's own conditions and T <=
//          tmax, T + K <= min(dcap, nmax).  With FO1_DONE in st_in the lane's
//          head = [M, T] goes on to the caller's out_head whatever follows.
//   k_gp_one
//   copy   member[0 .. K) from the lane to the caller's out_member.
//   stage  source code c names delivery c (c < T) or T + the compact rank of a
//          local pick: s_key[c] its subscriber id, s_msg[c] its message (16
//          bits: a message index is below FO1_TOPICS), s_pq[r] the entry
//          position of rank r.  The local picks (sub_of[member[q]] != NONE) are
//          counted per wave, the counts scanned over the waves, and compacted
//          in ascending entry position (a ballot and popcount per step).
//   picks  the P ranks sorted stably by message: the digit pass below over the
//          two low digits, one all picks agree on skipped.
//   merge  delivery p goes to p + the picks with a message < t_p, the pick of
//          sorted rank r to r + the deliveries with a message <= t_r: binary
//          searches over s_msg.  Only codes move: the merged order is one of the
//          two index arrays, the sort below looks keys up through the code.
//   sort   the N = T + P codes stably by s_key: k_gs_one's pass, a copy for
//          the reason given above k_gs_one (gp1_pass; k_gs_one keeps its own).
//   out    heads, groups and the payload as k_gs_one; topic from s_msg, value
//          gathered from the lane's deliveries or the entries through s_pq.
// LDS: 32 KiB keys + 2 x 16 KiB codes + 16 KiB messages + 16 KiB entry
// positions + 16 KiB bins + 96 B.  With 16384 codes the same layout takes 208
// KiB of the CU's 160: the limit is 8192 (the assertions below).
constexpr uint32_t GP1_WAVES = FO1_BLOCK / 64;
constexpr uint64_t GP1_LDS_MAX = 160 * 1024;
constexpr uint64_t gp1_lds(uint64_t codes) {
    return codes * 4 + 2 * codes * 2 + codes * 2 + codes * 2 + GP1_WAVES * GS_BINS * 4 + GP1_WAVES * 4 + GS_BINS / 64 * 4 + 4 * 4;
}
static_assert(gp1_lds(GP1_DELIVERIES) <= GP1_LDS_MAX, "k_gp_one: the staged codes must fit the CU's LDS");
static_assert(gp1_lds(2 * GP1_DELIVERIES) > GP1_LDS_MAX, "k_gp_one: twice the codes would fit: raise GP1_DELIVERIES");
static_assert(GP1_DELIVERIES <= 0x10000u && FO1_ENTRIES <= 0x10000u && FO1_TOPICS <= 0x10000u,
              "k_gp_one: codes, entry positions and messages are staged as 16 bits");
static_assert(GP1_DELIVERIES <= GS1_DELIVERIES, "k_gp_one reads the lane arrays k_gs_one's request sizes");

__global__ __launch_bounds__(64) void k_pd_gate(const uint32_t *__restrict__ st_in, const uint64_t *__restrict__ head,
                                                const uint32_t *__restrict__ doff, uint32_t n_dests,
                                                const uint32_t *fail, uint64_t vcap, uint64_t cap, uint64_t dcap,
                                                uint64_t tmax, uint64_t nmax, uint64_t *__restrict__ out_head,
                                                uint32_t *__restrict__ gate, uint32_t *__restrict__ status) {
    if (threadIdx.x) return;
    const uint32_t state = st_in[FO1_ST_STATE], total = st_in[FO1_ST_TOTAL];
    uint32_t reason = PD1_R_NONE, t32 = 0, k32 = 0;
    if (state != FO1_DONE || n_dests > FO1_MAX_DESTS) {
        reason = PD1_R_STATE;   // k_dp_one wrote nothing: the head is an older run's
    } else {
        const uint64_t M = head[0], T = head[1];
        const uint64_t K = doff[n_dests + 1];
        const uint32_t failed = fail ? __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
        out_head[0] = M;
        out_head[1] = T;
        t32 = T > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)T;
        k32 = (uint32_t)K;
        if (total > vcap) reason = PD1_R_VCAP;
        else if (failed) reason = PD1_R_FAIL;
        else if (total > cap) reason = PD1_R_CAP;
        else if (T + K > dcap) reason = PD1_R_DCAP;
        else if (T > tmax || T + K > nmax || K > FO1_ENTRIES) reason = PD1_R_LARGE;
    }
    *gate = reason;
    status[PD1_ST_REASON] = reason;
    status[PD1_ST_T] = t32;
    status[PD1_ST_K] = k32;
    status[PD1_ST_STATE] = reason == PD1_R_NONE ? PD1_GO : PD1_SKIP;
}

// One stable 8-bit LSD pass of the codes src[0 .. n) into dst by (keys[code] >> shift) & 255: wave w owns
// the positions [w * D, (w + 1) * D); a row of bins per wave, scanned over the waves and then the bins; in
// the scatter the lanes of a step with the same digit rank themselves by a peer mask (k_gs_one's pass)
template <class Key>
__device__ __forceinline__ void gp1_pass(const Key *keys, const uint16_t *src, uint16_t *dst, uint32_t n, uint32_t shift,
                                         uint32_t *s_h, uint32_t *s_bw, uint32_t tid, uint32_t lane, uint32_t wv) {
    const uint32_t D = ((n + GP1_WAVES - 1) / GP1_WAVES + 63) & ~63u;
    const uint32_t d0 = wv * D < n ? wv * D : n, d1 = d0 + D < n ? d0 + D : n;
    uint32_t *my_h = s_h + wv * GS_BINS;
    for (uint32_t i = tid; i < GP1_WAVES * GS_BINS; i += FO1_BLOCK) s_h[i] = 0;
    __syncthreads();
    for (uint32_t p0 = d0; p0 < d1; p0 += 64) {
        const uint32_t p = p0 + lane;
        if (p < d1) atomicAdd(&my_h[((uint32_t)keys[src[p]] >> shift) & (GS_BINS - 1)], 1u);
    }
    __syncthreads();
    uint32_t tot = 0;
    if (tid < GS_BINS)
        for (uint32_t q = 0; q < GP1_WAVES; q++) {
            const uint32_t x = s_h[q * GS_BINS + tid];
            s_h[q * GS_BINS + tid] = tot;
            tot += x;
        }
    const uint32_t binc = gs_incl_scan32(tot, lane);
    if (tid < GS_BINS && lane == 63) s_bw[wv] = binc;
    __syncthreads();
    if (tid < GS_BINS) {
        uint32_t exc = binc - tot;
        for (uint32_t q = 0; q < wv; q++) exc += s_bw[q];
        for (uint32_t q = 0; q < GP1_WAVES; q++) s_h[q * GS_BINS + tid] += exc;
    }
    __syncthreads();
    for (uint32_t p0 = d0; p0 < d1; p0 += 64) {   // (wave-uniform)
        const uint32_t p = p0 + lane;
        const bool ok = p < d1;
        const uint32_t ix = ok ? src[p] : 0u;
        const uint32_t d = ok ? ((uint32_t)keys[ix] >> shift) & (GS_BINS - 1) : 0u;
        const uint64_t peers = gs_match(d, ok);
        uint32_t at = 0;
        if (ok) at = my_h[d] + gs_below(peers, lane);
        gs1_wave_sync();
        if (ok && (peers >> lane) == 1ull) my_h[d] += (uint32_t)__popcll(peers);   // (the run's last lane)
        gs1_wave_sync();
        if (ok && at < n) dst[at] = (uint16_t)ix;   // (at < n always: the histogram saw these keys)
    }
    __syncthreads();
}

__global__ __launch_bounds__(FO1_BLOCK) void k_gp_one(
    const uint32_t *__restrict__ gate, const uint64_t *__restrict__ head, const uint32_t *__restrict__ in_t,
    const uint32_t *__restrict__ in_v, const uint32_t *__restrict__ in_s, const uint32_t *__restrict__ doff,
    uint32_t n_dests, const uint32_t *__restrict__ e_t, const uint32_t *__restrict__ e_v,
    const uint32_t *__restrict__ member, const uint32_t *__restrict__ sub_of, uint64_t sub_of_len, uint64_t cap,
    uint64_t dcap, uint32_t *__restrict__ out_member, uint32_t *__restrict__ out_dt, uint32_t *__restrict__ out_dv,
    uint32_t *__restrict__ out_ds, uint64_t *__restrict__ out_ghead, uint32_t *__restrict__ out_gsub,
    uint32_t *__restrict__ out_goff, uint64_t gcap, uint32_t *__restrict__ status) {
    __shared__ uint32_t s_key[GP1_DELIVERIES];
    __shared__ __attribute__((aligned(4))) uint16_t s_ix[2][GP1_DELIVERIES];
    __shared__ __attribute__((aligned(4))) uint16_t s_msg[GP1_DELIVERIES];
    __shared__ __attribute__((aligned(4))) uint16_t s_pq[GP1_DELIVERIES];
    __shared__ uint32_t s_h[GP1_WAVES * GS_BINS];
    __shared__ uint32_t s_wt[GP1_WAVES];
    __shared__ uint32_t s_bw[GS_BINS / 64];
    __shared__ uint32_t s_red[4];   // the AND and the OR of the picks' messages, of all keys
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (*gate != 0) {   // (block-uniform) the run does not stand, or not in one workgroup: no pick was made
        if (tid == 0) status[GP1_ST_STATE] = GP1_SKIPPED;
        return;
    }
    uint32_t T = head[1] < GP1_DELIVERIES ? (uint32_t)head[1] : GP1_DELIVERIES;   // (the gate: T + K <= GP1_DELIVERIES)
    uint32_t K = doff[n_dests + 1];
    if (K > cap) K = (uint32_t)cap;                      // (never: K <= total <= cap)
    if (K > GP1_DELIVERIES - T) K = GP1_DELIVERIES - T;   // (never)
    if (tid == 0) {
        s_red[0] = s_red[2] = 0xFFFFFFFFu;
        s_red[1] = s_red[3] = 0;
    }
    // ---- the picks to the caller
    for (uint32_t i = tid; i < K; i += FO1_BLOCK) out_member[i] = member[i];
    // ---- the deliveries' keys and messages
    uint32_t k_and = 0xFFFFFFFFu, k_or = 0, m_and = 0xFFFFFFFFu, m_or = 0;
    for (uint32_t i = tid; i < T; i += FO1_BLOCK) {
        const uint32_t key = in_s[i];
        s_key[i] = key;
        s_msg[i] = (uint16_t)in_t[i];
        k_and &= key;
        k_or |= key;
    }
    // ---- the local picks, counted and compacted in ascending entry position
    const uint32_t C = ((K + GP1_WAVES - 1) / GP1_WAVES + 63) & ~63u;
    const uint32_t c0 = wv * C < K ? wv * C : K, c1 = c0 + C < K ? c0 + C : K;
    uint32_t n_loc = 0;
    for (uint32_t q0 = c0; q0 < c1; q0 += 64) {   // (wave-uniform)
        const uint32_t q = q0 + lane;
        const bool f = q < c1 && gp_local(member, sub_of, sub_of_len, q) != GP_NONE;
        n_loc += (uint32_t)__popcll(__ballot(f));
    }
    if (lane == 0) s_wt[wv] = n_loc;
    __syncthreads();
    uint32_t base = 0, P = 0;
    for (uint32_t q = 0; q < GP1_WAVES; q++) {
        if (q < wv) base += s_wt[q];
        P += s_wt[q];
    }
    const uint32_t N = T + P;   // (<= GP1_DELIVERIES: P <= K)
    for (uint32_t q0 = c0; q0 < c1; q0 += 64) {   // (wave-uniform)
        const uint32_t q = q0 + lane;
        const uint32_t ls = q < c1 ? gp_local(member, sub_of, sub_of_len, q) : GP_NONE;
        const bool f = ls != GP_NONE;
        const uint64_t m = __ballot(f);
        const uint32_t r = base + gs_below(m, lane);
        if (f && r < P) {   // (r < P always: the count above saw these entries)
            const uint32_t t = e_t[q];
            s_key[T + r] = ls;
            s_msg[T + r] = (uint16_t)t;
            s_pq[r] = (uint16_t)q;
            s_ix[0][r] = (uint16_t)r;
            k_and &= ls;
            k_or |= ls;
            m_and &= t;
            m_or |= t;
        }
        base += (uint32_t)__popcll(m);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        k_and &= __shfl_xor(k_and, d, 64);
        k_or |= __shfl_xor(k_or, d, 64);
        m_and &= __shfl_xor(m_and, d, 64);
        m_or |= __shfl_xor(m_or, d, 64);
    }
    if (lane == 0) {
        atomicAnd(&s_red[0], m_and);
        atomicOr(&s_red[1], m_or);
        atomicAnd(&s_red[2], k_and);
        atomicOr(&s_red[3], k_or);
    }
    __syncthreads();
    const uint32_t mdiff = P ? (s_red[0] ^ s_red[1]) & 0xFFFFu : 0u;   // bits on which two picks' messages differ
    const uint32_t diff = N ? s_red[2] ^ s_red[3] : 0u;                // on which two keys differ
    // ---- the picks by message
    uint32_t cur = 0, run = 0;
    for (uint32_t shift = 0; shift < 16; shift += 8) {   // (block-uniform)
        if (!((mdiff >> shift) & (GS_BINS - 1))) continue;
        run++;
        gp1_pass(s_msg + T, s_ix[cur], s_ix[cur ^ 1], P, shift, s_h, s_bw, tid, lane, wv);
        cur ^= 1;
    }
    // ---- merged by message into the other index array
    {
        const uint16_t *R = s_ix[cur];
        uint16_t *Mg = s_ix[cur ^ 1];
        for (uint32_t i = tid; i < N; i += FO1_BLOCK) {
            uint32_t lo = 0, code;
            if (i < T) {   // the picks with a message below mine
                const uint32_t t = s_msg[i];
                uint32_t hi = P;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_msg[T + R[mid]] < t) lo = mid + 1;
                    else hi = mid;
                }
                code = i;
                lo += i;
            } else {       // the deliveries with a message at or below mine
                const uint32_t r = i - T, c = R[r];
                const uint32_t t = s_msg[T + c];
                uint32_t hi = T;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_msg[mid] <= t) lo = mid + 1;
                    else hi = mid;
                }
                code = T + c;
                lo += r;
            }
            if (lo < N) Mg[lo] = (uint16_t)code;   // (always: a permutation of [0, N))
        }
        cur ^= 1;
    }
    __syncthreads();
    // ---- the merged codes by subscriber
    for (uint32_t pass = 0, shift = 0; pass < GS_PASSES; pass++, shift += 8) {   // (block-uniform)
        if (!((diff >> shift) & (GS_BINS - 1))) continue;
        run++;
        gp1_pass(s_key, s_ix[cur], s_ix[cur ^ 1], N, shift, s_h, s_bw, tid, lane, wv);
        cur ^= 1;
    }
    // ---- heads, groups and the payload
    const uint16_t *I = s_ix[cur];
    const uint32_t D = ((N + GP1_WAVES - 1) / GP1_WAVES + 63) & ~63u;
    const uint32_t d0 = wv * D < N ? wv * D : N, d1 = d0 + D < N ? d0 + D : N;
    uint32_t n_heads = 0;
    for (uint32_t p0 = d0; p0 < d1; p0 += 64) {   // (wave-uniform)
        const uint32_t p = p0 + lane;
        const bool h = p < d1 && (p == 0 || s_key[I[p - 1]] != s_key[I[p]]);
        n_heads += (uint32_t)__popcll(__ballot(h));
    }
    if (lane == 0) s_wt[wv] = n_heads;   // (the compaction's counts were read before the barriers above)
    __syncthreads();
    uint32_t g0 = 0, G = 0;
    for (uint32_t q = 0; q < GP1_WAVES; q++) {
        if (q < wv) g0 += s_wt[q];
        G += s_wt[q];
    }
    for (uint32_t p0 = d0; p0 < d1; p0 += 64) {   // (wave-uniform)
        const uint32_t p = p0 + lane;
        const bool ok = p < d1;
        uint32_t code = ok ? I[p] : 0u;
        if (code >= N) code = 0;   // (never: I is a permutation of [0, N))
        const uint32_t key = ok ? s_key[code] : 0u;
        const bool h = ok && (p == 0 || s_key[I[p - 1]] != key);
        const uint64_t hm = __ballot(h);
        if (h) {
            const uint64_t g = (uint64_t)g0 + gs_below(hm, lane);
            if (g < gcap) out_gsub[g] = key;
            if (g <= gcap) out_goff[g] = p;   // (g == gcap < G: where the first group left out starts)
        }
        g0 += (uint32_t)__popcll(hm);
        if (ok && p < dcap) {   // (p < dcap always: the gate)
            out_dt[p] = s_msg[code];
            out_dv[p] = code < T ? in_v[code] : e_v[s_pq[code - T]];
            out_ds[p] = key;
        }
    }
    if (tid == 0) {
        if (G <= gcap) out_goff[G] = N;
        out_ghead[0] = G;
        out_ghead[1] = N;
        status[GP1_ST_RUN] = run;
        status[GP1_ST_SKIPPED] = 2 * GS_PASSES - run;
        status[GP1_ST_G] = G;
        status[GP1_ST_P] = P;
        status[GP1_ST_N] = N;
        status[GP1_ST_STATE] = GP1_GROUPED;
    }
}

}  // namespace

hipError_t launch_pd_gate(const uint32_t *status_in, const uint64_t *head, const uint32_t *dest_offsets, uint32_t n_dests,
                          const uint32_t *fail, uint64_t vcap, uint64_t cap, uint64_t dcap, uint64_t tmax, uint64_t nmax,
                          uint64_t *out_head, uint32_t *gate, uint32_t *status, hipStream_t s) {
    if (!status_in || !head || !dest_offsets || !out_head || !gate || !status || !n_dests || n_dests > FO1_MAX_DESTS ||
        (((uintptr_t)head | (uintptr_t)out_head) & 7))
        return hipErrorInvalidValue;
    if (tmax > GP1_DELIVERIES) tmax = GP1_DELIVERIES;
    if (nmax > GP1_DELIVERIES) nmax = GP1_DELIVERIES;
    hipLaunchKernelGGL(k_pd_gate, dim3(1), dim3(64), 0, s, status_in, head, dest_offsets, n_dests, fail, vcap, cap, dcap,
                       tmax, nmax, out_head, gate, status);
    return hipGetLastError();
}

hipError_t launch_group_picks_one(const uint32_t *gate, const uint64_t *head, const uint32_t *in_topic,
                                  const uint32_t *in_value, const uint32_t *in_sub, const uint32_t *dest_offsets,
                                  uint32_t n_dests, const uint32_t *e_topic, const uint32_t *e_value, const uint32_t *member,
                                  const uint32_t *sub_of, uint64_t sub_of_len, uint64_t cap, uint64_t dcap,
                                  uint32_t *out_member, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                                  uint64_t *out_ghead, uint32_t *out_gsub, uint32_t *out_goff, uint64_t gcap,
                                  uint32_t *status, hipStream_t s) {
    if (!gate || !head || !dest_offsets || !out_ghead || !out_goff || !status || !n_dests || n_dests > FO1_MAX_DESTS ||
        (((uintptr_t)head | (uintptr_t)out_ghead) & 7))
        return hipErrorInvalidValue;
    if (!sub_of) sub_of_len = 0;
    if (sub_of_len > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (cap > FO1_ENTRIES) cap = FO1_ENTRIES;
    if (dcap > GP1_DELIVERIES) dcap = GP1_DELIVERIES;
    if (!in_topic || !in_value || !in_sub || !e_topic || !e_value || !member ||
        (cap && !out_member) || (dcap && (!out_dtopic || !out_dvalue || !out_dsub)) || (gcap && !out_gsub))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gp_one, dim3(1), dim3(FO1_BLOCK), 0, s, gate, head, in_topic, in_value, in_sub, dest_offsets,
                       n_dests, e_topic, e_value, member, sub_of, sub_of_len, cap, dcap, out_member, out_dtopic,
                       out_dvalue, out_dsub, out_ghead, out_gsub, out_goff, gcap, status);
    return hipGetLastError();
}

hipError_t launch_group_one(const uint32_t *status_in, const uint64_t *head, const uint32_t *in_topic,
                            const uint32_t *in_value, const uint32_t *in_sub, uint64_t dcap, uint64_t dp1_max,
                            uint64_t *out_head, uint32_t *out_dtopic, uint32_t *out_dvalue, uint32_t *out_dsub,
                            uint64_t *out_ghead, uint32_t *out_gsub, uint32_t *out_goff, uint64_t gcap, uint32_t *status,
                            hipStream_t s) {
    if (!status_in || !head || !out_head || !out_ghead || !out_goff || !status ||
        (((uintptr_t)head | (uintptr_t)out_head | (uintptr_t)out_ghead) & 7))
        return hipErrorInvalidValue;
    if (dcap > GS1_DELIVERIES) dcap = GS1_DELIVERIES;
    if (dp1_max > GS1_DELIVERIES) dp1_max = GS1_DELIVERIES;
    if ((dcap && (!in_topic || !in_value || !in_sub || !out_dtopic || !out_dvalue || !out_dsub)) || (gcap && !out_gsub))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gs_one, dim3(1), dim3(FO1_BLOCK), 0, s, status_in, head, in_topic, in_value, in_sub, dcap, dp1_max,
                       out_head, out_dtopic, out_dvalue, out_dsub, out_ghead, out_gsub, out_goff, gcap, status);
    return hipGetLastError();
}

hipError_t launch_group_subs(const FanoutScratch &fs, const uint64_t *head, const uint32_t *in_topic,
                             const uint32_t *in_value, const uint32_t *in_sub, uint64_t cap, uint64_t *ghead,
                             uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap, uint32_t *out_topic,
                             uint32_t *out_value, uint32_t *out_sub, uint32_t *out_perm, hipStream_t s) {
    if (!head || !ghead || !out_goff || (((uintptr_t)head | (uintptr_t)ghead | (uintptr_t)out_goff) & 7))
        return hipErrorInvalidValue;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (!fs.gs_fix || cap > fs.gs_cap || (cap && (!fs.gs_k[0] || !in_topic || !in_value || !in_sub || !out_topic ||
                                                   !out_value || !out_sub)) || (gcap && !out_gsub))
        return hipErrorInvalidValue;
    const GsBufs b{fs.gs_fix, {fs.gs_k[0], fs.gs_k[1]}, {fs.gs_p[0], fs.gs_p[1]}};
    const dim3 g(GS_GRID), t(GS_BLOCK), one(1), wide(1024);
    hipLaunchKernelGGL(k_gs_pre, g, t, 0, s, head, cap, in_sub, b.fix);
    hipLaunchKernelGGL(k_gs_plan, one, wide, 0, s, head, cap, b.fix);
    for (uint32_t p = 0; p < GS_PASSES; p++) {
        hipLaunchKernelGGL(k_gs_hist, g, t, 0, s, head, cap, in_sub, b, p);
        hipLaunchKernelGGL(k_gs_scan, dim3(GS_BINS), t, 0, s, head, cap, b.fix, p);
        hipLaunchKernelGGL(k_gs_scatter, g, t, 0, s, head, cap, in_sub, b, p);
    }
    hipLaunchKernelGGL(k_gs_heads, g, t, 0, s, head, cap, in_sub, b);
    hipLaunchKernelGGL(k_gs_gscan, one, wide, 0, s, head, cap, b.fix, ghead, out_goff, gcap);
    hipLaunchKernelGGL(k_gs_emit, g, t, 0, s, head, cap, in_topic, in_value, in_sub, b, out_gsub, out_goff, gcap,
                       out_topic, out_value, out_sub, out_perm);
    return hipGetLastError();
}

hipError_t launch_group_picks(const FanoutScratch &fs, const uint64_t *head, const uint32_t *in_topic,
                              const uint32_t *in_value, const uint32_t *in_sub, uint64_t cap, uint32_t n_dests,
                              const uint64_t *dest_offsets, const uint32_t *e_topic, const uint32_t *e_value,
                              const uint32_t *member, uint64_t ecap, const uint32_t *sub_of, uint64_t sub_of_len,
                              uint64_t *ghead, uint32_t *out_gsub, uint64_t *out_goff, uint64_t gcap, uint32_t *out_topic,
                              uint32_t *out_value, uint32_t *out_sub, uint32_t *out_src, uint64_t out_cap,
                              uint32_t msg_passes, hipStream_t s) {
    if (!head || !dest_offsets || !ghead || !out_goff ||
        (((uintptr_t)head | (uintptr_t)dest_offsets | (uintptr_t)ghead | (uintptr_t)out_goff) & 7))
        return hipErrorInvalidValue;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (ecap > 0xFFFFFFFFull) ecap = 0xFFFFFFFFull;
    if (out_cap > 0xFFFFFFFFull) out_cap = 0xFFFFFFFFull;
    const uint64_t all = cap + ecap;
    if (all > 0xFFFFFFFFull || !n_dests || n_dests > FO_MAX_DESTS || sub_of_len > 0xFFFFFFFFull ||
        (sub_of_len && !sub_of))
        return hipErrorInvalidValue;
    if (!fs.gs_fix || !fs.gp_fix || all > fs.gs_cap || all > fs.gp_cap || ecap > fs.gp_ecap ||
        (all && !fs.gs_k[0]) || (cap && (!in_topic || !in_value || !in_sub)) ||
        (ecap && (!e_topic || !e_value || !member)) || (out_cap && (!out_topic || !out_value || !out_sub)) ||
        (gcap && !out_gsub))
        return hipErrorInvalidValue;
    const GsBufs b{fs.gs_fix, {fs.gs_k[0], fs.gs_k[1]}, {fs.gs_p[0], fs.gs_p[1]}};
    uint32_t *gfix = fs.gp_fix;
    const uint64_t *ph = reinterpret_cast<const uint64_t *>(gfix + GP_PH);
    const uint64_t *mh = reinterpret_cast<const uint64_t *>(gfix + GP_MH);
    uint32_t *mt = fs.gp_m[0], *mv = fs.gp_m[1], *ms = fs.gp_m[2], *msrc = fs.gp_m[3];
    uint32_t *pt = fs.gp_c[0], *pv = fs.gp_c[1], *ps = fs.gp_c[2];
    const dim3 g(GS_GRID), t(GS_BLOCK), one(1), wide(1024);
    hipLaunchKernelGGL(k_gp_count, g, t, 0, s, n_dests, dest_offsets, ecap, member, sub_of, sub_of_len, gfix);
    hipLaunchKernelGGL(k_gp_scan, one, wide, 0, s, head, cap, gfix);
    hipLaunchKernelGGL(k_gp_compact, g, t, 0, s, n_dests, dest_offsets, ecap, e_topic, e_value, member, sub_of,
                       sub_of_len, gfix, pt, pv, ps);
    // the P picks by message
    hipLaunchKernelGGL(k_gs_pre, g, t, 0, s, ph, ecap, pt, b.fix);
    hipLaunchKernelGGL(k_gs_plan, one, wide, 0, s, ph, ecap, b.fix);
    // (a digit above the caller's bound on the topic indices is one all picks agree on: k_gs_plan skips
    // it, the pass's three kernels would return at once and are not queued)
    for (uint32_t p = 0; p < GS_PASSES && p < msg_passes; p++) {
        hipLaunchKernelGGL(k_gs_hist, g, t, 0, s, ph, ecap, pt, b, p);
        hipLaunchKernelGGL(k_gs_scan, dim3(GS_BINS), t, 0, s, ph, ecap, b.fix, p);
        hipLaunchKernelGGL(k_gs_scatter, g, t, 0, s, ph, ecap, pt, b, p);
    }
    hipLaunchKernelGGL(k_gp_merge, g, t, 0, s, head, cap, in_topic, in_value, in_sub, ecap, b, gfix, pt, pv, ps, mt, mv,
                       ms, msrc);
    // the N merged deliveries by subscriber
    hipLaunchKernelGGL(k_gs_pre, g, t, 0, s, mh, all, ms, b.fix);
    hipLaunchKernelGGL(k_gs_plan, one, wide, 0, s, mh, all, b.fix);
    for (uint32_t p = 0; p < GS_PASSES; p++) {
        hipLaunchKernelGGL(k_gs_hist, g, t, 0, s, mh, all, ms, b, p);
        hipLaunchKernelGGL(k_gs_scan, dim3(GS_BINS), t, 0, s, mh, all, b.fix, p);
        hipLaunchKernelGGL(k_gs_scatter, g, t, 0, s, mh, all, ms, b, p);
    }
    hipLaunchKernelGGL(k_gs_heads, g, t, 0, s, mh, all, ms, b);
    hipLaunchKernelGGL(k_gs_gscan, one, wide, 0, s, mh, all, b.fix, ghead, out_goff, gcap);
    hipLaunchKernelGGL(k_gp_emit, g, t, 0, s, mh, all, mt, mv, ms, msrc, b, out_gsub, out_goff, gcap, out_topic, out_value,
                       out_sub, out_src, out_cap);
    return hipGetLastError();
}

}  // namespace tmx
