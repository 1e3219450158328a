// tm_share.hip -- emqx_shared_sub:dispatch/3's pick on the device, for gfx950:
// ONE member per (message, {Group, To}) entry of the aggregated route arrays.
//
// do_route2/2's shared arm looks the members of {Group, Topic} up and picks
// one by the group's strategy (apps/emqx/src/emqx_shared_sub.erl:335-406).
// On the device an entry's value gives its slot (slot_of[v]: the caller's
// dense id of a {Group, To} pair), the slot gives one 16-byte record (pos,
// cnt, n_local, meta) and a state word.  The stateless strategies (random,
// local, the two hashes) and the singleton rule are a gather.  The stateful
// ones (both round robins, sticky) need each entry's RANK among the call's
// entries of the same slot in entry order, and one transition of the slot's
// state word per call; include/tmatch.h has the definition.
//
// The fan-out's fixed grid, FO_GRID one-wave blocks, no block waits for
// another; 5 + 3 P launches, P = ceil(bits(n_slots - 1) / FO_MAX_BITS):
//   k_sh_mark     block k owns the entries [k * chunk, (k + 1) * chunk) of [0, E):
//                 value -> slot -> record; every entry that needs no rank gets
//                 its member here; key[q] = the slot of an entry that does
//                 (NONE otherwise); per block the ranked / with-slot / picked
//                 counts;
//   k_sh_scan     the exclusive scan of the FO_GRID ranked counts, N their
//                 total; head = [entries with a slot, entries with a pick];
//   k_sh_compact  the (slot, q) pairs of the ranked entries, in q order;
//   P times k_sh_hist / k_sh_dscan / k_sh_scatter: the fan-out's stable digit
//                 pass on the slot, least significant digit first -- the pairs
//                 end up sorted by (slot, q), whatever the timing;
//   k_sh_state    block k owns a chunk of the N sorted pairs: the first
//                 position of every pair's run of equal slots (a 64-ary search
//                 for the chunk's first, a wave max-scan of the run heads after
//                 it); the LAST pair of a run knows m and applies the slot's
//                 whole transition in one compare-and-swap loop on the state
//                 word, and leaves the idx of rank 0 at the run's first
//                 position;
//   k_sh_pick     rank = position - first position; the member is gathered and
//                 stored at out_member[q].
// Bytes per entry: 8 read + 4 gathered + 16 gathered (mark), 4 + 4 written; per
// ranked entry 8 written (compact), 16 read + 8 written per digit pass, 12 read +
// 4 written (state), 16 read + 16 + 4 gathered + 4 scattered (pick).
#include <hip/hip_runtime.h>

#include "tm_dev.h"

namespace tmx {

namespace {

constexpr uint32_t SH_NONE = 0xFFFFFFFFu;
static_assert(FO_GRID % 256 == 0, "k_sh_scan / k_sh_dscan: 256 threads share a row evenly");

__device__ __forceinline__ uint64_t sh_entries(const uint64_t *doff, uint32_t n_dests, uint64_t cap) {
    const uint64_t total = doff[n_dests + 1];
    return total < cap ? total : cap;
}

// the positions block `blk` owns: [c0, c1) of [0, N)
__device__ __forceinline__ void sh_chunk(uint64_t N, uint32_t blk, uint64_t &c0, uint64_t &c1) {
    const uint64_t chunk = ((N + FO_GRID - 1) / FO_GRID + 63) & ~63ull;
    c0 = (uint64_t)blk * chunk;
    c1 = c0 + chunk < N ? c0 + chunk : N;
    if (c0 > c1) c0 = c1;
}

__device__ __forceinline__ uint32_t sh_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    return x;
}

__device__ __forceinline__ uint32_t sh_incl_max(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d && y > x) x = y;
    }
    return x;
}

// R(a, b) of include/tmatch.h
__device__ __forceinline__ uint32_t sh_hash(uint32_t seed, uint32_t a, uint32_t b) {
    uint32_t x = seed ^ (a * 0x9E3779B1u) ^ (b * 0x85EBCA77u);
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

struct ShareTabs {
    const uint32_t *slot_of; uint64_t slot_of_len;
    const uint4 *rec; uint64_t n_slots;
    const uint32_t *pool; uint64_t pool_len;
    const uint32_t *key_c, *key_t; uint64_t n_topics;
    uint32_t seed;
};

// slot s's record under the definition's rules: a span outside the pool is an
// empty list, n_local <= cnt
__device__ __forceinline__ void sh_record(const ShareTabs &T, uint32_t s, uint32_t &pos, uint32_t &cnt, uint32_t &nl,
                                          uint32_t &meta) {
    const uint4 r = T.rec[s];
    pos = r.x;
    cnt = (uint64_t)r.x + r.y > T.pool_len ? 0u : r.y;
    nl = r.z < cnt ? r.z : cnt;
    meta = r.w;
}

__device__ __forceinline__ uint32_t sh_key(const uint32_t *key, uint64_t n_topics, uint32_t t) {
    return key && t < n_topics ? key[t] : 0u;
}

// the idx of a stateless strategy (cnt >= 2); anything else: as RANDOM (sticky's initial pick)
__device__ __forceinline__ uint32_t sh_stateless(const ShareTabs &T, uint32_t strat, uint32_t t, uint32_t s, uint32_t cnt,
                                                 uint32_t nl) {
    switch (strat) {
    case SH_HASH_CLIENTID: return sh_key(T.key_c, T.n_topics, t) % cnt;
    case SH_HASH_TOPIC: return sh_key(T.key_t, T.n_topics, t) % cnt;
    case SH_LOCAL:
        if (nl == 1) return 0u;
        return sh_hash(T.seed, t, s) % (nl ? nl : cnt);
    default: return sh_hash(T.seed, t, s) % cnt;
    }
}

__global__ __launch_bounds__(64) void k_sh_mark(const uint64_t *doff, uint32_t n_dests, uint64_t cap, const uint32_t *in_t,
                                                const uint32_t *in_v, ShareTabs T, uint32_t *state, uint32_t *out_member,
                                                uint32_t *key, uint32_t *blk_cnt) {
    const uint32_t lane = threadIdx.x;
    uint64_t c0, c1;
    sh_chunk(sh_entries(doff, n_dests, cap), blockIdx.x, c0, c1);
    uint32_t n_rank = 0, n_slot = 0, n_pick = 0;
    for (uint64_t q0 = c0; q0 < c1; q0 += 64) {
        const uint64_t q = q0 + lane;
        const bool ok = q < c1;
        uint32_t s = SH_NONE, member = SH_NONE;
        bool ranked = false, picked = false;
        if (ok) {
            const uint32_t v = in_v[q], t = in_t[q];
            if (v < T.slot_of_len) s = T.slot_of[v];
            if (s >= T.n_slots) s = SH_NONE;
            if (s != SH_NONE) {
                uint32_t pos, cnt, nl, meta;
                sh_record(T, s, pos, cnt, nl, meta);
                const uint32_t strat = meta & 0xFFu;
                if (cnt && strat < SH_STRATEGIES) {
                    picked = true;
                    if (cnt == 1) {
                        member = T.pool[pos];
                        if (strat == SH_STICKY) state[s] = 0u;   // (every entry of s stores the same word)
                    } else if (strat == SH_ROUND_ROBIN || strat == SH_ROUND_ROBIN_PER_GROUP || strat == SH_STICKY) {
                        ranked = true;
                    } else {
                        member = T.pool[(uint64_t)pos + sh_stateless(T, strat, t, s, cnt, nl)];
                    }
                }
            }
            if (!ranked) out_member[q] = member;
            key[q] = ranked ? s : SH_NONE;
        }
        n_rank += (uint32_t)__popcll(__ballot(ranked));
        n_slot += (uint32_t)__popcll(__ballot(ok && s != SH_NONE));
        n_pick += (uint32_t)__popcll(__ballot(picked));
    }
    if (lane == 0) {   // (every block, every run: nothing of an earlier run survives)
        blk_cnt[blockIdx.x] = n_rank;
        blk_cnt[FO_GRID + 1 + blockIdx.x] = n_slot;
        blk_cnt[2 * FO_GRID + 1 + blockIdx.x] = n_pick;
    }
}

// the FO_GRID ranked counts -> their exclusive scan in place, N into blk_cnt[FO_GRID]; head
__global__ __launch_bounds__(256) void k_sh_scan(uint32_t *blk_cnt, uint64_t *head) {
    constexpr int PER = FO_GRID / 256;
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_h[2][4];
    uint32_t *row = blk_cnt + threadIdx.x * PER;
    const uint32_t *rs = blk_cnt + FO_GRID + 1 + threadIdx.x * PER, *rp = rs + FO_GRID;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x[PER], sum = 0;
    uint64_t hs = 0, hp = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { x[k] = row[k]; sum += x[k]; hs += rs[k]; hp += rp[k]; }
    const uint32_t inc = sh_incl_scan(sum, lane);
#pragma unroll
    for (int d = 32; d; d >>= 1) { hs += __shfl_xor(hs, d, 64); hp += __shfl_xor(hp, d, 64); }
    if (lane == 63) { s_w[wv] = inc; s_h[0][wv] = hs; s_h[1][wv] = hp; }
    __syncthreads();
    uint32_t base = inc - sum;
    for (uint32_t q = 0; q < wv; q++) base += s_w[q];
#pragma unroll
    for (int k = 0; k < PER; k++) { row[k] = base; base += x[k]; }
    if (threadIdx.x == 255) {
        blk_cnt[FO_GRID] = base;
        head[0] = s_h[0][0] + s_h[0][1] + s_h[0][2] + s_h[0][3];
        head[1] = s_h[1][0] + s_h[1][1] + s_h[1][2] + s_h[1][3];
    }
}

__global__ __launch_bounds__(64) void k_sh_compact(const uint64_t *doff, uint32_t n_dests, uint64_t cap, const uint32_t *key,
                                                   const uint32_t *blk_cnt, uint32_t *out_s, uint32_t *out_q) {
    const uint32_t lane = threadIdx.x;
    uint64_t c0, c1;
    sh_chunk(sh_entries(doff, n_dests, cap), blockIdx.x, c0, c1);
    const uint32_t N = blk_cnt[FO_GRID];
    uint32_t base = blk_cnt[blockIdx.x];
    for (uint64_t q0 = c0; q0 < c1; q0 += 64) {
        const uint64_t q = q0 + lane;
        const uint32_t k = q < c1 ? key[q] : SH_NONE;
        const uint64_t m = __ballot(k != SH_NONE);
        const uint32_t dst = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (k != SH_NONE && dst < N) {   // (dst < N always: k_sh_mark counted these keys)
            out_s[dst] = k;
            out_q[dst] = (uint32_t)q;
        }
        base += (uint32_t)__popcll(m);
    }
}

// ---- the digit pass over the N compacted pairs (tm_fanout.hip's, on the slot)
__global__ __launch_bounds__(64) void k_sh_hist(const uint32_t *blk_cnt, const uint32_t *in_s, uint32_t shift,
                                                uint32_t bits, uint32_t *tab) {
    __shared__ uint32_t s_h[FO_BINS];
    const uint32_t lane = threadIdx.x, nb = 1u << bits, mask = nb - 1;
    for (uint32_t i = lane; i < nb; i += 64) s_h[i] = 0;
    __syncthreads();
    uint64_t c0, c1;
    sh_chunk(blk_cnt[FO_GRID], blockIdx.x, c0, c1);
    for (uint64_t p = c0 + lane; p < c1; p += 64) atomicAdd(&s_h[(in_s[p] >> shift) & mask], 1u);
    __syncthreads();
    for (uint32_t i = lane; i < nb; i += 64) tab[(uint64_t)i * FO_GRID + blockIdx.x] = s_h[i];
}

// one block per bin: its row of FO_GRID block counts -> exclusive scan in place, the total into tot[bin]
__global__ __launch_bounds__(256) void k_sh_dscan(uint32_t *tab, uint32_t *tot) {
    constexpr int PER = FO_GRID / 256;
    __shared__ uint32_t s_w[4];
    uint32_t *row = tab + (uint64_t)blockIdx.x * FO_GRID + threadIdx.x * PER;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { x[k] = row[k]; sum += x[k]; }
    const uint32_t inc = sh_incl_scan(sum, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = inc - sum;
    for (uint32_t q = 0; q < wv; q++) base += s_w[q];
#pragma unroll
    for (int k = 0; k < PER; k++) { row[k] = base; base += x[k]; }
    if (threadIdx.x == 255) tot[blockIdx.x] = base;
}

__global__ __launch_bounds__(64) void k_sh_scatter(const uint32_t *blk_cnt, const uint32_t *in_s, const uint32_t *in_q,
                                                   uint32_t shift, uint32_t bits, const uint32_t *tab, const uint32_t *tot,
                                                   uint32_t *out_s, uint32_t *out_q) {
    __shared__ uint32_t s_base[FO_BINS];
    const uint32_t lane = threadIdx.x, nb = 1u << bits, mask = nb - 1;
    // every block scans the bins' totals itself (at most 8 rounds of one wave)
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < nb; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t x = i < nb ? tot[i] : 0u;
        const uint32_t inc = sh_incl_scan(x, lane);
        if (i < nb) s_base[i] = carry + inc - x + tab[(uint64_t)i * FO_GRID + blockIdx.x];
        carry += __shfl(inc, 63, 64);
    }
    __syncthreads();
    const uint32_t N = blk_cnt[FO_GRID];
    uint64_t c0, c1;
    sh_chunk(N, blockIdx.x, c0, c1);
    for (uint64_t p0 = c0; p0 < c1; p0 += 64) {
        const uint64_t p = p0 + lane;
        const bool ok = p < c1;
        const uint32_t s = ok ? in_s[p] : 0u, q = ok ? in_q[p] : 0u;
        const uint32_t d = (s >> shift) & mask;
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
        if (ok && dst < N) {   // (dst < N always: the histogram saw these slots)
            out_s[dst] = s;
            out_q[dst] = q;
        }
    }
}

// the first index of the ascending S[0 .. hi) whose word is >= key, by the whole
// wave, 64 probes a round (tm_dev.h fo_topic_at's search)
__device__ __forceinline__ uint32_t sh_lower(const uint32_t *S, uint32_t hi, uint32_t key, uint32_t lane) {
    uint32_t lo = 0;
    while (lo < hi) {
        const uint32_t step = (uint32_t)(((uint64_t)hi - lo + 63) / 64);
        const uint64_t idx = (uint64_t)lo + (uint64_t)lane * step;
        const bool in = idx < hi;
        const bool ge = in && S[idx] >= key;
        const uint64_t m_ge = __ballot(ge), m_in = __ballot(in);
        if (!m_ge) {
            lo = lo + ((uint32_t)__popcll(m_in) - 1) * step + 1;   // every probe < key
        } else {
            const uint32_t f = (uint32_t)__builtin_ctzll(m_ge);
            hi = lo + f * step;
            if (f) lo = lo + (f - 1) * step + 1;
        }
    }
    return lo;
}

__global__ __launch_bounds__(64) void k_sh_state(const uint32_t *blk_cnt, const uint32_t *S, const uint32_t *Q,
                                                 const uint32_t *in_t, uint64_t E, const uint64_t *doff, uint32_t n_dests,
                                                 ShareTabs T, uint32_t *state, uint32_t *first, uint32_t *base0) {
    const uint32_t lane = threadIdx.x;
    const uint32_t N = blk_cnt[FO_GRID];
    uint64_t c0, c1;
    sh_chunk(N, blockIdx.x, c0, c1);
    if (c0 >= c1) return;   // (block-uniform)
    const uint64_t Ein = sh_entries(doff, n_dests, E);
    uint32_t cur = sh_lower(S, (uint32_t)c0, S[c0], lane);   // the run the chunk starts in
    for (uint64_t p0 = c0; p0 < c1; p0 += 64) {
        const uint64_t p = p0 + lane;
        const bool ok = p < c1;
        uint32_t s = 0;
        bool head = false, tail = false;
        if (ok) {
            s = S[p];
            head = p == 0 || S[p - 1] != s;
            tail = p + 1 == N || S[p + 1] != s;
        }
        uint32_t st = sh_incl_max(head ? (uint32_t)p : 0u, lane);
        if (st < cur) st = cur;
        cur = __shfl(st, 63, 64);
        if (ok) first[p] = st;
        if (!ok || !tail) continue;   // (no wave operation below)
        // one lane per (call, slot): the whole transition in one compare-and-swap loop
        uint32_t pos, cnt, nl, meta;
        sh_record(T, s, pos, cnt, nl, meta);
        if (cnt < 2) { base0[st] = 0; continue; }   // (never: k_sh_mark ranked this slot)
        const uint32_t strat = meta & 0xFFu;
        const uint64_t last = (uint64_t)p - st;   // rank m - 1
        uint32_t b0 = 0;
        for (;;) {
            const uint32_t c = __hip_atomic_load(&state[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t nw;
            if (strat == SH_ROUND_ROBIN) {
                b0 = c == SH_NONE ? sh_hash(T.seed, SH_NONE, s) % cnt : (uint32_t)(((uint64_t)c + 1) % cnt);
                nw = (uint32_t)((b0 + last) % cnt);
            } else if (strat == SH_ROUND_ROBIN_PER_GROUP) {
                const uint32_t c00 = c == SH_NONE ? 0u : c;
                b0 = (c00 < cnt ? c00 : cnt) % cnt;
                nw = (uint32_t)((b0 + last) % cnt) + 1u;
            } else {   // SH_STICKY
                if (c < cnt) {
                    b0 = c;
                } else {
                    const uint32_t q0 = Q[st];   // the rank-0 entry
                    const uint32_t t = q0 < Ein ? in_t[q0] : 0u;
                    b0 = sh_stateless(T, (meta >> 8) & 0xFFu, t, s, cnt, nl);
                }
                nw = b0;
            }
            if (nw == c || atomicCAS(&state[s], c, nw) == c) break;
        }
        base0[st] = b0;
    }
}

__global__ __launch_bounds__(64) void k_sh_pick(const uint32_t *blk_cnt, const uint32_t *S, const uint32_t *Q,
                                                const uint32_t *first, const uint32_t *base0, uint64_t E,
                                                const uint64_t *doff, uint32_t n_dests, ShareTabs T, uint32_t *out_member) {
    const uint32_t lane = threadIdx.x;
    const uint32_t N = blk_cnt[FO_GRID];
    const uint64_t Ein = sh_entries(doff, n_dests, E);
    uint64_t c0, c1;
    sh_chunk(N, blockIdx.x, c0, c1);
    for (uint64_t p = c0 + lane; p < c1; p += 64) {
        const uint32_t s = S[p], q = Q[p], st = first[p];
        const uint32_t b0 = st < N ? base0[st] : 0u;
        uint32_t pos, cnt, nl, meta;
        sh_record(T, s, pos, cnt, nl, meta);
        uint32_t member = SH_NONE;
        if (cnt) {
            const uint64_t idx = (meta & 0xFFu) == SH_STICKY ? b0 % cnt : (b0 + ((uint64_t)p - st)) % cnt;
            member = T.pool[pos + idx];   // (inside the pool: pos + cnt <= pool_len)
        }
        if (q < Ein) out_member[q] = member;
    }
}

}  // namespace

uint32_t share_passes(uint64_t n_slots) {
    uint32_t bits = 0;
    while (n_slots > ((uint64_t)1 << bits)) bits++;   // the slots are below n_slots
    return (bits + FO_MAX_BITS - 1) / FO_MAX_BITS;
}

hipError_t launch_share_pick(const FanoutScratch &fs, uint32_t n_dests, const uint64_t *dest_offsets,
                             const uint32_t *in_topic, const uint32_t *in_value, uint64_t cap, const uint32_t *key_clientid,
                             const uint32_t *key_topic, uint64_t n_topics, uint32_t seed, const uint32_t *slot_of,
                             uint64_t slot_of_len, const uint32_t *slot_rec, uint64_t n_slots, const uint32_t *pool,
                             uint64_t pool_len, uint32_t *state, uint64_t *head, uint32_t *out_member, hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS || ((uintptr_t)slot_rec & 15)) return hipErrorInvalidValue;
    if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
    if (!slot_of) slot_of_len = 0;
    if (!slot_rec || !state) n_slots = 0;
    if (n_slots > 0xFFFFFFFFull) n_slots = 0xFFFFFFFFull;   // (0xFFFFFFFF is "none")
    if (!pool) pool_len = 0;
    if (!fs.tab || !fs.tot || !fs.sh_key || !fs.sh_cnt || cap > fs.sh_cap) return hipErrorInvalidValue;
    const ShareTabs T{slot_of, slot_of_len, reinterpret_cast<const uint4 *>(slot_rec), n_slots, pool, pool_len,
                      key_clientid, key_topic, n_topics, seed};
    const dim3 g(FO_GRID), b(64);
    hipLaunchKernelGGL(k_sh_mark, g, b, 0, s, dest_offsets, n_dests, cap, in_topic, in_value, T, state, out_member,
                       fs.sh_key, fs.sh_cnt);
    hipLaunchKernelGGL(k_sh_scan, dim3(1), dim3(256), 0, s, fs.sh_cnt, head);
    hipLaunchKernelGGL(k_sh_compact, g, b, 0, s, dest_offsets, n_dests, cap, fs.sh_key, fs.sh_cnt, fs.sh_s[0], fs.sh_q[0]);
    uint32_t bits_left = 0;
    while (n_slots > ((uint64_t)1 << bits_left)) bits_left++;
    int cur = 0;
    for (uint32_t shift = 0; bits_left; cur ^= 1) {
        const uint32_t bits = bits_left < (uint32_t)FO_MAX_BITS ? bits_left : (uint32_t)FO_MAX_BITS;
        hipLaunchKernelGGL(k_sh_hist, g, b, 0, s, fs.sh_cnt, fs.sh_s[cur], shift, bits, fs.tab);
        hipLaunchKernelGGL(k_sh_dscan, dim3(1u << bits), dim3(256), 0, s, fs.tab, fs.tot);
        hipLaunchKernelGGL(k_sh_scatter, g, b, 0, s, fs.sh_cnt, fs.sh_s[cur], fs.sh_q[cur], shift, bits, fs.tab, fs.tot,
                           fs.sh_s[cur ^ 1], fs.sh_q[cur ^ 1]);
        shift += bits;
        bits_left -= bits;
    }
    // the buffers the last pass read are free: the runs' first positions and rank-0 idx
    hipLaunchKernelGGL(k_sh_state, g, b, 0, s, fs.sh_cnt, fs.sh_s[cur], fs.sh_q[cur], in_topic, cap, dest_offsets, n_dests, T,
                       state, fs.sh_s[cur ^ 1], fs.sh_q[cur ^ 1]);
    hipLaunchKernelGGL(k_sh_pick, g, b, 0, s, fs.sh_cnt, fs.sh_s[cur], fs.sh_q[cur], fs.sh_s[cur ^ 1], fs.sh_q[cur ^ 1], cap,
                       dest_offsets, n_dests, T, out_member);
    return hipGetLastError();
}

}  // namespace tmx
