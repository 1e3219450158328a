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

// one entry's mark: value -> slot -> record.  An entry that needs no rank gets
// its member (NONE: no pick); `ranked`: a stateful strategy with cnt >= 2
__device__ __forceinline__ void sh_mark_entry(const ShareTabs &T, uint32_t v, uint32_t t, uint32_t *state, uint32_t &s,
                                              uint32_t &member, bool &ranked, bool &picked) {
    if (v < T.slot_of_len) s = T.slot_of[v];
    if (s >= T.n_slots) s = SH_NONE;
    if (s == SH_NONE) return;
    uint32_t pos, cnt, nl, meta;
    sh_record(T, s, pos, cnt, nl, meta);
    const uint32_t strat = meta & 0xFFu;
    if (!cnt || strat >= SH_STRATEGIES) return;
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

// slot s's whole transition for a call with m = last + 1 ranked entries, in one
// compare-and-swap loop on the state word: -> the idx of rank 0.  topic0(): the
// topic of the rank-0 entry (sticky's initial pick; asked for only then)
template <class Topic0>
__device__ __forceinline__ uint32_t sh_transition(const ShareTabs &T, uint32_t *state, uint32_t s, uint32_t cnt, uint32_t nl,
                                                  uint32_t meta, uint64_t last, Topic0 topic0) {
    const uint32_t strat = meta & 0xFFu;
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
            b0 = c < cnt ? c : sh_stateless(T, (meta >> 8) & 0xFFu, topic0(), s, cnt, nl);
            nw = b0;
        }
        if (nw == c || atomicCAS(&state[s], c, nw) == c) break;
    }
    return b0;
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
            sh_mark_entry(T, in_v[q], in_t[q], state, s, member, ranked, picked);
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
        const uint64_t last = (uint64_t)p - st;   // rank m - 1
        const uint32_t b0 = sh_transition(T, state, s, cnt, nl, meta, last, [&]() -> uint32_t {
            const uint32_t q0 = Q[st];   // the rank-0 entry
            return q0 < Ein ? in_t[q0] : 0u;
        });
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

// ---- a micro-batch (tm_publish_batch32): ONE workgroup of FO1_BLOCK threads
// picks for the K <= FO1_ENTRIES aggregated entries k_ag_one left on the lane
// (u32 offsets), launch_share_pick's definition to the letter.
//   gate   the run that queued this launch may be run again, so the kernel
//          picks (and moves state) only when that run stands: the fan-out
//          completed, the value scratch held the batch (total <= vcap), the
//          caller has room (total <= cap) and the lane's fail word is down;
//          else it writes SH1_SKIPPED and nothing more;
//   mark   wave w owns the entries [w * C, (w + 1) * C), C = ceil(K / 16)
//          rounded up to 64: sh_mark_entry; s_key[q] = the member of an entry
//          that needs no rank, the slot of one that does (its bit in s_bal);
//   rank   the ranked entries' q, compacted in q order as 16-bit indices, sorted
//          by slot: stable digit passes of 8 bits, least significant first, as
//          many as the largest slot present has digits (k_fo_one's pass: a row
//          of bins per wave, the scan over waves then bins, the peer-mask
//          scatter) between two index arrays -- sorted by (slot, q) whatever
//          the timing; the run heads' running maximum gives every position its
//          run's first;
//   pick   the LAST position of a run applies sh_transition and leaves the idx
//          of rank 0 in s_key at the run's rank-0 entry; every position gathers
//          its member, and s_key[0 .. K) goes out to out_member (mapped host
//          memory: consecutive threads, consecutive words, never read).
// status (mapped host memory): [SH1_ST_STATE], [SH1_ST_HEAD ..] = the head as
// two u64.  LDS: 64 KiB keys + 2 x 32 KiB indices + 16 KiB bins + 2 KiB bits.
constexpr uint32_t SH1_WAVES = FO1_BLOCK / 64;
constexpr uint32_t SH1_STEPS = FO1_ENTRIES / FO1_BLOCK;   // 64-entry steps of a wave, at most
constexpr uint32_t SH1_BINS = 256;
constexpr uint32_t SH1_NOF = 0xFFFFu;                     // "no run head in my chunk before me"
static_assert(FO1_ENTRIES <= SH1_NOF, "k_sh_one: positions are staged as 16 bits");
static_assert(SH1_BINS <= FO1_BLOCK && SH1_BINS % 64 == 0, "k_sh_one: one thread per bin, whole waves of them");

__device__ __forceinline__ void sh_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the first position of p's run: what the wave's scan left, or the last head of the nearest wave before it that saw one
__device__ __forceinline__ uint32_t sh1_first(const uint16_t *F, const uint32_t *s_wt, uint32_t p, uint32_t wv) {
    uint32_t f = F[p];
    if (f != SH1_NOF) return f;
    f = 0;   // (position 0 is a head: some wave before this one saw it)
    for (uint32_t q = wv; q-- > 0;)
        if (s_wt[q]) { f = s_wt[q] - 1; break; }
    return f;
}

__global__ __launch_bounds__(FO1_BLOCK) void k_sh_one(const uint32_t *st_in, const uint32_t *fail, const uint32_t *doff,
                                                      uint32_t n_dests, const uint32_t *in_t, const uint32_t *in_v,
                                                      uint64_t vcap, uint64_t cap, ShareTabs T, uint32_t *state,
                                                      uint32_t *out_member, uint32_t *status) {
    __shared__ uint32_t s_key[FO1_ENTRIES];
    __shared__ __attribute__((aligned(4))) uint16_t s_ix[2][FO1_ENTRIES];
    __shared__ uint32_t s_h[SH1_WAVES * SH1_BINS];
    __shared__ uint64_t s_bal[FO1_ENTRIES / 64];
    __shared__ uint32_t s_wt[SH1_WAVES];
    __shared__ uint32_t s_bw[SH1_BINS / 64];
    __shared__ uint32_t s_red[3];   // the largest ranked slot, the entries with a slot, with a pick
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t fo_state = st_in[FO1_ST_STATE], total = st_in[FO1_ST_TOTAL];
    const uint32_t failed = fail ? __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
    if (fo_state != FO1_DONE || total > vcap || total > cap || failed || n_dests > FO1_MAX_DESTS) {   // (block-uniform)
        if (tid == 0) status[SH1_ST_STATE] = SH1_SKIPPED;
        return;
    }
    uint32_t K = doff[n_dests + 1];
    if (K > FO1_ENTRIES) K = FO1_ENTRIES;   // (never: k_fo_one completed)
    if (K > cap) K = (uint32_t)cap;         // (never: K <= total <= cap)
    if (tid < 3) s_red[tid] = 0;
    __syncthreads();
    // ---- mark
    const uint32_t C = ((K + SH1_WAVES - 1) / SH1_WAVES + 63) & ~63u;   // (<= 64 * SH1_STEPS)
    const uint32_t c0 = wv * C < K ? wv * C : K, c1 = c0 + C < K ? c0 + C : K;
    uint32_t n_rank = 0, n_slot = 0, n_pick = 0, smax = 0;
    for (uint32_t q0 = c0; q0 < c1; q0 += 64) {
        const uint32_t q = q0 + lane;
        const bool ok = q < c1;
        uint32_t s = SH_NONE, member = SH_NONE;
        bool ranked = false, picked = false;
        if (ok) {
            sh_mark_entry(T, in_v[q], in_t[q], state, s, member, ranked, picked);
            s_key[q] = ranked ? s : member;
        }
        const uint64_t m = __ballot(ranked);
        if (lane == 0) s_bal[q0 >> 6] = m;   // (c0 is a multiple of 64 here: c0 < c1)
        n_rank += (uint32_t)__popcll(m);
        n_slot += (uint32_t)__popcll(__ballot(ok && s != SH_NONE));
        n_pick += (uint32_t)__popcll(__ballot(picked));
        if (ranked && s > smax) smax = s;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint32_t y = __shfl_xor(smax, d, 64);
        if (y > smax) smax = y;
    }
    if (lane == 0) {
        s_wt[wv] = n_rank;
        atomicMax(&s_red[0], smax);
        atomicAdd(&s_red[1], n_slot);
        atomicAdd(&s_red[2], n_pick);
    }
    __syncthreads();
    // ---- rank: the ranked entries' q in q order ...
    uint32_t base = 0, N = 0;
    for (uint32_t q = 0; q < SH1_WAVES; q++) {
        if (q < wv) base += s_wt[q];
        N += s_wt[q];
    }
    for (uint32_t q0 = c0; q0 < c1; q0 += 64) {
        const uint64_t m = s_bal[q0 >> 6];
        if ((m >> lane) & 1ull) s_ix[0][base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(q0 + lane);
        base += (uint32_t)__popcll(m);
    }
    const uint32_t top = s_red[0];
    uint32_t passes = N > 1 ? (32u - (uint32_t)__clz(top | 1u) + 7u) / 8u : 0u;   // (one entry is sorted)
    if (top == 0) passes = 0;                                                     // (so is one slot, 0)
    __syncthreads();
    // ... sorted by slot.  Wave w owns the positions [w * D, (w + 1) * D) of [0, N)
    const uint32_t D = ((N + SH1_WAVES - 1) / SH1_WAVES + 63) & ~63u;
    const uint32_t d0 = wv * D < N ? wv * D : N, d1 = d0 + D < N ? d0 + D : N;
    uint32_t *my_h = s_h + wv * SH1_BINS;
    uint32_t cur = 0;
    for (uint32_t pass = 0, shift = 0; pass < passes; pass++, shift += 8, cur ^= 1) {   // (block-uniform)
        const uint16_t *src = s_ix[cur];
        uint16_t *dst_ix = s_ix[cur ^ 1];
        for (uint32_t i = tid; i < SH1_WAVES * SH1_BINS; i += FO1_BLOCK) s_h[i] = 0;
        __syncthreads();
        for (uint32_t p0 = d0; p0 < d1; p0 += 64) {
            const uint32_t p = p0 + lane;
            if (p < d1) atomicAdd(&my_h[(s_key[src[p]] >> shift) & (SH1_BINS - 1)], 1u);
        }
        __syncthreads();
        // bin b: its counts' exclusive scan over the waves, then over the bins
        uint32_t tot = 0;
        if (tid < SH1_BINS)
            for (uint32_t q = 0; q < SH1_WAVES; q++) {
                const uint32_t x = s_h[q * SH1_BINS + tid];
                s_h[q * SH1_BINS + tid] = tot;
                tot += x;
            }
        const uint32_t binc = sh_incl_scan(tot, lane);
        if (tid < SH1_BINS && lane == 63) s_bw[wv] = binc;
        __syncthreads();
        if (tid < SH1_BINS) {
            uint32_t exc = binc - tot;
            for (uint32_t q = 0; q < wv; q++) exc += s_bw[q];
            for (uint32_t q = 0; q < SH1_WAVES; q++) s_h[q * SH1_BINS + tid] += exc;
        }
        __syncthreads();
        // the stable scatter: waves, steps and lanes are in position order
        for (uint32_t p0 = d0; p0 < d1; p0 += 64) {   // (wave-uniform)
            const uint32_t p = p0 + lane;
            const bool ok = p < d1;
            const uint32_t ix = ok ? src[p] : 0u;
            const uint32_t d = ok ? (s_key[ix] >> shift) & (SH1_BINS - 1) : 0u;
            uint64_t peers = __ballot(ok);
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const bool bit = (d >> k) & 1u;
                const uint64_t m = __ballot(ok && bit);
                peers &= bit ? m : ~m;
            }
            uint32_t dst = 0;
            if (ok) dst = my_h[d] + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
            sh_wave_sync();
            if (ok && (peers >> lane) == 1ull) my_h[d] += (uint32_t)__popcll(peers);
            sh_wave_sync();
            if (ok && dst < N) dst_ix[dst] = (uint16_t)ix;   // (dst < N always: the histogram saw these slots)
        }
        __syncthreads();
    }
    // ---- pick.  I: the ranked entries by (slot, q); F: every position's run's first
    const uint16_t *I = s_ix[cur];
    uint16_t *F = s_ix[cur ^ 1];
    uint32_t rs[SH1_STEPS];   // the position's slot, then its member
    uint32_t tails = 0;       // bit k: step k's position is its run's last
    uint32_t carry = 0;       // the last head at or before the step, + 1 (0: none in my chunk so far)
#pragma unroll
    for (uint32_t k = 0; k < SH1_STEPS; k++) {
        if (k * 64 >= D) break;   // (block-uniform)
        const uint32_t p = d0 + k * 64 + lane;
        const bool ok = p < d1;
        const uint32_t s = ok ? s_key[I[p]] : SH_NONE;
        rs[k] = s;
        const bool head = ok && (p == 0 || s_key[I[p - 1]] != s);
        const bool tail = ok && (p + 1 == N || s_key[I[p + 1]] != s);
        uint32_t x = sh_incl_max(head ? p + 1 : 0u, lane);
        if (carry > x) x = carry;
        carry = __shfl(x, 63, 64);
        if (ok) F[p] = x ? (uint16_t)(x - 1) : (uint16_t)SH1_NOF;
        if (tail) tails |= 1u << k;
    }
    if (lane == 0) s_wt[wv] = carry;   // (the compaction's reads of s_wt lie behind a barrier)
    __syncthreads();
    // one lane per (call, slot): the whole transition; the idx of rank 0 replaces the slot at the rank-0 entry
#pragma unroll
    for (uint32_t k = 0; k < SH1_STEPS; k++) {
        if (k * 64 >= D) break;
        if (!((tails >> k) & 1u)) continue;   // (no wave operation below)
        const uint32_t p = d0 + k * 64 + lane, s = rs[k];
        const uint32_t f = sh1_first(F, s_wt, p, wv);
        const uint32_t q0 = I[f];   // the rank-0 entry
        uint32_t pos, cnt, nl, meta;
        sh_record(T, s, pos, cnt, nl, meta);
        uint32_t b0 = 0;
        if (cnt >= 2)   // (always: the mark ranked this slot)
            b0 = sh_transition(T, state, s, cnt, nl, meta, (uint64_t)(p - f), [&]() -> uint32_t { return in_t[q0]; });
        s_key[q0] = b0;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < SH1_STEPS; k++) {
        if (k * 64 >= D) break;
        const uint32_t p = d0 + k * 64 + lane;
        if (p >= d1) continue;
        const uint32_t s = rs[k], f = sh1_first(F, s_wt, p, wv), b0 = s_key[I[f]];
        uint32_t pos, cnt, nl, meta;
        sh_record(T, s, pos, cnt, nl, meta);
        uint32_t member = SH_NONE;
        if (cnt) {
            const uint64_t idx = (meta & 0xFFu) == SH_STICKY ? b0 % cnt : (b0 + (uint64_t)(p - f)) % cnt;
            member = T.pool[pos + idx];   // (inside the pool: pos + cnt <= pool_len)
        }
        rs[k] = member;
    }
    __syncthreads();   // (every b0 is read: the members take the keys' place)
#pragma unroll
    for (uint32_t k = 0; k < SH1_STEPS; k++) {
        if (k * 64 >= D) break;
        const uint32_t p = d0 + k * 64 + lane;
        if (p < d1) s_key[I[p]] = rs[k];
    }
    __syncthreads();
    for (uint32_t i = tid; i < K; i += FO1_BLOCK) out_member[i] = s_key[i];
    if (tid == 0) {
        status[SH1_ST_HEAD] = s_red[1];
        status[SH1_ST_HEAD + 1] = 0;
        status[SH1_ST_HEAD + 2] = s_red[2];
        status[SH1_ST_HEAD + 3] = 0;
        status[SH1_ST_STATE] = SH1_PICKED;
    }
}

}  // namespace

hipError_t launch_share_one(const uint32_t *status_in, const uint32_t *fail, const uint32_t *dest_offsets, uint32_t n_dests,
                            const uint32_t *in_topic, const uint32_t *in_value, uint64_t vcap, uint64_t cap,
                            const uint32_t *key_clientid, const uint32_t *key_topic, uint64_t n_topics, uint32_t seed,
                            const uint32_t *slot_of, uint64_t slot_of_len, const uint32_t *slot_rec, uint64_t n_slots,
                            const uint32_t *pool, uint64_t pool_len, uint32_t *state, uint32_t *out_member, uint32_t *status,
                            hipStream_t s) {
    if (!n_dests || n_dests > FO_MAX_DESTS || ((uintptr_t)slot_rec & 15) || !status_in || !status) return hipErrorInvalidValue;
    if (cap && !out_member) return hipErrorInvalidValue;
    if (!slot_of) slot_of_len = 0;
    if (!slot_rec || !state) n_slots = 0;
    if (n_slots > 0xFFFFFFFFull) n_slots = 0xFFFFFFFFull;   // (0xFFFFFFFF is "none")
    if (!pool) pool_len = 0;
    const ShareTabs T{slot_of, slot_of_len, reinterpret_cast<const uint4 *>(slot_rec), n_slots, pool, pool_len,
                      key_clientid, key_topic, n_topics, seed};
    hipLaunchKernelGGL(k_sh_one, dim3(1), dim3(FO1_BLOCK), 0, s, status_in, fail, dest_offsets, n_dests, in_topic, in_value,
                       vcap, cap, T, state, out_member, status);
    return hipGetLastError();
}

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
