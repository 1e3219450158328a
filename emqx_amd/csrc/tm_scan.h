// tm_scan.h -- the tokeniser's scan: split a topic on '/' and park every
// level's word in the frontier store, a 16-byte chunk and a word end at a time.
//
// Shared by the gfx950 kernels (tm_kernels.hip, tokenize) and by a host build
// (tests/scan_cpu), so the scan is a TM_HD template over
//   Src  ld16(p): the aligned 16-byte granule at byte offset p as four
//        little-endian dwords (.x .y .z .w);
//   St   put_word(level, b0, b1, len) and St::maxl, the levels it stores.
//
// Per chunk the '/' positions become a 16-bit mask (the exact zero-byte test of
// count_slashes, four bytes at a time) and the loop runs once per word end, not
// once per byte: the lanes of a wave end their words at different byte
// positions, so a byte loop made the wave execute both sides of nearly every
// step.  A word's length comes from positions, its first VINL bytes from the
// chunk's dwords (dword select + byte alignment), appended to what earlier
// chunks carried over.
#pragma once
#include "tm_layout.h"

namespace tmx {

struct ScanOut {
    uint32_t lev;    // levels parked (early: levels ended before byte p)
    bool bad;        // NEED: a level past the stored ones is exactly '+' or '#'
    bool early;      // !NEED: left once lev > St::maxl, at chunk p < end
    uint64_t p;
};

// '/' positions of a chunk: bit k = byte k is '/'
TM_HD uint32_t slash_mask16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    auto z = [](uint32_t w) {   // bit 7 of every byte that is '/'
        const uint32_t x = w ^ 0x2F2F2F2Fu;   // '/' bytes -> 0
        return ~((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x)) & 0x80808080u;
    };
    auto pack8 = [](uint32_t a, uint32_t b) {   // a's four flags -> bits 0-3, b's -> bits 4-7
        uint32_t t = (a >> 7) | (b >> 3);       // bits 8i (a), 8i + 4 (b)
        t |= t >> 7;
        t |= t >> 14;
        return t & 0xFFu;
    };
    return pack8(z(w0), z(w1)) | pack8(z(w2), z(w3)) << 8;
}

// The scan of tokenize's deferred path.  A word of <= VINL bytes parks
// (b0, b1, len), a longer one (len, start - beg, 255); an empty level parks
// length 0.  NEED stores scan every level (chunks loaded two ahead) and flag
// a '+' / '#' level past the stored ones; the others leave at the first chunk
// boundary with lev > St::maxl.  Only granules that hold a byte of
// [beg, end) are read.
template <bool NEED, class Src, class St>
TM_HD ScanOut scan_levels(const Src &src, uint64_t beg, uint64_t end, St &st) {
    using V = decltype(src.ld16(beg));
    V z = V(); z.x = 0; z.y = 0; z.z = 0; z.w = 0;
    const uint64_t p0 = beg & ~15ull;
    // aligned 16-byte loads (the first two issued together): a chunk shares its 16-byte granule with a valid
    // byte, so it never crosses a page the caller does not own
    const V c0 = p0 < end ? src.ld16(p0) : z;
    const V c1 = p0 + 16 < end ? src.ld16(p0 + 16) : z;
    uint32_t lev = 0, len = 0, ws = 0;   // ws: the word's start, from beg
    uint64_t acc = 0;                    // the word's first VINL bytes, little endian
    bool bad = false;
    uint32_t ci = 0;
    uint64_t p = p0;
    V ra = c0, rb = c1;   // NEED: chunks loaded two ahead (deep topics run hundreds of bytes)
    for (; p < end; p += 16, ci++) {
        if (!NEED && lev > St::maxl) break;   // deeper than the main walk's store
        V v;
        if (NEED) {
            v = ra; ra = rb;
            rb = p + 32 < end ? src.ld16(p + 32) : z;
        } else {
            v = ci == 0 ? c0 : ci == 1 ? c1 : src.ld16(p);
        }
        const uint32_t k0 = p < beg ? (uint32_t)(beg - p) : 0;
        const uint32_t k1 = end - p < 16 ? (uint32_t)(end - p) : 16;
        const uint32_t rel = (uint32_t)(p - beg);   // (wraps below beg; only rel + k, k >= k0, is used)
        // word ends inside [k0, k1), then the chunk's end as a last stop
        uint32_t m = (slash_mask16(v.x, v.y, v.z, v.w) & ((1u << k1) - (1u << k0))) | 1u << k1;
        uint32_t s = k0;
        for (;;) {
            const uint32_t e = (uint32_t)__builtin_ctz(m);
            m &= m - 1;
            // append bytes [s, e) of the chunk to the word
            const uint32_t n = e - s, d = s >> 2, sh = (s & 3) * 8;
            const uint32_t x0 = d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
            const uint32_t x1 = d == 0 ? v.y : d == 1 ? v.z : d == 2 ? v.w : 0u;
            const uint32_t x2 = d == 0 ? v.z : d == 1 ? v.w : 0u;
            const uint32_t lo = (uint32_t)(((uint64_t)x1 << 32 | x0) >> sh);
            const uint32_t hi = (uint32_t)(((uint64_t)x2 << 32 | x1) >> sh);
            uint64_t x = (uint64_t)hi << 32 | lo;
            if (n < VINL) x &= (1ull << (8 * n)) - 1ull;
            if (len < VINL) acc |= x << (8 * len);
            len += n;
            if (e == k1) break;
            // a '/' ends the word
            if (lev < St::maxl) {
                if (len <= VINL) st.put_word(lev, (uint32_t)acc, (uint32_t)(acc >> 32), len);
                else st.put_word(lev, len, ws, 255);
            } else if (NEED) {
                bad |= len == 1 && ((acc & 0xFFu) == '+' || (acc & 0xFFu) == '#');
            }
            lev++;
            len = 0; acc = 0; s = e + 1; ws = rel + s;
        }
    }
    ScanOut o;
    o.p = p;
    o.early = !NEED && p < end;
    if (!o.early) {   // the last word
        if (lev < St::maxl) {
            if (len <= VINL) st.put_word(lev, (uint32_t)acc, (uint32_t)(acc >> 32), len);
            else st.put_word(lev, len, ws, 255);
        } else if (NEED) {
            bad |= len == 1 && ((acc & 0xFFu) == '+' || (acc & 0xFFu) == '#');
        }
        lev++;
    }
    o.lev = lev;
    o.bad = bad;
    return o;
}

}  // namespace tmx
