// scan_check.cpp -- host check of the tokeniser's word-at-a-time scan
// (emqx_amd/csrc/tm_scan.h) against the plain byte loop it replaced, kept
// here as the reference.  Stand-alone (own main), built by
// tests/test_scan_cpu.py with -fsanitize=address,undefined.
//
// Compared field by field: the level count, every stored level's
// (b0, b1, len) or (len, start, 255), `bad`, the '$' flag and the early exit
// (taken or not, and the chunk it left at).  The byte source aborts on any
// load that is not an aligned 16-byte granule holding a byte of the topic.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/tm_scan.h"

using namespace tmx;

struct Chunk { uint32_t x, y, z, w; };

struct HostSrc {
    const uint8_t *g;
    uint64_t size, beg, end;
    Chunk ld16(uint64_t p) const {
        if (p % 16 || p + 16 > size || !(p < end && p + 16 > beg)) {
            fprintf(stderr, "load discipline: ld16(%llu) for [%llu, %llu) of %llu\n", (unsigned long long)p,
                    (unsigned long long)beg, (unsigned long long)end, (unsigned long long)size);
            abort();
        }
        Chunk c;
        memcpy(&c, g + p, 16);   // (little-endian host, as the device)
        return c;
    }
    uint32_t byte(uint64_t p) const { return g[p]; }
};

template <uint32_t ML>
struct RecStore {
    static constexpr uint32_t maxl = ML;
    uint32_t b0[ML], b1[ML], len[ML], puts;
    RecStore() : puts(0) { memset(b0, 0xEE, sizeof b0); memset(b1, 0xEE, sizeof b1); memset(len, 0xEE, sizeof len); }
    void put_word(uint32_t l, uint32_t a, uint32_t b, uint32_t n) {
        if (l >= ML) { fprintf(stderr, "put_word past the store: level %u\n", l); abort(); }
        b0[l] = a; b1[l] = b; len[l] = n & 0xFFu; puts++;
    }
};

// the byte-at-a-time scan of tokenize's deferred path, as it was
template <bool NEED, class Src, class St>
ScanOut scan_reference(const Src &src, uint64_t beg, uint64_t end, St &st) {
    const uint64_t p0 = beg & ~15ull;
    const Chunk z = {0, 0, 0, 0};
    const Chunk c0 = p0 < end ? src.ld16(p0) : z;
    const Chunk c1 = p0 + 16 < end ? src.ld16(p0 + 16) : z;
    uint32_t lev = 0, len = 0, b0 = 0, b1 = 0;
    uint64_t ws = beg;
    bool bad = false;
    auto park = [&]() {
        if (lev < St::maxl) {
            if (len <= VINL) st.put_word(lev, b0, b1, len);
            else st.put_word(lev, len, (uint32_t)(ws - beg), 255);
        } else if (NEED) {
            bad |= len == 1 && ((b0 & 0xFFu) == '+' || (b0 & 0xFFu) == '#');
        }
        lev++;
    };
    uint32_t ci = 0;
    uint64_t p = p0;
    Chunk ra = c0, rb = c1;
    for (; p < end; p += 16, ci++) {
        if (!NEED && lev > St::maxl) break;
        Chunk v;
        if (NEED) {
            v = ra; ra = rb;
            rb = p + 32 < end ? src.ld16(p + 32) : z;
        } else {
            v = ci == 0 ? c0 : ci == 1 ? c1 : src.ld16(p);
        }
        const uint32_t k0 = p < beg ? (uint32_t)(beg - p) : 0;
        const uint32_t k1 = end - p < 16 ? (uint32_t)(end - p) : 16;
        for (uint32_t k = 0; k < 16; k++) {
            if (k < k0 || k >= k1) continue;
            const uint32_t word = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
            const uint32_t c = (word >> ((k & 3) * 8)) & 0xFFu;
            if (c == '/') {
                park();
                len = 0; b0 = 0; b1 = 0; ws = p + k + 1;
            } else {
                const uint32_t sh = (len & 3) * 8;
                b0 |= len < 4 ? c << sh : 0u;
                b1 |= len - 4 < 4 ? c << sh : 0u;
                len++;
            }
        }
    }
    ScanOut o;
    o.p = p;
    o.early = !NEED && p < end;
    if (!o.early) park();
    o.lev = lev;
    o.bad = bad;
    return o;
}

// what tokenize derives from the parked levels: badarg over the stored
// levels, and base_init's '$' flag
template <class St, class Src>
void derived(const St &st, const Src &src, uint64_t beg, uint32_t L, bool &bad, bool &dollar) {
    for (uint32_t l = 0; l < L && l < St::maxl; l++) {
        const uint32_t n = st.len[l], c = st.b0[l] & 0xFFu;
        bad |= n == 1 && (c == '+' || c == '#');
    }
    dollar = st.len[0] == 255 ? src.byte(beg) == '$' : st.len[0] >= 1 && (st.b0[0] & 0xFFu) == '$';
}

static uint64_t g_cases = 0;

template <bool NEED, uint32_t ML>
void check(const std::vector<uint8_t> &buf, uint64_t beg, uint64_t end) {
    HostSrc src{buf.data(), buf.size(), beg, end};
    RecStore<ML> a, b;
    const ScanOut ra = scan_reference<NEED>(src, beg, end, a);
    const ScanOut rb = scan_levels<NEED>(src, beg, end, b);
    bool bad_a = ra.bad, bad_b = rb.bad, dol_a = false, dol_b = false;
    if (!ra.early) derived(a, src, beg, ra.lev, bad_a, dol_a);
    if (!rb.early) derived(b, src, beg, rb.lev, bad_b, dol_b);
    const bool same = ra.lev == rb.lev && ra.early == rb.early && ra.p == rb.p && bad_a == bad_b && dol_a == dol_b &&
                      a.puts == b.puts && !memcmp(a.b0, b.b0, sizeof a.b0) && !memcmp(a.b1, b.b1, sizeof a.b1) &&
                      !memcmp(a.len, b.len, sizeof a.len);
    g_cases++;
    if (same) return;
    fprintf(stderr, "MISMATCH need=%d maxl=%u align=%llu topic='%.*s'\n", (int)NEED, ML, (unsigned long long)(beg & 15),
            (int)(end - beg), (const char *)buf.data() + beg);
    fprintf(stderr, "  reference: lev %u early %d p %llu bad %d dollar %d\n", ra.lev, ra.early, (unsigned long long)ra.p,
            bad_a, dol_a);
    fprintf(stderr, "  scan:      lev %u early %d p %llu bad %d dollar %d\n", rb.lev, rb.early, (unsigned long long)rb.p,
            bad_b, dol_b);
    for (uint32_t l = 0; l < ML; l++)
        if (a.b0[l] != b.b0[l] || a.b1[l] != b.b1[l] || a.len[l] != b.len[l])
            fprintf(stderr, "  level %u: reference (%08x, %08x, %u)  scan (%08x, %08x, %u)\n", l, a.b0[l], a.b1[l], a.len[l],
                    b.b0[l], b.b1[l], b.len[l]);
    exit(1);
}

template <uint32_t ML>
void check_both(const std::vector<uint8_t> &buf, uint64_t beg, uint64_t end) {
    check<false, ML>(buf, beg, end);
    check<true, ML>(buf, beg, end);
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*, [0, n)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

// a buffer padded to a 16-byte multiple with the topic at `beg`; the bytes
// around the topic are '/' and letters, which the scan must not see
static std::vector<uint8_t> place(const std::string &t, uint64_t beg) {
    const uint64_t size = (beg + t.size() + 15) / 16 * 16 + (t.empty() && beg % 16 == 0 ? 16 : 0);
    std::vector<uint8_t> buf(size);
    for (uint64_t i = 0; i < size; i++) buf[i] = (i * 7 + beg) % 3 ? '/' : 'x';
    memcpy(buf.data() + beg, t.data(), t.size());
    return buf;
}

int main() {
    // every string over {a, /, +, #, $} up to 7 bytes, at all 16 start alignments
    // (maxl 2 as well: the early exit and the levels past the store)
    const char sym[5] = {'a', '/', '+', '#', '$'};
    for (uint32_t n = 0; n <= 7; n++) {
        uint32_t total = 1;
        for (uint32_t i = 0; i < n; i++) total *= 5;
        for (uint32_t code = 0; code < total; code++) {
            std::string t(n, ' ');
            for (uint32_t i = 0, c = code; i < n; i++, c /= 5) t[i] = sym[c % 5];
            for (uint64_t al = 0; al < 16; al++) {
                const std::vector<uint8_t> buf = place(t, 16 + al);
                check_both<2>(buf, 16 + al, 16 + al + n);
                check_both<8>(buf, 16 + al, 16 + al + n);
                check_both<32>(buf, 16 + al, 16 + al + n);
            }
        }
    }
    // seeded random topics up to 300 bytes: word lengths 0-20, up to 70 levels
    const char alpha[] = "abcdefgh+#$xyz01";
    for (uint32_t it = 0; it < 60000; it++) {
        const uint32_t levels = 1 + rnd(it % 4 == 0 ? 70 : 12);
        const uint32_t wmax = it % 3 == 0 ? 21 : it % 3 == 1 ? 10 : 3;
        std::string t;
        for (uint32_t l = 0; l < levels; l++) {
            uint32_t wl = rnd(wmax);
            if (t.size() + wl + 1 > 300) break;
            if (l) t += '/';
            if (wl == 1 && rnd(3) == 0) { t += "+#$"[rnd(3)]; continue; }
            for (uint32_t i = 0; i < wl; i++) t += alpha[rnd(16)];
        }
        const uint64_t beg = rnd(48);
        const std::vector<uint8_t> buf = place(t, beg);
        check_both<2>(buf, beg, beg + t.size());
        check_both<8>(buf, beg, beg + t.size());
        check_both<32>(buf, beg, beg + t.size());
    }
    // seeded random topics over all 256 byte values (topics are arbitrary binaries: NUL, the high-bit twins
    // 0xAF / 0xAB / 0xA3 / 0xA4 of '/', '+', '#', '$' and the neighbours 0x2E / 0x30 of '/' drawn more often)
    const uint8_t hot[] = {0x00, 0xAF, 0xAB, 0xA3, 0xA4, 0x2E, 0x30, 0x80, 0xFF, 0x7F, '+', '#', '$'};
    for (uint32_t it = 0; it < 60000; it++) {
        const uint32_t n = rnd(it % 4 == 0 ? 301 : it % 4 == 1 ? 40 : 18);
        const uint32_t slash = it % 5 == 0 ? 3 : it % 5 == 1 ? 20 : 8;   // one byte in `slash` is a '/'
        std::string t;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t c = rnd(slash) == 0 ? '/' : rnd(4) == 0 ? hot[rnd(sizeof hot)] : rnd(256);
            t += (char)c;
        }
        const uint64_t beg = rnd(48);
        const std::vector<uint8_t> buf = place(t, beg);
        check_both<2>(buf, beg, beg + t.size());
        check_both<8>(buf, beg, beg + t.size());
        check_both<32>(buf, beg, beg + t.size());
    }
    // slash_mask16 against a byte loop: every pair of byte values at every pair of adjacent positions of a
    // chunk, over backgrounds that hold no '/', only '/', and the bytes one bit away from it
    const uint8_t bg[] = {0x00, 0x2F, 0xAF, 0x2E, 0xFF};
    for (uint32_t g = 0; g < sizeof bg; g++)
        for (uint32_t pos = 0; pos + 1 < 16; pos++)
            for (uint32_t a = 0; a < 256; a++)
                for (uint32_t b = 0; b < 256; b++) {
                    uint8_t c[16];
                    memset(c, bg[g], 16);
                    c[pos] = (uint8_t)a;
                    c[pos + 1] = (uint8_t)b;
                    uint32_t w[4], want = 0;
                    memcpy(w, c, 16);
                    for (uint32_t k = 0; k < 16; k++) want |= (c[k] == '/' ? 1u : 0u) << k;
                    const uint32_t got = slash_mask16(w[0], w[1], w[2], w[3]);
                    g_cases++;
                    if (got == want) continue;
                    fprintf(stderr, "MISMATCH slash_mask16: bytes %02x %02x at %u over %02x: %04x, byte loop %04x\n", a, b, pos,
                            bg[g], got, want);
                    return 1;
                }
    printf("scan ok: %llu cases\n", (unsigned long long)g_cases);
    return 0;
}
