// hints_check.cpp -- the vocab-entry hint functions of emqx_amd/csrc/tm_layout.h
// on the CPU (stand-alone: own main, nothing but the shared header).
//
//  1. hint_alive(hint_of_sum(s), lq, L, wq) false  =>  child_alive(s, lq, L, wq, wq2)
//     false, for random child summaries s built the way the host builds them
//     (flags of Q and QQ, Blooms of random child sets, saturated past
//     PSUM_BLOOM children) and for arbitrary 64-bit summaries; a live slot's
//     hint is never 0 (0 means "no child").
//  2. The hint's Bloom is the slot's folded: a word in Q's child set always has
//     its hint bit set.
//  3. vocab_short_eq accepts exactly equal (len, b0, b1), whatever the hint bits
//     of the entry's tag; a fresh short word's tag is its length alone.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../emqx_amd/csrc/tm_layout.h"

using namespace tmx;

static uint64_t g_s = 0x243f6a8885a308d3ull;
static uint64_t rnd() { g_s += 0x9e3779b97f4a7c15ull; return mix64(g_s); }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t bloom_of(const std::vector<uint32_t> &kids) {
    if (kids.size() > PSUM_BLOOM) return (1ull << PSUM_BLOOM) - 1;
    uint64_t m = 0;
    for (uint32_t w : kids) m |= 1ull << psum_bit(child_hash(w));
    return m;
}

static void check_pair(uint64_t sum, uint32_t lq, uint32_t L, uint32_t wq, uint32_t wq2) {
    const uint32_t lo = (uint32_t)sum, hi = (uint32_t)(sum >> 32);
    const uint32_t h = hint_of_sum(lo, hi);
    CHECK(h != 0 && (h & HINT_CHILD) && h <= HINT_MASK, "hint %x of a live slot", h);
    if (!hint_alive(h, lq, L, wq))
        CHECK(!child_alive(lo, hi, lq, L, wq, wq2), "hint %x dead, slot %llx alive (lq %u L %u wq %u wq2 %u)", h,
              (unsigned long long)sum, lq, L, wq, wq2);
}

int main() {
    uint64_t dead_hint = 0, dead_slot = 0, cases = 0;
    for (int it = 0; it < 400000; it++) {
        // Q's and QQ's flags and child sets, as node_psum lays them out
        const uint32_t fq = below(16), fqq = (fq & PSUM_PLUS) ? below(16) : 0;
        const uint32_t nk[] = {0, 1, 2, 3, 7, 8, 12, 28, 29, 40};
        std::vector<uint32_t> kq(nk[below(10)]), kqq((fq & PSUM_PLUS) ? nk[below(10)] : 0);
        const uint32_t space = 1u << (4 + below(20));
        for (auto &w : kq) w = below(space);
        for (auto &w : kqq) w = below(space);
        const uint64_t sum = fq | (uint64_t)fqq << PSUM_QQ | bloom_of(kq) << PSUM_BQ | bloom_of(kqq) << PSUM_BQQ;
        const uint32_t h = hint_of_sum((uint32_t)sum, (uint32_t)(sum >> 32));
        for (uint32_t w : kq) CHECK((h >> hint_bit(child_hash(w))) & 1u, "child %u not in hint %x", w, h);
        for (int k = 0; k < 8; k++) {
            const uint32_t L = 1 + below(8), lq = 1 + below(L);   // a child is entered at 1 <= lq <= L
            // the topic's next words: a child of Q / QQ, a random word, or unknown to the vocab
            uint32_t wq = NONE, wq2 = NONE;
            if (lq < L) { const uint32_t c = below(4); wq = c == 0 ? NONE : c == 1 && !kq.empty() ? kq[below((uint32_t)kq.size())] : below(space); }
            if (lq + 1 < L) { const uint32_t c = below(4); wq2 = c == 0 ? NONE : c == 1 && !kqq.empty() ? kqq[below((uint32_t)kqq.size())] : below(space); }
            check_pair(sum, lq, L, wq, wq2);
            cases++;
            dead_hint += !hint_alive(h, lq, L, wq);
            dead_slot += !child_alive((uint32_t)sum, (uint32_t)(sum >> 32), lq, L, wq, wq2);
        }
        // any 64 bits at all
        const uint64_t any = rnd() & rnd();
        const uint32_t L = 1 + below(8), lq = 1 + below(L);
        check_pair(any, lq, L, lq < L ? below(space) : NONE, lq + 1 < L ? below(space) : NONE);
    }
    // the shadow is useful, not only safe: it finds most of the dead slots
    CHECK(dead_hint * 2 > dead_slot && dead_hint <= dead_slot, "dead by hint %llu, by slot %llu of %llu",
          (unsigned long long)dead_hint, (unsigned long long)dead_slot, (unsigned long long)cases);

    // short-word compare: exactly (len, b0, b1), hints ignored
    for (int it = 0; it < 400000; it++) {
        const uint32_t len = below(VINL + 1);
        uint32_t b0 = (uint32_t)rnd(), b1 = (uint32_t)rnd();
        if (len < 8) b1 &= len > 4 ? (1u << (8 * (len - 4))) - 1 : 0;
        if (len < 4) b0 &= len ? (1u << (8 * len)) - 1 : 0;
        CHECK(vocab_tag(rnd(), len) == len, "fresh tag of a short word");
        const uint32_t tag = vocab_tag(0, len) | (uint32_t)rnd() << HINT_SHIFT0;
        CHECK(vocab_short_eq(tag, b0, b1, len, b0, b1), "equal word refused");
        CHECK(!vocab_short_eq(tag, b0, b1, (len + 1 + below(VINL)) % (VINL + 1), b0, b1), "another length accepted");
        CHECK(!vocab_short_eq(tag, b0, b1, len, b0 ^ (1u << below(32)), b1), "other bytes (b0) accepted");
        CHECK(!vocab_short_eq(tag, b0, b1, len, b0, b1 ^ (1u << below(32))), "other bytes (b1) accepted");
    }
    // "a" and "a\0" pack to the same bytes: the length tells them apart
    CHECK(!vocab_short_eq(vocab_tag(0, 1), 'a', 0, 2, 'a', 0), "a vs a NUL");
    // a long word's tag keeps its length byte above VINL: no short compare takes it
    for (uint32_t len = VINL + 1; len < 300; len++) CHECK((vocab_tag(rnd(), len) & 0xFFu) > VINL, "long tag");
    static_assert(HINT_SHIFT0 == 8 && HINT_SHIFT1 == HINT_SHIFT0 + HINT_BITS && HINT_SHIFT1 + HINT_BITS == 32, "tag layout");
    static_assert((NLIT_MASK & (NLIT_HDESC | NLIT_ANX0 | NLIT_ANX1)) == 0, "nlit flags");
    static_assert(PSUM_BLOOM == 4 * HINT_BLOOM, "the hint's Bloom folds the slot's four to one");

    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("hints ok: %llu cases, dead by hint %llu, by slot %llu\n", (unsigned long long)cases,
           (unsigned long long)dead_hint, (unsigned long long)dead_slot);
    return 0;
}
