// tm_subs.h -- the host side of the value -> local subscriber list table
// (tm_set_subscribers): a pool of u32 subscriber ids and one (position, count)
// span per value.  No HIP here: tests/subs_cpu drives it on its own.
//
// A value's list lives in a block of 2^c words (the scheme tm_layout.h uses
// for `vals`): a new list that fits the value's block is written in place, a
// longer one takes a block from its class's free list or from the pool's end
// and the old block goes to its own free list.  Every write widens a dirty
// range (spans and pool separately) that the device copies are brought up to
// date from.  `tight` is what the live lists need (the sum of their smallest
// blocks); when the rest of the pool -- free blocks, blocks larger than their
// list needs -- exceeds the live words the pool is rewritten tight in value
// order and everything is dirty.  Right after a compaction the pool holds at
// most 2 x the live words.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

namespace tmx {

struct SubPool {
    std::vector<uint32_t> span;   // [2 v] the list's position in `pool`, [2 v + 1] its count
    std::vector<uint32_t> pool;
    std::vector<uint8_t> cls;     // per value: 1 + its block's class (the block holds 1 << class words), 0: no block
    std::vector<uint32_t> free_[33];   // per class: positions of free blocks
    uint64_t live = 0;            // words of the lists
    uint64_t tight = 0;           // words of the smallest blocks that would hold them
    uint64_t compactions = 0;
    // dirty since take_dirty(): span words [s_lo, s_hi), pool words [p_lo, p_hi);
    // `whole`: the pool was rewritten (its size may have shrunk): all of both
    uint64_t s_lo = 0, s_hi = 0, p_lo = 0, p_hi = 0;
    bool whole = false;

    static uint32_t class_of(uint32_t n) {   // the smallest c with (1 << c) >= n, n >= 1
        uint32_t c = 0;
        while (((uint64_t)1 << c) < n) c++;
        return c;
    }
    static void widen(uint64_t &lo, uint64_t &hi, uint64_t a, uint64_t b) {
        if (a >= b) return;
        if (hi > lo) { lo = std::min(lo, a); hi = std::max(hi, b); }
        else { lo = a; hi = b; }
    }
    uint64_t garbage() const { return pool.size() - tight; }
    uint64_t values() const { return span.size() / 2; }

    void release(uint32_t v) {
        if (!cls[v]) return;
        const uint32_t c = cls[v] - 1u, cnt = span[2 * (uint64_t)v + 1];
        free_[c].push_back(span[2 * (uint64_t)v]);
        live -= cnt;
        tight -= (uint64_t)1 << class_of(cnt);
        cls[v] = 0;
    }

    // value v's list becomes ids[0 .. n).  false: the pool would pass 2^32 - 1
    // words (nothing changed); std::bad_alloc passes through.
    bool set(uint32_t v, const uint32_t *ids, uint32_t n) {
        const uint64_t need = 2 * ((uint64_t)v + 1);
        if (need > span.size()) {
            // the spans between the old end and v are (0, 0) on the host: they
            // go up too, so no device span below the length is one the host never wrote
            const uint64_t old = span.size();
            cls.resize((uint64_t)v + 1, 0);
            span.resize(need, 0);
            widen(s_lo, s_hi, old, need);
        }
        uint32_t *sp = &span[2 * (uint64_t)v];
        if (!n) {
            if (cls[v]) {
                release(v);
                sp[0] = sp[1] = 0;
                widen(s_lo, s_hi, 2 * (uint64_t)v, need);
                maybe_compact();
            }
            return true;
        }
        const uint32_t c = class_of(n);
        if (cls[v] && cls[v] - 1u >= c) {   // fits its block: in place
            live = live - sp[1] + n;
            tight = tight - ((uint64_t)1 << class_of(sp[1])) + ((uint64_t)1 << c);
        } else {
            uint32_t pos;
            if (!free_[c].empty()) {
                pos = free_[c].back();
                free_[c].pop_back();
            } else {
                const uint64_t end = pool.size() + ((uint64_t)1 << c);
                if (end > 0xFFFFFFFFull) return false;
                pos = (uint32_t)pool.size();
                pool.resize(end, 0);
                widen(p_lo, p_hi, pos, end);   // (the block's tail too: every word below the length is the host's)
            }
            release(v);
            cls[v] = (uint8_t)(c + 1);
            sp[0] = pos;
            live += n;
            tight += (uint64_t)1 << c;
        }
        sp[1] = n;
        std::copy(ids, ids + n, pool.begin() + sp[0]);
        widen(p_lo, p_hi, sp[0], (uint64_t)sp[0] + n);
        widen(s_lo, s_hi, 2 * (uint64_t)v, need);
        maybe_compact();
        return true;
    }

    void maybe_compact() {
        if (garbage() > live) compact();
    }

    // the pool rewritten tight, in value order
    void compact() {
        std::vector<uint32_t> np;
        np.reserve(tight);
        for (uint64_t v = 0; v < cls.size(); v++) {
            if (!cls[v]) continue;
            const uint32_t pos = span[2 * v], cnt = span[2 * v + 1], c = class_of(cnt);
            span[2 * v] = (uint32_t)np.size();
            np.insert(np.end(), pool.begin() + pos, pool.begin() + pos + cnt);
            np.resize(np.size() + (((uint64_t)1 << c) - cnt), 0);
            cls[v] = (uint8_t)(c + 1);
        }
        pool.swap(np);
        for (auto &f : free_) f.clear();
        compactions++;
        whole = true;
        s_lo = 0; s_hi = span.size();
        p_lo = 0; p_hi = pool.size();
    }

    // what changed since the last call; the ranges start empty again
    void take_dirty(uint64_t &slo, uint64_t &shi, uint64_t &plo, uint64_t &phi, bool &all) {
        slo = s_lo; shi = s_hi; plo = p_lo; phi = p_hi; all = whole;
        s_lo = s_hi = p_lo = p_hi = 0;
        whole = false;
    }
};

}  // namespace tmx
