// image_walk.h -- a plain reference walker over a DevIndex and two audits of the
// derived state the walk kernels trust (tests/test_image_cpu.py).
//
// The walker decides everything from the PRIMARY structure alone: Node.plus,
// the inline kw / kc pairs or a scan of the node's whole ctab range for the
// wid, the hash_* / exact_* runs with RUN_INLINE, the vocab by byte comparison
// and the exact table by full key comparison.  It never asks a Bloom, a
// summary, a hint, a bitmap or a fingerprint whether to go on.  It visits in
// the reference's order ('#' terminal, '+' subtree, literal subtree, the exact
// key last; at the topic's end the node's own terminal before its '#'), skips
// the root's '#' and '+' for a '$' topic, and applies the NLIT_HDESC seek of
// tm_layout.h.  Its cut (the topic ends at such a node) keeps the pending
// literal branches up to the innermost '+' of the path; visiting recursively
// in this order, the only branches still pending belong to '+' edges of the
// path, so the cut drops nothing here and is only counted.
//
// Audit by use (during every walk): wherever the primary structure says a
// child exists and its subtree gave at least one hit for this topic, whatever
// the parent holds about that child must say "alive" -- else a kernel that
// trusts it loses exactly these hits.
//
// Full audit (over a whole DevIndex): every derived word recomputed from the
// primary structure and compared, with code written here (the TM_HD helpers of
// tm_layout.h excepted, as in tests/hints_cpu/hints_check.cpp).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../emqx_amd/csrc/tm_dev.h"
#include "fake_hip.h"

namespace imgw {

using namespace tmx;

// what the driver is doing (scenario, step, check), named by every failure
inline std::string &context() { static std::string c; return c; }

[[noreturn]] inline void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "IMAGE CHECK FAILED: [%s] ", context().c_str());
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    fflush(stderr);
    exit(1);
}

inline std::string show(const uint8_t *p, size_t n) {
    std::string o;
    char b[8];
    for (size_t i = 0; i < n && i < 200; i++) {
        if (p[i] >= 0x20 && p[i] < 0x7f && p[i] != '\\') o.push_back((char)p[i]);
        else { snprintf(b, sizeof b, "\\x%02x", p[i]); o += b; }
    }
    return o;
}

// ---- sizes of the tables a view points at, from the fake's allocation sizes

struct Bounds { size_t nodes, ctab, vals, wpool, wseq, wbits, vocab, exact, xfp; };
inline Bounds bounds_of(const DevIndex &ix) {
    Bounds b;
    b.nodes = fake_hip_room(ix.nodes) / sizeof(Node);
    b.ctab = fake_hip_room(ix.ctab) / sizeof(CSlot);
    b.vals = fake_hip_room(ix.vals) / 4;
    b.wpool = fake_hip_room(ix.wpool);
    b.wseq = fake_hip_room(ix.wseq) / 4;
    b.wbits = fake_hip_room(ix.wbits) / 4;
    b.vocab = fake_hip_room(ix.vocab) / sizeof(VocabEntry);
    b.exact = fake_hip_room(ix.exact) / sizeof(ExactEntry);
    b.xfp = fake_hip_room(ix.xfp) / 2;
    return b;
}

inline uint32_t nlit_of(const Node &n) { return n.nlit & NLIT_MASK; }
inline bool table_mode(const Node &n) { return nlit_of(n) > KINL; }
inline bool wide_mode(const Node &n) { return nlit_of(n) >= WIDE_LIT; }   // the host turns a node wide at WIDE_LIT children

// ---- words

inline void pack_short(const uint8_t *p, uint32_t n, uint32_t &b0, uint32_t &b1) {
    b0 = b1 = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (i < 4) b0 |= (uint32_t)p[i] << (8 * i);
        else b1 |= (uint32_t)p[i] << (8 * (i - 4));
    }
}
inline uint64_t hash_word(const uint8_t *p, uint32_t n) {
    if (n <= VINL) {
        uint32_t b0, b1;
        pack_short(p, n, b0, b1);
        return word_hash_short(b0, b1, n);
    }
    uint64_t x = FNV_OFF;
    for (uint32_t i = 0; i < n; i++) x = (x ^ p[i]) * FNV_PRIME;
    return word_hash_finish(x, n);
}

// does vocab entry e hold the bytes (p, n)?  Bytes and length only.
inline bool entry_is(const DevIndex &ix, const Bounds &bd, const VocabEntry &e, const uint8_t *p, uint32_t n) {
    const uint32_t tl = e.tag & 0xFFu;
    if (n <= VINL) {
        uint32_t b0, b1;
        pack_short(p, n, b0, b1);
        return vocab_short_eq(e.tag, e.b0, e.b1, n, b0, b1);
    }
    if (tl <= VINL || e.b1 != n) return false;
    if ((size_t)e.b0 + n > bd.wpool) die("vocab entry of wid %u: word bytes [%u, +%u) leave wpool (%zu bytes)", e.wid, e.b0, n, bd.wpool);
    return !memcmp(ix.wpool + e.b0, p, n);
}

// wid of (p, n), or NONE; *slot: its vocab slot
inline uint32_t find_word(const DevIndex &ix, const Bounds &bd, const uint8_t *p, uint32_t n, uint32_t *slot) {
    const uint64_t h = hash_word(p, n);
    if ((size_t)ix.vmask + 1 > bd.vocab) die("vmask %u past the vocab allocation (%zu entries)", ix.vmask, bd.vocab);
    uint32_t s = (uint32_t)h & ix.vmask;
    for (uint32_t probes = 0; probes <= ix.vmask; probes++, s = (s + 1) & ix.vmask) {
        const VocabEntry &e = ix.vocab[s];
        if (e.wid == NONE) return NONE;
        if (entry_is(ix, bd, e, p, n)) { if (slot) *slot = s; return e.wid; }
    }
    return NONE;
}

// ---- a topic

struct Level { uint32_t off, len, wid, hint[ANX_SLOTS]; bool has_hint; };
struct Topic {
    const uint8_t *p = nullptr; uint32_t n = 0;
    std::vector<Level> lv;
    int err = 0;          // 1: a '+' / '#' level (badarg), 2: more than MAX_LEVELS levels
    bool dollar = false, all_found = true;
};

inline void parse_topic(const DevIndex &ix, const Bounds &bd, const uint8_t *p, uint32_t n, Topic &t) {
    t = Topic{};
    t.p = p; t.n = n;
    uint32_t s = 0;
    uint64_t levels = 0;
    for (uint32_t i = 0; i <= n; i++)
        if (i == n || p[i] == '/') {
            const uint32_t len = i - s;
            if (len == 1 && (p[s] == '+' || p[s] == '#')) t.err = 1;
            levels++;
            if (levels <= (uint64_t)MAX_LEVELS) t.lv.push_back(Level{s, len, NONE, {0, 0}, false});
            s = i + 1;
        }
    if (t.err == 1) { t.lv.clear(); return; }
    if (levels > (uint64_t)MAX_LEVELS) { t.err = 2; t.lv.clear(); return; }
    t.dollar = t.lv[0].len >= 1 && p[t.lv[0].off] == '$';
    for (Level &l : t.lv) {
        uint32_t slot = NONE;
        l.wid = find_word(ix, bd, p + l.off, l.len, &slot);
        if (l.wid == NONE) { t.all_found = false; continue; }
        if (l.len <= VINL) {
            l.has_hint = true;
            l.hint[0] = (ix.vocab[slot].tag >> HINT_SHIFT0) & HINT_MASK;
            l.hint[1] = (ix.vocab[slot].tag >> HINT_SHIFT1) & HINT_MASK;
        }
    }
}

// ---- the walk

struct UseStats {
    uint64_t topics = 0, nodes = 0, hits = 0, cuts = 0, seeks = 0;
    uint64_t psum_used = 0, slot_sum_used = 0, bloom_used = 0, wbits_used = 0, hint_used[ANX_SLOTS] = {0, 0};
    uint64_t xfp_used = 0, xfp_path_slots = 0;
};

struct Walker {
    const DevIndex &ix;
    Bounds bd;
    UseStats &st;
    const Topic *t = nullptr;
    std::vector<uint32_t> *out = nullptr;
    std::vector<uint32_t> path;   // node ids from the root, for messages

    Walker(const DevIndex &ix_, UseStats &st_) : ix(ix_), bd(bounds_of(ix_)), st(st_) {}

    std::string where(uint32_t level) const {
        std::string s = "topic '" + show(t->p, t->n) + "', node path";
        char b[16];
        for (uint32_t id : path) { snprintf(b, sizeof b, " %u", id); s += b; }
        if (level < t->lv.size())
            s += ", word '" + show(t->p + t->lv[level].off, t->lv[level].len) + "'";
        return s;
    }
    const Node &node(uint32_t id) const {
        if (id >= bd.nodes) die("node id %u past the nodes allocation (%zu)", id, bd.nodes);
        return ix.nodes[id];
    }
    uint64_t emit(uint32_t off, uint32_t cnt) {
        const uint32_t c = cnt & RUN_CNT;
        if (!c) return 0;
        if (cnt & RUN_INLINE) {
            if (c != 1) die("an inline run of %u values (%s)", c, where(NONE).c_str());
            out->push_back(off);
            return 1;
        }
        if (c == 1) die("a run of one value that is not inline (%s)", where(NONE).c_str());
        if ((size_t)off + c > bd.vals) die("value run [%u, +%u) leaves vals (%zu words) (%s)", off, c, bd.vals, where(NONE).c_str());
        for (uint32_t i = 0; i < c; i++) out->push_back(ix.vals[off + i]);
        return c;
    }
    // the literal child of n for wid w, from the inline pairs or the whole table range; *slot: its CSlot
    uint32_t lit_child(const Node &n, uint32_t w, const CSlot **slot) const {
        *slot = nullptr;
        if (!table_mode(n)) {
            for (uint32_t k = 0; k < KINL; k++) if (n.kw[k] == w) return n.kc[k];
            return NONE;
        }
        if ((size_t)n.kw[0] + n.kw[1] + 1 > bd.ctab) die("child table [%u, +%u] leaves ctab (%zu slots)", n.kw[0], n.kw[1], bd.ctab);
        for (uint32_t i = 0; i <= n.kw[1]; i++) {
            const CSlot &c = ix.ctab[n.kw[0] + i];
            if (c.wid == w) { *slot = &c; return c.child; }
        }
        return NONE;
    }

    struct R { uint64_t hits; };

    R visit(uint32_t id, uint32_t l) {
        const uint32_t L = (uint32_t)t->lv.size();
        const Node &n = node(id);
        path.push_back(id);
        st.nodes++;
        R r{0};
        const bool droot = t->dollar && l == 0;
        if (l == L) {
            r.hits += emit(n.exact_off, n.exact_cnt);
            if (!droot) r.hits += emit(n.hash_off, n.hash_cnt);
            if (n.nlit & NLIT_HDESC) st.cuts++;   // the cut (the header): nothing is left for it to drop
            path.pop_back();
            return r;
        }
        if (!droot) r.hits += emit(n.hash_off, n.hash_cnt);
        const uint32_t w = t->lv[l].wid;
        const uint32_t wq = l + 1 < L ? t->lv[l + 1].wid : NONE, wq2 = l + 2 < L ? t->lv[l + 2].wid : NONE;
        const CSlot *slot = nullptr;
        const uint32_t lit = w == NONE ? NONE : lit_child(n, w, &slot);
        if (n.nlit & NLIT_HDESC) st.seeks++;   // [P,'#',...] seeks to P/W past P's '+' subtree
        if (!droot && !(n.nlit & NLIT_HDESC) && n.plus != NONE) {
            const R q = visit(n.plus, l + 1);
            r.hits += q.hits;
            if (q.hits) {
                st.psum_used++;
                if (!child_alive(n.psum_lo, n.psum_hi, l + 1, L, wq, wq2))
                    die("audit by use: psum %08x:%08x of node %u calls its '+' child %u dead, but the child's subtree gave %llu "
                        "hits (%s)", n.psum_hi, n.psum_lo, id, n.plus, (unsigned long long)q.hits, where(l).c_str());
            }
            // A cut below (the topic ended at an NLIT_HDESC node) seeks to the literal branch of the
            // innermost '+' of its path -- this frame's, which is the one branch still to visit here:
            // in this visiting order the cut drops nothing, and without a '+' above it nothing is left.
        }
        if (lit != NONE) {
            const R q = visit(lit, l + 1);
            r.hits += q.hits;
            if (q.hits) audit_lit(n, id, l, w, slot, wq, wq2, q.hits);
        }
        path.pop_back();
        return r;
    }

    void audit_lit(const Node &n, uint32_t id, uint32_t l, uint32_t w, const CSlot *slot, uint32_t wq, uint32_t wq2,
                   uint64_t hits) {
        const uint32_t L = (uint32_t)t->lv.size();
        if (!table_mode(n)) return;   // an inline-mode parent keeps nothing about its children
        st.slot_sum_used++;
        if (!child_alive(slot->sum_lo, slot->sum_hi, l + 1, L, wq, wq2))
            die("audit by use: the slot summary %08x:%08x node %u holds of its child %u calls it dead, but its subtree gave "
                "%llu hits (%s)", slot->sum_hi, slot->sum_lo, id, slot->child, (unsigned long long)hits, where(l).c_str());
        if (!wide_mode(n)) {
            const uint32_t b = child_bit(child_hash(w));
            const uint32_t word = b < 64 ? n.kw[2 + (b >> 5)] : n.kc[(b >> 5) - 2];
            st.bloom_used++;
            if (!((word >> (b & 31)) & 1u))
                die("audit by use: Bloom bit %u of node %u is clear for child wid %u, whose subtree gave hits (%s)", b, id, w,
                    where(l).c_str());
        } else if (n.kw[2] != NONE) {
            st.wbits_used++;
            if (w >= ix.wcap) die("audit by use: wid %u of a wide node's child is past wcap %u (%s)", w, ix.wcap, where(l).c_str());
            if ((size_t)n.kw[2] + (w >> 5) >= bd.wbits) die("wide node %u: its bitmap leaves wbits (%s)", id, where(l).c_str());
            if (!((ix.wbits[n.kw[2] + (w >> 5)] >> (w & 31)) & 1u))
                die("audit by use: the bitmap of wide node %u has no bit for child wid %u, whose subtree gave hits (%s)", id, w,
                    where(l).c_str());
        }
        for (uint32_t s = 0; s < ANX_SLOTS; s++) {
            if (!(n.nlit & (s ? NLIT_ANX1 : NLIT_ANX0)) || !t->lv[l].has_hint) continue;
            const uint32_t h = t->lv[l].hint[s];
            st.hint_used[s]++;
            if (ix.anx_depth[s] != l)
                die("audit by use: node %u at depth %u carries the flag of annex slot %u, whose depth is %u (%s)", id, l, s,
                    ix.anx_depth[s], where(l).c_str());
            if (!(h & HINT_CHILD) || !hint_alive(h, l + 1, L, wq))
                die("audit by use: hint %03x (slot %u) of the word says annexed node %u has no live child for it, but the "
                    "child's subtree gave hits (%s)", h, s, id, where(l).c_str());
        }
    }

    // the topic's binary key, by full key comparison along the probe path
    uint64_t exact_key() {
        if (!t->all_found) return 0;
        const uint32_t L = (uint32_t)t->lv.size();
        uint64_t x = FNV_OFF;
        for (const Level &l : t->lv) x = seq_hash_step(x, l.wid);
        const uint64_t h = seq_hash_finish(x, L);
        if ((size_t)ix.xmask + 1 > bd.exact || (size_t)ix.xmask + 1 > bd.xfp)
            die("xmask %u past the exact (%zu) or xfp (%zu) allocation", ix.xmask, bd.exact, bd.xfp);
        uint32_t s = (uint32_t)h & ix.xmask;
        std::vector<uint32_t> crossed;
        for (uint32_t probes = 0; probes <= ix.xmask; probes++, s = (s + 1) & ix.xmask) {
            const ExactEntry &e = ix.exact[s];
            if (e.nlev == NONE) return 0;
            crossed.push_back(s);
            if (e.nlev != L) continue;
            const uint32_t *ws = e.wids;
            if (L > XINL) {
                if ((size_t)e.seq_off + L > bd.wseq) die("exact slot %u: wid run [%u, +%u) leaves wseq (%zu)", s, e.seq_off, L, bd.wseq);
                ws = ix.wseq + e.seq_off;
            }
            bool eq = true;
            for (uint32_t i = 0; i < L && eq; i++) eq = ws[i] == t->lv[i].wid;
            if (!eq) continue;
            const uint64_t got = emit(e.val_off, e.val_cnt);
            if (got) {
                st.xfp_used++;
                if (ix.xfp[s] != exact_fp(h))
                    die("audit by use: xfp[%u] = %04x, the key's fingerprint is %04x (%s)", s, ix.xfp[s], exact_fp(h),
                        where(NONE).c_str());
                for (uint32_t c : crossed) {
                    st.xfp_path_slots++;
                    if (!ix.xfp[c])
                        die("audit by use: xfp[%u] is 0 on the probe path of the key in slot %u (%s)", c, s, where(NONE).c_str());
                }
            }
            return got;
        }
        return 0;
    }

    // -> err (0 / 1 / 2); the hits in traversal order appended to *vals
    int match(const uint8_t *p, uint32_t n, std::vector<uint32_t> &vals) {
        Topic tp;
        parse_topic(ix, bd, p, n, tp);
        st.topics++;
        if (tp.err) return tp.err;
        t = &tp;
        out = &vals;
        path.clear();
        const size_t before = vals.size();
        visit(ROOT, 0);
        path.clear();
        exact_key();
        st.hits += vals.size() - before;
        t = nullptr;
        return 0;
    }
};

// ---- the full audit

struct AuditStats {
    uint64_t nodes = 0, deepest = 0, words = 0, long_words = 0, exact_keys = 0, long_keys = 0;
    uint64_t compared = 0;                 // derived words compared for equality
    uint64_t psum = 0, slot_sums = 0, blooms = 0, bitmaps = 0, dense_wide = 0, hints[ANX_SLOTS] = {0, 0},
             hints_nonzero[ANX_SLOTS] = {0, 0}, xfp = 0, qq_saturated = 0, q_saturated = 0, hdesc_nodes = 0;
    uint64_t ctab_wrapped = 0, exact_wrapped = 0, vocab_wrapped = 0;   // entries that sit below their home slot
    uint64_t wpool_end = 0, wseq_end = 0;                               // the pools' live extents
    uint64_t depth_slack = 0, xlen_extra = 0, hdesc_extra = 0, bloom_extra = 0;          // sufficiency fields larger than needed (reported)
    std::unordered_map<uint32_t, uint64_t> node_path, wid_bytes;        // id -> hash of its path / of its bytes
    std::vector<uint32_t> wide_ids, bloom_ids;                          // wide nodes / table-mode nodes with a Bloom
    std::unordered_map<uint32_t, uint32_t> word_off;                    // long words: wid -> offset in wpool
    std::unordered_map<uint64_t, uint32_t> key_off;                     // long binary keys: hash -> offset in wseq
};

struct Auditor {
    const DevIndex &ix;
    Bounds bd;
    AuditStats &a;
    std::vector<uint32_t> wslot;   // wid -> vocab slot
    uint32_t anx_node[ANX_SLOTS] = {NONE, NONE};

    Auditor(const DevIndex &ix_, AuditStats &a_) : ix(ix_), bd(bounds_of(ix_)), a(a_) {}

    static uint64_t flags_of(const Node &n) {
        return (uint64_t)((n.hash_cnt & RUN_CNT) ? PSUM_HASH : 0) | ((n.exact_cnt & RUN_CNT) ? PSUM_EXACT : 0) |
               (n.plus != NONE ? PSUM_PLUS : 0) | ((n.nlit & NLIT_HDESC) ? PSUM_HDESC : 0);
    }
    const Node &node(uint32_t id) const {
        if (id >= bd.nodes) die("full audit: node id %u past the nodes allocation (%zu)", id, bd.nodes);
        return ix.nodes[id];
    }
    // the children of a node from the primary structure: (wid, child, slot or null)
    struct Kid { uint32_t wid, child; const CSlot *slot; uint32_t at; };
    void kids_of(uint32_t id, std::vector<Kid> &out) const {
        const Node &n = node(id);
        out.clear();
        if (!table_mode(n)) {
            for (uint32_t k = 0; k < KINL; k++) {
                if (n.kw[k] != NONE) out.push_back(Kid{n.kw[k], n.kc[k], nullptr, k});
                else if (n.kc[k] != NONE) die("full audit: node %u: inline pair %u has no word but child %u", id, k, n.kc[k]);
            }
            return;
        }
        const uint32_t mask = n.kw[1];
        if ((mask & (mask + 1)) != 0 || (size_t)n.kw[0] + mask + 1 > bd.ctab)
            die("full audit: node %u: child table [%u, +%u] is not a power of two inside ctab (%zu)", id, n.kw[0], mask, bd.ctab);
        for (uint32_t i = 0; i <= mask; i++) {
            const CSlot &c = ix.ctab[n.kw[0] + i];
            if (c.wid != NONE) out.push_back(Kid{c.wid, c.child, &c, i});
        }
    }
    uint64_t bloom28(const std::vector<Kid> &k) const {
        if (k.size() > PSUM_BLOOM) return (1ull << PSUM_BLOOM) - 1;
        uint64_t m = 0;
        for (const Kid &c : k) m |= 1ull << psum_bit(child_hash(c.wid));
        return m;
    }
    // the summary a parent keeps of node q, from the primary structure
    uint64_t summary(uint32_t q) const {
        std::vector<Kid> k;
        kids_of(q, k);
        const Node &n = node(q);
        uint64_t m = flags_of(n) | bloom28(k) << PSUM_BQ;
        if (k.size() > PSUM_BLOOM) a.q_saturated++;
        if (n.plus != NONE) {
            std::vector<Kid> kk;
            kids_of(n.plus, kk);
            m |= flags_of(node(n.plus)) << PSUM_QQ | bloom28(kk) << PSUM_BQQ;
            if (kk.size() > PSUM_BLOOM) a.qq_saturated++;
        }
        return m;
    }
    void run_ok(uint32_t off, uint32_t cnt, const char *what, uint32_t id) const {
        const uint32_t c = cnt & RUN_CNT;
        if (cnt & RUN_INLINE) { if (c != 1) die("full audit: %s of %u: an inline run of %u values", what, id, c); return; }
        if (!c) return;
        if (c == 1) die("full audit: %s of %u: one value, not inline", what, id);
        // (+ 3: the emit kernel copies runs in 16-byte loads that may overhang one by 3 words, tm_host.cpp collect)
        if ((size_t)off + c + 3 > bd.vals) die("full audit: %s of %u: run [%u, +%u) and a quad's overhang leave vals (%zu)", what, id, off, c, bd.vals);
        for (uint32_t i = 1; i < c; i++)
            if (ix.vals[off + i - 1] >= ix.vals[off + i]) die("full audit: %s of %u: values not ascending at %u", what, id, i);
    }

    void vocab() {
        if ((size_t)ix.vmask + 1 > bd.vocab || (ix.vmask & (ix.vmask + 1)))
            die("full audit: vmask %u is no power of two minus one inside the vocab allocation (%zu)", ix.vmask, bd.vocab);
        for (uint32_t s = 0; s <= ix.vmask; s++) {
            const VocabEntry &e = ix.vocab[s];
            if (e.wid == NONE) continue;
            a.words++;
            const uint32_t tl = e.tag & 0xFFu;
            std::string w;
            if (tl <= VINL) {
                for (uint32_t i = 0; i < tl; i++) w.push_back((char)(((i < 4 ? e.b0 : e.b1) >> (8 * (i % 4))) & 0xFF));
                uint32_t b0, b1;
                pack_short(reinterpret_cast<const uint8_t *>(w.data()), tl, b0, b1);
                if (b0 != e.b0 || b1 != e.b1) die("full audit: vocab slot %u: a short word's padding is not zero", s);
            } else {
                a.long_words++;
                if (e.b1 <= VINL || (size_t)e.b0 + e.b1 > bd.wpool)
                    die("full audit: vocab slot %u: long word [%u, +%u) leaves wpool (%zu)", s, e.b0, e.b1, bd.wpool);
                w.assign(reinterpret_cast<const char *>(ix.wpool + e.b0), e.b1);
                if (tl != (e.b1 < 255 ? e.b1 : 255)) die("full audit: vocab slot %u: tag length %u for a word of %u bytes", s, tl, e.b1);
                a.wpool_end = std::max<uint64_t>(a.wpool_end, (uint64_t)e.b0 + e.b1);
                a.word_off[e.wid] = e.b0;
            }
            const uint64_t h = hash_word(reinterpret_cast<const uint8_t *>(w.data()), (uint32_t)w.size());
            if (tl > VINL) {
                a.compared++;
                if (e.tag != vocab_tag(h, (uint32_t)w.size())) die("full audit: vocab slot %u: tag %08x, the word's is %08x", s, e.tag, vocab_tag(h, (uint32_t)w.size()));
            }
            const uint32_t home = (uint32_t)h & ix.vmask;
            if (s < home) a.vocab_wrapped++;
            for (uint32_t j = home; j != s; j = (j + 1) & ix.vmask)
                if (ix.vocab[j].wid == NONE) die("full audit: vocab slot %u (wid %u): empty slot %u between its home %u and it", s, e.wid, j, home);
            if (e.wid >= wslot.size()) wslot.resize((size_t)e.wid + 1, NONE);
            if (wslot[e.wid] != NONE) die("full audit: wid %u in vocab slots %u and %u", e.wid, wslot[e.wid], s);
            wslot[e.wid] = s;
            a.wid_bytes[e.wid] = hash_word(reinterpret_cast<const uint8_t *>(w.data()), (uint32_t)w.size()) ^ (uint64_t)w.size() << 56;
        }
    }

    void exact() {
        if ((size_t)ix.xmask + 1 > bd.exact || (size_t)ix.xmask + 1 > bd.xfp || (ix.xmask & (ix.xmask + 1)))
            die("full audit: xmask %u is no power of two minus one inside exact (%zu) and xfp (%zu)", ix.xmask, bd.exact, bd.xfp);
        uint64_t mask_need = 0;
        uint32_t max_need = 0;
        for (uint32_t s = 0; s <= ix.xmask; s++) {
            const ExactEntry &e = ix.exact[s];
            a.compared++;
            if (e.nlev == NONE) {
                if (ix.xfp[s]) die("full audit: xfp[%u] = %04x on an empty exact slot", s, ix.xfp[s]);
                continue;
            }
            a.exact_keys++;
            a.xfp++;
            const uint32_t *ws = e.wids;
            if (e.nlev > XINL) {
                a.long_keys++;
                if ((size_t)e.seq_off + e.nlev > bd.wseq) die("full audit: exact slot %u: wid run [%u, +%u) leaves wseq (%zu)", s, e.seq_off, e.nlev, bd.wseq);
                ws = ix.wseq + e.seq_off;
                a.wseq_end = std::max<uint64_t>(a.wseq_end, (uint64_t)e.seq_off + e.nlev);
            }
            uint64_t x = FNV_OFF;
            for (uint32_t i = 0; i < e.nlev; i++) {
                if (ws[i] >= wslot.size() || wslot[ws[i]] == NONE) die("full audit: exact slot %u: level %u uses wid %u, which the vocab lacks", s, i, ws[i]);
                x = seq_hash_step(x, ws[i]);
            }
            const uint64_t h = seq_hash_finish(x, e.nlev);
            a.compared += 2;
            if (e.h_lo != (uint32_t)h || e.h_hi != (uint32_t)(h >> 32)) die("full audit: exact slot %u: stored hash differs from its key's", s);
            if (ix.xfp[s] != exact_fp(h)) die("full audit: xfp[%u] = %04x, the key's fingerprint is %04x", s, ix.xfp[s], exact_fp(h));
            const uint32_t home = (uint32_t)h & ix.xmask;
            if (s < home) a.exact_wrapped++;
            for (uint32_t j = home; j != s; j = (j + 1) & ix.xmask)
                if (ix.exact[j].nlev == NONE) die("full audit: exact slot %u: empty slot %u between its home %u and it", s, j, home);
            if (e.nlev > XINL) a.key_off[h] = e.seq_off;
            if (!(e.val_cnt & RUN_CNT)) die("full audit: exact slot %u is live with no value", s);
            run_ok(e.val_off, e.val_cnt, "exact slot", s);
            if (e.nlev < 64) mask_need |= 1ull << e.nlev;
            max_need = std::max(max_need, e.nlev);
        }
        if ((ix.xlen_mask & mask_need) != mask_need) die("full audit: xlen_mask %016llx lacks a live key length (needed %016llx)", (unsigned long long)ix.xlen_mask, (unsigned long long)mask_need);
        if (ix.xlen_max < max_need) die("full audit: xlen_max %u below the longest live key (%u levels)", ix.xlen_max, max_need);
        a.xlen_extra = (uint64_t)__builtin_popcountll(ix.xlen_mask & ~mask_need) + (ix.xlen_max - max_need);
    }

    void tree() {
        struct Item { uint32_t id, depth; uint64_t ph; };
        std::vector<Item> stack{Item{ROOT, 0, 0x1234567ull}};
        std::vector<Kid> kids;
        std::vector<uint8_t> seen(bd.nodes, 0);
        while (!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            const Node &n = node(it.id);
            if (seen[it.id]) die("full audit: node %u reached twice", it.id);
            seen[it.id] = 1;
            a.nodes++;
            a.deepest = std::max<uint64_t>(a.deepest, it.depth);
            a.node_path[it.id] = it.ph;
            run_ok(n.hash_off, n.hash_cnt, "'#' terminal of node", it.id);
            run_ok(n.exact_off, n.exact_cnt, "exact terminal of node", it.id);
            if (n.nlit & NLIT_HDESC) a.hdesc_nodes++;
            kids_of(it.id, kids);
            a.compared++;
            if (nlit_of(n) != kids.size()) die("full audit: node %u: nlit says %u literal children, the structure holds %zu", it.id, nlit_of(n), kids.size());
            // '+' child
            a.compared += 2;
            if (n.plus == NONE) {
                if (n.psum_lo || n.psum_hi) die("full audit: node %u has no '+' child but psum %08x:%08x", it.id, n.psum_hi, n.psum_lo);
            } else {
                const uint64_t m = summary(n.plus);
                a.psum++;
                if (n.psum_lo != (uint32_t)m || n.psum_hi != (uint32_t)(m >> 32))
                    die("full audit: node %u: psum %08x:%08x, its '+' child %u sums to %08x:%08x", it.id, n.psum_hi, n.psum_lo, n.plus, (uint32_t)(m >> 32), (uint32_t)m);
                stack.push_back(Item{n.plus, it.depth + 1, mix64(it.ph ^ 0xABCDull)});
            }
            for (uint32_t s = 0; s < ANX_SLOTS; s++)
                if (n.nlit & (s ? NLIT_ANX1 : NLIT_ANX0)) {
                    if (anx_node[s] != NONE) die("full audit: nodes %u and %u both carry the flag of annex slot %u", anx_node[s], it.id, s);
                    anx_node[s] = it.id;
                    a.compared++;
                    if (ix.anx_depth[s] != it.depth) die("full audit: annex slot %u: node %u at depth %u, anx_depth %u", s, it.id, it.depth, ix.anx_depth[s]);
                    if (!wide_mode(n)) die("full audit: annexed node %u has %u children: not wide", it.id, nlit_of(n));
                    if ((n.nlit & (NLIT_ANX0 | NLIT_ANX1)) == (NLIT_ANX0 | NLIT_ANX1)) die("full audit: node %u carries both annex flags", it.id);
                }
            if (table_mode(n)) {
                const uint32_t mask = n.kw[1];
                uint32_t bloom[6] = {0, 0, 0, 0, 0, 0};
                for (const Kid &k : kids) {
                    const uint32_t h = child_hash(k.wid), home = h & mask;
                    if (k.at < home) a.ctab_wrapped++;
                    for (uint32_t j = home; j != k.at; j = (j + 1) & mask)
                        if (ix.ctab[n.kw[0] + j].wid == NONE) die("full audit: node %u: child slot %u (wid %u): empty slot %u between its home %u and it", it.id, k.at, k.wid, j, home);
                    const uint64_t m = summary(k.child);
                    a.slot_sums++;
                    a.compared += 2;
                    if (k.slot->sum_lo != (uint32_t)m || k.slot->sum_hi != (uint32_t)(m >> 32))
                        die("full audit: node %u: the slot of child %u (wid %u) holds summary %08x:%08x, the child sums to %08x:%08x", it.id, k.child, k.wid, k.slot->sum_hi, k.slot->sum_lo, (uint32_t)(m >> 32), (uint32_t)m);
                    const uint32_t b = child_bit(h);
                    bloom[b >> 5] |= 1u << (b & 31);
                }
                if (wide_mode(n)) a.wide_ids.push_back(it.id);
                if (!wide_mode(n)) {
                    const uint32_t have[6] = {n.kw[2], n.kw[3], n.kc[0], n.kc[1], n.kc[2], n.kc[3]};
                    // A superset by design: child_remove (tm_host.cpp) clears no bit -- a Bloom cannot forget one
                    // word -- and to_table / from_wide build it anew on every table move.  Extra bits are reported.
                    a.blooms++;
                    a.bloom_ids.push_back(it.id);
                    a.compared += 6;
                    for (int j = 0; j < 6; j++) {
                        if ((have[j] & bloom[j]) != bloom[j]) die("full audit: node %u: Bloom word %d is %08x, its children need %08x", it.id, j, have[j], bloom[j]);
                        a.bloom_extra += (uint64_t)__builtin_popcount(have[j] & ~bloom[j]);
                    }
                } else if (n.kw[2] == NONE) {
                    a.dense_wide++;
                } else {
                    const uint32_t words = ix.wcap / 32;
                    if (!ix.wcap || (size_t)n.kw[2] + words > bd.wbits) die("full audit: wide node %u: bitmap [%u, +%u) leaves wbits (%zu)", it.id, n.kw[2], words, bd.wbits);
                    std::vector<uint32_t> bm(words, 0);
                    for (const Kid &k : kids) {
                        if (k.wid >= ix.wcap) die("full audit: wide node %u: child wid %u past wcap %u", it.id, k.wid, ix.wcap);
                        bm[k.wid >> 5] |= 1u << (k.wid & 31);
                    }
                    a.bitmaps++;
                    a.compared += words;
                    for (uint32_t j = 0; j < words; j++)
                        if (ix.wbits[n.kw[2] + j] != bm[j]) die("full audit: wide node %u: bitmap word %u is %08x, its children give %08x", it.id, j, ix.wbits[n.kw[2] + j], bm[j]);
                }
            }
            for (const Kid &k : kids) {
                if (k.wid >= wslot.size() || wslot[k.wid] == NONE) die("full audit: node %u: an edge with wid %u, which the vocab lacks", it.id, k.wid);
                stack.push_back(Item{k.child, it.depth + 1, mix64(it.ph ^ a.wid_bytes[k.wid])});
            }
        }
        if (ix.depth < a.deepest) die("full audit: depth %u, the deepest reachable node is at %llu", ix.depth, (unsigned long long)a.deepest);
        a.depth_slack = ix.depth - a.deepest;
        if (a.hdesc_nodes && !ix.hdesc) die("full audit: %llu NLIT_HDESC nodes reachable, hdesc is 0", (unsigned long long)a.hdesc_nodes);
        a.hdesc_extra = !a.hdesc_nodes && ix.hdesc;
    }

    void hints() {
        std::vector<Kid> kids;
        for (uint32_t s = 0; s < ANX_SLOTS; s++) {
            a.compared++;
            if (anx_node[s] == NONE) {
                if (ix.anx_depth[s] != NONE) die("full audit: anx_depth[%u] = %u, no reachable node carries the slot's flag", s, ix.anx_depth[s]);
                continue;
            }
            kids_of(anx_node[s], kids);
            std::unordered_map<uint32_t, uint32_t> want;
            for (const Kid &k : kids) want[k.wid] = hint_of_sum(k.slot->sum_lo, k.slot->sum_hi);
            for (uint32_t v = 0; v <= ix.vmask; v++) {
                const VocabEntry &e = ix.vocab[v];
                if (e.wid == NONE || (e.tag & 0xFFu) > VINL) continue;
                const uint32_t have = (e.tag >> (s ? HINT_SHIFT1 : HINT_SHIFT0)) & HINT_MASK;
                const auto f = want.find(e.wid);
                const uint32_t w = f == want.end() ? 0 : f->second;
                a.hints[s]++;
                a.compared++;
                a.hints_nonzero[s] += w != 0;
                if (have != w) die("full audit: vocab slot %u (wid %u): hint field %u is %03x, annexed node %u gives %03x", v, e.wid, s, have, anx_node[s], w);
            }
        }
    }

    void run() {
        vocab();
        exact();
        tree();
        hints();
    }
};

}  // namespace imgw

namespace fake {
imgw::UseStats use_stats();   // summed over every launch so far (fake_launch.cpp)
}
