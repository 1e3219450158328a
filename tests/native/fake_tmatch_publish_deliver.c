/*
 * fake_tmatch_publish_deliver.c -- TEST INFRASTRUCTURE: tm_publish_deliver_batch32
 * for the stand-in libtmatch (fake_tmatch.c + fake_tmatch_route.c +
 * fake_tmatch_dispatch.c), so c_src/tmatch_nif_publish_deliver.c runs on the
 * CPU (tests/test_publish_deliver32_cpu.py,
 * tests/native/nif_publish_deliver_check.c).  The route outputs and the head
 * are fake_tmatch_dispatch.c's.  Direct delivery r of value v goes to
 * subscriber fake_pd_direct_sub(v, r) = (v * 16 + r) % 13.  The pick of kept
 * entry q (topic t, value v): none (0xFFFFFFFF) when v % 5 == 0, else
 * fake_pd_member(v, key_clientid[t], key_topic[t], seed, moves) with a NULL key
 * array read as zeros and `moves` the number of calls that picked before this
 * one.  Member m is local subscriber fake_pd_local(m) = m % 13, or not a
 * connection of this node (0xFFFFFFFF) when m % 3 == 0.  As the library, the
 * call picks nothing, moves nothing and writes no delivery, member or group
 * under TM_ECAP from cap (total > cap) or from dcap (T + K > dcap), with
 * out_ghead = [0, 0]; otherwise the T direct deliveries and the P local picks
 * are merged by message (inside one message the direct ones first, then the
 * picks in ascending entry position) and sorted stably by subscriber (insertion
 * sorts: nothing to share with the library's radix passes); out_ghead = [G, N],
 * the first min(G, gcap) subscribers and offsets and the end entry are written;
 * TM_ECAP when G > gcap, the picks standing.  Counts its calls and keeps the
 * three capacities of each of the last few.
 */
#include <stdlib.h>
#include <string.h>

#include "tmatch.h"
#include "tmatch_nif_publish_deliver.h"

static long n_pd, n_moves;
static uint64_t caps[8], dcaps[8], gcaps[8];

uint32_t fake_pd_direct_sub(uint32_t v, uint32_t r) { return (v * 16 + r) % 13; }
uint32_t fake_pd_member(uint32_t v, uint32_t kc, uint32_t kt, uint32_t seed, long moves) {
    return (v * 2u + 1u + kc * 3u + kt * 7u + seed * 11u + (uint32_t)moves * 13u) & 0x7FFFFFFFu;
}
uint32_t fake_pd_local(uint32_t m) { return m == 0xFFFFFFFFu || m % 3 == 0 ? 0xFFFFFFFFu : m % 13; }

/* a stable insertion sort of the positions p[0 .. n) by key[p[i]] */
static void sort_by(uint32_t *p, uint64_t n, const uint32_t *key) {
    for (uint64_t i = 1; i < n; i++) {
        const uint32_t x = p[i];
        uint64_t j = i;
        for (; j > 0 && key[p[j - 1]] > key[x]; j--) p[j] = p[j - 1];
        p[j] = x;
    }
}

int tm_publish_deliver_batch32(tm_index *h, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                               uint32_t local_dest, uint32_t flags, uint32_t *doff, uint32_t *out_topic,
                               uint32_t *out_values, uint64_t cap, uint64_t *head, uint32_t *dt, uint32_t *dv, uint32_t *ds,
                               uint64_t dcap, const uint32_t *key_clientid, const uint32_t *key_topic, uint32_t seed,
                               uint32_t *out_member, uint64_t *ghead, uint32_t *gsub, uint32_t *goff, uint64_t gcap,
                               uint8_t *err) {
    caps[n_pd % 8] = cap;
    dcaps[n_pd % 8] = dcap;
    gcaps[n_pd % 8] = gcap;
    n_pd++;
    if (!(flags & TM_ROUTE_AGGRE) || (cap && !out_member) || !ghead || !goff || (gcap && !gsub)) return TM_EINVAL;
    /* the sizes first: the route outputs and [M, T], no delivery written */
    int rc = tm_dispatch_batch32(h, n, tb, to, n_dests, local_dest, flags, doff, out_topic, out_values, cap, head, NULL,
                                 NULL, NULL, 0, err);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    const uint64_t total = doff[n_dests + 1], T = head[1];
    ghead[0] = ghead[1] = 0;
    if (total > cap || T + total > dcap) return TM_ECAP;   /* no pick, no state moved, nothing merged */
    const uint64_t all = T + total;
    uint32_t *t = malloc(4 * (all + 1)), *v = malloc(4 * (all + 1)), *s = malloc(4 * (all + 1)), *p = malloc(4 * (all + 1));
    uint64_t hd[2];
    rc = tm_dispatch_batch32(h, n, tb, to, n_dests, local_dest, flags, doff, out_topic, out_values, cap, hd, t, v, s, T, err);
    if (rc != TM_OK) { free(t); free(v); free(s); free(p); return rc; }
    for (uint64_t i = 0; i < T; i++) s[i] = fake_pd_direct_sub(v[i], s[i] - v[i] * 16);   /* (the stand-in's id: v * 16 + r) */
    uint64_t N = T;
    for (uint64_t q = 0; q < total; q++) {
        const uint32_t et = out_topic[q], ev = out_values[q];
        const uint32_t m = ev % 5 == 0 ? 0xFFFFFFFFu
                                       : fake_pd_member(ev, key_clientid ? key_clientid[et] : 0,
                                                        key_topic ? key_topic[et] : 0, seed, n_moves);
        out_member[q] = m;
        if (fake_pd_local(m) == 0xFFFFFFFFu) continue;
        t[N] = et; v[N] = ev; s[N] = fake_pd_local(m);
        N++;
    }
    n_moves++;
    for (uint64_t i = 0; i < N; i++) p[i] = (uint32_t)i;
    sort_by(p, N, t);   /* by message: the direct ones before the picks, the picks in entry order */
    sort_by(p, N, s);   /* by subscriber */
    uint64_t G = 0;
    for (uint64_t i = 0; i < N; i++) {
        dt[i] = t[p[i]];
        dv[i] = v[p[i]];
        ds[i] = s[p[i]];
        if (i == 0 || ds[i] != ds[i - 1]) {
            if (G < gcap) gsub[G] = ds[i];
            if (G <= gcap) goff[G] = (uint32_t)i;
            G++;
        }
    }
    if (G <= gcap) goff[G] = (uint32_t)N;
    ghead[0] = G;
    ghead[1] = N;
    free(t); free(v); free(s); free(p);
    return G > gcap ? TM_ECAP : TM_OK;
}

long fake_pd_count(void) { return n_pd; }
long fake_pd_moves(void) { return n_moves; }
uint64_t fake_pd_cap(long call) { return caps[call % 8]; }
uint64_t fake_pd_dcap(long call) { return dcaps[call % 8]; }
uint64_t fake_pd_gcap(long call) { return gcaps[call % 8]; }
uint64_t fake_pd_direct(const tmn_set *s) { return tmn_direct(s); }
uint64_t fake_pd_group_room(const tmn_set *s) {
    const uint64_t a = s->gsub.cap / 4, b = s->goff.cap / 4;
    return b ? (a < b - 1 ? a : b - 1) : 0;
}
