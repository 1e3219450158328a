/*
 * fake_tmatch_deliver.c -- TEST INFRASTRUCTURE: tm_deliver_batch32 for the
 * stand-in libtmatch (fake_tmatch.c + fake_tmatch_route.c +
 * fake_tmatch_dispatch.c), so c_src/tmatch_nif_deliver.c runs on the CPU
 * (tests/test_deliver32_cpu.py, tests/native/nif_deliver_check.c).  The route
 * outputs and the deliveries are fake_tmatch_dispatch.c's, except that the
 * delivery r of value v goes to subscriber fake_deliver_sub(v, r) = (v * 16 +
 * r) % mod (mod: fake_deliver_mod, 13 at first; 0: v * 65536 + r, a group of
 * its own for every delivery of a value that occurs once in the bucket).  The
 * first W = min(T, dcap) of them are sorted stably by subscriber (an insertion
 * sort: nothing to share with the library's radix passes); out_ghead = [G, W],
 * the first min(G, gcap) subscribers and offsets and the end entry are
 * written.  TM_ECAP when total > cap, T > dcap or G > gcap, as the library
 * does.  Counts its calls and keeps the three capacities of each of the last
 * few.
 */
#include <stdlib.h>
#include <string.h>

#include "tmatch.h"
#include "tmatch_nif_deliver.h"

static long n_deliver;
static uint64_t caps[8], dcaps[8], gcaps[8];
static uint32_t mod = 13;

void fake_deliver_mod(uint32_t m) { mod = m; }
uint32_t fake_deliver_sub(uint32_t v, uint32_t r) { return mod ? (v * 16 + r) % mod : v * 65536 + r; }

int tm_deliver_batch32(tm_index *h, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                       uint32_t local_dest, uint32_t flags, uint32_t *doff, uint32_t *out_topic, uint32_t *out_values,
                       uint64_t cap, uint64_t *head, uint32_t *dt, uint32_t *dv, uint32_t *ds, uint64_t dcap,
                       uint64_t *ghead, uint32_t *gsub, uint32_t *goff, uint64_t gcap, uint8_t *err) {
    caps[n_deliver % 8] = cap;
    dcaps[n_deliver % 8] = dcap;
    gcaps[n_deliver % 8] = gcap;
    n_deliver++;
    if (!ghead || !goff || (gcap && !gsub)) return TM_EINVAL;
    uint32_t *t = malloc(4 * (dcap + 1)), *v = malloc(4 * (dcap + 1)), *s = malloc(4 * (dcap + 1));
    int rc = tm_dispatch_batch32(h, n, tb, to, n_dests, local_dest, flags, doff, out_topic, out_values, cap, head, t, v, s,
                                 dcap, err);
    if (rc != TM_OK && rc != TM_ECAP) { free(t); free(v); free(s); return rc; }
    const uint64_t W = head[1] < dcap ? head[1] : dcap;
    uint32_t *p = malloc(4 * (W + 1));
    for (uint64_t i = 0; i < W; i++) {
        s[i] = fake_deliver_sub(v[i], s[i] - v[i] * 16);   /* (the dispatch stand-in's id is v * 16 + r) */
        uint64_t j = i;                                    /* stable: equal ids keep their order */
        for (; j > 0 && s[p[j - 1]] > s[i]; j--) p[j] = p[j - 1];
        p[j] = (uint32_t)i;
    }
    uint64_t G = 0;
    for (uint64_t i = 0; i < W; i++) {
        dt[i] = t[p[i]];
        dv[i] = v[p[i]];
        ds[i] = s[p[i]];
        if (i == 0 || ds[i] != ds[i - 1]) {
            if (G < gcap) gsub[G] = ds[i];
            if (G <= gcap) goff[G] = (uint32_t)i;
            G++;
        }
    }
    if (G <= gcap) goff[G] = (uint32_t)W;
    ghead[0] = G;
    ghead[1] = W;
    free(t); free(v); free(s); free(p);
    return rc == TM_ECAP || G > gcap ? TM_ECAP : TM_OK;
}

long fake_deliver_count(void) { return n_deliver; }
uint64_t fake_deliver_cap(long call) { return caps[call % 8]; }
uint64_t fake_deliver_dcap(long call) { return dcaps[call % 8]; }
uint64_t fake_deliver_gcap(long call) { return gcaps[call % 8]; }
uint64_t fake_set_group_cap(tmn_set *s) { return s->gsub.cap < s->goff.cap ? s->gsub.cap : s->goff.cap; }
