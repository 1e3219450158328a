/*
 * fake_tmatch_aggre.c -- TEST INFRASTRUCTURE: tm_route_batch32_ex for the
 * stand-in libtmatch (fake_tmatch.c + fake_tmatch_route.c), so
 * c_src/tmatch_nif_aggre.c runs on the CPU (tests/test_aggre_cpu.py).  Flags 0
 * is the stand-in's tm_route_batch32.  TM_ROUTE_AGGRE applies the header's rule
 * to that call's whole output with the filter id of value v = 1000 i + k being
 * k / (2 (n_dests + 1)): a bucket holds a topic's k, k + D, k + 2 D, ... (D =
 * n_dests + 1), so every second one shares its predecessor's filter.  TM_ECAP
 * when the total BEFORE aggregation exceeds cap, the offsets then holding those
 * sizes, as the library does.  Counts its calls and keeps the cap of each of
 * the last few.
 */
#include <stdlib.h>
#include <string.h>

#include "tmatch.h"

static long n_aggre;
static uint64_t acaps[8];

int tm_route_batch32_ex(tm_index *h, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                        uint32_t *doff, uint32_t *out_topic, uint32_t *out_values, uint64_t cap, uint8_t *err,
                        uint32_t flags) {
    if (flags & ~TM_ROUTE_AGGRE) return TM_EINVAL;
    if (!flags) return tm_route_batch32(h, n, tb, to, n_dests, doff, out_topic, out_values, cap, err);
    acaps[n_aggre % 8] = cap;
    n_aggre++;
    int rc = tm_route_batch32(h, n, tb, to, n_dests, doff, NULL, NULL, 0, err);   /* the sizes */
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    const uint64_t total = doff[n_dests + 1];
    if (total > cap) return TM_ECAP;
    uint32_t *t = malloc(4 * (total + 1)), *v = malloc(4 * (total + 1));
    uint32_t *raw = malloc(4 * ((size_t)n_dests + 2));
    rc = tm_route_batch32(h, n, tb, to, n_dests, raw, t, v, total, err);
    if (rc == TM_OK) {
        const uint32_t D = n_dests + 1;
        uint64_t k = 0;
        for (uint32_t b = 0; b <= n_dests; b++) {
            doff[b] = (uint32_t)k;
            for (uint64_t q = raw[b]; q < raw[b + 1]; q++) {
                const int same = q > raw[b] && b < n_dests && t[q] == t[q - 1] &&
                                 (v[q] % 1000) / (2 * D) == (v[q - 1] % 1000) / (2 * D);
                if (same) continue;
                out_topic[k] = t[q];
                out_values[k] = v[q];
                k++;
            }
        }
        doff[n_dests + 1] = (uint32_t)k;
    }
    free(t);
    free(v);
    free(raw);
    return rc;
}

long fake_aggre_count(void) { return n_aggre; }
uint64_t fake_aggre_cap(long call) { return acaps[call % 8]; }
