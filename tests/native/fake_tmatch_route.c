/*
 * fake_tmatch_route.c -- TEST INFRASTRUCTURE: tm_route_batch32 for the
 * stand-in libtmatch (fake_tmatch.c), so c_src/tmatch_nif_route.c runs on the
 * CPU (tests/test_route32_cpu.py).  Topics match as in fake_tmatch.c (topic i:
 * one value per byte, 1000 * i + k; '+' first: badarg; '!' first: err flag 4;
 * '~' first: TM_EDEVICE); value v goes to destination v % (n_dests + 1), the
 * last of them being the unrouted bucket.  The partition is stable, the
 * offsets hold the full bucket sizes and TM_ECAP is returned when the total
 * exceeds cap, as the library does.  Counts its calls and keeps the cap of
 * each of the last few.
 */
#include <stdlib.h>
#include <string.h>

#include "tmatch.h"
#include "tmatch_nif_route.h"

static long n_route;
static uint64_t caps[8];

int tm_route_batch32(tm_index *h, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                     uint32_t *doff, uint32_t *out_topic, uint32_t *out_values, uint64_t cap, uint8_t *err) {
    (void)h;
    caps[n_route % 8] = cap;
    n_route++;
    for (uint64_t i = 0; i < n; i++)
        if (to[i + 1] > to[i] && tb[to[i]] == '~') return TM_EDEVICE;
    uint32_t *fill = calloc((size_t)n_dests + 2, 4);
    memset(doff, 0, 4 * ((size_t)n_dests + 2));
    for (int pass = 0; pass < 2; pass++) {
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t len = to[i + 1] - to[i];
            err[i] = len && tb[to[i]] == '+' ? 1 : len && tb[to[i]] == '!' ? 4 : 0;
            for (uint64_t k = 0; !err[i] && k < len; k++) {
                const uint32_t v = (uint32_t)(1000 * i + k), b = v % (n_dests + 1);
                if (pass == 0) {
                    doff[b + 1]++;
                } else {
                    const uint64_t pos = (uint64_t)doff[b] + fill[b]++;
                    if (pos < cap) { out_topic[pos] = (uint32_t)i; out_values[pos] = v; }
                }
            }
        }
        if (pass == 0)
            for (uint32_t b = 0; b <= n_dests; b++) doff[b + 1] += doff[b];
    }
    free(fill);
    return doff[n_dests + 1] > cap ? TM_ECAP : TM_OK;
}

long fake_route_count(void) { return n_route; }
uint64_t fake_route_cap(long call) { return caps[call % 8]; }
const uint32_t *fake_set_route_topics(tmn_set *s) { return tmn_route_topics(s); }
uint64_t fake_set_route_cap(tmn_set *s) { return s->rtopic.cap; }
