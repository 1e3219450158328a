/*
 * fake_tmatch_dispatch.c -- TEST INFRASTRUCTURE: tm_dispatch_batch32 for the
 * stand-in libtmatch (fake_tmatch.c + fake_tmatch_route.c), so
 * c_src/tmatch_nif_dispatch.c runs on the CPU (tests/test_dispatch32_cpu.py,
 * tests/native/nif_dispatch_check.c).  The route outputs are
 * fake_tmatch_route.c's (flags are ignored: nothing is aggregated); value v of
 * the local bucket has ((v % 1000) % 7) * mult subscribers, v * 16 + r for r =
 * 0, 1, ... (mult: fake_dispatch_mult, 1 at first), in entry order and list
 * order.  out_head = [M, T]; the first min(T, dcap) deliveries are written;
 * TM_ECAP when total > cap or T > dcap, as the library does.  Counts its calls
 * and keeps the cap and dcap of each of the last few.
 */
#include <stdlib.h>
#include <string.h>

#include "tmatch.h"
#include "tmatch_nif_dispatch.h"

static long n_dispatch;
static uint64_t caps[8], dcaps[8];
static uint32_t mult = 1;

void fake_dispatch_mult(uint32_t m) { mult = m; }
uint32_t fake_dispatch_subs(uint32_t v) { return ((v % 1000) % 7) * mult; }

int tm_dispatch_batch32(tm_index *h, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                        uint32_t local_dest, uint32_t flags, uint32_t *doff, uint32_t *out_topic, uint32_t *out_values,
                        uint64_t cap, uint64_t *head, uint32_t *dt, uint32_t *dv, uint32_t *ds, uint64_t dcap,
                        uint8_t *err) {
    (void)flags;
    caps[n_dispatch % 8] = cap;
    dcaps[n_dispatch % 8] = dcap;
    n_dispatch++;
    if (!n_dests || local_dest >= n_dests || !head) return TM_EINVAL;
    /* the whole fan-out first (the library's lives in its lane's scratch), then the caller's part of it */
    int rc = tm_route_batch32(h, n, tb, to, n_dests, doff, NULL, NULL, 0, err);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    const uint64_t total = doff[n_dests + 1];
    uint32_t *t = malloc(4 * (total + 1)), *v = malloc(4 * (total + 1));
    rc = tm_route_batch32(h, n, tb, to, n_dests, doff, t, v, total, err);
    if (rc != TM_OK) { free(t); free(v); return rc; }
    for (uint64_t q = 0; q < total && q < cap; q++) { out_topic[q] = t[q]; out_values[q] = v[q]; }
    uint64_t T = 0;
    for (uint64_t q = doff[local_dest]; q < doff[local_dest + 1]; q++)
        for (uint32_t r = 0; r < fake_dispatch_subs(v[q]); r++, T++)
            if (T < dcap) { dt[T] = t[q]; dv[T] = v[q]; ds[T] = v[q] * 16 + r; }
    head[0] = doff[local_dest + 1] - doff[local_dest];
    head[1] = T;
    free(t); free(v);
    return total > cap || T > dcap ? TM_ECAP : TM_OK;
}

long fake_dispatch_count(void) { return n_dispatch; }
uint64_t fake_dispatch_cap(long call) { return caps[call % 8]; }
uint64_t fake_dispatch_dcap(long call) { return dcaps[call % 8]; }
uint64_t fake_set_delivery_cap(tmn_set *s) { return s->dsub.cap; }
