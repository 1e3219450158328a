/*
 * tmatch_nif_route.c -- route fan-out over the NIF core's buffer sets (see
 * tmatch_nif_route.h).
 */
#include "tmatch_nif_route.h"

int tmn_route(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests) {
    return tmn_route_with(s, h, n, n_dests, tm_route_batch32);
}

int tmn_route_dest(const tmn_set *s, uint32_t d, uint64_t *b, uint64_t *e) {
    const uint32_t *doff = s->rdoff.p;
    *b = *e = 0;
    if (!s->route_dests || d > s->route_dests) return TM_EINVAL;
    *b = doff[d];
    *e = doff[d + 1];
    return 0;
}
