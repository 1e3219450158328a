/*
 * tmatch_nif_aggre.c -- aggregated route fan-out over the NIF core's buffer
 * sets (see tmatch_nif_aggre.h).
 */
#include "tmatch_nif_aggre.h"

static int route_aggre_call(tm_index *h, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                            uint32_t *doff, uint32_t *topic, uint32_t *vals, uint64_t cap, uint8_t *err) {
    return tm_route_batch32_ex(h, n, tb, to, n_dests, doff, topic, vals, cap, err, TM_ROUTE_AGGRE);
}

/* (TM_ECAP here: the offsets hold the sizes before aggregation, which is the room the rerun needs) */
int tmn_route_aggre(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests) {
    return tmn_route_with(s, h, n, n_dests, route_aggre_call);
}
