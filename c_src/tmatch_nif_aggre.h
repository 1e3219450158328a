/*
 * tmatch_nif_aggre.h -- tmn_route with emqx_broker:aggre/1 applied on the
 * device (tm_route_batch32_ex with TM_ROUTE_AGGRE, include/tmatch.h): each
 * destination's slice holds one entry per (topic, filter), so a shared group
 * with members on several nodes gets a message once and the batcher no longer
 * dedupes the slices (emqx_broker.erl:408-424).
 *
 * Its own translation unit: tmatch_nif_route.c stays loadable against a
 * libtmatch that predates tm_route_batch32_ex.
 */
#ifndef TMATCH_NIF_AGGRE_H
#define TMATCH_NIF_AGGRE_H

#include "tmatch_nif_route.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmn_route's contract with aggregated slices: the index's filter table
 * (tm_set_route_filters) says which values share a filter.  TM_ECAP means the
 * entries BEFORE aggregation did not fit (the fan-out needs that room; the
 * bucket offsets then hold those sizes): the buffers grow to that total and the
 * batch runs again, as in tmn_route.  The slices are read with tmn_route_dest /
 * tmn_route_topics / tmn_vals / tmn_route_err. */
int tmn_route_aggre(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests);

#ifdef __cplusplus
}
#endif
#endif /* TMATCH_NIF_AGGRE_H */
