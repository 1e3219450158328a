/*
 * tmatch_nif_route.h -- route fan-out for the NIF's micro-batches, ERTS-free
 * like tmatch_nif_core.h and over the same buffer sets: the batch tmn_pack
 * packed goes through tm_route_batch32 (include/tmatch.h), which matches and
 * fans it out in place when the set's buffers are the index's pinned memory,
 * and comes back as one (topic index, value) slice per destination -- what a
 * batched broker forwards once per node per micro-batch instead of once per
 * hit (emqx_broker.erl:401-406).
 *
 * Its own translation unit: tmatch_nif_core.c stays loadable against a
 * libtmatch that predates tm_route_batch32.
 */
#ifndef TMATCH_NIF_ROUTE_H
#define TMATCH_NIF_ROUTE_H

#include "tmatch_nif_core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The packed batch of n topics routed over n_dests destinations (1 .. 65536).
 * Sizes the entry buffers from what the set already holds (>=
 * TMN_IDS_PER_TOPIC per topic) and on TM_ECAP (bucket offsets valid, entries
 * truncated) grows them to the exact total and runs the batch again, as
 * tmn_match does.  TM_EDEVICE: the device failed the batch (or a topic is
 * flagged err 4) -- never a per-topic badarg.  Per-topic flags: tmn_route_err. */
int tmn_route(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests);

/* Destination d's slice of the last tmn_route: 0 and entries [*b, *e) of
 * tmn_route_topics() / tmn_vals(), in topic order and traversal order inside a
 * topic; d == n_dests is the bucket of values without a destination.
 * TM_EINVAL (and an empty slice) for d > n_dests. */
int tmn_route_dest(const tmn_set *s, uint32_t d, uint64_t *b, uint64_t *e);
static inline const uint32_t *tmn_route_topics(const tmn_set *s) { return (const uint32_t *)s->rtopic.p; }
/* topic i's flag: 0, TMN_ERR_BADARG or TMN_ERR_TOO_DEEP (it has no entries then) */
static inline int tmn_route_err(const tmn_set *s, uint32_t i) { return ((const uint8_t *)s->err.p)[i]; }

#ifdef __cplusplus
}
#endif
#endif /* TMATCH_NIF_ROUTE_H */
