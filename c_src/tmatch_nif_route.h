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

/* What tmn_route does around the library call, with the call as a parameter
 * (tm_route_batch32's arguments; TM_ECAP: the offsets hold the entries the
 * rerun needs room for): tmn_route and tmn_route_aggre
 * (tmatch_nif_aggre.c) are this with their call, so the two cannot drift. */
typedef int (*tmn_route_call)(tm_index *h, uint64_t n, const uint8_t *topic_bytes, const uint32_t *topic_offsets,
                              uint32_t n_dests, uint32_t *out_dest_offsets, uint32_t *out_topic, uint32_t *out_values,
                              uint64_t cap, uint8_t *out_err);
static inline int tmn_route_with(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, tmn_route_call call) {
    s->route_dests = 0;
    if (!n_dests || n_dests > 65536) return TM_EINVAL;
    uint32_t *doff = tmn_get(h, &s->rdoff, 4ull * ((uint64_t)n_dests + 2));
    uint8_t *err = tmn_get(h, &s->err, (uint64_t)n + 1);
    /* capacity: what the set already holds, at least TMN_IDS_PER_TOPIC entries per topic */
    const uint64_t want = (uint64_t)TMN_IDS_PER_TOPIC * n + 1024;
    const uint64_t have = s->vals.cap < s->rtopic.cap ? s->vals.cap / 4 : s->rtopic.cap / 4;
    uint64_t cap = have > want ? have : want;
    uint32_t *vals = tmn_get(h, &s->vals, 4 * cap);
    uint32_t *topic = tmn_get(h, &s->rtopic, 4 * cap);
    if (!doff || !err || !vals || !topic) return TM_ENOMEM;
    cap = (s->vals.cap < s->rtopic.cap ? s->vals.cap : s->rtopic.cap) / 4;
    int rc = call(h, n, s->blob.p, s->offs.p, n_dests, doff, topic, vals, cap, err);
    /* TM_ECAP: the bucket offsets hold the full sizes, so rerun with room for
       every entry (again if concurrent inserts grew the total in between) */
    for (int tries = 0; rc == TM_ECAP && tries < 4; tries++) {
        s->reruns++;
        const uint64_t total = doff[n_dests + 1];
        vals = tmn_get(h, &s->vals, 4 * total);
        topic = tmn_get(h, &s->rtopic, 4 * total);
        if (!vals || !topic) return TM_ENOMEM;
        cap = (s->vals.cap < s->rtopic.cap ? s->vals.cap : s->rtopic.cap) / 4;
        rc = call(h, n, s->blob.p, s->offs.p, n_dests, doff, topic, vals, cap, err);
    }
    for (uint32_t i = 0; rc == TM_OK && i < n; i++)
        if (err[i] > TMN_ERR_TOO_DEEP) rc = TM_EDEVICE;
    if (rc == TM_OK) s->route_dests = n_dests;
    return rc;
}

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
