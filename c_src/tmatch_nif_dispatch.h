/*
 * tmatch_nif_dispatch.h -- tmn_route / tmn_route_aggre with the local node's
 * dispatch/2 applied on the device (tm_dispatch_batch32, include/tmatch.h):
 * besides one (topic index, value) slice per destination the batch comes back
 * with the local bucket expanded to one (topic index, value, subscriber id)
 * delivery per subscriber of each entry's value -- the {deliver, To, Msg}
 * messages do_dispatch2/2 sends (emqx_broker.erl:726-760), in entry order and
 * list order, with the index's own subscriber table (tm_set_subscribers).
 *
 * Its own translation unit: tmatch_nif_route.c and tmatch_nif_aggre.c stay
 * loadable against a libtmatch that predates tm_dispatch_batch32.  The head and
 * the three delivery buffers live in the set (tmn_set.dhead, dtopic, dvalue,
 * dsub) and are released with it; a set that never dispatched has none.
 */
#ifndef TMATCH_NIF_DISPATCH_H
#define TMATCH_NIF_DISPATCH_H

#include "tmatch_nif_route.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The packed batch of n topics routed over n_dests destinations (1 .. 65536)
 * and bucket local_dest (< n_dests) dispatched; flags: 0 or TM_ROUTE_AGGRE.
 * The entry buffers are sized as tmn_route sizes them, the delivery buffers
 * from what the set already holds (>= TMN_IDS_PER_TOPIC per topic).  On
 * TM_ECAP the bucket offsets hold the full entry count (before aggregation
 * under TM_ROUTE_AGGRE) and the head the delivery count: ONE rerun grows
 * whichever did not fit to the exact totals (again, a few times at most, only
 * if concurrent writes grew them in between).  Grown buffers stay with the
 * set.  TM_EDEVICE: the device failed the batch (or a topic is flagged err 4)
 * -- never a per-topic badarg; nothing is left to read then.  The slices are
 * read with tmn_route_dest / tmn_route_topics / tmn_vals / tmn_route_err. */
int tmn_dispatch(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t flags);

/* The deliveries of the last tmn_dispatch: 0 and *count entries of *topics /
 * *values / *subs (topic index, route value, subscriber id); TM_EINVAL and
 * none when the set's last tmn_dispatch did not succeed. */
int tmn_deliveries(const tmn_set *s, const uint32_t **topics, const uint32_t **values, const uint32_t **subs,
                   uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* TMATCH_NIF_DISPATCH_H */
