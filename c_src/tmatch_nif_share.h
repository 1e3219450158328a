/*
 * tmatch_nif_share.h -- tmn_dispatch under aggre/1 with the shared-subscription
 * pick applied on the device (tm_publish_batch32, include/tmatch.h): besides
 * the slices and the local node's deliveries the batch comes back with ONE
 * picked member per kept entry -- what emqx_shared_sub:dispatch/3 picks for a
 * {To, Group} destination by the group's strategy (0xFFFFFFFF: the entry is no
 * shared destination, or its group has no subscribers) -- with the index's own
 * share tables and state words (tm_set_share_slots, tm_set_share_members).
 *
 * Its own translation unit: the older units stay loadable against a libtmatch
 * that predates tm_publish_batch32.  The per-topic key words and the member
 * array live in the set (tmn_set.skc, skt, smember), in tm_host_alloc memory, so
 * the batch runs in place; they are released with the set, and a set that
 * never published has none.
 */
#ifndef TMATCH_NIF_SHARE_H
#define TMATCH_NIF_SHARE_H

#include "tmatch_nif_dispatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The key words of the packed batch's n topics, for hash_clientid / hash_topic
 * (and sticky's initial pick): the BEAM's phash2 of each message's sender and
 * topic, copied into the set.  Either array may be NULL (all zero, as
 * tm_publish_batch32 reads a NULL array); both NULL: none.  They hold for the
 * set's tmn_publish calls of n topics until set again; tmn_publish with another
 * n while keys are set is TM_EINVAL.  TM_ENOMEM: no pinned memory. */
int tmn_share_keys(tmn_set *s, tm_index *h, uint32_t n, const uint32_t *clientid_words, const uint32_t *topic_words);

/* The packed batch of n topics routed over n_dests destinations under aggre/1,
 * bucket local_dest dispatched, and one member picked per kept entry (seed:
 * tm_publish_batch32's, for random / local / a fresh round robin).  Buffers and
 * the TM_ECAP rerun as tmn_dispatch: the entry buffers (the members with them)
 * and the delivery buffers are sized BEFORE the first call from what the set
 * already holds (>= TMN_IDS_PER_TOPIC per topic), and ONE rerun grows
 * whichever did not fit to the exact totals.  What the rerun means for the
 * state words differs by kind:
 *   - TM_ECAP from the entries (total > cap): the library made no pick and
 *     moved no state; the rerun is the batch's only pick.
 *   - TM_ECAP from the deliveries alone: the picks of the first call stood and
 *     its state has moved; the rerun picks AGAIN, exactly as a broker that
 *     resubmits the batch would -- a round robin has then advanced twice for
 *     this batch, and the members returned are the second call's.  Sized as
 *     above this is rare (a local bucket with more than TMN_IDS_PER_TOPIC
 *     deliveries per topic on a set that has not seen such a batch yet), and
 *     sticky sizes keep it from repeating.
 * TM_EDEVICE: the device failed the batch (or a topic is flagged err 4);
 * nothing is left to read then.  Slices, deliveries and flags are read as
 * after tmn_dispatch, the members with tmn_picks. */
int tmn_publish(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t seed);

/* The picks of the set's last tmn_publish: 0 and *count members, members[q]
 * for entry q of the slices (tmn_route_dest's positions); TM_EINVAL and none
 * when the set's last dispatching call was no successful tmn_publish (or
 * tmn_publish_deliver, tmatch_nif_publish_deliver.h). */
int tmn_picks(const tmn_set *s, const uint32_t **members, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* TMATCH_NIF_SHARE_H */
