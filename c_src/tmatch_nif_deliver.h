/*
 * tmatch_nif_deliver.h -- tmn_dispatch with the local bucket's deliveries
 * grouped by subscriber on the device (tm_deliver_batch32, include/tmatch.h):
 * the hand-off a micro-batched broker makes is one list per subscriber per
 * batch, the subscriber's deliveries in publish order -- what a connection
 * process gathers from its mailbox (emqx_connection.erl:611-612).  The three
 * delivery arrays come back sorted stably by subscriber id, with the G
 * distinct subscribers and their G + 1 offsets.
 *
 * Its own translation unit: tmatch_nif_dispatch.c stays loadable against a
 * libtmatch that predates tm_deliver_batch32.  The group head and the two
 * group buffers live in the set (tmn_set.ghead, gsub, goff) and are released
 * with it; a set that never delivered has none.
 */
#ifndef TMATCH_NIF_DELIVER_H
#define TMATCH_NIF_DELIVER_H

#include "tmatch_nif_dispatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmn_dispatch's arguments and buffer sizing; the group buffers start with
 * room for a group per TMN_IDS_PER_TOPIC deliveries' worth of topics (what
 * the set already holds, if more).  On TM_ECAP the bucket offsets hold the
 * full entry count, the head the delivery count and the group head the group
 * count: ONE rerun per kind grows whichever did not fit to the exact total
 * (deliveries that did not fit hide groups: the groups then get room for a
 * group per delivery, so that rerun is the last).  TM_EDEVICE: the device
 * failed the batch (or a topic is flagged err 4); nothing is left to read
 * then.  The slices are read as after tmn_dispatch, the grouped deliveries
 * with tmn_deliveries, the groups with tmn_groups. */
int tmn_deliver(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t flags);

/* The groups of the last tmn_deliver: 0, *count subscriber ids in *subs
 * (ascending) and *count + 1 offsets in *offs -- subscriber g owns the
 * deliveries [offs[g], offs[g + 1]) of tmn_deliveries' arrays; TM_EINVAL and
 * none when the set's last call was not a tmn_deliver (or a
 * tmn_publish_deliver, tmatch_nif_publish_deliver.h) that succeeded. */
int tmn_groups(const tmn_set *s, const uint32_t **subs, const uint32_t **offs, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* TMATCH_NIF_DELIVER_H */
