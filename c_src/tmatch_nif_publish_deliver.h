/*
 * tmatch_nif_publish_deliver.h -- tmn_publish with the local picks merged into
 * the local bucket's deliveries and the whole grouped by subscriber on the
 * device (tm_publish_deliver_batch32, include/tmatch.h): the last link of the
 * publish chain.  One connection process finds its direct deliveries
 * (do_dispatch2/2) and the shared-subscription picks that fell on it
 * (emqx_shared_sub:dispatch/3) in one mailbox; the batch comes back with one
 * list per local subscriber holding both kinds in publish order, besides the
 * slices and ONE picked member per kept entry as after tmn_publish.
 *
 * Its own translation unit: the older units stay loadable against a libtmatch
 * that predates tm_publish_deliver_batch32.  It uses the set's key words
 * (tmn_share_keys), its member array (tmn_set.smember) and its group buffers
 * (tmn_set.ghead, gsub, goff), all in tm_host_alloc memory, so the batch runs
 * in place.
 */
#ifndef TMATCH_NIF_PUBLISH_DELIVER_H
#define TMATCH_NIF_PUBLISH_DELIVER_H

#include "tmatch_nif_deliver.h"
#include "tmatch_nif_share.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmn_publish's arguments (the keys set with tmn_share_keys; another n while
 * keys are set is TM_EINVAL).  The entry buffers (the members with them) are
 * sized as tmn_publish sizes them, the delivery buffers for twice that (they
 * take T + K: the direct deliveries and at most a pick per entry), and the
 * group buffers ALWAYS have room for a group per delivery slot, so G > gcap
 * cannot occur and no rerun is ever made for the groups.  On TM_ECAP there is
 * ONE rerun per kind, each sized exactly:
 *   - total > cap: the entry buffers grow to out_dest_offsets[n_dests + 1];
 *   - T + K > dcap: the delivery buffers grow to out_head[1] +
 *     out_dest_offsets[n_dests + 1] (K then: the entries fitted), the group
 *     buffers with them.
 * NEITHER has moved state: under both the library makes no pick, so whichever
 * call succeeds is the batch's only pick and a round robin advances once.
 * This is unlike tmn_publish's rerun for the deliveries alone, whose first
 * call's picks stood and which therefore picks twice.
 * TM_EDEVICE: the device failed the batch (or a topic is flagged err 4);
 * nothing is left to read then.  The slices and flags are read as after
 * tmn_dispatch, the members with tmn_picks, the N merged and grouped
 * deliveries with tmn_deliveries, the groups with tmn_groups; tmn_direct gives
 * T, the direct deliveries among the N. */
int tmn_publish_deliver(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t seed);

/* T of the set's last successful tmn_publish_deliver (the head's second word) */
static inline uint64_t tmn_direct(const tmn_set *s) { return s->dispatched == 4 ? ((const uint64_t *)s->dhead.p)[1] : 0; }

#ifdef __cplusplus
}
#endif
#endif /* TMATCH_NIF_PUBLISH_DELIVER_H */
