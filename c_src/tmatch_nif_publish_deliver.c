/*
 * tmatch_nif_publish_deliver.c -- route fan-out, local dispatch, the shared-
 * subscription pick and the merge and grouping by subscriber over the NIF
 * core's buffer sets (see tmatch_nif_publish_deliver.h).
 */
#include "tmatch_nif_publish_deliver.h"

static uint64_t min3(uint64_t a, uint64_t b, uint64_t c) {
    const uint64_t m = a < b ? a : b;
    return m < c ? m : c;
}

int tmn_publish_deliver(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t seed) {
    s->route_dests = 0;
    s->deliveries = 0;
    s->dispatched = 0;
    s->picks = 0;
    s->groups = 0;
    if (!n_dests || n_dests > 65536 || local_dest >= n_dests) return TM_EINVAL;
    if (s->key_mask && s->key_n != n) return TM_EINVAL;
    const uint32_t *kc = (s->key_mask & 1u) ? s->skc.p : 0, *kt = (s->key_mask & 2u) ? s->skt.p : 0;
    uint32_t *doff = tmn_get(h, &s->rdoff, 4ull * ((uint64_t)n_dests + 2));
    uint8_t *err = tmn_get(h, &s->err, (uint64_t)n + 1);
    uint64_t *head = tmn_get(h, &s->dhead, 16);
    uint64_t *ghead = tmn_get(h, &s->ghead, 16);
    /* capacity: what the set already holds, at least TMN_IDS_PER_TOPIC entries per topic and twice that
       in deliveries (T + K) */
    const uint64_t want = (uint64_t)TMN_IDS_PER_TOPIC * n + 1024;
    const uint64_t have = min3(s->vals.cap, s->rtopic.cap, s->smember.cap) / 4;
    const uint64_t dhave = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
    uint64_t cap = have > want ? have : want, dcap = dhave > 2 * want ? dhave : 2 * want;
    int rc = TM_ECAP;
    for (int tries = 0; rc == TM_ECAP && tries < 5; tries++) {
        uint32_t *vals = tmn_get(h, &s->vals, 4 * cap);
        uint32_t *topic = tmn_get(h, &s->rtopic, 4 * cap);
        uint32_t *member = tmn_get(h, &s->smember, 4 * cap);
        uint32_t *dt = tmn_get(h, &s->dtopic, 4 * dcap);
        uint32_t *dv = tmn_get(h, &s->dvalue, 4 * dcap);
        uint32_t *ds = tmn_get(h, &s->dsub, 4 * dcap);
        if (!doff || !err || !head || !ghead || !vals || !topic || !member || !dt || !dv || !ds) return TM_ENOMEM;
        cap = min3(s->vals.cap, s->rtopic.cap, s->smember.cap) / 4;
        dcap = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
        /* a group per delivery slot, whatever the delivery buffers hold by now */
        uint32_t *gs = tmn_get(h, &s->gsub, 4 * dcap);
        uint32_t *go = tmn_get(h, &s->goff, 4 * (dcap + 1));
        if (!gs || !go) return TM_ENOMEM;
        if (tries) s->reruns++;
        rc = tm_publish_deliver_batch32(h, n, s->blob.p, s->offs.p, n_dests, local_dest, TM_ROUTE_AGGRE, doff, topic, vals,
                                        cap, head, dt, dv, ds, dcap, kc, kt, seed, member, ghead, gs, go, dcap, err);
        /* TM_ECAP: no pick was made and no state has moved, from whichever of
           the two.  From the entries the bucket offsets hold the full
           (un-aggregated) total; once they fit they hold K, and with the head
           the exact T + K */
        if (rc == TM_ECAP) {
            if (doff[n_dests + 1] > cap) cap = doff[n_dests + 1];
            else if (head[1] + doff[n_dests + 1] > dcap) dcap = head[1] + doff[n_dests + 1];
            else break;   /* (never: the groups have room for every delivery) */
        }
    }
    for (uint32_t i = 0; rc == TM_OK && i < n; i++)
        if (err[i] > TMN_ERR_TOO_DEEP) rc = TM_EDEVICE;
    if (rc == TM_OK) {
        s->route_dests = n_dests;
        s->deliveries = ghead[1];
        s->picks = doff[n_dests + 1];
        s->groups = ghead[0];
        s->dispatched = 4;
    }
    return rc;
}
