/*
 * tmatch_nif_deliver.c -- route fan-out, local dispatch and the grouping by
 * subscriber over the NIF core's buffer sets (see tmatch_nif_deliver.h).
 */
#include "tmatch_nif_deliver.h"

static uint64_t min3(uint64_t a, uint64_t b, uint64_t c) {
    const uint64_t m = a < b ? a : b;
    return m < c ? m : c;
}

/* groups the two group buffers hold: gsub takes one word a group, goff one more than that */
static uint64_t group_room(const tmn_set *s) {
    const uint64_t a = s->gsub.cap / 4, b = s->goff.cap / 4;
    return b ? (a < b - 1 ? a : b - 1) : 0;
}

int tmn_deliver(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t flags) {
    s->route_dests = 0;
    s->deliveries = 0;
    s->dispatched = 0;
    s->groups = 0;
    if (!n_dests || n_dests > 65536 || local_dest >= n_dests) return TM_EINVAL;
    uint32_t *doff = tmn_get(h, &s->rdoff, 4ull * ((uint64_t)n_dests + 2));
    uint8_t *err = tmn_get(h, &s->err, (uint64_t)n + 1);
    uint64_t *head = tmn_get(h, &s->dhead, 16);
    uint64_t *ghead = tmn_get(h, &s->ghead, 16);
    /* capacity: what the set already holds, at least TMN_IDS_PER_TOPIC entries / deliveries / groups per topic */
    const uint64_t want = (uint64_t)TMN_IDS_PER_TOPIC * n + 1024;
    const uint64_t have = (s->vals.cap < s->rtopic.cap ? s->vals.cap : s->rtopic.cap) / 4;
    const uint64_t dhave = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
    const uint64_t ghave = group_room(s);
    uint64_t cap = have > want ? have : want, dcap = dhave > want ? dhave : want, gcap = ghave > want ? ghave : want;
    int rc = TM_ECAP;
    for (int tries = 0; rc == TM_ECAP && tries < 5; tries++) {
        uint32_t *vals = tmn_get(h, &s->vals, 4 * cap);
        uint32_t *topic = tmn_get(h, &s->rtopic, 4 * cap);
        uint32_t *dt = tmn_get(h, &s->dtopic, 4 * dcap);
        uint32_t *dv = tmn_get(h, &s->dvalue, 4 * dcap);
        uint32_t *ds = tmn_get(h, &s->dsub, 4 * dcap);
        uint32_t *gs = tmn_get(h, &s->gsub, 4 * gcap);
        uint32_t *go = tmn_get(h, &s->goff, 4 * (gcap + 1));
        if (!doff || !err || !head || !ghead || !vals || !topic || !dt || !dv || !ds || !gs || !go) return TM_ENOMEM;
        cap = (s->vals.cap < s->rtopic.cap ? s->vals.cap : s->rtopic.cap) / 4;
        dcap = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
        gcap = group_room(s);
        if (tries) s->reruns++;
        rc = tm_deliver_batch32(h, n, s->blob.p, s->offs.p, n_dests, local_dest, flags, doff, topic, vals, cap, head, dt,
                                dv, ds, dcap, ghead, gs, go, gcap, err);
        /* TM_ECAP: the bucket offsets hold the full sizes, the head the
           delivery total and the group head the groups of the deliveries that
           fitted.  All of them fitted: the group count is exact.  Some did
           not: the rerun's groups get room for a group per delivery, so it
           cannot come up short of groups (again only if concurrent writes
           grew a total in between) */
        if (rc == TM_ECAP) {
            const int short_d = head[1] > dcap;
            if (doff[n_dests + 1] > cap) cap = doff[n_dests + 1];
            if (short_d) dcap = head[1];
            if (short_d && dcap > gcap) gcap = dcap;
            if (!short_d && ghead[0] > gcap) gcap = ghead[0];
        }
    }
    for (uint32_t i = 0; rc == TM_OK && i < n; i++)
        if (err[i] > TMN_ERR_TOO_DEEP) rc = TM_EDEVICE;
    if (rc == TM_OK) {
        s->route_dests = n_dests;
        s->deliveries = head[1];
        s->groups = ghead[0];
        s->dispatched = 3;
    }
    return rc;
}

int tmn_groups(const tmn_set *s, const uint32_t **subs, const uint32_t **offs, uint64_t *count) {
    *subs = *offs = 0;
    *count = 0;
    if (s->dispatched != 3 && s->dispatched != 4) return TM_EINVAL;
    *subs = s->gsub.p;
    *offs = s->goff.p;
    *count = s->groups;
    return 0;
}
