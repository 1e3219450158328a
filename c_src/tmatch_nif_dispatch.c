/*
 * tmatch_nif_dispatch.c -- route fan-out plus local dispatch over the NIF
 * core's buffer sets (see tmatch_nif_dispatch.h).
 */
#include "tmatch_nif_dispatch.h"

static uint64_t min3(uint64_t a, uint64_t b, uint64_t c) {
    const uint64_t m = a < b ? a : b;
    return m < c ? m : c;
}

int tmn_dispatch(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t flags) {
    s->route_dests = 0;
    s->deliveries = 0;
    s->dispatched = 0;
    if (!n_dests || n_dests > 65536 || local_dest >= n_dests) return TM_EINVAL;
    uint32_t *doff = tmn_get(h, &s->rdoff, 4ull * ((uint64_t)n_dests + 2));
    uint8_t *err = tmn_get(h, &s->err, (uint64_t)n + 1);
    uint64_t *head = tmn_get(h, &s->dhead, 16);
    /* capacity: what the set already holds, at least TMN_IDS_PER_TOPIC entries / deliveries per topic */
    const uint64_t want = (uint64_t)TMN_IDS_PER_TOPIC * n + 1024;
    const uint64_t have = (s->vals.cap < s->rtopic.cap ? s->vals.cap : s->rtopic.cap) / 4;
    const uint64_t dhave = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
    uint64_t cap = have > want ? have : want, dcap = dhave > want ? dhave : want;
    int rc = TM_ECAP;
    for (int tries = 0; rc == TM_ECAP && tries < 5; tries++) {
        uint32_t *vals = tmn_get(h, &s->vals, 4 * cap);
        uint32_t *topic = tmn_get(h, &s->rtopic, 4 * cap);
        uint32_t *dt = tmn_get(h, &s->dtopic, 4 * dcap);
        uint32_t *dv = tmn_get(h, &s->dvalue, 4 * dcap);
        uint32_t *ds = tmn_get(h, &s->dsub, 4 * dcap);
        if (!doff || !err || !head || !vals || !topic || !dt || !dv || !ds) return TM_ENOMEM;
        cap = (s->vals.cap < s->rtopic.cap ? s->vals.cap : s->rtopic.cap) / 4;
        dcap = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
        if (tries) s->reruns++;
        rc = tm_dispatch_batch32(h, n, s->blob.p, s->offs.p, n_dests, local_dest, flags, doff, topic, vals, cap, head,
                                 dt, dv, ds, dcap, err);
        /* TM_ECAP: the bucket offsets hold the full sizes and the head the
           delivery total, so the rerun has room for both (again only if
           concurrent writes grew a total in between) */
        if (rc == TM_ECAP) {
            if (doff[n_dests + 1] > cap) cap = doff[n_dests + 1];
            if (head[1] > dcap) dcap = head[1];
        }
    }
    for (uint32_t i = 0; rc == TM_OK && i < n; i++)
        if (err[i] > TMN_ERR_TOO_DEEP) rc = TM_EDEVICE;
    if (rc == TM_OK) {
        s->route_dests = n_dests;
        s->deliveries = head[1];
        s->dispatched = 1;
    }
    return rc;
}

int tmn_deliveries(const tmn_set *s, const uint32_t **topics, const uint32_t **values, const uint32_t **subs,
                   uint64_t *count) {
    *topics = *values = *subs = 0;
    *count = 0;
    if (!s->dispatched) return TM_EINVAL;
    *topics = s->dtopic.p;
    *values = s->dvalue.p;
    *subs = s->dsub.p;
    *count = s->deliveries;
    return 0;
}
