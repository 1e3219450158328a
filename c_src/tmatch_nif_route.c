/*
 * tmatch_nif_route.c -- route fan-out over the NIF core's buffer sets (see
 * tmatch_nif_route.h).
 */
#include "tmatch_nif_route.h"

int tmn_route(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests) {
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
    int rc = tm_route_batch32(h, n, s->blob.p, s->offs.p, n_dests, doff, topic, vals, cap, err);
    /* TM_ECAP: the bucket offsets hold the full sizes, so rerun with room for
       every entry (again if concurrent inserts grew the total in between) */
    for (int tries = 0; rc == TM_ECAP && tries < 4; tries++) {
        s->reruns++;
        const uint64_t total = doff[n_dests + 1];
        vals = tmn_get(h, &s->vals, 4 * total);
        topic = tmn_get(h, &s->rtopic, 4 * total);
        if (!vals || !topic) return TM_ENOMEM;
        cap = (s->vals.cap < s->rtopic.cap ? s->vals.cap : s->rtopic.cap) / 4;
        rc = tm_route_batch32(h, n, s->blob.p, s->offs.p, n_dests, doff, topic, vals, cap, err);
    }
    for (uint32_t i = 0; rc == TM_OK && i < n; i++)
        if (err[i] > TMN_ERR_TOO_DEEP) rc = TM_EDEVICE;
    if (rc == TM_OK) s->route_dests = n_dests;
    return rc;
}

int tmn_route_dest(const tmn_set *s, uint32_t d, uint64_t *b, uint64_t *e) {
    const uint32_t *doff = s->rdoff.p;
    *b = *e = 0;
    if (!s->route_dests || d > s->route_dests) return TM_EINVAL;
    *b = doff[d];
    *e = doff[d + 1];
    return 0;
}
