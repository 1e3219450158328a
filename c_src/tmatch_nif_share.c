/*
 * tmatch_nif_share.c -- route fan-out, local dispatch and the shared-
 * subscription pick over the NIF core's buffer sets (see tmatch_nif_share.h).
 */
#include "tmatch_nif_share.h"

#include <string.h>

static uint64_t min3(uint64_t a, uint64_t b, uint64_t c) {
    const uint64_t m = a < b ? a : b;
    return m < c ? m : c;
}

int tmn_share_keys(tmn_set *s, tm_index *h, uint32_t n, const uint32_t *clientid_words, const uint32_t *topic_words) {
    s->key_n = 0;
    s->key_mask = 0;
    if (!clientid_words && !topic_words) return TM_OK;
    if (clientid_words) {
        uint32_t *kc = tmn_get(h, &s->skc, 4ull * n + 4);
        if (!kc) return TM_ENOMEM;
        memcpy(kc, clientid_words, 4ull * n);
        s->key_mask |= 1u;
    }
    if (topic_words) {
        uint32_t *kt = tmn_get(h, &s->skt, 4ull * n + 4);
        if (!kt) { s->key_mask = 0; return TM_ENOMEM; }
        memcpy(kt, topic_words, 4ull * n);
        s->key_mask |= 2u;
    }
    s->key_n = n;
    return TM_OK;
}

int tmn_publish(tmn_set *s, tm_index *h, uint32_t n, uint32_t n_dests, uint32_t local_dest, uint32_t seed) {
    s->route_dests = 0;
    s->deliveries = 0;
    s->dispatched = 0;
    s->picks = 0;
    if (!n_dests || n_dests > 65536 || local_dest >= n_dests) return TM_EINVAL;
    if (s->key_mask && s->key_n != n) return TM_EINVAL;
    const uint32_t *kc = (s->key_mask & 1u) ? s->skc.p : 0, *kt = (s->key_mask & 2u) ? s->skt.p : 0;
    uint32_t *doff = tmn_get(h, &s->rdoff, 4ull * ((uint64_t)n_dests + 2));
    uint8_t *err = tmn_get(h, &s->err, (uint64_t)n + 1);
    uint64_t *head = tmn_get(h, &s->dhead, 16);
    /* capacity: what the set already holds, at least TMN_IDS_PER_TOPIC entries / deliveries per topic --
       both BEFORE the first call: a rerun for the deliveries alone picks a second time */
    const uint64_t want = (uint64_t)TMN_IDS_PER_TOPIC * n + 1024;
    const uint64_t have = min3(s->vals.cap, s->rtopic.cap, s->smember.cap) / 4;
    const uint64_t dhave = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
    uint64_t cap = have > want ? have : want, dcap = dhave > want ? dhave : want;
    int rc = TM_ECAP;
    for (int tries = 0; rc == TM_ECAP && tries < 5; tries++) {
        uint32_t *vals = tmn_get(h, &s->vals, 4 * cap);
        uint32_t *topic = tmn_get(h, &s->rtopic, 4 * cap);
        uint32_t *member = tmn_get(h, &s->smember, 4 * cap);
        uint32_t *dt = tmn_get(h, &s->dtopic, 4 * dcap);
        uint32_t *dv = tmn_get(h, &s->dvalue, 4 * dcap);
        uint32_t *ds = tmn_get(h, &s->dsub, 4 * dcap);
        if (!doff || !err || !head || !vals || !topic || !member || !dt || !dv || !ds) return TM_ENOMEM;
        cap = min3(s->vals.cap, s->rtopic.cap, s->smember.cap) / 4;
        dcap = min3(s->dtopic.cap, s->dvalue.cap, s->dsub.cap) / 4;
        if (tries) s->reruns++;
        rc = tm_publish_batch32(h, n, s->blob.p, s->offs.p, n_dests, local_dest, TM_ROUTE_AGGRE, doff, topic, vals, cap,
                                head, dt, dv, ds, dcap, kc, kt, seed, member, err);
        /* TM_ECAP: the bucket offsets hold the full sizes and the head the
           delivery total, so the rerun has room for both.  From the entries:
           no state has moved.  From the deliveries alone: it has, and the
           rerun moves it again (tmatch_nif_share.h) */
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
        s->picks = doff[n_dests + 1];
        s->dispatched = 2;
    }
    return rc;
}

int tmn_picks(const tmn_set *s, const uint32_t **members, uint64_t *count) {
    *members = 0;
    *count = 0;
    if (s->dispatched != 2 && s->dispatched != 4) return TM_EINVAL;
    *members = s->smember.p;
    *count = s->picks;
    return 0;
}
