/*
 * nif_chain_shim.c -- TEST INFRASTRUCTURE: handles for ctypes over all seven
 * ERTS-free units of c_src/ linked against the real libtmatch
 * (tests/test_gpu_nif_chain.py, tests/test_gpu_nif_match.py): what ctypes
 * cannot reach by itself -- a pool on a live index, the static inline readers,
 * the set's bookkeeping words, its buffer capacities and the sizing constant.
 */
#include <stdlib.h>

#include "tmatch_nif_aggre.h"
#include "tmatch_nif_publish_deliver.h"

tmn_pool *shim_pool_new(tm_index *h, uint32_t in_flags) {
    tmn_pool *p = malloc(sizeof *p);
    if (!p) return NULL;
    tmn_pool_init(p, h);
    p->in_flags = in_flags;
    return p;
}
void shim_pool_free(tmn_pool *p) { tmn_pool_destroy(p); free(p); }
int shim_pool_count(tmn_pool *p) { return p->npool; }
const uint32_t *shim_vals(tmn_set *s) { return tmn_vals(s); }
const uint32_t *shim_route_topics(tmn_set *s) { return tmn_route_topics(s); }
const uint8_t *shim_err(tmn_set *s) { return (const uint8_t *)s->err.p; }
uint64_t shim_direct(tmn_set *s) { return tmn_direct(s); }
uint64_t shim_reruns(tmn_set *s) { return s->reruns; }
uint32_t shim_in_flags(tmn_set *s) { return s->in_flags; }          /* what the set asks for */
uint32_t shim_input_flags(tmn_set *s) { return s->blob.flags; }     /* what its topic bytes got */
uint32_t shim_dispatched(tmn_set *s) { return s->dispatched; }
uint32_t shim_ids_per_topic(void) { return TMN_IDS_PER_TOPIC; }

/* capacities in 32-bit words: 0 entries (the members with them, once allocated), 1 deliveries, 2 groups, 3 values */
uint64_t shim_cap(tmn_set *s, int what) {
    uint64_t a, b, c;
    switch (what) {
    case 0:
        a = s->vals.cap, b = s->rtopic.cap;
        c = s->smember.p ? s->smember.cap : a;
        break;
    case 1: a = s->dtopic.cap, b = s->dvalue.cap, c = s->dsub.cap; break;
    case 2: a = s->gsub.cap, b = s->goff.cap >= 4 ? s->goff.cap - 4 : 0, c = a; break;
    default: a = b = c = s->vals.cap; break;
    }
    if (b < a) a = b;
    if (c < a) a = c;
    return a / 4;
}

/* the words a fresh buffer asked to hold `words` ends up with (tmn_get's growth rule, on the real allocator) */
uint64_t shim_first_cap(tm_index *h, uint64_t words) {
    tmn_buf b = {0, 0, 0};
    if (!tmn_get(h, &b, 4 * words)) return 0;
    tm_host_free(h, b.p);
    return b.cap / 4;
}
