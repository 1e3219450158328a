/*
 * nif_route_shim.c -- TEST INFRASTRUCTURE: handles for ctypes over the NIF
 * core (c_src/tmatch_nif_core.c + tmatch_nif_route.c) linked against the real
 * libtmatch (tests/test_gpu_route_batch32.py): a pool on a live index with the
 * NIF's input placement, and the set's result arrays.
 */
#include <stdlib.h>

#include "tmatch_nif_route.h"

tmn_pool *shim_pool_new(tm_index *h, uint32_t in_flags) {
    tmn_pool *p = malloc(sizeof *p);
    if (!p) return NULL;
    tmn_pool_init(p, h);
    p->in_flags = in_flags;
    return p;
}
void shim_pool_free(tmn_pool *p) { tmn_pool_destroy(p); free(p); }
const uint32_t *shim_vals(tmn_set *s) { return tmn_vals(s); }
const uint32_t *shim_route_topics(tmn_set *s) { return tmn_route_topics(s); }
const uint8_t *shim_err(tmn_set *s) { return (const uint8_t *)s->err.p; }
uint64_t shim_reruns(tmn_set *s) { return s->reruns; }
uint32_t shim_input_flags(tmn_set *s) { return s->blob.flags; }
