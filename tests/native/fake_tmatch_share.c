/*
 * fake_tmatch_share.c -- TEST INFRASTRUCTURE: tm_publish_batch32 for the
 * stand-in libtmatch (fake_tmatch.c + fake_tmatch_route.c +
 * fake_tmatch_dispatch.c), so c_src/tmatch_nif_share.c runs on the CPU
 * (tests/test_publish32_cpu.py, tests/native/nif_share_check.c).  The route
 * outputs, the head and the deliveries are fake_tmatch_dispatch.c's.  The pick
 * of kept entry q (topic t, value v): none (0xFFFFFFFF) when v % 5 == 0, else
 * fake_share_member(v, key_clientid[t], key_topic[t], seed, moves) with a NULL
 * key array read as zeros and `moves` the number of calls that picked before
 * this one -- the stand-in's state: it advances once per call that picks.  As
 * the library, the call picks nothing and moves nothing under TM_ECAP from cap
 * (total > cap), and picks under TM_ECAP from dcap alone.  TM_EINVAL without
 * TM_ROUTE_AGGRE or without out_member while cap > 0.  Counts its calls and
 * keeps the cap, the dcap and the key pointers of each of the last few.
 */
#include <stdlib.h>
#include <string.h>

#include "tmatch.h"
#include "tmatch_nif_share.h"

static long n_publish, n_moves;
static uint64_t caps[8], dcaps[8];
static const void *keys[8][2];

uint32_t fake_share_member(uint32_t v, uint32_t kc, uint32_t kt, uint32_t seed, long moves) {
    return (v * 2u + 1u + kc * 3u + kt * 7u + seed * 11u + (uint32_t)moves * 13u) & 0x7FFFFFFFu;
}

int tm_publish_batch32(tm_index *h, uint64_t n, const uint8_t *tb, const uint32_t *to, uint32_t n_dests,
                       uint32_t local_dest, uint32_t flags, uint32_t *doff, uint32_t *out_topic, uint32_t *out_values,
                       uint64_t cap, uint64_t *head, uint32_t *dt, uint32_t *dv, uint32_t *ds, uint64_t dcap,
                       const uint32_t *key_clientid, const uint32_t *key_topic, uint32_t seed, uint32_t *out_member,
                       uint8_t *err) {
    caps[n_publish % 8] = cap;
    dcaps[n_publish % 8] = dcap;
    keys[n_publish % 8][0] = key_clientid;
    keys[n_publish % 8][1] = key_topic;
    n_publish++;
    if (!(flags & TM_ROUTE_AGGRE) || (cap && !out_member)) return TM_EINVAL;
    const int rc = tm_dispatch_batch32(h, n, tb, to, n_dests, local_dest, flags, doff, out_topic, out_values, cap, head,
                                       dt, dv, ds, dcap, err);
    if (rc != TM_OK && rc != TM_ECAP) return rc;
    const uint64_t total = doff[n_dests + 1];
    if (total > cap) return TM_ECAP;   /* no pick, no state moved */
    for (uint64_t q = 0; q < total; q++) {
        const uint32_t t = out_topic[q], v = out_values[q];
        out_member[q] = v % 5 == 0 ? 0xFFFFFFFFu
                                   : fake_share_member(v, key_clientid ? key_clientid[t] : 0, key_topic ? key_topic[t] : 0,
                                                       seed, n_moves);
    }
    n_moves++;
    return rc;
}

long fake_publish_count(void) { return n_publish; }
long fake_share_moves(void) { return n_moves; }
uint64_t fake_publish_cap(long call) { return caps[call % 8]; }
uint64_t fake_publish_dcap(long call) { return dcaps[call % 8]; }
int fake_publish_keys(long call) { return (keys[call % 8][0] ? 1 : 0) | (keys[call % 8][1] ? 2 : 0); }
uint64_t fake_set_member_cap(tmn_set *s) { return s->smember.cap; }
int fake_set_keys_in_set(tmn_set *s, long call) {
    return (!keys[call % 8][0] || keys[call % 8][0] == s->skc.p) && (!keys[call % 8][1] || keys[call % 8][1] == s->skt.p);
}
