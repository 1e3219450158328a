/*
 * nif_share_check.c -- TEST INFRASTRUCTURE: a stand-alone driver of
 * c_src/tmatch_nif_core.c + tmatch_nif_route.c + tmatch_nif_dispatch.c +
 * tmatch_nif_share.c over the stand-in libtmatch (fake_tmatch.c,
 * fake_tmatch_route.c, fake_tmatch_dispatch.c, fake_tmatch_share.c), built
 * with -fsanitize=address,undefined and run as a subprocess by
 * tests/test_publish32_cpu.py: slices, picks and deliveries, key words NULL or
 * given, one rerun per kind of TM_ECAP (from the entries: one pick; from the
 * deliveries alone: the rerun picks again), err 4 -> TM_EDEVICE, tmn_give and
 * the pool's destruction (every buffer freed).  Prints "ok" and exits 0, or
 * the line of the first failed check and exits 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tmatch_nif_share.h"

long fake_count(int what);
void fake_dispatch_mult(uint32_t m);
uint32_t fake_dispatch_subs(uint32_t v);
long fake_publish_count(void);
long fake_share_moves(void);
uint64_t fake_publish_cap(long call);
uint64_t fake_publish_dcap(long call);
int fake_publish_keys(long call);
int fake_set_keys_in_set(tmn_set *s, long call);
uint32_t fake_share_member(uint32_t v, uint32_t kc, uint32_t kt, uint32_t seed, long moves);

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static tm_index *const H = (tm_index *)0x1;

static void pack(tmn_set *s, uint32_t n, const char *const *topics) {
    uint64_t lens[16];
    for (uint32_t i = 0; i < n; i++) lens[i] = strlen(topics[i]);
    CHECK(tmn_pack(s, H, n, (const uint8_t *const *)topics, lens) == TM_OK);
}

/* the slices, the picks and the deliveries against the fakes' rules, recomputed here */
static void verify(const tmn_set *s, uint32_t n, const char *const *topics, uint32_t n_dests, uint32_t local,
                   const uint32_t *kc, const uint32_t *kt, uint32_t seed) {
    const uint32_t *dt, *dv, *ds, *mem;
    uint64_t count, picks, at = 0, entries = 0, none = 0;
    const long moves = fake_share_moves() - 1;   /* the call that stands was the last to pick */
    CHECK(tmn_deliveries(s, &dt, &dv, &ds, &count) == 0);
    CHECK(tmn_picks(s, &mem, &picks) == 0);
    for (uint32_t d = 0; d <= n_dests; d++) {
        uint64_t b, e, q;
        CHECK(tmn_route_dest(s, d, &b, &e) == 0);
        q = b;
        for (uint32_t i = 0; i < n; i++) {
            const size_t len = topics[i][0] == '+' ? 0 : strlen(topics[i]);
            for (size_t k = 0; k < len; k++) {
                const uint32_t v = (uint32_t)(1000 * i + k);
                if (v % (n_dests + 1) != d) continue;
                CHECK(q < e && q < picks && tmn_route_topics(s)[q] == i && tmn_vals(s)[q] == v);
                if (v % 5 == 0) { CHECK(mem[q] == 0xFFFFFFFFu); none++; }
                else CHECK(mem[q] == fake_share_member(v, kc ? kc[i] : 0, kt ? kt[i] : 0, seed, moves));
                q++;
                if (d != local) continue;
                for (uint32_t r = 0; r < fake_dispatch_subs(v); r++, at++)
                    CHECK(at < count && dt[at] == i && dv[at] == v && ds[at] == v * 16 + r);
            }
        }
        CHECK(q == e);
        entries += e - b;
    }
    CHECK(at == count && entries > 0 && entries == picks && none > 0 && none < picks);
}

int main(void) {
    static char longx[3001], longy[201];
    memset(longx, 'x', 3000);
    memset(longy, 'y', 200);
    const char *small[] = {"abcde", "+x", "", "xyz", "0123456789"};
    const char *shorty[] = {"abcdefg", "hijklmn"};
    const char *big[] = {longx, longy};
    const uint32_t kc5[] = {11, 22, 33, 44, 55}, kt5[] = {5, 4, 3, 2, 1};
    tmn_pool pool;
    tmn_pool_init(&pool, H);

    /* 1. slices, picks and deliveries; key words NULL or given; the other calls on the same set */
    tmn_set *s = tmn_take(&pool);
    CHECK(s);
    pack(s, 5, small);
    {
        const uint32_t *m;
        uint64_t cnt = 7;
        CHECK(tmn_picks(s, &m, &cnt) == TM_EINVAL && cnt == 0 && !m);   /* nothing published yet */
    }
    long c0 = fake_publish_count(), m0 = fake_share_moves();
    CHECK(tmn_publish(s, H, 5, 3, 1, 9) == TM_OK);
    CHECK(fake_publish_count() - c0 == 1 && fake_share_moves() - m0 == 1 && s->reruns == 0);
    CHECK(fake_publish_keys(c0) == 0);
    verify(s, 5, small, 3, 1, 0, 0, 9);
    CHECK(tmn_share_keys(s, H, 5, kc5, kt5) == TM_OK);
    c0 = fake_publish_count();
    CHECK(tmn_publish(s, H, 5, 3, 0, 3) == TM_OK);
    CHECK(fake_publish_keys(c0) == 3 && fake_set_keys_in_set(s, c0));
    verify(s, 5, small, 3, 0, kc5, kt5, 3);
    CHECK(tmn_share_keys(s, H, 5, 0, kt5) == TM_OK);
    c0 = fake_publish_count();
    CHECK(tmn_publish(s, H, 5, 3, 2, 3) == TM_OK && fake_publish_keys(c0) == 2 && fake_set_keys_in_set(s, c0));
    verify(s, 5, small, 3, 2, 0, kt5, 3);
    CHECK(tmn_share_keys(s, H, 5, kc5, 0) == TM_OK);
    c0 = fake_publish_count();
    CHECK(tmn_publish(s, H, 5, 3, 2, 4) == TM_OK && fake_publish_keys(c0) == 1);
    verify(s, 5, small, 3, 2, kc5, 0, 4);
    CHECK(tmn_publish(s, H, 4, 3, 2, 4) == TM_EINVAL);          /* keys set for another n */
    CHECK(tmn_share_keys(s, H, 5, 0, 0) == TM_OK);
    c0 = fake_publish_count();
    CHECK(tmn_publish(s, H, 5, 3, 1, 1) == TM_OK && fake_publish_keys(c0) == 0);
    verify(s, 5, small, 3, 1, 0, 0, 1);
    CHECK(tmn_route_err(s, 1) == TMN_ERR_BADARG && tmn_route_err(s, 0) == 0);
    CHECK(tmn_publish(s, H, 5, 3, 3, 0) == TM_EINVAL && tmn_publish(s, H, 5, 0, 0, 0) == TM_EINVAL);
    {
        const uint32_t *a, *b, *c, *m;
        uint64_t cnt = 7;
        CHECK(tmn_picks(s, &m, &cnt) == TM_EINVAL && cnt == 0 && !m);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_dispatch(s, H, 5, 3, 1, TM_ROUTE_AGGRE) == TM_OK);   /* a plain dispatch: deliveries, no picks */
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == 0 && tmn_picks(s, &m, &cnt) == TM_EINVAL);
    }
    CHECK(tmn_match(s, H, 5, TM_ORDER_TRAVERSAL) == TM_OK);
    tmn_give(&pool, s);

    /* 2. TM_ECAP from dcap alone: few entries, long lists -- the first call's picks stood, the rerun picks again */
    s = tmn_take(&pool);
    fake_dispatch_mult(2000);
    pack(s, 2, shorty);
    c0 = fake_publish_count();
    m0 = fake_share_moves();
    uint64_t r0 = s->reruns;
    CHECK(tmn_publish(s, H, 2, 1, 0, 5) == TM_OK);
    CHECK(fake_publish_count() - c0 == 2 && s->reruns - r0 == 1 && fake_share_moves() - m0 == 2);
    CHECK(fake_publish_cap(c0) == fake_publish_cap(c0 + 1));                 /* the entries fitted */
    CHECK(fake_publish_dcap(c0) < s->deliveries && s->deliveries <= fake_publish_dcap(c0 + 1));
    verify(s, 2, shorty, 1, 0, 0, 0, 5);
    c0 = fake_publish_count();
    CHECK(tmn_publish(s, H, 2, 1, 0, 5) == TM_OK && fake_publish_count() - c0 == 1);   /* sticky */
    tmn_give(&pool, s);

    /* 3. from cap alone: many entries, short lists (a new set: the first one's sizes are sticky) -- ONE pick */
    tmn_set *s2 = tmn_take(&pool), *s3 = tmn_take(&pool);
    CHECK(s2 == s && s3 && s3 != s);
    tmn_give(&pool, s2);
    s = s3;
    fake_dispatch_mult(1);
    pack(s, 2, big);
    c0 = fake_publish_count();
    m0 = fake_share_moves();
    CHECK(tmn_publish(s, H, 2, 4, 2, 6) == TM_OK);
    CHECK(fake_publish_count() - c0 == 2 && s->reruns == 1 && fake_share_moves() - m0 == 1);
    CHECK(fake_publish_cap(c0) < 3200 && fake_publish_cap(c0 + 1) >= 3200);
    CHECK(fake_publish_dcap(c0) == fake_publish_dcap(c0 + 1) && s->deliveries <= fake_publish_dcap(c0));
    CHECK(s->smember.cap >= 4 * 3200);
    verify(s, 2, big, 4, 2, 0, 0, 6);
    c0 = fake_publish_count();
    CHECK(tmn_publish(s, H, 2, 4, 2, 6) == TM_OK && fake_publish_count() - c0 == 1 && s->reruns == 1);
    tmn_give(&pool, s);

    /* 4. from both at once: still one rerun, and one pick (the first call made none) */
    s = calloc(1, sizeof *s);   /* (a fresh set, as tmn_take makes one for an empty pool; it joins the pool below) */
    CHECK(s);
    fake_dispatch_mult(40);
    pack(s, 2, big);
    c0 = fake_publish_count();
    m0 = fake_share_moves();
    CHECK(tmn_publish(s, H, 2, 4, 2, 7) == TM_OK);
    CHECK(fake_publish_count() - c0 == 2 && s->reruns == 1 && fake_share_moves() - m0 == 1);
    CHECK(fake_publish_cap(c0) < 3200 && fake_publish_cap(c0 + 1) >= 3200);
    CHECK(fake_publish_dcap(c0) < s->deliveries && s->deliveries <= fake_publish_dcap(c0 + 1));
    verify(s, 2, big, 4, 2, 0, 0, 7);

    /* 5. a batch the device failed: TM_EDEVICE, nothing left to read */
    fake_dispatch_mult(1);
    const char *flagged[] = {"ab", "!x", "cd"}, *failed[] = {"ab", "~x"};
    for (int k = 0; k < 2; k++) {
        const uint32_t *a, *b, *c, *m;
        uint64_t cnt, b0, e0;
        pack(s, k ? 2 : 3, k ? failed : flagged);
        CHECK(tmn_publish(s, H, k ? 2 : 3, 2, 0, 0) == TM_EDEVICE);
        CHECK(tmn_picks(s, &m, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_route_dest(s, 0, &b0, &e0) == TM_EINVAL);
    }
    const char *fine[] = {"abcdefgh", "+x"};
    pack(s, 2, fine);
    CHECK(tmn_publish(s, H, 2, 2, 1, 8) == TM_OK);
    verify(s, 2, fine, 2, 1, 0, 0, 8);
    tmn_give(&pool, s);

    /* 6. every buffer goes with the pool: the key words and the members too */
    const long f0 = fake_count(1);
    tmn_pool_destroy(&pool);
    CHECK(fake_count(0) == fake_count(1) && fake_count(0) > 20 && fake_count(1) - f0 >= 3 * 9 + 2);
    printf("ok\n");
    return 0;
}
