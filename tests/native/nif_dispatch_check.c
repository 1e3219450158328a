/*
 * nif_dispatch_check.c -- TEST INFRASTRUCTURE: a stand-alone driver of
 * c_src/tmatch_nif_core.c + tmatch_nif_route.c + tmatch_nif_dispatch.c over the
 * stand-in libtmatch (fake_tmatch.c, fake_tmatch_route.c,
 * fake_tmatch_dispatch.c), built with -fsanitize=address,undefined and run as a
 * subprocess by tests/test_dispatch32_cpu.py: the slices and deliveries, one
 * rerun per kind of TM_ECAP with sticky sizes, err 4 -> TM_EDEVICE, tmn_match
 * on the same set, tmn_give and the pool's destruction (every buffer freed).
 * Prints "ok" and exits 0, or the line of the first failed check and exits 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tmatch_nif_dispatch.h"

long fake_count(int what);
void fake_dispatch_mult(uint32_t m);
uint32_t fake_dispatch_subs(uint32_t v);
long fake_dispatch_count(void);
uint64_t fake_dispatch_cap(long call);
uint64_t fake_dispatch_dcap(long call);

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static tm_index *const H = (tm_index *)0x1;

static void pack(tmn_set *s, uint32_t n, const char *const *topics) {
    uint64_t lens[16];
    for (uint32_t i = 0; i < n; i++) lens[i] = strlen(topics[i]);
    CHECK(tmn_pack(s, H, n, (const uint8_t *const *)topics, lens) == TM_OK);
}

/* the slices and the deliveries against the fakes' rule, recomputed here */
static void verify(const tmn_set *s, uint32_t n, const char *const *topics, uint32_t n_dests, uint32_t local) {
    const uint32_t *dt, *dv, *ds;
    uint64_t count, at = 0, entries = 0;
    CHECK(tmn_deliveries(s, &dt, &dv, &ds, &count) == 0);
    for (uint32_t d = 0; d <= n_dests; d++) {
        uint64_t b, e, q;
        CHECK(tmn_route_dest(s, d, &b, &e) == 0);
        q = b;
        for (uint32_t i = 0; i < n; i++) {
            const size_t len = topics[i][0] == '+' ? 0 : strlen(topics[i]);
            for (size_t k = 0; k < len; k++) {
                const uint32_t v = (uint32_t)(1000 * i + k);
                if (v % (n_dests + 1) != d) continue;
                CHECK(q < e && tmn_route_topics(s)[q] == i && tmn_vals(s)[q] == v);
                q++;
                if (d != local) continue;
                for (uint32_t r = 0; r < fake_dispatch_subs(v); r++, at++)
                    CHECK(at < count && dt[at] == i && dv[at] == v && ds[at] == v * 16 + r);
            }
        }
        CHECK(q == e);
        entries += e - b;
    }
    CHECK(at == count && entries > 0);
}

int main(void) {
    static char longx[3001], longy[201];
    memset(longx, 'x', 3000);
    memset(longy, 'y', 200);
    const char *small[] = {"abcde", "+x", "", "xyz", "0123456789"};
    const char *shorty[] = {"abcdefg", "hijklmn"};
    const char *big[] = {longx, longy};
    tmn_pool pool;
    tmn_pool_init(&pool, H);

    /* 1. slices and deliveries; the route's accessors and tmn_match on the same set */
    tmn_set *s = tmn_take(&pool);
    CHECK(s);
    pack(s, 5, small);
    long c0 = fake_dispatch_count();
    CHECK(tmn_dispatch(s, H, 5, 3, 1, 0) == TM_OK);
    CHECK(fake_dispatch_count() - c0 == 1 && s->reruns == 0);
    verify(s, 5, small, 3, 1);
    CHECK(tmn_dispatch(s, H, 5, 3, 0, TM_ROUTE_AGGRE) == TM_OK);
    verify(s, 5, small, 3, 0);
    CHECK(tmn_route_err(s, 1) == TMN_ERR_BADARG && tmn_route_err(s, 0) == 0);
    CHECK(tmn_dispatch(s, H, 5, 3, 3, 0) == TM_EINVAL && tmn_dispatch(s, H, 5, 0, 0, 0) == TM_EINVAL);
    {
        const uint32_t *a, *b, *c;
        uint64_t cnt = 7;
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0 && !a && !b && !c);
    }
    CHECK(tmn_match(s, H, 5, TM_ORDER_TRAVERSAL) == TM_OK);
    tmn_give(&pool, s);

    /* 2. TM_ECAP from dcap alone: few entries, long lists */
    s = tmn_take(&pool);
    fake_dispatch_mult(2000);
    pack(s, 2, shorty);
    c0 = fake_dispatch_count();
    uint64_t r0 = s->reruns;
    CHECK(tmn_dispatch(s, H, 2, 1, 0, 0) == TM_OK);
    CHECK(fake_dispatch_count() - c0 == 2 && s->reruns - r0 == 1);
    CHECK(fake_dispatch_cap(c0) == fake_dispatch_cap(c0 + 1));                 /* the entries fitted */
    CHECK(fake_dispatch_dcap(c0) < s->deliveries && s->deliveries <= fake_dispatch_dcap(c0 + 1));
    verify(s, 2, shorty, 1, 0);
    c0 = fake_dispatch_count();
    CHECK(tmn_dispatch(s, H, 2, 1, 0, 0) == TM_OK && fake_dispatch_count() - c0 == 1);   /* sticky */
    tmn_give(&pool, s);

    /* 3. from cap alone: many entries, short lists (a new set: the first one's sizes are sticky) */
    tmn_set *s2 = tmn_take(&pool), *s3 = tmn_take(&pool);
    CHECK(s2 == s && s3 && s3 != s);
    tmn_give(&pool, s2);
    s = s3;
    fake_dispatch_mult(1);
    pack(s, 2, big);
    c0 = fake_dispatch_count();
    CHECK(tmn_dispatch(s, H, 2, 4, 2, 0) == TM_OK);
    CHECK(fake_dispatch_count() - c0 == 2 && s->reruns == 1);
    CHECK(fake_dispatch_cap(c0) < 3200 && fake_dispatch_cap(c0 + 1) >= 3200);
    CHECK(fake_dispatch_dcap(c0) == fake_dispatch_dcap(c0 + 1) && s->deliveries <= fake_dispatch_dcap(c0));
    verify(s, 2, big, 4, 2);
    c0 = fake_dispatch_count();
    CHECK(tmn_dispatch(s, H, 2, 4, 2, 0) == TM_OK && fake_dispatch_count() - c0 == 1 && s->reruns == 1);
    tmn_give(&pool, s);

    /* 4. from both at once: still one rerun */
    s = calloc(1, sizeof *s);   /* (a fresh set, as tmn_take makes one for an empty pool; it joins the pool below) */
    CHECK(s);
    fake_dispatch_mult(40);
    pack(s, 2, big);
    c0 = fake_dispatch_count();
    CHECK(tmn_dispatch(s, H, 2, 4, 2, 0) == TM_OK);
    CHECK(fake_dispatch_count() - c0 == 2 && s->reruns == 1);
    CHECK(fake_dispatch_cap(c0) < 3200 && fake_dispatch_cap(c0 + 1) >= 3200);
    CHECK(fake_dispatch_dcap(c0) < s->deliveries && s->deliveries <= fake_dispatch_dcap(c0 + 1));
    verify(s, 2, big, 4, 2);
    c0 = fake_dispatch_count();
    CHECK(tmn_dispatch(s, H, 2, 4, 2, 0) == TM_OK && fake_dispatch_count() - c0 == 1 && s->reruns == 1);

    /* 5. a batch the device failed: TM_EDEVICE, nothing left to read */
    fake_dispatch_mult(1);
    const char *flagged[] = {"ab", "!x", "cd"}, *failed[] = {"ab", "~x"};
    for (int k = 0; k < 2; k++) {
        const uint32_t *a, *b, *c;
        uint64_t cnt, b0, e0;
        pack(s, k ? 2 : 3, k ? failed : flagged);
        CHECK(tmn_dispatch(s, H, k ? 2 : 3, 2, 0, 0) == TM_EDEVICE);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_route_dest(s, 0, &b0, &e0) == TM_EINVAL);
    }
    const char *fine[] = {"ab", "+x"};
    pack(s, 2, fine);
    CHECK(tmn_dispatch(s, H, 2, 2, 1, 0) == TM_OK);
    verify(s, 2, fine, 2, 1);
    tmn_give(&pool, s);

    /* 6. every buffer goes with the pool */
    tmn_pool_destroy(&pool);
    CHECK(fake_count(0) == fake_count(1) && fake_count(0) > 20);
    printf("ok\n");
    return 0;
}
