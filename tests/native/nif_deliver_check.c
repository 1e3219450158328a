/*
 * nif_deliver_check.c -- TEST INFRASTRUCTURE: a stand-alone driver of
 * c_src/tmatch_nif_core.c + tmatch_nif_route.c + tmatch_nif_dispatch.c +
 * tmatch_nif_deliver.c over the stand-in libtmatch (fake_tmatch.c,
 * fake_tmatch_route.c, fake_tmatch_dispatch.c, fake_tmatch_deliver.c), built
 * with -fsanitize=address,undefined and run as a subprocess by
 * tests/test_deliver32_cpu.py: slices, groups and grouped deliveries, one rerun
 * per kind of TM_ECAP (entries, deliveries, groups, all at once), err 4 ->
 * TM_EDEVICE, tmn_give and the pool's destruction (every buffer freed).
 * Prints "ok" and exits 0, or the line of the first failed check and exits 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tmatch_nif_deliver.h"

long fake_count(int what);
void fake_dispatch_mult(uint32_t m);
uint32_t fake_dispatch_subs(uint32_t v);
void fake_deliver_mod(uint32_t m);
uint32_t fake_deliver_sub(uint32_t v, uint32_t r);
long fake_deliver_count(void);
uint64_t fake_deliver_cap(long call);
uint64_t fake_deliver_dcap(long call);
uint64_t fake_deliver_gcap(long call);

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static tm_index *const H = (tm_index *)0x1;

static void pack(tmn_set *s, uint32_t n, const char *const *topics) {
    uint64_t lens[16];
    for (uint32_t i = 0; i < n; i++) lens[i] = strlen(topics[i]);
    CHECK(tmn_pack(s, H, n, (const uint8_t *const *)topics, lens) == TM_OK);
}

/* the slices against the fakes' rules, and the groups against the deliveries in dispatch order: group g
   holds exactly the deliveries of its subscriber, in that order, and the subscribers ascend */
static void verify(const tmn_set *s, uint32_t n, const char *const *topics, uint32_t n_dests, uint32_t local) {
    const uint32_t *dt, *dv, *ds, *gs, *go;
    uint64_t count, groups, T = 0;
    CHECK(tmn_deliveries(s, &dt, &dv, &ds, &count) == 0);
    CHECK(tmn_groups(s, &gs, &go, &groups) == 0);
    uint32_t *et = malloc(4 * (count + 1)), *ev = malloc(4 * (count + 1)), *es = malloc(4 * (count + 1));
    CHECK(et && ev && es);
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
                for (uint32_t r = 0; r < fake_dispatch_subs(v); r++, T++) {
                    CHECK(T < count);
                    et[T] = i; ev[T] = v; es[T] = fake_deliver_sub(v, r);
                }
            }
        }
        CHECK(q == e);
    }
    CHECK(T == count && go[0] == 0 && go[groups] == count && (count == 0) == (groups == 0));
    for (uint64_t g = 0; g < groups; g++) {
        CHECK(go[g] < go[g + 1] && (g == 0 || gs[g - 1] < gs[g]));
        uint64_t at = go[g];
        for (uint64_t i = 0; i < count; i++)
            if (es[i] == gs[g]) {
                CHECK(at < go[g + 1] && dt[at] == et[i] && dv[at] == ev[i] && ds[at] == gs[g]);
                at++;
            }
        CHECK(at == go[g + 1]);
    }
    free(et); free(ev); free(es);
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

    /* 1. slices, groups and grouped deliveries; the other calls on the same set */
    tmn_set *s = tmn_take(&pool);
    CHECK(s);
    pack(s, 5, small);
    {
        const uint32_t *a, *b;
        uint64_t cnt = 7;
        CHECK(tmn_groups(s, &a, &b, &cnt) == TM_EINVAL && cnt == 0 && !a && !b);   /* nothing delivered yet */
    }
    long c0 = fake_deliver_count();
    for (uint32_t local = 0; local < 3; local++) {
        CHECK(tmn_deliver(s, H, 5, 3, local, local ? TM_ROUTE_AGGRE : 0) == TM_OK && s->reruns == 0);
        verify(s, 5, small, 3, local);
        CHECK(s->groups > 1 && s->groups <= 13 && s->deliveries > s->groups);
    }
    CHECK(fake_deliver_count() - c0 == 3);
    CHECK(tmn_route_err(s, 1) == TMN_ERR_BADARG && tmn_route_err(s, 0) == 0);
    CHECK(tmn_deliver(s, H, 5, 3, 3, 0) == TM_EINVAL && tmn_deliver(s, H, 5, 0, 0, 0) == TM_EINVAL);
    {
        const uint32_t *a, *b, *c;
        uint64_t cnt = 7;
        CHECK(tmn_groups(s, &a, &b, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_dispatch(s, H, 5, 3, 1, 0) == TM_OK);                  /* a plain dispatch: deliveries, no groups */
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == 0 && tmn_groups(s, &a, &b, &cnt) == TM_EINVAL);
        CHECK(tmn_deliver(s, H, 5, 3, 1, 0) == TM_OK && tmn_groups(s, &a, &b, &cnt) == 0 && cnt > 1);
    }
    CHECK(tmn_match(s, H, 5, TM_ORDER_TRAVERSAL) == TM_OK);
    tmn_give(&pool, s);

    /* 2. TM_ECAP from the groups alone: a plain dispatch grew the delivery buffers, every delivery its own group */
    s = tmn_take(&pool);
    fake_dispatch_mult(200);
    fake_deliver_mod(0);
    pack(s, 2, shorty);
    CHECK(tmn_dispatch(s, H, 2, 1, 0, 0) == TM_OK && s->reruns == 1);
    c0 = fake_deliver_count();
    CHECK(tmn_deliver(s, H, 2, 1, 0, 0) == TM_OK);
    CHECK(fake_deliver_count() - c0 == 2 && s->reruns == 2 && s->groups == s->deliveries);
    CHECK(fake_deliver_cap(c0) == fake_deliver_cap(c0 + 1) && fake_deliver_dcap(c0) == fake_deliver_dcap(c0 + 1));
    CHECK(fake_deliver_gcap(c0) < s->groups && s->groups <= fake_deliver_gcap(c0 + 1));
    verify(s, 2, shorty, 1, 0);
    c0 = fake_deliver_count();
    CHECK(tmn_deliver(s, H, 2, 1, 0, 0) == TM_OK && fake_deliver_count() - c0 == 1 && s->reruns == 2);   /* sticky */
    tmn_give(&pool, s);

    /* 3. from the deliveries (a new set): the groups get room for a group per delivery, one rerun */
    tmn_set *s2 = tmn_take(&pool), *s3 = tmn_take(&pool);
    CHECK(s2 == s && s3 && s3 != s);
    tmn_give(&pool, s2);
    s = s3;
    pack(s, 2, shorty);
    c0 = fake_deliver_count();
    CHECK(tmn_deliver(s, H, 2, 1, 0, 0) == TM_OK);
    CHECK(fake_deliver_count() - c0 == 2 && s->reruns == 1 && s->groups == s->deliveries);
    CHECK(fake_deliver_dcap(c0) < s->deliveries && s->deliveries <= fake_deliver_dcap(c0 + 1));
    CHECK(fake_deliver_gcap(c0 + 1) >= s->deliveries && fake_deliver_cap(c0) == fake_deliver_cap(c0 + 1));
    verify(s, 2, shorty, 1, 0);
    tmn_give(&pool, s);

    /* 4. from the entries alone: many entries, short lists, few groups */
    s = calloc(1, sizeof *s);   /* (a fresh set, as tmn_take makes one for an empty pool; it joins the pool below) */
    CHECK(s);
    fake_dispatch_mult(1);
    fake_deliver_mod(13);
    pack(s, 2, big);
    c0 = fake_deliver_count();
    CHECK(tmn_deliver(s, H, 2, 15, 2, 0) == TM_OK);
    CHECK(fake_deliver_count() - c0 == 2 && s->reruns == 1 && s->groups == 13);
    CHECK(fake_deliver_cap(c0) < 3200 && fake_deliver_cap(c0 + 1) >= 3200);
    CHECK(fake_deliver_dcap(c0) == fake_deliver_dcap(c0 + 1) && fake_deliver_gcap(c0) == fake_deliver_gcap(c0 + 1));
    CHECK(s->deliveries <= fake_deliver_dcap(c0));
    verify(s, 2, big, 15, 2);
    tmn_give(&pool, s);

    /* 5. from all three at once: still one rerun */
    s = calloc(1, sizeof *s);
    CHECK(s);
    fake_dispatch_mult(2);
    fake_deliver_mod(0);
    pack(s, 2, big);
    c0 = fake_deliver_count();
    CHECK(tmn_deliver(s, H, 2, 4, 2, 0) == TM_OK);
    CHECK(fake_deliver_count() - c0 == 2 && s->reruns == 1 && s->groups < s->deliveries);   /* (values of both topics) */
    CHECK(fake_deliver_cap(c0) < 3200 && fake_deliver_cap(c0 + 1) >= 3200);
    CHECK(fake_deliver_dcap(c0) < s->deliveries && s->deliveries <= fake_deliver_dcap(c0 + 1));
    CHECK(fake_deliver_gcap(c0) < s->groups && s->groups <= fake_deliver_gcap(c0 + 1));
    verify(s, 2, big, 4, 2);

    /* 6. a batch the device failed: TM_EDEVICE, nothing left to read */
    fake_dispatch_mult(1);
    fake_deliver_mod(13);
    const char *flagged[] = {"ab", "!x", "cd"}, *failed[] = {"ab", "~x"};
    for (int k = 0; k < 2; k++) {
        const uint32_t *a, *b, *c;
        uint64_t cnt, b0, e0;
        pack(s, k ? 2 : 3, k ? failed : flagged);
        CHECK(tmn_deliver(s, H, k ? 2 : 3, 2, 0, 0) == TM_EDEVICE);
        CHECK(tmn_groups(s, &a, &b, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_route_dest(s, 0, &b0, &e0) == TM_EINVAL);
    }
    const char *fine[] = {"abcdefgh", "+x"};
    pack(s, 2, fine);
    CHECK(tmn_deliver(s, H, 2, 2, 1, 0) == TM_OK);
    verify(s, 2, fine, 2, 1);
    tmn_give(&pool, s);

    /* 7. every buffer goes with the pool: the group head and the two group buffers too */
    const long f0 = fake_count(1);
    tmn_pool_destroy(&pool);
    CHECK(fake_count(0) == fake_count(1) && fake_count(0) > 20 && fake_count(1) - f0 >= 4 * 11);
    printf("ok\n");
    return 0;
}
