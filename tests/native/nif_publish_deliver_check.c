/*
 * nif_publish_deliver_check.c -- TEST INFRASTRUCTURE: a stand-alone driver of
 * c_src/tmatch_nif_core.c + tmatch_nif_route.c + tmatch_nif_dispatch.c +
 * tmatch_nif_share.c + tmatch_nif_deliver.c + tmatch_nif_publish_deliver.c over
 * the stand-in libtmatch (fake_tmatch.c, fake_tmatch_route.c,
 * fake_tmatch_dispatch.c, fake_tmatch_share.c, fake_tmatch_deliver.c,
 * fake_tmatch_publish_deliver.c), built with -fsanitize=address,undefined and
 * run as a subprocess by tests/test_publish_deliver32_cpu.py: slices, picks,
 * merged and grouped deliveries, one rerun per kind of TM_ECAP (entries,
 * deliveries, one after the other) with the stand-in's state moved once each
 * time, err 4 -> TM_EDEVICE, one set through every entry point in turn with the
 * readers refusing the wrong kind and the calls refused before any library call
 * (the CPU twin of tests/test_gpu_nif_chain.py), tmn_give and the pool's
 * destruction (every buffer freed).  Prints "ok" and exits 0, or the line of the
 * first failed check and exits 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tmatch_nif_publish_deliver.h"

long fake_count(int what);
void fake_dispatch_mult(uint32_t m);
uint32_t fake_dispatch_subs(uint32_t v);
uint32_t fake_pd_direct_sub(uint32_t v, uint32_t r);
uint32_t fake_pd_member(uint32_t v, uint32_t kc, uint32_t kt, uint32_t seed, long moves);
uint32_t fake_pd_local(uint32_t m);
long fake_pd_count(void);
long fake_pd_moves(void);
uint64_t fake_pd_cap(long call);
uint64_t fake_pd_dcap(long call);
uint64_t fake_pd_gcap(long call);
long fake_publish_count(void);
long fake_deliver_count(void);
long fake_dispatch_count(void);
long fake_route_count(void);

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static tm_index *const H = (tm_index *)0x1;
static const uint32_t NONE = 0xFFFFFFFFu;

static void pack(tmn_set *s, uint32_t n, const char *const *topics) {
    uint64_t lens[16];
    for (uint32_t i = 0; i < n; i++) lens[i] = strlen(topics[i]);
    CHECK(tmn_pack(s, H, n, (const uint8_t *const *)topics, lens) == TM_OK);
}

/* the slices and the picks against the fakes' rules (the pick of the call that moved the stand-in's state
   last), and the groups against the merged deliveries in publish order: message by message the direct ones
   (bucket order), then the local picks (entry order); group g holds exactly its subscriber's, in that order */
static void verify(const tmn_set *s, uint32_t n, const char *const *topics, uint32_t n_dests, uint32_t local,
                   const uint32_t *kc, const uint32_t *kt, uint32_t seed) {
    const uint32_t *dt, *dv, *ds, *gs, *go, *mem;
    uint64_t count, groups, picks, T = 0, P = 0, q = 0;
    const long moves = fake_pd_moves() - 1;
    CHECK(tmn_deliveries(s, &dt, &dv, &ds, &count) == 0);
    CHECK(tmn_groups(s, &gs, &go, &groups) == 0);
    CHECK(tmn_picks(s, &mem, &picks) == 0);
    /* per message: its direct deliveries, then its picks; at most `count` of each kind */
    uint32_t *xt = malloc(4 * (count + 1)), *xv = malloc(4 * (count + 1)), *xs = malloc(4 * (count + 1));
    uint32_t *pt = malloc(4 * (count + 1)), *pv = malloc(4 * (count + 1)), *ps = malloc(4 * (count + 1));
    CHECK(xt && xv && xs && pt && pv && ps);
    for (uint32_t d = 0; d <= n_dests; d++) {
        uint64_t b, e;
        CHECK(tmn_route_dest(s, d, &b, &e) == 0 && b == q);
        for (uint32_t i = 0; i < n; i++) {
            const size_t len = topics[i][0] == '+' ? 0 : strlen(topics[i]);
            for (size_t k = 0; k < len; k++) {
                const uint32_t v = (uint32_t)(1000 * i + k);
                if (v % (n_dests + 1) != d) continue;
                CHECK(q < e && q < picks && tmn_route_topics(s)[q] == i && tmn_vals(s)[q] == v);
                const uint32_t m = v % 5 == 0 ? NONE : fake_pd_member(v, kc ? kc[i] : 0, kt ? kt[i] : 0, seed, moves);
                CHECK(mem[q] == m);
                q++;
                if (fake_pd_local(m) != NONE) {
                    CHECK(P < count);
                    pt[P] = i; pv[P] = v; ps[P] = fake_pd_local(m);
                    P++;
                }
                if (d != local) continue;
                for (uint32_t r = 0; r < fake_dispatch_subs(v); r++, T++) {
                    CHECK(T < count);
                    xt[T] = i; xv[T] = v; xs[T] = fake_pd_direct_sub(v, r);
                }
            }
        }
        CHECK(q == e);
    }
    CHECK(q == picks && T + P == count && T == tmn_direct(s));
    CHECK(go[0] == 0 && go[groups] == count && (count == 0) == (groups == 0));
    for (uint64_t g = 0; g < groups; g++) {
        CHECK(go[g] < go[g + 1] && (g == 0 || gs[g - 1] < gs[g]));
        uint64_t at = go[g];
        for (uint32_t i = 0; i < n; i++) {
            for (uint64_t k = 0; k < T; k++)
                if (xt[k] == i && xs[k] == gs[g]) {
                    CHECK(at < go[g + 1] && dt[at] == i && dv[at] == xv[k] && ds[at] == gs[g]);
                    at++;
                }
            for (uint64_t k = 0; k < P; k++)
                if (pt[k] == i && ps[k] == gs[g]) {
                    CHECK(at < go[g + 1] && dt[at] == i && dv[at] == pv[k] && ds[at] == gs[g]);
                    at++;
                }
        }
        CHECK(at == go[g + 1]);
    }
    free(xt); free(xv); free(xs); free(pt); free(pv); free(ps);
}

int main(void) {
    static char longx[3001], longy[201];
    memset(longx, 'x', 3000);
    memset(longy, 'y', 200);
    const char *small[] = {"abcde", "+x", "", "xyz", "0123456789"};
    const char *shorty[] = {"abcdefg", "hijklmn"};
    const char *big[] = {longx, longy};
    const uint32_t kc[5] = {11, 22, 33, 44, 55}, kt[5] = {5, 4, 3, 2, 1};
    tmn_pool pool;
    tmn_pool_init(&pool, H);

    /* 1. slices, picks, merged and grouped deliveries; the other calls on the same set */
    tmn_set *s = tmn_take(&pool);
    CHECK(s);
    pack(s, 5, small);
    long c0 = fake_pd_count(), m0 = fake_pd_moves();
    for (uint32_t local = 0; local < 3; local++) {
        CHECK(tmn_share_keys(s, H, 5, local ? kc : 0, local == 2 ? 0 : kt) == TM_OK);
        CHECK(tmn_publish_deliver(s, H, 5, 3, local, 7 + local) == TM_OK && s->reruns == 0);
        verify(s, 5, small, 3, local, local ? kc : 0, local == 2 ? 0 : kt, 7 + local);
        CHECK(s->groups > 1 && s->groups <= 13 && s->deliveries > s->groups && s->deliveries > tmn_direct(s));
    }
    CHECK(fake_pd_count() - c0 == 3 && fake_pd_moves() - m0 == 3);
    CHECK(tmn_route_err(s, 1) == TMN_ERR_BADARG && tmn_route_err(s, 0) == 0);
    CHECK(tmn_publish_deliver(s, H, 4, 3, 0, 0) == TM_EINVAL);            /* the keys are for five topics */
    CHECK(tmn_publish_deliver(s, H, 5, 3, 3, 0) == TM_EINVAL && tmn_publish_deliver(s, H, 5, 0, 0, 0) == TM_EINVAL);
    {
        const uint32_t *a, *b, *c;
        uint64_t cnt = 7;
        CHECK(tmn_groups(s, &a, &b, &cnt) == TM_EINVAL && cnt == 0 && tmn_picks(s, &a, &cnt) == TM_EINVAL);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0 && tmn_direct(s) == 0);
        CHECK(tmn_publish(s, H, 5, 3, 1, 0) == TM_OK);                    /* a plain publish: picks, no groups */
        CHECK(tmn_picks(s, &a, &cnt) == 0 && tmn_groups(s, &a, &b, &cnt) == TM_EINVAL);
        CHECK(tmn_deliver(s, H, 5, 3, 1, 0) == TM_OK);                    /* a plain deliver: groups, no picks */
        CHECK(tmn_groups(s, &a, &b, &cnt) == 0 && tmn_picks(s, &a, &cnt) == TM_EINVAL);
        CHECK(tmn_publish_deliver(s, H, 5, 3, 1, 0) == TM_OK && tmn_groups(s, &a, &b, &cnt) == 0 && cnt > 1);
        CHECK(tmn_picks(s, &a, &cnt) == 0 && cnt > 1);
    }
    CHECK(tmn_share_keys(s, H, 0, 0, 0) == TM_OK);
    tmn_give(&pool, s);

    /* 2. TM_ECAP from the deliveries (T + K > dcap): one rerun sized exactly, the state moved once */
    s = calloc(1, sizeof *s);   /* (a fresh set, as tmn_take makes one for an empty pool; it joins the pool below) */
    CHECK(s);
    fake_dispatch_mult(400);
    pack(s, 2, shorty);
    c0 = fake_pd_count(), m0 = fake_pd_moves();
    CHECK(tmn_publish_deliver(s, H, 2, 1, 0, 3) == TM_OK);
    CHECK(fake_pd_count() - c0 == 2 && s->reruns == 1 && fake_pd_moves() - m0 == 1);
    CHECK(fake_pd_cap(c0) == fake_pd_cap(c0 + 1) && fake_pd_dcap(c0) < tmn_direct(s) + s->picks);
    CHECK(fake_pd_dcap(c0 + 1) >= tmn_direct(s) + s->picks && fake_pd_gcap(c0 + 1) == fake_pd_dcap(c0 + 1));
    CHECK(fake_pd_gcap(c0) == fake_pd_dcap(c0));
    verify(s, 2, shorty, 1, 0, 0, 0, 3);
    c0 = fake_pd_count();
    CHECK(tmn_publish_deliver(s, H, 2, 1, 0, 3) == TM_OK && fake_pd_count() - c0 == 1 && s->reruns == 1);   /* sticky */
    tmn_give(&pool, s);

    /* 3. from the entries (total > cap): one rerun, the state moved once */
    s = calloc(1, sizeof *s);
    CHECK(s);
    fake_dispatch_mult(1);
    pack(s, 2, big);
    c0 = fake_pd_count(), m0 = fake_pd_moves();
    CHECK(tmn_publish_deliver(s, H, 2, 15, 2, 0) == TM_OK);
    CHECK(fake_pd_count() - c0 == 2 && s->reruns == 1 && fake_pd_moves() - m0 == 1 && s->picks == 3200);
    CHECK(fake_pd_cap(c0) < 3200 && fake_pd_cap(c0 + 1) >= 3200 && fake_pd_dcap(c0) == fake_pd_dcap(c0 + 1));
    verify(s, 2, big, 15, 2, 0, 0, 0);
    tmn_give(&pool, s);

    /* 4. one after the other: the entries first, then T + K with K exact -- two reruns, the state moved once */
    s = calloc(1, sizeof *s);
    CHECK(s);
    fake_dispatch_mult(3);
    pack(s, 2, big);
    c0 = fake_pd_count(), m0 = fake_pd_moves();
    CHECK(tmn_publish_deliver(s, H, 2, 1, 0, 9) == TM_OK);
    CHECK(fake_pd_count() - c0 == 3 && s->reruns == 2 && fake_pd_moves() - m0 == 1);
    CHECK(fake_pd_cap(c0) < 3200 && fake_pd_cap(c0 + 1) >= 3200 && fake_pd_cap(c0 + 2) == fake_pd_cap(c0 + 1));
    CHECK(fake_pd_dcap(c0 + 1) == fake_pd_dcap(c0) && fake_pd_dcap(c0 + 1) < tmn_direct(s) + s->picks);
    CHECK(fake_pd_dcap(c0 + 2) >= tmn_direct(s) + s->picks);
    verify(s, 2, big, 1, 0, 0, 0, 9);

    /* 5. a batch the device failed: TM_EDEVICE, nothing left to read */
    fake_dispatch_mult(1);
    const char *flagged[] = {"ab", "!x", "cd"}, *failed[] = {"ab", "~x"};
    for (int k = 0; k < 2; k++) {
        const uint32_t *a, *b, *c;
        uint64_t cnt, b0, e0;
        pack(s, k ? 2 : 3, k ? failed : flagged);
        CHECK(tmn_publish_deliver(s, H, k ? 2 : 3, 2, 0, 0) == TM_EDEVICE);
        CHECK(tmn_groups(s, &a, &b, &cnt) == TM_EINVAL && cnt == 0 && tmn_picks(s, &a, &cnt) == TM_EINVAL);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0);
        CHECK(tmn_route_dest(s, 0, &b0, &e0) == TM_EINVAL);
    }
    const char *fine[] = {"abcdefgh", "+x"};
    pack(s, 2, fine);
    CHECK(tmn_publish_deliver(s, H, 2, 2, 1, 0) == TM_OK);
    verify(s, 2, fine, 2, 1, 0, 0, 0);
    tmn_give(&pool, s);

    /* 5b. the CPU twin of tests/test_gpu_nif_chain.py's "one set through every entry point" and "refusals":
       tmn_route, tmn_dispatch, tmn_publish, tmn_deliver, tmn_publish_deliver, tmn_match, tmn_first and back on
       ONE set; after each, every reader either reads that call's kind or refuses (TM_EINVAL, nothing handed
       out); a refused call leaves nothing to read, makes no library call, and the set works afterwards */
    s = tmn_take(&pool);
    CHECK(s);
    {
        const uint32_t *a, *b, *c;
        uint64_t cnt, b0, e0;
        const char *five[] = {"abcde", "+x", "", "xyz", "0123456789"};
        const uint64_t r0 = s->reruns;                                 /* (a pooled set: it has rerun above) */
#define REFUSES_PICKS (cnt = 7, a = five_marker, tmn_picks(s, &a, &cnt) == TM_EINVAL && cnt == 0 && a == 0)
#define REFUSES_GROUPS (cnt = 7, a = b = five_marker, tmn_groups(s, &a, &b, &cnt) == TM_EINVAL && cnt == 0 && a == 0 && b == 0)
#define REFUSES_DELIVERIES \
    (cnt = 7, a = b = c = five_marker, tmn_deliveries(s, &a, &b, &c, &cnt) == TM_EINVAL && cnt == 0 && !a && !b && !c)
        const uint32_t marker_word = 0, *const five_marker = &marker_word;
        pack(s, 5, five);
        CHECK(tmn_share_keys(s, H, 5, kc, kt) == TM_OK);
        CHECK(tmn_route(s, H, 5, 3) == TM_OK && tmn_route_dest(s, 3, &b0, &e0) == 0 && e0 == 5 + 3 + 10);
        CHECK(tmn_route_dest(s, 4, &b0, &e0) == TM_EINVAL && b0 == 0 && e0 == 0);
        CHECK(tmn_dispatch(s, H, 5, 3, 1, 0) == TM_OK && tmn_deliveries(s, &a, &b, &c, &cnt) == 0 && cnt > 0);
        CHECK(REFUSES_PICKS && REFUSES_GROUPS && tmn_direct(s) == 0);
        CHECK(tmn_publish(s, H, 5, 3, 1, 4) == TM_OK && tmn_picks(s, &a, &cnt) == 0 && cnt == s->picks && cnt > 0);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == 0 && REFUSES_GROUPS && tmn_direct(s) == 0);
        CHECK(tmn_deliver(s, H, 5, 3, 1, 0) == TM_OK && tmn_groups(s, &a, &b, &cnt) == 0 && cnt == s->groups && cnt > 0);
        CHECK(tmn_deliveries(s, &a, &b, &c, &cnt) == 0 && REFUSES_PICKS && tmn_direct(s) == 0);
        CHECK(tmn_publish_deliver(s, H, 5, 3, 1, 4) == TM_OK && s->reruns == r0);
        verify(s, 5, five, 3, 1, kc, kt, 4);
        CHECK(tmn_direct(s) > 0 && tmn_direct(s) < s->deliveries);
        /* the match half on the same buffers: unique rows end at the distinct count, not at the next offset */
        for (uint32_t order = TM_ORDER_TRAVERSAL; order <= TM_ORDER_UNIQUE; order++) {
            CHECK(tmn_match(s, H, 5, order) == TM_OK);
            for (uint32_t i = 0; i < 5; i++) {
                const uint64_t len = i == 1 ? 0 : strlen(five[i]), want = order == TM_ORDER_UNIQUE ? (len + 1) / 2 : len;
                CHECK(tmn_row(s, 5, order, i, &b0, &e0) == (i == 1 ? TMN_ERR_BADARG : 0) && e0 - b0 == want);
                for (uint64_t k = 0; k < want; k++) CHECK(tmn_vals(s)[b0 + k] == 1000 * i + k);
            }
        }
        /* tmn_first twice, the second batch with other lengths: the u64 offsets are copied for each */
        const char *other[] = {"", "q", "+y", "zz"};
        uint32_t v;
        CHECK(tmn_first(s, H, 5) == TM_OK && tmn_first_row(s, 0, &v) == 1 && tmn_first_row(s, 1, &v) == 2);
        CHECK(tmn_first_row(s, 2, &v) == 0 && tmn_first_row(s, 4, &v) == 1 && v == 4000);
        pack(s, 4, other);
        CHECK(tmn_first(s, H, 4) == TM_OK && tmn_first_row(s, 0, &v) == 0 && tmn_first_row(s, 1, &v) == 1 && v == 1000);
        CHECK(tmn_first_row(s, 2, &v) == 2 && tmn_first_row(s, 3, &v) == 1 && v == 3000);
        /* and back */
        pack(s, 5, five);
        CHECK(tmn_publish_deliver(s, H, 5, 3, 1, 4) == TM_OK);
        verify(s, 5, five, 3, 1, kc, kt, 4);
        /* refusals: no library call, nothing left to read, whichever of the three was asked */
        c0 = fake_pd_count(), m0 = fake_pd_moves();
        const long alloc0 = fake_count(0);
        for (int k = 0; k < 15; k++) {
            const uint32_t n = k % 5 == 3 ? 4 : k % 5 == 4 ? 6 : 5;                    /* the keys are for five */
            const uint32_t nd = k % 5 == 0 ? 0 : k % 5 == 1 ? 65537 : 3, ld = k % 5 == 2 ? 3 : 1;
            if (k / 5 == 1 && n != 5) continue;                                        /* (tmn_deliver has no keys) */
            CHECK(tmn_publish_deliver(s, H, 5, 3, 1, 4) == TM_OK);                     /* something to take away */
            const long before = fake_pd_count() + fake_publish_count() + fake_deliver_count() + fake_dispatch_count() + fake_route_count();
            const int rc = k / 5 == 0 ? tmn_publish(s, H, n, nd, ld, 4) : k / 5 == 1 ? tmn_deliver(s, H, n, nd, ld, 0)
                                                                                     : tmn_publish_deliver(s, H, n, nd, ld, 4);
            CHECK(rc == TM_EINVAL);
            CHECK(fake_pd_count() + fake_publish_count() + fake_deliver_count() + fake_dispatch_count() + fake_route_count() == before);
            CHECK(REFUSES_PICKS && REFUSES_GROUPS && REFUSES_DELIVERIES && tmn_direct(s) == 0);
            CHECK(tmn_route_dest(s, 0, &b0, &e0) == TM_EINVAL && b0 == 0 && e0 == 0);
        }
        CHECK(fake_count(0) == alloc0 && s->reruns == r0);
        CHECK(tmn_publish_deliver(s, H, 5, 3, 1, 4) == TM_OK);
        verify(s, 5, five, 3, 1, kc, kt, 4);
        CHECK(tmn_share_keys(s, H, 0, 0, 0) == TM_OK);
#undef REFUSES_PICKS
#undef REFUSES_GROUPS
#undef REFUSES_DELIVERIES
    }
    tmn_give(&pool, s);

    /* 6. every buffer goes with the pool: the members, the group head and the two group buffers too */
    const long f0 = fake_count(1);
    tmn_pool_destroy(&pool);
    CHECK(fake_count(0) == fake_count(1) && fake_count(0) > 20 && fake_count(1) - f0 >= 4 * 12);
    printf("ok\n");
    return 0;
}
