/* reduce_units.c -- the host twin of the reduced Beast output (msd_pos_host_reduce_enable, _update_reduce, _reduce_wire,
 * _reduce_timers, with msd_trk_impl.h's msd_trk_reduce behind them), driven by a stand-alone program so that a sanitizer
 * build can watch it (scripts/sanitize.sh builds it with -fsanitize=address,undefined).  Mode S records of 60 aircraft on
 * three receivers -- field bytes pseudo-random, so every member of the table is accepted and refused now and then --,
 * Mode A/C replies and address 0 in between, go through a 64-slot table at the intervals 0, 125, 8000 and 15000 in calls
 * of 1 to 300 records with an expiry once per second of the stream's clock, now and then with a clock that steps back.
 * Checks as it goes: cutting changes no verdict and no timer; whichever update call feeds a record, the timers are the
 * same; the stream is msd_beast_frame_out on the records the delivery conditions let through, for every flag; a short
 * buffer gets the size and no byte; a rolled-back call moves no timer and writes no verdict; reset forgets the timers and
 * leaves the tracker enabled; an enabled tracker's rows are a plain one's. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msd_pos_host.h"
#include "msd_wire.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

#define CHECK(c)                                                                                                        \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "reduce_units: %s:%d: %s\n", __FILE__, __LINE__, #c);                                     \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

enum { NRX = 3, CAP = 64, N = 4000, TIMERS = MSD_AC_N + 1 };

static void make(size_t n, uint64_t *clock, msd_message *m, msd_fields *f, uint32_t *r)
{
    static const uint8_t df[8] = {17, 17, 17, 18, 4, 5, 11, 20};
    for (size_t i = 0; i < n; ++i) {
        unsigned char *b = (unsigned char *)&f[i];
        for (size_t k = 0; k < sizeof f[i]; ++k)
            b[k] = (unsigned char)rnd();
        b = (unsigned char *)&m[i];
        for (size_t k = 0; k < sizeof m[i]; ++k)
            b[k] = (unsigned char)rnd();
        const uint32_t a = rnd() % 60;
        *clock += rnd() % 40;
        m[i].sysTimestampMsg = rnd() % 50 == 0 ? *clock - rnd() % 3000 : *clock;
        m[i].timestampMsg &= 0xFFFFFFFFFFFFull;
        m[i].signalLevel = (double)(rnd() % 1000) / 999.0;
        m[i].crc = rnd() % 2 ? 0 : rnd() & 0xFFFFFF;
        m[i].msgtype = df[rnd() % 8];
        m[i].msgbits = m[i].msgtype == 4 || m[i].msgtype == 5 || m[i].msgtype == 11 ? 56 : 112;
        m[i].correctedbits = (uint8_t)(rnd() % 8 == 0 ? 1 + rnd() % 2 : 0);
        m[i].iid = (uint8_t)(rnd() % 3 == 0 ? rnd() % 128 : 0);
        if (rnd() % 9 == 0)
            memset(m[i].msg, 0x1A, sizeof m[i].msg);
        r[i] = a % NRX;
        f[i].addr = 0x400000 + 977 * a;
        f[i].source = (uint8_t)(rnd() % 8);
        f[i].altitude_baro = 1000 + 100 * (int32_t)(a % 40) + (rnd() % 8 == 0 ? (int32_t)(rnd() % 4000) - 2000 : 0);
        f[i].altitude_geom = (int32_t)(rnd() % 127000) - 1000;
        f[i].altitude_baro_unit = 0;
        f[i].altitude_geom_unit = (uint8_t)(rnd() % 3);
        f[i].cpr_lat &= 0x1FFFF;
        f[i].cpr_lon &= 0x1FFFF;
        f[i].cpr_type &= 1;
        f[i].cpr_odd &= 1;
        f[i].metype &= 31;
        f[i].airground &= 3;
        f[i].heading_type = (uint8_t)(rnd() % 6);
        f[i].sil_type &= 3;
        if (rnd() % 4) f[i].cpr_valid = 0;
        if (rnd() % 3) f[i].altitude_baro_valid = 0;
        if (rnd() % 3) f[i].squawk_valid = 0;
        if (rnd() % 3) f[i].opstatus &= ~1u;
        if (rnd() % 3) f[i].velocity_valid = 0;
        if (rnd() % 2) f[i].geom_delta_valid = 0;
        if (rnd() % 2) f[i].altitude_geom_valid = 0;
        if (rnd() % 20 == 0) { /* a Mode A/C reply, or a junk address: neither reaches the tracker */
            if (rnd() % 2) {
                m[i].msgtype = 32;
                m[i].msgbits = 16;
            } else {
                f[i].addr = 0;
            }
        }
    }
}

static msd_pos_host *tracker(int table, int interval)
{
    msd_pos_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.capacity = CAP;
    cfg.receivers = NRX;
    msd_pos_host *p = NULL;
    CHECK((table ? msd_pos_host_create_table(&cfg, &p) : msd_pos_host_create(&cfg, &p)) == 0);
    if (interval >= 0)
        CHECK(msd_pos_host_reduce_enable(p, (uint32_t)interval) == 0);
    return p;
}

/* the stream through p in calls of 1 .. 300 records (cut = 0: of 300), an expiry whenever the clock passes a second;
 * mode 0: update_reduce always; 1: the three update calls in turn, verdicts only where the call delivers them; 2: the two
 * calls a tracker that does not reduce has */
static void run(msd_pos_host *p, const msd_message *m, const msd_fields *f, const uint32_t *r, msd_position *out, uint8_t *fwd,
                int cut, int mode)
{
    uint64_t next_expire = m[0].sysTimestampMsg + 1000;
    size_t at = 0, calls = 0;
    msd_pos_nicrc *q = malloc(sizeof *q * 300);
    CHECK(q);
    memset(fwd, 0xEE, N);
    while (at < N) {
        size_t k = cut ? 1 + rnd() % 300 : 300;
        if (k > N - at)
            k = N - at;
        if (m[at].sysTimestampMsg >= next_expire) {
            CHECK(msd_pos_host_expire(p, next_expire) == 0);
            while (m[at].sysTimestampMsg >= next_expire)
                next_expire += 1000;
        }
        for (size_t i = 1; i < k; ++i) /* a call ends in front of the record that passes the second */
            if (m[at + i].sysTimestampMsg >= next_expire) {
                k = i;
                break;
            }
        const int which = mode == 0 ? 2 : (int)(calls++ % (mode == 1 ? 3 : 2));
        if (which == 0)
            CHECK(msd_pos_host_update(p, m + at, f + at, r + at, k, out + at) == 0);
        else if (which == 1)
            CHECK(msd_pos_host_update_nicrc(p, m + at, f + at, r + at, k, out + at, q) == 0);
        else
            CHECK(msd_pos_host_update_reduce(p, m + at, f + at, r + at, k, out + at, calls % 2 ? q : NULL, fwd + at) == 0);
        at += k;
    }
    free(q);
}

static void same_timers(const msd_pos_host *a, const msd_pos_host *b)
{
    uint64_t ta[TIMERS], tb[TIMERS];
    for (uint32_t k = 0; k < 60; ++k) {
        const int ra = msd_pos_host_reduce_timers(a, k % NRX, 0x400000 + 977 * k, ta);
        const int rb = msd_pos_host_reduce_timers(b, k % NRX, 0x400000 + 977 * k, tb);
        CHECK(ra == rb && (ra == 0 || ra == -ENOENT));
        if (ra == 0)
            CHECK(memcmp(ta, tb, sizeof ta) == 0);
    }
}

int main(void)
{
    msd_message *m = malloc(sizeof *m * N);
    msd_fields *f = malloc(sizeof *f * N);
    uint32_t *r = malloc(sizeof *r * N);
    msd_position *o1 = malloc(sizeof *o1 * N), *o2 = malloc(sizeof *o2 * N);
    uint8_t *v1 = malloc(N), *v2 = malloc(N);
    uint8_t *bytes = malloc((size_t)N * MSD_BEAST_MAX), *want = malloc((size_t)N * MSD_BEAST_MAX);
    uint32_t *ends = malloc(sizeof *ends * N);
    CHECK(m && f && r && o1 && o2 && v1 && v2 && bytes && want && ends);
    static const int intervals[4] = {0, 125, 8000, 15000};
    uint64_t forwarded = 0, delivered = 0;
    for (int round = 0; round < 4; ++round) {
        uint64_t clock = 1600000000000ull + 100000ull * (uint64_t)round;
        make(N, &clock, m, f, r);
        const int I = intervals[round];
        msd_pos_host *whole = tracker(1, I), *cut = tracker(1, I), *mixed = tracker(1, I), *plain = tracker(1, -1);
        run(whole, m, f, r, o1, v1, 0, 0);
        run(cut, m, f, r, o2, v2, 1, 0);
        CHECK(memcmp(v1, v2, N) == 0 && memcmp(o1, o2, sizeof *o1 * N) == 0);
        same_timers(whole, cut);
        run(mixed, m, f, r, o2, v2, 1, 1);
        for (size_t i = 0; i < N; ++i)
            CHECK(v2[i] == 0xEE || v2[i] == v1[i]);
        same_timers(whole, mixed);
        run(plain, m, f, r, o2, v2, 1, 2);
        for (size_t i = 0; i < N; ++i) {
            CHECK((v1[i] & ~3u) == 0);
            if (m[i].msgtype == 32 || f[i].addr == 0)
                CHECK(v1[i] == 0);
            forwarded += v1[i] & MSD_REDUCE_FORWARD;
        }
        /* the stream, for every flag: msd_beast_frame_out on the records that are let through */
        for (uint32_t flags = 0; flags < 4; ++flags) {
            const int verbatim = (flags & MSD_WIRE_VERBATIM) != 0;
            size_t len = 0, need = 0;
            for (size_t i = 0; i < N; ++i)
                if ((v1[i] & MSD_REDUCE_FORWARD) && (flags || (v1[i] & MSD_REDUCE_SEEN_TWICE)))
                    len += msd_beast_frame_out(&m[i], verbatim, want + len);
            memset(bytes, 0xAA, (size_t)N * MSD_BEAST_MAX);
            if (len) {
                CHECK(msd_pos_host_reduce_wire(whole, m, v1, N, flags, bytes, len - 1, &need, ends) == -ENOSPC);
                CHECK(need == len && bytes[0] == 0xAA && bytes[len - 1] == 0xAA);
            }
            CHECK(msd_pos_host_reduce_wire(whole, m, v1, N, flags, bytes, len, &need, ends) == 0);
            CHECK(need == len && memcmp(bytes, want, len) == 0 && bytes[len] == 0xAA && ends[N - 1] == len);
            CHECK(msd_pos_host_reduce_wire(whole, m, v1, N, flags, bytes, len, &need, NULL) == 0);
            delivered += len;
        }
        size_t need = 7;
        CHECK(msd_pos_host_reduce_wire(whole, NULL, NULL, 0, 0, NULL, 0, &need, NULL) == 0 && need == 0);
        CHECK(msd_pos_host_reduce_wire(whole, m, v1, N, 4, bytes, 1, &need, NULL) == -EINVAL);
        CHECK(msd_pos_host_reduce_wire(whole, m, NULL, N, 0, bytes, 1, &need, NULL) == -EINVAL);
        CHECK(msd_pos_host_reduce_wire(whole, m, v1, N, 0, bytes, 1, NULL, NULL) == -EINVAL);
        CHECK(msd_pos_host_reduce_wire(plain, m, v1, N, 0, bytes, 1, &need, NULL) == -EINVAL);
        CHECK(msd_pos_host_update_reduce(plain, m, f, r, 10, o2, NULL, v2) == -EINVAL);
        CHECK(memcmp(o1, o2, sizeof *o1 * N) == 0); /* an enabled tracker's rows are a plain one's */
        /* a call that does not fit is rolled back: no timer moves, no verdict is written */
        msd_fields *g = malloc(sizeof *g * 200);
        CHECK(g);
        memcpy(g, f, sizeof *g * 200);
        for (size_t i = 0; i < 200; ++i)
            if (g[i].addr)
                g[i].addr = 0x700000 + (uint32_t)i;
        msd_pos_host *twin = tracker(1, I);
        run(twin, m, f, r, o2, v2, 0, 0);
        memset(v2, 0xEE, 200);
        CHECK(msd_pos_host_update_reduce(whole, m, g, r, 200, o2, NULL, v2) == -ENOSPC);
        for (size_t i = 0; i < 200; ++i)
            CHECK(v2[i] == 0xEE);
        same_timers(whole, twin);
        CHECK(msd_pos_host_reduce_enable(whole, (uint32_t)I) == 0 && msd_pos_host_reduce_enable(whole, (uint32_t)I + 1) == -EINVAL);
        CHECK(msd_pos_host_reset(whole) == 0);
        uint64_t t[TIMERS];
        CHECK(msd_pos_host_reduce_timers(whole, 0, 0x400000, t) == -ENOENT);
        run(whole, m, f, r, o2, v2, 1, 0);
        CHECK(memcmp(v1, v2, N) == 0);
        free(g);
        msd_pos_host_destroy(twin);
        msd_pos_host_destroy(whole);
        msd_pos_host_destroy(cut);
        msd_pos_host_destroy(mixed);
        msd_pos_host_destroy(plain);
    }
    msd_pos_host *no_table = tracker(0, -1);
    CHECK(msd_pos_host_reduce_enable(no_table, 125) == -EINVAL);
    msd_pos_host_destroy(no_table);
    msd_pos_host *t = tracker(1, -1);
    CHECK(msd_pos_host_reduce_enable(t, 15001) == -EINVAL && msd_pos_host_reduce_enable(NULL, 1) == -EINVAL);
    msd_pos_host_destroy(t);
    CHECK(forwarded > 1000 && forwarded < 4u * N && delivered > 0);
    printf("reduce_units: ok, %llu of %d records forwarded, %llu bytes over the four flag sets\n",
           (unsigned long long)forwarded, 4 * N, (unsigned long long)delivered);
    free(m), free(f), free(r), free(o1), free(o2), free(v1), free(v2), free(bytes), free(want), free(ends);
    return 0;
}
