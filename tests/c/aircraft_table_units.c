/* aircraft_table_units.c -- the host twin of the aircraft table (msd_pos_host_create_table, _update_nicrc, _snapshot,
 * _expire with msd_trk_impl.h behind them) and msd_aircraft_to_float, driven by a stand-alone program so that a
 * sanitizer build can watch them (scripts/sanitize.sh builds it with -fsanitize=address,undefined).  Records with
 * pseudo-random field bytes -- every flag, type and raw value the feed function branches on -- of 60 aircraft on two
 * receivers go through a 64-slot table in calls of 1 to 300 records, with expiry in between, snapshots into buffers of
 * exactly the size needed, one entry too few and none, a call that overflows the table, and a reset.  Altitudes stay
 * within what a 13-bit altitude code can say; the reference's own arithmetic on them is int.  Checks as it goes: the
 * snapshot is in key order, `set` is `decoded`, a rolled-back call changes no byte, cutting changes no byte. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msd_pos_host.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

#define CHECK(c)                                                                                                        \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "aircraft_table_units: %s:%d: %s\n", __FILE__, __LINE__, #c);                             \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

static void make(size_t n, uint32_t first_addr, uint32_t aircraft, uint64_t *clock, msd_message *m, msd_fields *f, uint32_t *r)
{
    for (size_t i = 0; i < n; ++i) {
        unsigned char *b = (unsigned char *)&f[i];
        for (size_t k = 0; k < sizeof f[i]; ++k)
            b[k] = (unsigned char)rnd();
        memset(&m[i], 0, sizeof m[i]);
        const uint32_t a = rnd() % aircraft;
        *clock += rnd() % 4 == 0 ? rnd() % 20000 : rnd() % 50;
        m[i].sysTimestampMsg = rnd() % 50 == 0 ? *clock - rnd() % 3000 : *clock; /* now and then a step back */
        m[i].msgtype = (uint8_t)(rnd() % 40 == 0 ? 32 : (rnd() % 2 ? 17 : rnd() % 25));
        m[i].crc = rnd() % 2 ? 0 : rnd() & 0xFFFFFF;
        m[i].signalLevel = rnd() % 6 == 0 ? 0.0 : (double)(rnd() % 1000) / 1000.0;
        f[i].addr = rnd() % 60 == 0 ? 0 : first_addr + a * 977u + (a % 7 == 0 ? MSD_NON_ICAO_ADDRESS : 0);
        r[i] = a & 1u;
        f[i].source = (uint8_t)(rnd() % 8);
        f[i].altitude_baro = (int32_t)(rnd() % 127000) - 1000;
        f[i].altitude_geom = (int32_t)(rnd() % 127000) - 1000;
        f[i].altitude_baro_unit = (uint8_t)(rnd() % 3);
        f[i].altitude_geom_unit = (uint8_t)(rnd() % 3);
        f[i].nav_mcp_altitude = (int32_t)(rnd() % 65536);
        f[i].nav_fms_altitude = (int32_t)(rnd() % 65536);
        f[i].cpr_lat &= 0x1FFFF;
        f[i].cpr_lon &= 0x1FFFF;
        f[i].cpr_type &= 1;
        f[i].cpr_odd &= 1;
        f[i].metype &= 31;
        f[i].airground &= 3;
        f[i].heading_type = (uint8_t)(rnd() % 6);
        f[i].sil_type &= 3;
        /* most records carry a few members, not all of them */
        if (rnd() % 4) f[i].cpr_valid = 0;
        if (rnd() % 3) f[i].altitude_baro_valid = 0;
        if (rnd() % 3) f[i].opstatus &= ~1u;
        if (rnd() % 3) f[i].velocity_valid = 0;
    }
}

int main(void)
{
    enum { N = 20000, CAP = 64 };
    msd_pos_receiver rx[2] = {{52.0, 4.0, 300 * 1852.0, 1, 0}, {0, 0, 0, 0, 0}};
    msd_pos_config cfg = {0, 0, CAP, 2, rx};
    msd_pos_host *whole = NULL, *cut = NULL, *plain = NULL;
    CHECK(msd_pos_host_create_table(&cfg, &whole) == 0 && msd_pos_host_create_table(&cfg, &cut) == 0);
    CHECK(msd_pos_host_create(&cfg, &plain) == 0);
    msd_message *m = malloc(sizeof *m * N);
    msd_fields *f = malloc(sizeof *f * N);
    uint32_t *r = malloc(sizeof *r * N);
    msd_position *o1 = malloc(sizeof *o1 * N), *o2 = malloc(sizeof *o2 * N);
    msd_pos_nicrc *q1 = malloc(sizeof *q1 * N), *q2 = malloc(sizeof *q2 * N);
    CHECK(m && f && r && o1 && o2 && q1 && q2);
    uint64_t clock = 1600000000000ull;
    size_t n = 0, decoded = 0;
    msd_aircraft_float fl;

    CHECK(msd_pos_host_snapshot(plain, NULL, 0, &n) == -EINVAL && msd_pos_host_update_nicrc(plain, m, f, r, 1, o1, q1) == -EINVAL);
    CHECK(msd_pos_host_snapshot(whole, NULL, 0, &n) == 0 && n == 0);
    for (int round = 0; round < 6; ++round) {
        make(N, 0x400000, 60, &clock, m, f, r);
        CHECK(msd_pos_host_update_nicrc(whole, m, f, r, N, o1, q1) == 0);
        for (size_t base = 0; base < N;) { /* the same stream in calls of 1 to 300 records */
            size_t k = 1 + rnd() % 300;
            if (k > N - base)
                k = N - base;
            CHECK(msd_pos_host_update_nicrc(cut, m + base, f + base, r + base, k, o2 + base, q2 + base) == 0);
            base += k;
        }
        CHECK(memcmp(o1, o2, sizeof *o1 * N) == 0 && memcmp(q1, q2, sizeof *q1 * N) == 0);
        for (size_t i = 0; i < N; ++i) {
            CHECK(q1[i].set == o1[i].decoded);
            decoded += o1[i].decoded;
        }
        CHECK(msd_pos_host_update(plain, m, f, r, N, o2) == 0 && memcmp(o1, o2, sizeof *o1 * N) == 0);

        CHECK(msd_pos_host_snapshot(whole, NULL, 0, &n) == -ENOSPC && n > 0 && n <= 60);
        msd_aircraft *s1 = malloc(sizeof *s1 * n), *s2 = malloc(sizeof *s2 * n), *s3 = malloc(sizeof *s3 * (n - 1) + 1);
        size_t n2 = 0;
        CHECK(s1 && s2 && s3);
        CHECK(msd_pos_host_snapshot(whole, s3, n - 1, &n2) == -ENOSPC && n2 == n);
        CHECK(msd_pos_host_snapshot(whole, s1, n, &n2) == 0 && n2 == n && msd_pos_host_snapshot(cut, s2, n, &n2) == 0 && n2 == n);
        CHECK(memcmp(s1, s2, sizeof *s1 * n) == 0);
        for (size_t i = 0; i < n; ++i) {
            if (i)
                CHECK(s1[i - 1].receiver < s1[i].receiver || (s1[i - 1].receiver == s1[i].receiver && s1[i - 1].addr < s1[i].addr));
            msd_aircraft_to_float(&s1[i], &fl);
            for (int k = 0; k < MSD_AC_N; ++k)
                (void)msd_aircraft_valid(&s1[i], k, clock);
        }
        /* a call that brings ten aircraft too many is rolled back: no byte of the snapshot changes */
        uint64_t c2 = clock;
        make(500, 0x700000, 14, &c2, m, f, r);
        for (size_t i = 0; i < 500; i += 2)
            f[i].addr = 0x400000 + (uint32_t)(rnd() % 60) * 977u; /* known aircraft in between */
        CHECK(msd_pos_host_update_nicrc(whole, m, f, r, 500, o2, q2) == -ENOSPC);
        CHECK(msd_pos_host_snapshot(whole, s2, n, &n2) == 0 && n2 == n && memcmp(s1, s2, sizeof *s1 * n) == 0);
        free(s1), free(s2), free(s3);
        clock += round % 2 ? 61000 : 700;
        CHECK(msd_pos_host_expire(whole, clock) == 0 && msd_pos_host_expire(cut, clock) == 0 && msd_pos_host_expire(plain, clock) == 0);
    }
    CHECK(decoded > 100);
    CHECK(msd_pos_host_reset(whole) == 0 && msd_pos_host_snapshot(whole, NULL, 0, &n) == 0 && n == 0);
    msd_pos_host_destroy(whole), msd_pos_host_destroy(cut), msd_pos_host_destroy(plain);
    free(m), free(f), free(r), free(o1), free(o2), free(q1), free(q2);
    printf("aircraft_table_units: ok (%zu positions decoded)\n", decoded);
    return 0;
}
