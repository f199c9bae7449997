/* modeac_units.c -- the host twin of the Mode A/C matching (msd_pos_host_modeac_enable, _match, _codes, _hits and the
 * counting and hit resets inside msd_pos_host_update, with msd_modeac_impl.h behind them) and msd_mode_c_to_a, driven by
 * a stand-alone program so that a sanitizer build can watch them (scripts/sanitize.sh builds it with
 * -fsanitize=address,undefined).  Mode S records of 60 aircraft on three receivers -- squawks from a handful of codes,
 * altitudes from -1300 ft up, field bytes otherwise pseudo-random -- and Mode A/C replies on those codes, on the codes
 * of those altitudes and on any of the 4096, go through a 64-slot table in calls of 1 to 300 records with expiry and a
 * match once per second of the stream's clock, now and then with a clock that steps back.  Checks as it goes: cutting
 * changes no byte, row j of the hits is row j of the snapshot, the counts add up to the replies fed less the cleared ones,
 * a rolled-back call counts nothing, reset leaves the tracker enabled, an enabled tracker's rows are a plain one's. */
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
            fprintf(stderr, "modeac_units: %s:%d: %s\n", __FILE__, __LINE__, #c);                                     \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

enum { NRX = 3, CAP = 64, N = 4000 };
static const uint16_t squawks[6] = {0x1200, 0x7000, 0x2345, 0x7700, 0x0000, 0x7777};

static int altitude_of(uint32_t a)
{
    return -1300 + 100 * (int)(a % 40) + (a % 3 == 0 ? 50 : 0);
}

static size_t make(size_t n, uint64_t *clock, msd_message *m, msd_fields *f, uint32_t *r)
{
    size_t replies = 0;
    for (size_t i = 0; i < n; ++i) {
        unsigned char *b = (unsigned char *)&f[i];
        for (size_t k = 0; k < sizeof f[i]; ++k)
            b[k] = (unsigned char)rnd();
        memset(&m[i], 0, sizeof m[i]);
        const uint32_t a = rnd() % 60;
        *clock += rnd() % 40;
        m[i].sysTimestampMsg = rnd() % 50 == 0 ? *clock - rnd() % 3000 : *clock;
        m[i].crc = rnd() % 2 ? 0 : rnd() & 0xFFFFFF;
        r[i] = a % NRX;
        f[i].source = (uint8_t)(rnd() % 8);
        f[i].altitude_baro = altitude_of(a) + (rnd() % 8 == 0 ? (int32_t)(rnd() % 400) - 200 : 0);
        f[i].altitude_geom = (int32_t)(rnd() % 127000) - 1000;
        f[i].altitude_baro_unit = 0;
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
        f[i].squawk = squawks[(a + (rnd() % 16 == 0)) % 6];
        if (rnd() % 4) f[i].cpr_valid = 0;
        if (rnd() % 3) f[i].altitude_baro_valid = 0;
        if (rnd() % 3) f[i].squawk_valid = 0;
        if (rnd() % 3) f[i].opstatus &= ~1u;
        if (rnd() % 3) f[i].velocity_valid = 0;
        if (rnd() % 3 == 0) { /* a Mode A/C reply */
            m[i].msgtype = 32;
            ++replies;
            const uint32_t kind = rnd() % 4;
            unsigned code = kind == 0   ? squawks[rnd() % 6]
                            : kind == 1 ? msd_mode_c_to_a((altitude_of(rnd() % 60) + 49) / 100 + (int)(rnd() % 3) - 1)
                            : kind == 2 ? (rnd() & 0x7777u)
                                        : squawks[a % 6];
            if (rnd() % 10 == 0)
                code |= 0x0080u; /* SPI */
            f[i].squawk = (uint16_t)code;
            f[i].addr = (code & 0xFF7Fu) | MSD_NON_ICAO_ADDRESS;
        } else {
            m[i].msgtype = (uint8_t)(rnd() % 2 ? 17 : rnd() % 25);
            f[i].addr = rnd() % 60 == 0 ? 0 : 0x400000 + a * 977u + (a % 7 == 0 ? MSD_NON_ICAO_ADDRESS : 0);
        }
    }
    return replies;
}

static uint64_t total(msd_pos_host *p, msd_modeac_code *codes)
{
    uint64_t sum = 0;
    for (uint32_t rx = 0; rx < NRX; ++rx) {
        CHECK(msd_pos_host_modeac_codes(p, rx, codes) == 0);
        for (int i = 0; i < 4096; ++i)
            sum += codes[i].count;
    }
    return sum;
}

int main(void)
{
    msd_pos_config cfg = {0, 0, CAP, NRX, NULL};
    msd_pos_host *whole = NULL, *cut = NULL, *plain = NULL, *bare = NULL;
    CHECK(msd_pos_host_create_table(&cfg, &whole) == 0 && msd_pos_host_create_table(&cfg, &cut) == 0);
    CHECK(msd_pos_host_create_table(&cfg, &plain) == 0 && msd_pos_host_create(&cfg, &bare) == 0);
    msd_message *m = malloc(sizeof *m * N);
    msd_fields *f = malloc(sizeof *f * N);
    uint32_t *r = malloc(sizeof *r * N);
    msd_position *o1 = malloc(sizeof *o1 * N), *o2 = malloc(sizeof *o2 * N);
    msd_pos_nicrc *q1 = malloc(sizeof *q1 * N), *q2 = malloc(sizeof *q2 * N);
    msd_modeac_code *c1 = malloc(sizeof *c1 * 4096), *c2 = malloc(sizeof *c2 * 4096);
    CHECK(m && f && r && o1 && o2 && q1 && q2 && c1 && c2);
    size_t n = 0;

    /* the Gillham table: 1280 altitudes from -1200 ft, each with one code; nothing outside */
    unsigned valid = 0;
    for (int c = -20; c < 4100; ++c)
        valid += msd_mode_c_to_a(c) != 0;
    CHECK(valid == 1280 && msd_mode_c_to_a(-13) == 0 && msd_mode_c_to_a(-12) != 0 && msd_mode_c_to_a(1267) != 0 && msd_mode_c_to_a(1268) == 0);
    CHECK(msd_mode_c_to_a(-2147483647 - 1) == 0 && msd_mode_c_to_a(2147483647) == 0);

    /* refused where they do not apply */
    CHECK(msd_pos_host_modeac_enable(NULL) == -EINVAL && msd_pos_host_modeac_enable(bare) == -EINVAL);
    CHECK(msd_pos_host_modeac_match(whole, 0, 0) == -EINVAL && msd_pos_host_modeac_codes(whole, 0, c1) == -EINVAL);
    CHECK(msd_pos_host_modeac_hits(whole, NULL, 0, &n) == -EINVAL);
    CHECK(msd_pos_host_modeac_enable(whole) == 0 && msd_pos_host_modeac_enable(whole) == 0 && msd_pos_host_modeac_enable(cut) == 0);
    CHECK(msd_pos_host_modeac_codes(whole, NRX, c1) == -EINVAL && msd_pos_host_modeac_codes(whole, 0, NULL) == -EINVAL);
    CHECK(msd_pos_host_modeac_hits(whole, NULL, 0, &n) == 0 && n == 0 && msd_pos_host_modeac_hits(whole, NULL, 0, NULL) == -EINVAL);

    uint64_t clock = 1600000000000ull, fed = 0, hits_seen = 0, ambiguous = 0, cleared_seen = 0;
    for (int round = 0; round < 40; ++round) {
        const size_t replies = make(N, &clock, m, f, r);
        const uint64_t before = total(whole, c1);
        CHECK(msd_pos_host_update_nicrc(whole, m, f, r, N, o1, q1) == 0);
        for (size_t base = 0; base < N;) {
            size_t k = 1 + rnd() % 300;
            if (k > N - base)
                k = N - base;
            CHECK(msd_pos_host_update_nicrc(cut, m + base, f + base, r + base, k, o2 + base, q2 + base) == 0);
            base += k;
        }
        CHECK(memcmp(o1, o2, sizeof *o1 * N) == 0 && memcmp(q1, q2, sizeof *q1 * N) == 0);
        CHECK(msd_pos_host_update_nicrc(plain, m, f, r, N, o2, q2) == 0);
        CHECK(memcmp(o1, o2, sizeof *o1 * N) == 0 && memcmp(q1, q2, sizeof *q1 * N) == 0);
        CHECK(total(whole, c1) == before + replies);
        fed += replies;

        /* a call that brings aircraft too many is rolled back and counts nothing */
        uint64_t c3 = clock;
        (void)make(300, &c3, m, f, r);
        for (size_t i = 0; i < 300; ++i)
            if (m[i].msgtype != 32)
                f[i].addr = 0x700000 + (uint32_t)i;
        CHECK(msd_pos_host_update_nicrc(whole, m, f, r, 300, o2, q2) == -ENOSPC);
        CHECK(total(whole, c1) == before + replies);

        const uint64_t now = round % 7 == 3 ? clock - 9000 : clock, message_now = round % 5 == 4 ? clock + 80000 : clock;
        CHECK(msd_pos_host_expire(whole, clock) == 0 && msd_pos_host_expire(cut, clock) == 0 && msd_pos_host_expire(plain, clock) == 0);
        CHECK(msd_pos_host_modeac_match(whole, now, message_now) == 0 && msd_pos_host_modeac_match(cut, now, message_now) == 0);
        for (uint32_t rx = 0; rx < NRX; ++rx) {
            CHECK(msd_pos_host_modeac_codes(whole, rx, c1) == 0 && msd_pos_host_modeac_codes(cut, rx, c2) == 0);
            CHECK(memcmp(c1, c2, sizeof *c1 * 4096) == 0);
            for (int i = 0; i < 4096; ++i) {
                CHECK(c1[i].lastcount == c1[i].count && c1[i].age <= 15 && (c1[i].count || !c1[i].match || c1[i].age == 0));
                ambiguous += c1[i].match == 0xFFFFFFFFu;
            }
        }
        cleared_seen += before + replies - total(whole, c1);

        CHECK(msd_pos_host_modeac_hits(whole, NULL, 0, &n) == -ENOSPC && n > 0 && n <= 60);
        msd_aircraft *s1 = malloc(sizeof *s1 * n), *s2 = malloc(sizeof *s2 * n);
        msd_modeac_hit *h1 = malloc(sizeof *h1 * n), *h2 = malloc(sizeof *h2 * n), *h3 = malloc(sizeof *h3 * (n - 1) + 1);
        size_t n2 = 0;
        CHECK(s1 && s2 && h1 && h2 && h3);
        CHECK(msd_pos_host_modeac_hits(whole, h3, n - 1, &n2) == -ENOSPC && n2 == n);
        CHECK(msd_pos_host_modeac_hits(whole, h1, n, &n2) == 0 && n2 == n && msd_pos_host_modeac_hits(cut, h2, n, &n2) == 0 && n2 == n);
        CHECK(memcmp(h1, h2, sizeof *h1 * n) == 0);
        CHECK(msd_pos_host_snapshot(whole, s1, n, &n2) == 0 && n2 == n && msd_pos_host_snapshot(plain, s2, n, &n2) == 0 && n2 == n);
        CHECK(memcmp(s1, s2, sizeof *s1 * n) == 0); /* the table entries do not know about the matching */
        for (size_t i = 0; i < n; ++i) {
            CHECK(h1[i].receiver == s1[i].receiver && h1[i].addr == s1[i].addr && h1[i].mode_a_hit <= 1 && h1[i].mode_c_hit <= 1);
            for (int k = 0; k < 6; ++k)
                CHECK(h1[i].pad[k] == 0);
            hits_seen += h1[i].mode_a_hit + h1[i].mode_c_hit;
        }
        free(s1), free(s2), free(h1), free(h2), free(h3);
        clock += round % 9 == 8 ? 61000 : 300;
    }
    CHECK(fed > 40000 && hits_seen > 100 && ambiguous > 10 && cleared_seen > 0);
    CHECK(msd_pos_host_reset(whole) == 0 && total(whole, c1) == 0 && msd_pos_host_modeac_hits(whole, NULL, 0, &n) == 0 && n == 0);
    const size_t replies = make(100, &clock, m, f, r);
    CHECK(msd_pos_host_update(whole, m, f, r, 100, o1) == 0 && total(whole, c1) == replies);
    msd_pos_host_destroy(whole), msd_pos_host_destroy(cut), msd_pos_host_destroy(plain), msd_pos_host_destroy(bare);
    free(m), free(f), free(r), free(o1), free(o2), free(q1), free(q2), free(c1), free(c2);
    printf("modeac_units: ok (%llu replies, %llu hits seen, %llu ambiguous codes, %llu replies cleared)\n", (unsigned long long)fed,
           (unsigned long long)hits_seen, (unsigned long long)ambiguous, (unsigned long long)cleared_seen);
    return 0;
}
