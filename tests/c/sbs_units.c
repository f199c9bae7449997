/* sbs_units.c -- the arithmetic of the SBS writer (msd_sbs_impl.h: what the device runs, without printf) held against
 * glibc on the CPU, by a stand-alone program so that a sanitizer build can watch it (scripts/sanitize.sh and
 * tests/test_sbs_units.py build it with -fsanitize=address,undefined).
 *   %1.5f   msd_sbs_put_f5 against snprintf on 10.5 million doubles of four kinds: random in +-180, the exact ties -- odd
 *           multiples of 1/64, the only (k + 0.5) 1e-5 a double holds --, dyadic values, magnitudes down to 2^-200
 *   %.0f    msd_sbs_round0 against snprintf on every float k / 8 in [0, 8192)
 *   dates   msd_sbs_civil against gmtime_r on every day from 1970 to 9999 and on random milliseconds up to 2^63
 *   track   msd_sbs_build_track_table against the literal expression of mode_s.c:835-839 printed by snprintf, for all
 *           4 x 1023^2 arguments and for the same arguments times 4 (ES type 19 subtype 2)
 *   lines   msd_sbs_line against the host twin's writer (msd_pos_host_sbs_wire: snprintf, gmtime_r, atan2) on records with
 *           pseudo-random bytes in every member, under every flag combination; no line is longer than MSD_SBS_MAX */
#define _DEFAULT_SOURCE /* gmtime_r, M_PI */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "msd_pos_host.h"
#include "msd_sbs_impl.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint32_t rnd(void)
{
    return (uint32_t)(rnd64() >> 32);
}

#define CHECK(c)                                                                                                        \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "sbs_units: %s:%d: %s\n", __FILE__, __LINE__, #c);                                        \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

static void f5_one(double x)
{
    char want[64];
    uint8_t got[64];
    msd_sbs_w w = {got, 0}, count = {NULL, 0};
    const int n = snprintf(want, sizeof want, "%1.5f", x);
    msd_sbs_put_f5(&w, x);
    msd_sbs_put_f5(&count, x);
    if (w.n != (uint32_t)n || count.n != w.n || memcmp(want, got, w.n) != 0) {
        fprintf(stderr, "sbs_units: %%1.5f of %a: printf %s, here %.*s\n", x, want, (int)w.n, (const char *)got);
        exit(1);
    }
}

static size_t f5_all(void)
{
    size_t n = 0;
    for (int i = 0; i < 6000000; ++i, ++n) /* random in +-180 */
        f5_one(((double)(int64_t)rnd64() / 9223372036854775808.0) * 180.0);
    for (int j = 1; j < 180 * 64; j += 2, n += 2) { /* every exact tie */
        f5_one(j / 64.0);
        f5_one(-j / 64.0);
    }
    for (int i = 0; i < 2000000; ++i, ++n) { /* dyadic: k / 2^b, and the doubles next to it */
        const unsigned b = rnd() % 40;
        const double x = (double)(rnd64() % ((uint64_t)180 << b)) / (double)((uint64_t)1 << b);
        f5_one(rnd() & 1 ? -x : x);
        if (i % 4 == 0) {
            f5_one(nextafter(x, 400.0));
            f5_one(nextafter(x, -400.0));
            n += 2;
        }
    }
    for (int i = 0; i < 1500000; ++i, ++n) { /* small magnitudes, subnormals' neighbourhood of 1e-5 included */
        const double x = ldexp(1.0 + (double)(rnd64() >> 12) / 4503599627370496.0, -(int)(rnd() % 201));
        f5_one(rnd() & 1 ? -x : x);
    }
    f5_one(0.0), f5_one(-0.0), f5_one(-0.000004), f5_one(0.000005), f5_one(90.0), f5_one(-90.0), f5_one(-180.0), f5_one(360.0);
    f5_one(5e-324), f5_one(-5e-324), f5_one(2.2250738585072014e-308);
    return n;
}

static void f0_all(void)
{
    for (unsigned k = 0; k < 8192u * 8u; ++k) {
        const float x = (float)k / 8.0f;
        char want[32];
        uint8_t got[32];
        msd_sbs_w w = {got, 0};
        const int n = snprintf(want, sizeof want, "%.0f", x);
        msd_sbs_put_uint(&w, msd_sbs_round0(x), 0);
        CHECK(w.n == (uint32_t)n && memcmp(want, got, w.n) == 0);
    }
    /* the halves modes_hip.h names: 22.5 -> 22, 67.5 -> 68, 15.5 and 16.5 -> 16, 359.7 -> 360 */
    CHECK(msd_sbs_round0(22.5f) == 22 && msd_sbs_round0(67.5f) == 68 && msd_sbs_round0(15.5f) == 16 && msd_sbs_round0(16.5f) == 16);
    CHECK(msd_sbs_round0(359.7f) == 360);
}

static void civil_one(uint64_t t)
{
    const time_t sec = (time_t)(t / 1000u);
    struct tm tm;
    msd_sbs_time c;
    CHECK(gmtime_r(&sec, &tm) != NULL);
    msd_sbs_civil(t, &c);
    CHECK(c.year == (uint64_t)((long long)tm.tm_year + 1900) && c.month == (unsigned)tm.tm_mon + 1 && c.day == (unsigned)tm.tm_mday);
    CHECK(c.hour == (unsigned)tm.tm_hour && c.min == (unsigned)tm.tm_min && c.sec == (unsigned)tm.tm_sec && c.ms == t % 1000u);
}

static void civil_all(void)
{
    const uint64_t days = (uint64_t)MSD_SBS_YEAR_10000_MS / 86400000u; /* 1970-01-01 .. 9999-12-31 */
    for (uint64_t d = 0; d < days; ++d) {
        civil_one(d * 86400000u);
        civil_one(d * 86400000u + 86399999u);
    }
    civil_one((uint64_t)MSD_SBS_YEAR_10000_MS); /* 10000-01-01 */
    for (int i = 0; i < 2000000; ++i) {
        civil_one(rnd64() % (uint64_t)MSD_SBS_YEAR_10000_MS);
        civil_one(rnd64() >> 1); /* years up to 292 million: the line prints them modulo 10000 */
    }
}

static unsigned printed_track(int ew, int ns)
{
    float ground_track = (float)(atan2(ew, ns) * 180.0 / M_PI);
    if (ground_track < 0)
        ground_track += 360;
    char s[32];
    snprintf(s, sizeof s, "%.0f", ground_track);
    return (unsigned)strtoul(s, NULL, 10);
}

static void track_all(uint16_t *table)
{
    msd_sbs_build_track_table(table);
    for (int sign = 0; sign < 4; ++sign)
        for (int a = 0; a < 1023; ++a)
            for (int b = 0; b < 1023; ++b) {
                const int ew = (sign & 2) ? -a : a, ns = (sign & 1) ? -b : b;
                const int32_t k = msd_sbs_track_index(ew, ns, 1);
                CHECK(k >= 0 && (uint32_t)k < MSD_SBS_TRACK_ENTRIES && k == msd_sbs_track_index(4 * ew, 4 * ns, 2));
                CHECK(table[k] <= 360);
                CHECK(table[k] == printed_track(ew, ns));
                /* subtype 2 carries both components times 4: the same entry must serve (a property of the libm; if this
                 * ever fails the table needs a plane for the x4 arguments) */
                CHECK(table[k] == printed_track(4 * ew, 4 * ns));
            }
    CHECK(msd_sbs_track_index(1023, 0, 1) < 0 && msd_sbs_track_index(0, -1023, 1) < 0 && msd_sbs_track_index(4088, 4088, 2) >= 0);
    CHECK(msd_sbs_track_index(4092, 0, 2) < 0 && msd_sbs_track_index(6, 4, 2) < 0 && msd_sbs_track_index(-1022, 1022, 1) >= 0);
}

enum { LINES = 20000 };

static void lines_all(const uint16_t *table)
{
    msd_pos_config cfg = {0, 0, 64, 1, NULL};
    msd_pos_host *p = NULL;
    CHECK(msd_pos_host_create_table(&cfg, &p) == 0 && msd_pos_host_sbs_enable(p) == 0 && msd_pos_host_sbs_enable(p) == 0);
    msd_message *m = calloc(LINES, sizeof *m);
    msd_fields *f = calloc(LINES, sizeof *f);
    msd_sbs_track *t = calloc(LINES, sizeof *t);
    uint8_t *out = malloc((size_t)LINES * MSD_SBS_MAX);
    uint32_t *ends = malloc(sizeof(uint32_t) * LINES);
    CHECK(m && f && t && out && ends);
    static const uint8_t df[12] = {0, 4, 5, 11, 16, 17, 17, 17, 18, 20, 21, 24};
    size_t longest = 0, written = 0;
    for (unsigned flags = 0; flags < 16; ++flags) {
        for (size_t i = 0; i < LINES; ++i) {
            unsigned char *b = (unsigned char *)&f[i];
            for (size_t k = 0; k < sizeof f[i]; ++k)
                b[k] = (unsigned char)rnd();
            b = (unsigned char *)&m[i];
            for (size_t k = 0; k < sizeof m[i]; ++k)
                b[k] = (unsigned char)rnd();
            b = (unsigned char *)&t[i];
            for (size_t k = 0; k < sizeof t[i]; ++k)
                b[k] = (unsigned char)rnd();
            m[i].msgtype = df[rnd() % 12];
            m[i].correctedbits = (uint8_t)(rnd() % 3);
            f[i].metype = (uint8_t)(rnd() % 32);
            f[i].airground = (uint8_t)(rnd() % 5);
            if (rnd() % 4)
                f[i].addr &= ~MSD_NON_ICAO_ADDRESS;
            if (rnd() % 3) { /* plausible values beside the random bytes */
                m[i].sysTimestampMsg = rnd64() % (uint64_t)(2 * MSD_SBS_YEAR_10000_MS);
                t[i].lat = ((double)(int64_t)rnd64() / 9223372036854775808.0) * 90.0;
                t[i].lon = ((double)(int64_t)rnd64() / 9223372036854775808.0) * 180.0;
                t[i].gs_selected = (float)(rnd() % 8000) / 8.0f;
                f[i].ew_vel = (int16_t)((int)(rnd() % 2045) - 1022);
                f[i].ns_vel = (int16_t)((int)(rnd() % 2045) - 1022);
                f[i].mesub = (uint8_t)(1 + rnd() % 2);
                if (f[i].mesub == 2) {
                    f[i].ew_vel = (int16_t)(f[i].ew_vel * 4);
                    f[i].ns_vel = (int16_t)(f[i].ns_vel * 4);
                }
                if (rnd() % 2)
                    f[i].heading_valid = 0;
                for (int k = 0; k < 8; ++k)
                    f[i].callsign[k] = (char)(rnd() % 5 ? 'A' + rnd() % 26 : ' ');
            }
            t[i].flags |= MSD_SBS_TRACKED;
            if (rnd() % 16 == 0)
                t[i].flags = 0;
        }
        msd_sbs_options opt = {1600000000000ull + rnd(), (int64_t)(rnd() % 86400000u) - 43200000, flags, 0};
        size_t len = 0;
        CHECK(msd_pos_host_sbs_wire(p, m, f, t, LINES, &opt, out, (size_t)LINES * MSD_SBS_MAX, &len, ends) == 0);
        size_t at = 0;
        for (size_t i = 0; i < LINES; ++i) {
            uint8_t line[MSD_SBS_MAX + 1];
            const uint32_t k = msd_sbs_line(&m[i], &f[i], &t[i], opt.flags, opt.now_ms, opt.utc_offset_ms, table, line);
            CHECK(k <= MSD_SBS_MAX);
            CHECK(k == msd_sbs_line(&m[i], &f[i], &t[i], opt.flags, opt.now_ms, opt.utc_offset_ms, table, NULL));
            if (ends[i] - at != k || memcmp(out + at, line, k) != 0) {
                fprintf(stderr, "sbs_units: record %zu, flags %u:\n twin %.*s here %.*s", i, flags, (int)(ends[i] - at),
                        (const char *)out + at, (int)k, (const char *)line);
                exit(1);
            }
            if (k > longest)
                longest = k;
            written += k != 0;
            at = ends[i];
        }
        CHECK(at == len);
    }
    CHECK(written > LINES && longest > 120);
    /* refusals */
    size_t len = 7;
    msd_sbs_options opt = {0, 0, 0, 0};
    CHECK(msd_pos_host_sbs_wire(p, NULL, NULL, NULL, 0, &opt, NULL, 0, &len, NULL) == 0 && len == 0);
    CHECK(msd_sbs_options_ok(&opt));
    opt.flags = 16;
    CHECK(!msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == -EINVAL);
    opt.flags = 0, opt.reserved = 1;
    CHECK(!msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == -EINVAL);
    opt.reserved = 0, opt.utc_offset_ms = -1;
    CHECK(!msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == -EINVAL);
    opt.now_ms = 1;
    CHECK(msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == 0);
    opt.now_ms = (uint64_t)MSD_SBS_YEAR_10000_MS, opt.utc_offset_ms = 0;
    CHECK(!msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == -EINVAL);
    opt.utc_offset_ms = -1;
    CHECK(msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == 0);
    opt.now_ms = ~(uint64_t)0, opt.utc_offset_ms = 2;
    CHECK(!msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == -EINVAL);
    opt.now_ms = 5, opt.utc_offset_ms = INT64_MIN;
    CHECK(!msd_sbs_options_ok(&opt) && msd_pos_host_sbs_wire(p, m, f, t, 1, &opt, out, 200, &len, ends) == -EINVAL);
    free(m), free(f), free(t), free(out), free(ends);
    msd_pos_host_destroy(p);
}

int main(void)
{
    uint16_t *table = malloc(sizeof(uint16_t) * MSD_SBS_TRACK_ENTRIES);
    CHECK(table);
    const size_t doubles = f5_all();
    CHECK(doubles >= 10000000);
    f0_all();
    civil_all();
    track_all(table);
    lines_all(table);
    free(table);
    printf("sbs_units: ok, %zu doubles\n", doubles);
    return 0;
}
