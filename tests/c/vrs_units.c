/* vrs_units.c -- the VRS writer's printing (msd_vrs_impl.h, what the device runs) held against glibc under a main of its
 * own: %f of ten million doubles (random values in +-360, every exact tie at six places in that range, +-0, the values
 * just under a carry), %.2f of the InHg product for every nav_qnh_raw in both encodings, %.0f of doubles around exact
 * halves and at random in [0, 2^32), the escaping of all 256 byte values, and whole objects of random table entries --
 * the longest one among them -- against the host twin's snprintf writer, with counted length == bytes written for each.
 * Built with -fsanitize=address,undefined by tests/test_vrs_units.py and scripts/sanitize.sh.  Prints `vrs_units: ok, N`. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msd_pos_host.h"
#include "msd_vrs_impl.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull, g_checks;

static uint64_t rnd(void)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

#define FAIL(...)                                                                                                     \
    do {                                                                                                              \
        fprintf(stderr, "vrs_units: %s:%d: ", __FILE__, __LINE__);                                                    \
        fprintf(stderr, __VA_ARGS__);                                                                                 \
        fprintf(stderr, "\n");                                                                                        \
        exit(1);                                                                                                      \
    } while (0)

static void fixed_is_printf(double x, unsigned places, uint32_t factor)
{
    char want[64];
    uint8_t got[64];
    const int k = snprintf(want, sizeof want, places == 6 ? "%f" : "%.2f", x);
    msd_vrs_w c = {NULL, 0}, w = {got, 0};
    msd_vrs_put_fixed(&c, x, places, factor);
    msd_vrs_put_fixed(&w, x, places, factor);
    if (c.n != w.n || (int)w.n != k || memcmp(got, want, (size_t)k))
        FAIL("%%.%uf of %a: %.*s, printf %s (counted %u)", places, x, (int)w.n, (const char *)got, want, c.n);
    g_checks++;
}

static void f6(double x)
{
    fixed_is_printf(x, 6, 1000000u);
}

static void round0_is_printf(double v)
{
    char want[64];
    uint8_t got[64];
    const int k = snprintf(want, sizeof want, "%.0f", v);
    msd_vrs_w w = {got, 0};
    msd_vrs_put_u64(&w, (uint64_t)rint(v), 0);
    if ((int)w.n != k || memcmp(got, want, (size_t)k))
        FAIL("%%.0f of %a: %.*s, printf %s", v, (int)w.n, (const char *)got, want);
    g_checks++;
}

static void percent_f(void)
{
    /* ten million random values: uniform in +-360, and with a random exponent down to 2^-80 */
    for (int i = 0; i < 5100000; ++i)
        f6((double)(int64_t)rnd() / 9223372036854775808.0 * 360.0);
    for (int i = 0; i < 5000000; ++i) {
        const double m = (double)(rnd() >> 11) / 9007199254740992.0 + 0.5;
        const double x = ldexp(m, (int)(rnd() % 89) - 80); /* up to 1.5 x 2^8 = 384: clipped */
        f6((rnd() & 1) ? -fmin(x, 360.0) : fmin(x, 360.0));
    }
    /* x 10^6 ends in exactly .5 only for x = m / 128 with m odd (10^6 = 2^6 5^6): every one of them within +-360 */
    for (int m = 1; m < 360 * 128; m += 2) {
        f6(m / 128.0);
        f6(-m / 128.0);
    }
    f6(0.0);
    f6(-0.0);
    f6(360.0);
    f6(-360.0);
    const double carry[] = {9.9999995, 179.9999995, 0.9999995, 99.9999995, 359.9999995, 0.0000005, 89.9999995, 0.4999995};
    for (unsigned i = 0; i < sizeof carry / sizeof carry[0]; ++i)
        for (int sign = -1; sign <= 1; sign += 2) {
            const double x = sign * carry[i];
            f6(x);
            f6(nextafter(x, INFINITY));
            f6(nextafter(x, -INFINITY));
        }
    /* the smallest values: below half a unit of the sixth place everything is 0.000000 with its sign */
    f6(4.9e-324);
    f6(-4.9e-324);
    f6(2.2250738585072014e-308);
    f6(4.9999999999999996e-7);
    f6(5.0000000000000004e-7);
}

static void in_hg(void)
{
    for (unsigned commb = 0; commb < 2; ++commb)
        for (unsigned raw = 0; raw < 65536; ++raw) {
            msd_aircraft a;
            msd_aircraft_float fl;
            memset(&a, 0, sizeof a);
            a.nav_qnh_raw = (uint16_t)raw;
            a.nav_qnh_commb = (uint8_t)commb;
            a.source[MSD_AC_NAV_QNH] = 7;
            a.updated[MSD_AC_NAV_QNH] = 1;
            msd_aircraft_to_float(&a, &fl);
            const float qnh = commb ? (float)(800 + raw * 0.1) : (float)(800.0 + ((int)raw - 1) * 0.8);
            if (memcmp(&qnh, &fl.nav_qnh, sizeof qnh))
                FAIL("nav_qnh of raw %u commb %u: %a, msd_aircraft_to_float %a", raw, commb, qnh, fl.nav_qnh);
            fixed_is_printf(qnh * 0.02952998307, 2, 100u);
        }
}

static void percent_0f(void)
{
    const double halves[] = {0.5, 1.5, 2.5, 254.5, 3.5, 255.5, 4294967294.5, 4294967295.5, 0.0, 1.0, 4294967295.0};
    for (unsigned i = 0; i < sizeof halves / sizeof halves[0]; ++i) {
        round0_is_printf(halves[i]);
        round0_is_printf(nextafter(halves[i], INFINITY));
        if (halves[i] > 0)
            round0_is_printf(nextafter(halves[i], 0.0));
    }
    for (int i = 0; i < 1000000; ++i) {
        round0_is_printf((double)(rnd() >> 11) / 9007199254740992.0 * 4294967296.0);
        round0_is_printf((double)(rnd() % 1024u) + ((rnd() & 1) ? 0.5 : (double)(rnd() >> 11) / 9007199254740992.0));
    }
    /* the rule for what no decoder delivers */
    const double out[] = {-0.0, -1.0, -1e-300, NAN, -NAN, INFINITY, -INFINITY, 4294967296.0, 1e300};
    for (unsigned i = 0; i < sizeof out / sizeof out[0]; ++i) {
        if (msd_vrs_sig_printable(out[i]))
            FAIL("%a counts as a printable Sig", out[i]);
        g_checks++;
    }
    if (!msd_vrs_sig_printable(0.0) || !msd_vrs_sig_printable(4294967295.9999995))
        FAIL("the printable range of Sig");
}

static void escapes(void)
{
    for (unsigned b = 0; b < 256; ++b) {
        const char s[8] = {'A', (char)b, 'Z', 0, 'x', 'x', 'x', 'x'};
        char want[32];
        uint8_t got[32];
        int k;
        if (b == 0)
            k = snprintf(want, sizeof want, "A");
        else if (b == '"' || b == '\\')
            k = snprintf(want, sizeof want, "A\\%cZ", (int)b);
        else if (b < 32 || b > 127)
            k = snprintf(want, sizeof want, "A\\u%04xZ", b);
        else
            k = snprintf(want, sizeof want, "A%cZ", (int)b);
        msd_vrs_w c = {NULL, 0}, w = {got, 0};
        msd_vrs_put_escaped(&c, s, 8);
        msd_vrs_put_escaped(&w, s, 8);
        if (c.n != w.n || (int)w.n != k || memcmp(got, want, (size_t)k))
            FAIL("the escape of byte %u: %.*s, expected %s", b, (int)w.n, (const char *)got, want);
        g_checks++;
    }
    const char full[8] = {'1', '2', '3', '4', '5', '6', '7', '8'}; /* no NUL: eight bytes and no more */
    msd_vrs_w c = {NULL, 0};
    msd_vrs_put_escaped(&c, full, 8);
    if (c.n != 8)
        FAIL("a callsign without a NUL: %u bytes", c.n);
}

static uint16_t *g_table;

/* the device's object of an entry against the host twin's; -> its length */
static uint32_t object_is_the_twins(const msd_aircraft *a, uint64_t now, int comma)
{
    char want[MSD_VRS_AIRCRAFT_MAX + 2];
    uint8_t got[MSD_VRS_AIRCRAFT_MAX + 1];
    msd_vrs_head h;
    msd_vrs_head_of_entry(a, &h);
    const size_t k = msd_pos_host_vrs_object(a, now, comma, want);
    const uint32_t counted = msd_vrs_aircraft(&h, a, now, comma, g_table, NULL);
    if (counted > MSD_VRS_AIRCRAFT_MAX)
        FAIL("an object of %u bytes", counted);
    memset(got, 0xEE, sizeof got);
    const uint32_t n = msd_vrs_aircraft(&h, a, now, comma, g_table, got);
    if (n != counted || got[n] != 0xEE)
        FAIL("counted %u, wrote %u", counted, n);
    if (n != k || memcmp(got, want, k))
        FAIL("object: %.*s\nthe twin's: %s", (int)n, (const char *)got, want);
    g_checks++;
    return n;
}

static double odd_double(void)
{
    switch (rnd() % 12) {
    case 0: return NAN;
    case 1: return -1.0;
    case 2: return 1e12;
    case 3: return -0.0;
    case 4: return INFINITY;
    case 5: return 2105376.0; /* 255 x 8 of it / 8: above 2^29 */
    default: return (double)(rnd() % 100000) / 100000.0;
    }
}

static void objects(void)
{
    const uint64_t now = 1700000000000ull;
    for (int i = 0; i < 200000; ++i) {
        msd_aircraft a;
        uint8_t *b = (uint8_t *)&a;
        for (size_t j = 0; j < sizeof a; ++j)
            b[j] = (uint8_t)rnd();
        for (int j = 0; j < 8; ++j)
            a.signal_level[j] = odd_double();
        a.lat = (rnd() % 16) ? (double)(int64_t)rnd() / 9223372036854775808.0 * 90.0 : (rnd() & 1 ? NAN : 360.5);
        a.lon = (rnd() % 16) ? (double)(int64_t)rnd() / 9223372036854775808.0 * 180.0 : (rnd() & 1 ? -INFINITY : -360.0);
        for (int j = 0; j < MSD_AC_N; ++j) {
            a.source[j] = (uint8_t)(rnd() % 8);
            a.updated[j] = (rnd() % 8) ? now - rnd() % 140000 : rnd();
        }
        a.altitude_geom_expires = now - 70000 + rnd() % 140000;
        a.altitude_baro_reliable = (int32_t)(rnd() % 6);
        msd_aircraft_heading *hd[3] = {&a.track, &a.mag_heading, &a.true_heading};
        for (int j = 0; j < 3; ++j) {
            hd[j]->kind = (uint8_t)(rnd() % 5);
            if (rnd() & 1) {
                hd[j]->ew = (int16_t)((int)(rnd() % 2047) - 1023);
                hd[j]->ns = (int16_t)((int)(rnd() % 2047) - 1023);
            }
        }
        a.nav_qnh_commb &= 1;
        a.nav_heading_v2 &= 1;
        if (rnd() & 1)
            a.messages = rnd() % 100000;
        (void)object_is_the_twins(&a, now, (int)(rnd() & 1));
    }
    /* the longest object: every key, every value at its widest */
    msd_aircraft a;
    memset(&a, 0, sizeof a);
    for (int j = 0; j < MSD_AC_N; ++j) {
        a.source[j] = 7;
        a.updated[j] = now;
    }
    a.updated[MSD_AC_POSITION] = UINT64_MAX - 70000; /* (updated + 70 s does not wrap; now is below it) */
    a.altitude_geom_expires = now + 1;
    for (int j = 0; j < 8; ++j)
        a.signal_level[j] = 1.5e7;
    a.addr = 0xFFFFFF;
    a.altitude_baro_reliable = 3;
    a.alt_baro = a.alt_geom = a.nav_altitude_mcp = a.geom_rate = INT32_MIN;
    a.nav_qnh_raw = 65535;
    memset(a.callsign, 0xFF, 8);
    a.lat = a.lon = -360.0;
    a.gs = 0x80000000u;
    a.track.kind = MSD_HDG_SURFACE;
    a.track.raw = 65535;
    a.nav_heading_raw = 65535;
    a.squawk = 0xFFFF;
    a.adsb_version = 127;
    a.messages = UINT64_MAX;
    const uint32_t longest = object_is_the_twins(&a, now, 1);
    if (longest != MSD_VRS_AIRCRAFT_MAX)
        FAIL("the longest object has %u bytes, MSD_VRS_AIRCRAFT_MAX is %u", longest, (unsigned)MSD_VRS_AIRCRAFT_MAX);
}

static void options(void)
{
    msd_vrs_options o = {0, 0, 1, 0, 0};
    if (msd_vrs_part_shift(&o) != 11)
        FAIL("n_parts 1");
    o.n_parts = 8, o.part = 7;
    if (msd_vrs_part_shift(&o) != 8)
        FAIL("n_parts 8");
    o.n_parts = 2048, o.part = 2047;
    if (msd_vrs_part_shift(&o) != 0)
        FAIL("n_parts 2048");
    const uint32_t bad[][2] = {{0, 0}, {0, 3}, {0, 4096}, {8, 8}, {1, 1}, {0, 6}};
    for (unsigned i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
        o.part = bad[i][0], o.n_parts = bad[i][1];
        if (msd_vrs_part_shift(&o) >= 0)
            FAIL("part %u of %u was accepted", bad[i][0], bad[i][1]);
    }
    g_checks += 9;
}

int main(void)
{
    g_table = malloc(sizeof(uint16_t) * MSD_PB_TRACK_ENTRIES);
    if (!g_table)
        FAIL("out of memory");
    msd_pb_build_track_table(g_table);
    percent_f();
    in_hg();
    percent_0f();
    escapes();
    objects();
    options();
    free(g_table);
    printf("vrs_units: ok, %llu\n", (unsigned long long)g_checks);
    return 0;
}
