/* history_units.c -- the history_N.pb encoder (msd_history_impl.h: what the device runs) and the host twin's
 * (msd_pos_host_history_entry, host/msd_pos_host.c) held to each other and to their own rules on the CPU, by a stand-alone
 * program so that a sanitizer build can watch both (scripts/sanitize.sh and tests/test_history_units.py build it with
 * -fsanitize=address,undefined).
 *   lengths   every varint length an entry can hold: addresses of 1, 2, 3 and 4 bytes at each edge, altitudes of 1, 2, 3
 *             and 10 bytes at each edge, with and without each coordinate; the length without a destination == the bytes
 *             written, into a buffer of exactly that many bytes with guard bytes behind it
 *   twin      the same bytes from the host twin, which shares no code with the header
 *   longest   the constructed worst entry is MSD_HISTORY_ENTRY_MAX bytes; no random entry is longer
 *   rules     selection and the four altitude outcomes on entries with pseudo-random validities around `now`; the head
 * Prints `history_units: ok, N`. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msd_pos_host.h"
#include "msd_history_impl.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull, g_checks;

static uint64_t rnd(void)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

#define CHECK(c)                                                                                                        \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "history_units: %s:%d: %s\n", __FILE__, __LINE__, #c);                                    \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

#define GUARD 8

static unsigned varint_len(uint64_t v)
{
    unsigned n = 1;
    while (v >= 128) {
        v >>= 7;
        ++n;
    }
    return n;
}

/* the header's entry of `a` at `now` against the twin's -> its length.  Both write into heap blocks of exactly the
 * counted length plus guard bytes, so that a byte too many is the sanitizer's to see and a guard's to show */
static uint32_t entry_is_the_twins(const msd_aircraft *a, uint64_t now)
{
    msd_pb_head h;
    msd_pb_head_of_entry(a, &h);
    const int32_t alt = msd_history_altitude(a, now);
    const uint32_t counted = msd_history_entry(&h, alt, NULL);
    CHECK(counted >= 2 && counted <= MSD_HISTORY_ENTRY_MAX);
    uint8_t *got = malloc(counted + GUARD), *want = malloc(counted + GUARD);
    CHECK(got && want);
    memset(got, 0xEE, counted + GUARD);
    memset(want, 0xEE, counted + GUARD);
    const uint32_t n = msd_history_entry(&h, alt, got);
    CHECK(n == counted);
    CHECK(msd_pos_host_history_entry(a, now, NULL) == counted);
    CHECK(msd_pos_host_history_entry(a, now, want) == counted);
    for (unsigned i = 0; i < GUARD; ++i)
        CHECK(got[counted + i] == 0xEE && want[counted + i] == 0xEE);
    CHECK(memcmp(got, want, counted) == 0);
    CHECK(got[0] == 0x72 && got[1] == counted - 2);
    /* the length by the terms: what each member takes */
    uint32_t terms = 2;
    if (h.addr)
        terms += 1 + varint_len(h.addr);
    if (alt)
        terms += 1 + varint_len((uint64_t)(int64_t)alt);
    if (!(0 == a->lat))
        terms += 9;
    if (!(0 == a->lon))
        terms += 9;
    CHECK(terms == counted);
    free(got);
    free(want);
    g_checks++;
    return counted;
}

static void lengths(void)
{
    const uint64_t now = 1700000000000ull;
    static const uint32_t addrs[] = {0, 1, 127, 128, 16383, 16384, 2097151, 2097152, 0xFFFFFF, 0x1000000, 0x1FFFFFF};
    static const int32_t alts[] = {0, 1, 127, 128, 16383, 16384, 2097151, 2097152, 268435455, 268435456, INT32_MAX, -1, -975,
                                   -9999, INT32_MIN};
    static const double coords[] = {0.0, -0.0, 52.25, -179.999, 4.9e-324};
    for (unsigned i = 0; i < sizeof addrs / sizeof addrs[0]; ++i)
        for (unsigned j = 0; j < sizeof alts / sizeof alts[0]; ++j)
            for (unsigned k = 0; k < 5; ++k)
                for (unsigned l = 0; l < 5; ++l) {
                    msd_aircraft a;
                    memset(&a, 0, sizeof a);
                    a.addr = addrs[i];
                    a.source[MSD_AC_ALTITUDE_BARO] = 7;
                    a.updated[MSD_AC_ALTITUDE_BARO] = now;
                    a.altitude_baro_reliable = 3;
                    a.alt_baro = alts[j];
                    a.lat = coords[k];
                    a.lon = coords[l];
                    (void)entry_is_the_twins(&a, now);
                }
    msd_aircraft a;
    memset(&a, 0, sizeof a);
    a.lat = NAN; /* written: 0 == NaN is false */
    CHECK(entry_is_the_twins(&a, now) == 2 + 9);
    a.lat = 0;
    CHECK(entry_is_the_twins(&a, now) == 2); /* nothing to say: a tag and a length of 0 */
    /* the longest: the non-ICAO bit, a negative altitude, both coordinates */
    a.addr = 0x1000000u | 0x4840D6u;
    a.source[MSD_AC_AIRGROUND] = 4;
    a.updated[MSD_AC_AIRGROUND] = now;
    a.air_ground = 1;
    a.lat = -89.5;
    a.lon = 179.5;
    CHECK(entry_is_the_twins(&a, now) == MSD_HISTORY_ENTRY_MAX);
    CHECK(msd_history_altitude(&a, now) == -9999);
}

static void rules(void)
{
    const uint64_t now = 1700000000000ull;
    unsigned outcome[4] = {0, 0, 0, 0}, selected = 0, refused = 0;
    for (int i = 0; i < 200000; ++i) {
        msd_aircraft a;
        uint8_t *b = (uint8_t *)&a;
        for (size_t j = 0; j < sizeof a; ++j)
            b[j] = (uint8_t)rnd();
        for (int j = 0; j < MSD_AC_N; ++j) {
            a.source[j] = (uint8_t)(rnd() % 8);
            a.updated[j] = (rnd() % 8) ? now - 70000 - 2 + rnd() % 5 : now - rnd() % 140000;
        }
        a.altitude_geom_expires = (rnd() % 4) ? now - 2 + rnd() % 5 : now - 70000 + rnd() % 140000;
        a.altitude_baro_reliable = (int32_t)(rnd() % 6);
        a.air_ground = (uint8_t)(rnd() % 4);
        a.messages = rnd() % 4;
        a.seen = (rnd() % 4) ? now - 90000 - 2 + rnd() % 5 : now - 200000 + rnd() % 400000;
        a.lat = (rnd() % 8) ? (double)(int64_t)rnd() / 9223372036854775808.0 * 90.0 : (rnd() & 1 ? NAN : -0.0);
        a.lon = (rnd() % 8) ? (double)(int64_t)rnd() / 9223372036854775808.0 * 180.0 : 0.0;
        (void)entry_is_the_twins(&a, now);
        /* the rules, restated from net_io.c:2115-2146 on the entry's own members */
        const int ground = a.source[MSD_AC_AIRGROUND] >= 4 && now < a.updated[MSD_AC_AIRGROUND] + 70000 && a.air_ground == 1;
        const int baro = a.source[MSD_AC_ALTITUDE_BARO] != 0 && now < a.updated[MSD_AC_ALTITUDE_BARO] + 70000 &&
                         a.altitude_baro_reliable >= 3;
        const int geom = a.source[MSD_AC_ALTITUDE_GEOM] != 0 && now < a.altitude_geom_expires;
        const int32_t want = ground ? -9999 : baro ? a.alt_baro : geom ? a.alt_geom : 0;
        CHECK(msd_history_altitude(&a, now) == want);
        outcome[ground ? 0 : baro ? 1 : geom ? 2 : 3]++;
        msd_pb_head h;
        msd_pb_head_of_entry(&a, &h);
        const int sel = !(a.messages < 2) && !(now > a.seen + 90000) && a.source[MSD_AC_POSITION] != 0 &&
                        now < a.updated[MSD_AC_POSITION] + 70000;
        CHECK(msd_history_selected(&h, now) == sel);
        CHECK(msd_aircraft_valid(&a, MSD_AC_POSITION, now) == (a.source[MSD_AC_POSITION] != 0 && now < a.updated[MSD_AC_POSITION] + 70000));
        sel ? ++selected : ++refused;
        g_checks += 2;
    }
    CHECK(outcome[0] > 1000 && outcome[1] > 1000 && outcome[2] > 1000 && outcome[3] > 1000 && selected > 1000 && refused > 1000);
    /* the head: nothing below one second, else `now` in seconds */
    uint8_t head[MSD_HISTORY_HEADER_MAX + 1];
    memset(head, 0xEE, sizeof head);
    CHECK(msd_history_header(999, NULL) == 0 && msd_history_header(999, head) == 0 && head[0] == 0xEE);
    CHECK(msd_history_header(1000, head) == 2 && head[0] == 0x08 && head[1] == 0x01 && head[2] == 0xEE);
    const uint32_t widest = 1 + varint_len(UINT64_MAX / 1000); /* 55 bits: 8 bytes */
    CHECK(widest == 9 && msd_history_header(UINT64_MAX, NULL) == widest && msd_history_header(UINT64_MAX, head) == widest && head[widest] == 0xEE);
    msd_history_options o = {now, 0, 0};
    CHECK(msd_history_options_ok(&o) && !msd_history_options_ok(NULL));
    o.flags = 1;
    CHECK(!msd_history_options_ok(&o));
    o.flags = 0, o.reserved = 1;
    CHECK(!msd_history_options_ok(&o));
    g_checks += 7;
}

int main(void)
{
    lengths();
    rules();
    printf("history_units: ok, %llu\n", (unsigned long long)g_checks);
    return 0;
}
