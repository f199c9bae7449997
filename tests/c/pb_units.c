/* pb_units.c -- the aircraft.pb encoder (msd_pb_impl.h: what the device runs) held to its own rules on the CPU, by a
 * stand-alone program so that a sanitizer build can watch it (scripts/sanitize.sh and tests/test_pb_units.py build it with
 * -fsanitize=address,undefined).
 *   varints  0, 127, 128, 16383, 16384, 2^32 - 1, 2^63, 2^64 - 1 against bytes written by hand, every length read back;
 *            negative int32 values through the 10-byte path: the edges and a stride over all of them
 *   lengths  the length without a destination == the bytes written, for an entry with every field present, for one with
 *            none, and for entries with pseudo-random bytes in every member
 *   longest  the constructed worst entry is MSD_PB_AIRCRAFT_MAX bytes; no random entry is longer
 *   track    msd_pb_build_track_table against (int32_t) of msd_aircraft_to_float's value for all 4 x 1023^2 entries and
 *            for the same components times 4 (ES type 19 subtype 2), through msd_pb_track_index
 *   state    msd_pb_next_state: the saturated, wrapped seen_pos and the two sticky bits */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msd_pb_impl.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(c)                                                                                                        \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "pb_units: %s:%d: %s\n", __FILE__, __LINE__, #c);                                         \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

static size_t checks;

static uint64_t read_varint(const uint8_t *b, uint32_t n)
{
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; ++i) {
        CHECK(((b[i] & 128u) != 0) == (i + 1 < n));
        v |= (uint64_t)(b[i] & 127u) << (7u * i);
    }
    return v;
}

static void varint_one(uint64_t v, const uint8_t *want, uint32_t nwant)
{
    uint8_t got[16];
    memset(got, 0xEE, sizeof got);
    msd_pb_w w = {got, 0}, count = {NULL, 0};
    msd_pb_varint(&w, v);
    msd_pb_varint(&count, v);
    CHECK(w.n == count.n && w.n <= 10 && got[w.n] == 0xEE);
    CHECK(read_varint(got, w.n) == v);
    if (want)
        CHECK(w.n == nwant && memcmp(got, want, nwant) == 0);
    ++checks;
}

static void int32_one(int32_t v)
{
    uint8_t got[16];
    msd_pb_w w = {got, 0};
    msd_pb_int32(&w, 5, v);
    CHECK(w.n == 11 && got[0] == 0x28 && got[10] == 0x01);
    CHECK((int32_t)read_varint(got + 1, 10) == v && (int64_t)read_varint(got + 1, 10) == (int64_t)v);
    ++checks;
}

static void varints(void)
{
    static const uint8_t v0[] = {0x00}, v127[] = {0x7F}, v128[] = {0x80, 0x01}, v16383[] = {0xFF, 0x7F},
                         v16384[] = {0x80, 0x80, 0x01}, v32[] = {0xFF, 0xFF, 0xFF, 0xFF, 0x0F},
                         v63[] = {0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x01},
                         v64[] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x01};
    varint_one(0, v0, 1);
    varint_one(127, v127, 1);
    varint_one(128, v128, 2);
    varint_one(16383, v16383, 2);
    varint_one(16384, v16384, 3);
    varint_one(0xFFFFFFFFull, v32, 5);
    varint_one((uint64_t)1 << 63, v63, 10);
    varint_one(~(uint64_t)0, v64, 10);
    for (int k = 0; k < 64; ++k) {
        varint_one((uint64_t)1 << k, NULL, 0);
        varint_one(((uint64_t)1 << k) - 1u, NULL, 0);
    }
    int32_one(-1);
    int32_one(INT32_MIN);
    int32_one(INT32_MIN + 1);
    int32_one(-128);
    int32_one(-129);
    for (int64_t v = -1; v >= INT32_MIN; v -= 4099) /* every form: all ten bytes are the sign extension's */
        int32_one((int32_t)v);
    { /* a zero scalar writes nothing; -0.0 neither; NaN does */
        uint8_t got[16];
        msd_pb_w w = {got, 0};
        msd_pb_int32(&w, 5, 0);
        msd_pb_uint(&w, 1, 0);
        msd_pb_float(&w, 12, -0.0f);
        msd_pb_double(&w, 8, -0.0);
        CHECK(w.n == 0);
        msd_pb_float(&w, 12, NAN);
        CHECK(w.n == 5 && got[0] == 0x65);
    }
}

static uint32_t entry_both(const msd_aircraft *a, uint64_t state, const uint16_t *table, uint8_t *buf, size_t room)
{
    msd_pb_head h;
    msd_pb_head_of_entry(a, &h);
    memset(buf, 0xEE, room);
    const uint32_t want = msd_pb_aircraft(&h, a, state, table, NULL);
    CHECK(want + 1u <= room);
    const uint32_t got = msd_pb_aircraft(&h, a, state, table, buf);
    CHECK(got == want && buf[got] == 0xEE && buf[0] == 0x7A);
    ++checks;
    return got;
}

static void entries(const uint16_t *table)
{
    uint8_t buf[1024];
    msd_aircraft a;
    /* nothing: a fresh aircraft.  addr 0 cannot be, rssi of eight 1e-5 is written, valid_source is BA 09 00 */
    msd_trk_init(&a);
    a.addr_type = 0;
    {
        const uint32_t n = entry_both(&a, 0, table, buf, sizeof buf);
        static const uint8_t tail[] = {0xBA, 0x09, 0x00};
        CHECK(n == 2 + 5 + 3 && buf[1] == 8 && buf[2] == 0x65 && memcmp(buf + 7, tail, 3) == 0);
    }
    /* everything, at its longest */
    memset(&a, 0xFF, sizeof a);
    a.addr = 0x1FFFFFF;
    a.seen = a.messages = ~(uint64_t)0;
    a.lat = a.lon = -1.5;
    a.gs = a.ias = a.tas = 0xFFFFFFFFu;
    for (int i = 0; i < 8; ++i)
        a.signal_level[i] = 0.25;
    a.alt_baro = a.alt_geom = a.baro_rate = a.geom_rate = a.nav_altitude_mcp = a.nav_altitude_fms = -1;
    a.mag_heading.kind = a.true_heading.kind = a.track.kind = MSD_HDG_SURFACE;
    a.mag_heading.raw = a.true_heading.raw = a.track.raw = 0xFFFF;
    a.squawk = a.mach_raw = a.nav_qnh_raw = a.nav_heading_raw = a.rc = 0xFFFF;
    a.nav_heading_v2 = 0;
    a.roll_q = a.track_rate_q = -1;
    memcpy(a.callsign, "ABCDEFGH", 8);
    a.nav_modes = 63;
    a.adsb_version = 127;
    {
        const uint32_t n = entry_both(&a, MSD_PB_FLIGHT_ATTACHED | MSD_PB_NAV_MODES_ATTACHED | 0xFFFFFFFFu, table, buf, sizeof buf);
        if (n != MSD_PB_AIRCRAFT_MAX) {
            fprintf(stderr, "pb_units: the worst entry is %u bytes, MSD_PB_AIRCRAFT_MAX is %d\n", n, MSD_PB_AIRCRAFT_MAX);
            exit(1);
        }
    }
    /* pseudo-random bytes in every member: count == written, never beyond the longest */
    for (int k = 0; k < 200000; ++k) {
        uint64_t *w = (uint64_t *)&a;
        for (size_t i = 0; i < sizeof a / 8; ++i)
            w[i] = (k & 1) ? rnd64() : rnd64() & rnd64() & rnd64();
        const uint64_t state = rnd64() & (MSD_PB_FLIGHT_ATTACHED | MSD_PB_NAV_MODES_ATTACHED | 0xFFFFFFFFu);
        CHECK(entry_both(&a, state, table, buf, sizeof buf) <= MSD_PB_AIRCRAFT_MAX);
    }
    { /* the file's head */
        uint8_t hd[32];
        CHECK(msd_pb_header(999, 0, NULL) == 0);
        CHECK(msd_pb_header(~(uint64_t)0, ~(uint64_t)0, NULL) <= MSD_PB_HEADER_MAX);
        CHECK(msd_pb_header(~(uint64_t)0, ~(uint64_t)0, hd) == msd_pb_header(~(uint64_t)0, ~(uint64_t)0, NULL));
        CHECK(msd_pb_header(1000, 300, hd) == 5 && hd[0] == 0x08 && hd[1] == 1 && hd[2] == 0x10 && hd[3] == 0xAC && hd[4] == 0x02);
    }
}

static void track(const uint16_t *table)
{
    msd_aircraft a;
    msd_aircraft_float fl;
    msd_trk_init(&a);
    a.track.kind = MSD_HDG_VELOCITY;
    for (int ew = -1022; ew <= 1022; ++ew)
        for (int ns = -1022; ns <= 1022; ++ns)
            for (int scale = 1; scale <= 4; scale += 3) {
                a.track.ew = (int16_t)(ew * scale);
                a.track.ns = (int16_t)(ns * scale);
                msd_aircraft_to_float(&a, &fl);
                const int32_t k = msd_pb_track_index(a.track.ew, a.track.ns);
                CHECK(k >= 0 && (uint32_t)k < MSD_PB_TRACK_ENTRIES);
                if ((int32_t)table[k] != (int32_t)fl.track) {
                    fprintf(stderr, "pb_units: track of (%d, %d): table %u, float %a\n", a.track.ew, a.track.ns, table[k], fl.track);
                    exit(1);
                }
                CHECK(msd_pb_heading(&a.track, table) == (int32_t)fl.track);
                ++checks;
            }
    CHECK(msd_pb_track_index(1023, 0) < 0 && msd_pb_track_index(1024, 2) < 0 && msd_pb_track_index(4092, 0) < 0 &&
          msd_pb_track_index(4088, -4088) >= 0 && msd_pb_track_index(-32768, 0) < 0);
    /* the other kinds against the same yardstick */
    for (unsigned raw = 0; raw < 65536; ++raw)
        for (int kind = MSD_HDG_COMMB; kind <= MSD_HDG_SURFACE; ++kind) {
            a.track.kind = (uint8_t)kind;
            a.track.raw = (uint16_t)raw;
            msd_aircraft_to_float(&a, &fl);
            CHECK(msd_pb_heading(&a.track, table) == (int32_t)fl.track);
            ++checks;
        }
}

static void state(void)
{
    msd_aircraft a;
    msd_pb_head h;
    msd_trk_init(&a);
    a.messages = 2;
    a.source[MSD_AC_POSITION] = 7;
    a.updated[MSD_AC_POSITION] = 5000;
    msd_pb_head_of_entry(&a, &h);
    CHECK(msd_pb_next_state(0, &h, &a, 9999) == 4);
    CHECK(msd_pb_next_state(7, &h, &a, 75000) == 7); /* expired: the last value stays */
    CHECK(msd_pb_next_state(0, &h, &a, 4000) == 0xFFFFFFFFu); /* updated after now: the wrapped difference, saturated */
    a.source[MSD_AC_CALLSIGN] = 1;
    a.updated[MSD_AC_CALLSIGN] = 1000;
    CHECK(msd_pb_next_state(0, &h, &a, 70999) == (MSD_PB_FLIGHT_ATTACHED | 65));
    CHECK(msd_pb_next_state(0, &h, &a, 71000) == 66);
    CHECK(msd_pb_next_state(MSD_PB_FLIGHT_ATTACHED, &h, &a, 80000) == MSD_PB_FLIGHT_ATTACHED);
    h.messages = 1;
    CHECK(!msd_pb_selected(&h, 0));
    h.messages = 2;
    h.seen = 10000;
    CHECK(msd_pb_selected(&h, 100000) && !msd_pb_selected(&h, 100001) && msd_pb_selected(&h, 5));
    checks += 9;
}

int main(void)
{
    uint16_t *table = malloc(sizeof(uint16_t) * MSD_PB_TRACK_ENTRIES);
    CHECK(table);
    msd_pb_build_track_table(table);
    varints();
    entries(table);
    track(table);
    state();
    free(table);
    printf("pb_units: ok, %zu checks\n", checks);
    return 0;
}
