/* range_units.c -- the host object's receiver range (msd_pos_host_range_enable, _read, _distances, _margins, _pb with
 * msd_pos_impl.h's "the receiver range" behind them), driven by a stand-alone program so that a sanitizer build can watch
 * them (tests/test_range_units.py builds it with -fsanitize=address,undefined).  Position squitters of 60 aircraft on three
 * receivers -- one without a location, one with --max-range -- encoded here (CPR, airborne), with TIS-B records, Mode A/C
 * records and address 0 in between, go through a 64-slot table in calls of 1 to 300 records, with expiry in between; rows,
 * distances and the polar-range stream are read into buffers of exactly the size needed, one entry or byte too few and
 * none; a call overflows the table; a reset.  Checks as it goes: a rolled-back call changes no byte, cutting changes no
 * byte, a refused read writes nothing, an entry of the stream is 2 to 10 bytes, the buckets hold what some distance was. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msd_pos_host.h"
#include "msd_pos_impl.h"

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(void)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

#define CHECK(c)                                                                                                        \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "range_units: %s:%d: %s\n", __FILE__, __LINE__, #c);                                      \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

#define AIRCRAFT 60u
#define NRX 3u
static const msd_pos_receiver RX[NRX] = {{52.0, 4.0, 0.0, 1, 0}, {0.0, 0.0, 0.0, 0, 0}, {-33.9, 151.2, 250.0 * 1852.0, 1, 0}};
static long checks;
static int taken; /* a read has taken `longest`: from then on it is no longer the largest bucket */

/* 1090-WP-9-14: the 17-bit YZ, XZ of an airborne position */
static void cpr_encode(double lat, double lon, int odd, uint32_t *yz, uint32_t *xz)
{
    const double dlat = 360.0 / (odd ? 59 : 60);
    const double y = floor(131072 * msd_cpr_mod_double(lat, dlat) / dlat + 0.5);
    const double rlat = dlat * (y / 131072 + floor(lat / dlat));
    const double dlon = 360.0 / msd_cpr_n(rlat, odd);
    const double x = floor(131072 * msd_cpr_mod_double(lon, dlon) / dlon + 0.5);
    *yz = (uint32_t)y & 0x1FFFFu;
    *xz = (uint32_t)x & 0x1FFFFu;
}

static void make(size_t n, uint64_t *clock, msd_message *m, msd_fields *f, uint32_t *r)
{
    for (size_t i = 0; i < n; ++i) {
        memset(&m[i], 0, sizeof m[i]);
        memset(&f[i], 0, sizeof f[i]);
        const uint32_t a = rnd() % AIRCRAFT, rx = a % NRX;
        *clock += rnd() % 40;
        m[i].sysTimestampMsg = *clock;
        m[i].msgtype = 17;
        r[i] = rx;
        if (rnd() % 40 == 0) { /* the tracker skips these */
            m[i].msgtype = rnd() % 2 ? 32 : 11;
            f[i].addr = m[i].msgtype == 32 ? 0x7000 : 0;
            continue;
        }
        f[i].addr = 0x3C0000u + a * 977u;
        f[i].source = a % 11 == 5 ? 5 : 7; /* a few TIS-B aircraft: decoded, never evaluated */
        const double base_lat = RX[rx].latlon_valid ? RX[rx].lat : 10.0, base_lon = RX[rx].latlon_valid ? RX[rx].lon : 10.0;
        const double t = (double)(*clock % 1000000u) * 1e-6;
        const double lat = base_lat + 0.03 * (double)(a % 13) * (1.0 + t) - 0.2, lon = base_lon + 0.05 * (double)(a % 17) * (1.0 - t) - 0.4;
        uint32_t y, x;
        const int odd = (int)(rnd() & 1u);
        cpr_encode(lat, lon, odd, &y, &x);
        f[i].cpr_valid = 1;
        f[i].cpr_type = 1;
        f[i].cpr_odd = (uint8_t)odd;
        f[i].cpr_lat = y;
        f[i].cpr_lon = x;
        f[i].metype = 11;
    }
}

typedef struct state {
    msd_range_receiver rows[NRX];
    uint32_t dist[64];
    size_t live, pb_len;
    uint8_t pb[NRX * MSD_RANGE_BUCKETS * MSD_RANGE_PB_ENTRY_MAX];
    uint64_t end[NRX];
    msd_range_margins margins;
} state;

/* everything the range delivers, through buffers of exactly the size needed; refused reads write nothing */
static void observe(msd_pos_host *p, state *s)
{
    memset(s, 0, sizeof *s);
    for (uint32_t first = 0; first < NRX; ++first) { /* one row at a time into a heap row: the sanitizer sees one byte more */
        msd_range_receiver *row = malloc(sizeof *row);
        CHECK(row && msd_pos_host_range_read(p, first, 1, row, 0) == 0);
        s->rows[first] = *row;
        free(row);
    }
    msd_range_receiver all[NRX];
    CHECK(msd_pos_host_range_read(p, 0, NRX, all, 0) == 0 && memcmp(all, s->rows, sizeof all) == 0);
    CHECK(msd_pos_host_range_read(p, 1, NRX, all, 0) == -EINVAL && msd_pos_host_range_read(p, NRX + 1, 0, all, 0) == -EINVAL);
    size_t n = 99;
    CHECK(msd_pos_host_range_distances(p, NULL, 0, &n) == (n ? -ENOSPC : 0));
    s->live = n;
    if (n) {
        uint32_t *d = malloc(sizeof(uint32_t) * n), canary = 0xEEEEEEEEu;
        CHECK(d);
        d[0] = canary;
        CHECK(msd_pos_host_range_distances(p, d, n - 1, &n) == -ENOSPC && n == s->live && d[0] == canary);
        CHECK(msd_pos_host_range_distances(p, d, n, &n) == 0 && n == s->live && n <= 64);
        memcpy(s->dist, d, sizeof(uint32_t) * n);
        free(d);
    }
    size_t len = 0;
    CHECK(msd_pos_host_range_pb(p, NULL, 0, &len, NULL) == -ENOSPC && len >= NRX * MSD_RANGE_BUCKETS * 2u && len <= sizeof s->pb);
    uint8_t *b = malloc(len);
    CHECK(b);
    b[0] = 0xEE;
    size_t again = 0;
    CHECK(msd_pos_host_range_pb(p, b, len - 1, &again, s->end) == -ENOSPC && again == len && b[0] == 0xEE && s->end[0] == 0);
    CHECK(msd_pos_host_range_pb(p, b, len, &again, s->end) == 0 && again == len && s->end[NRX - 1] == len);
    memcpy(s->pb, b, len);
    s->pb_len = len;
    free(b);
    /* the stream entry by entry: 32 <len> [08 bucket] [10 varint], in bucket order, the buckets of the rows */
    size_t at = 0;
    for (uint32_t r = 0; r < NRX; ++r) {
        for (uint32_t bucket = 0; bucket < MSD_RANGE_BUCKETS; ++bucket) {
            CHECK(s->pb[at] == 0x32 && s->pb[at + 1] <= 8);
            const size_t stop = at + 2 + s->pb[at + 1];
            at += 2;
            if (bucket) {
                CHECK(s->pb[at] == 0x08 && s->pb[at + 1] == bucket);
                at += 2;
            }
            uint32_t v = 0;
            if (at < stop) {
                CHECK(s->pb[at++] == 0x10);
                for (unsigned shift = 0;; shift += 7) {
                    v |= (uint32_t)(s->pb[at] & 127u) << shift;
                    if (!(s->pb[at++] & 128u))
                        break;
                }
            }
            CHECK(at == stop && v == s->rows[r].polar_range[bucket]);
            ++checks;
        }
        CHECK(s->end[r] == at);
    }
    CHECK(at == len);
    CHECK(msd_pos_host_range_margins(p, &s->margins) == 0);
    /* the receiver without a location keeps nothing; longest is some bucket's value or just above it (the bucket truncates) */
    CHECK(s->rows[1].evaluated == 0 && s->rows[1].longest_m == 0);
    for (uint32_t r = 0; r < NRX; ++r) {
        uint32_t top = 0;
        for (uint32_t bucket = 0; bucket < MSD_RANGE_BUCKETS; ++bucket)
            top = s->rows[r].polar_range[bucket] > top ? s->rows[r].polar_range[bucket] : top;
        CHECK(s->rows[r].longest_m <= top && s->rows[r].longest_nm == s->rows[r].longest_m / 1852u);
        CHECK(RX[r].max_range_m == 0 ? taken || s->rows[r].longest_m == top : (double)s->rows[r].longest_m <= RX[r].max_range_m);
    }
    for (size_t j = 0; j < s->live; ++j)
        CHECK(s->dist[j] < 400000u);
}

static int same(const state *a, const state *b)
{
    return memcmp(a->rows, b->rows, sizeof a->rows) == 0 && a->live == b->live && memcmp(a->dist, b->dist, sizeof a->dist) == 0 &&
           a->pb_len == b->pb_len && memcmp(a->pb, b->pb, a->pb_len) == 0 &&
           memcmp(&a->margins, &b->margins, sizeof a->margins) == 0;
}

int main(void)
{
    msd_pos_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.capacity = 64;
    cfg.receivers = NRX;
    cfg.receiver = RX;
    msd_pos_host *whole = NULL, *cut = NULL, *plain = NULL;
    CHECK(msd_pos_host_create_table(&cfg, &whole) == 0 && msd_pos_host_create(&cfg, &cut) == 0 && msd_pos_host_create(&cfg, &plain) == 0);
    msd_range_receiver row;
    size_t n = 0;
    CHECK(msd_pos_host_range_read(whole, 0, 1, &row, 0) == -EINVAL && msd_pos_host_range_distances(whole, NULL, 0, &n) == -EINVAL);
    CHECK(msd_pos_host_range_enable(whole, 2) == -EINVAL && msd_pos_host_range_enable(whole, MSD_RANGE_POLAR) == 0);
    CHECK(msd_pos_host_range_enable(whole, 0) == 0 && msd_pos_host_range_enable(cut, MSD_RANGE_POLAR) == 0);
    CHECK(msd_pos_host_range_enable(plain, 0) == 0 && msd_pos_host_range_pb(plain, NULL, 0, &n, NULL) == -EINVAL);
    enum { MOST = 300 };
    msd_message *m = malloc(sizeof *m * MOST);
    msd_fields *f = malloc(sizeof *f * MOST);
    uint32_t *r = malloc(sizeof *r * MOST);
    msd_position *out = malloc(sizeof *out * MOST), *out2 = malloc(sizeof *out2 * MOST);
    state *a = malloc(sizeof *a), *b = malloc(sizeof *b);
    CHECK(m && f && r && out && out2 && a && b);
    uint64_t clock = 1600000000000ull;
    uint64_t evaluated = 0;
    for (int round = 0; round < 400; ++round) {
        const size_t k = 1 + rnd() % MOST;
        make(k, &clock, m, f, r);
        CHECK(msd_pos_host_update(whole, m, f, r, k, out) == 0);
        for (size_t i = 0; i < k;) { /* the same records in pieces */
            const size_t want = 1 + rnd() % 7, piece = want < k - i ? want : k - i;
            CHECK(msd_pos_host_update(cut, m + i, f + i, r + i, piece, out2 + i) == 0);
            i += piece;
        }
        CHECK(memcmp(out, out2, sizeof *out * k) == 0);
        CHECK(msd_pos_host_update(plain, m, f, r, k, out2) == 0 && memcmp(out, out2, sizeof *out * k) == 0);
        if (round % 7 == 3) {
            CHECK(msd_pos_host_expire(whole, clock) == 0 && msd_pos_host_expire(cut, clock) == 0 && msd_pos_host_expire(plain, clock) == 0);
        }
        if (round % 5 == 0) {
            observe(whole, a);
            observe(cut, b);
            CHECK(same(a, b));
            CHECK(a->rows[0].evaluated + a->rows[2].evaluated >= evaluated);
            evaluated = a->rows[0].evaluated + a->rows[2].evaluated;
            /* without the polar range: the same distances and longest, no bucket */
            msd_range_receiver rows[NRX];
            uint32_t d[64];
            CHECK(msd_pos_host_range_read(plain, 0, NRX, rows, 0) == 0 && msd_pos_host_range_distances(plain, d, 64, &n) == 0);
            CHECK(n == a->live && memcmp(d, a->dist, sizeof(uint32_t) * n) == 0);
            for (uint32_t x = 0; x < NRX; ++x) {
                CHECK(rows[x].longest_m == a->rows[x].longest_m && rows[x].evaluated == a->rows[x].evaluated);
                for (uint32_t bucket = 0; bucket < MSD_RANGE_BUCKETS; ++bucket)
                    CHECK(rows[x].polar_range[bucket] == 0);
            }
        }
        if (round == 200) { /* a call that does not fit: 64 slots, 70 new aircraft behind records that would move everything */
            observe(whole, a);
            make(200, &clock, m, f, r);
            for (size_t i = 200; i < 270; ++i) {
                m[i] = m[0];
                f[i] = f[0];
                r[i] = 0;
                m[i].msgtype = 17;
                f[i].addr = 0x500000u + (uint32_t)i;
            }
            CHECK(msd_pos_host_update(whole, m, f, r, 270, out) == -ENOSPC);
            observe(whole, b);
            CHECK(same(a, b));
            CHECK(msd_pos_host_update(whole, m, f, r, 200, out) == 0 && msd_pos_host_update(cut, m, f, r, 200, out2) == 0);
            CHECK(msd_pos_host_update(plain, m, f, r, 200, out2) == 0);
        }
        if (round == 300) { /* take longest: zeroed behind the read, the buckets stay */
            observe(whole, a);
            taken = 1;
            msd_range_receiver rows[NRX];
            CHECK(msd_pos_host_range_read(whole, 0, NRX, rows, MSD_RANGE_TAKE_LONGEST) == 0 && memcmp(rows, a->rows, sizeof rows) == 0);
            CHECK(msd_pos_host_range_read(cut, 0, NRX, rows, MSD_RANGE_TAKE_LONGEST) == 0);
            CHECK(msd_pos_host_range_read(plain, 0, NRX, rows, MSD_RANGE_TAKE_LONGEST) == 0);
            CHECK(msd_pos_host_range_read(whole, 0, NRX, rows, 0) == 0);
            for (uint32_t x = 0; x < NRX; ++x)
                CHECK(rows[x].longest_m == 0 && memcmp(rows[x].polar_range, a->rows[x].polar_range, sizeof rows[x].polar_range) == 0);
        }
    }
    CHECK(evaluated > 10000);
    CHECK(msd_pos_host_reset(whole) == 0);
    observe(whole, a);
    for (uint32_t x = 0; x < NRX; ++x) {
        CHECK(a->rows[x].evaluated == 0 && a->rows[x].longest_m == 0);
        for (uint32_t bucket = 0; bucket < MSD_RANGE_BUCKETS; ++bucket)
            CHECK(a->rows[x].polar_range[bucket] == 0);
    }
    CHECK(a->live == 0 && isinf(a->margins.min_range_margin_m) && isinf(a->margins.min_bearing_margin_deg));
    free(a), free(b), free(m), free(f), free(r), free(out), free(out2);
    msd_pos_host_destroy(whole), msd_pos_host_destroy(cut), msd_pos_host_destroy(plain);
    printf("range_units: ok, %ld checks, %llu ranges evaluated\n", checks, (unsigned long long)evaluated);
    return 0;
}
