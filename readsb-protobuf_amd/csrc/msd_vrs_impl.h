/* msd_vrs_impl.h -- the text of readsb's Virtual Radar Server feed (generateVRS net_io.c:3230-3377, jsonEscapeString
 * :1786-1805), one implementation of an aircraft's JSON object for the writer's kernels (msd_vrs_kernels.hip: the length
 * kernel counts what the store kernel writes) and for a stand-alone host program that holds the arithmetic against glibc
 * (tests/c/vrs_units.c); modes_hip.h "VRS output" has the contract.
 * The host twin's writer (host/msd_pos_host.c) does NOT use this file: it prints with snprintf and the reference's own
 * format strings and is what the device is compared with.
 *
 * No printf and no libm here: every conversion is integer arithmetic, or one exact IEEE instruction, whose result is
 * glibc's byte for byte.
 *   %f, %.2f of a double   the exactly rounded decimal, msd_sbs_scale5 generalised to a factor of 10^2 or 10^6: mantissa x
 *                          factor in 128 bits, shifted by the exponent, the remainder compared with a half, ties to even on
 *                          the exact binary value; the sign is kept (-0.000000)
 *   %.0f of a double       rint under the default rounding mode: round half to even, one instruction
 *   %d, %u, %llu, %04x, %06X   digits stored from the last one backwards
 *   the ground track       msd_pb_heading (msd_pb_impl.h): the int32_t conversion aircraft.pb writes, the velocity's out of
 *                          the truncating table; no atan2 on the device */
#ifndef MSD_VRS_IMPL_H
#define MSD_VRS_IMPL_H

#include <math.h>
#include <string.h>

#include "msd_pb_impl.h"

#define MSD_VRS_HEAD_LEN 11u /* {"acList":[ */
#define MSD_VRS_TAIL_LEN 3u  /* ]}\n */

/* out == NULL counts */
typedef struct msd_vrs_w {
    uint8_t *out;
    uint32_t n;
} msd_vrs_w;

MSD_HD void msd_vrs_putc(msd_vrs_w *w, char c)
{
    if (w->out)
        w->out[w->n] = (uint8_t)c;
    w->n++;
}

/* a literal: a key with what stands in front of its value, e.g. `,"Alt":` */
MSD_HD void msd_vrs_puts(msd_vrs_w *w, const char *s)
{
    for (; *s; ++s)
        msd_vrs_putc(w, *s);
}

/* %llu / %0<width>u: the digits from the last one backwards, no array on a lane's stack */
MSD_HD void msd_vrs_put_u64(msd_vrs_w *w, uint64_t v, unsigned width)
{
    unsigned k = 1;
    for (uint64_t x = v; x >= 10u; x /= 10u)
        ++k;
    if (k < width)
        k = width;
    if (w->out)
        for (unsigned i = k; i-- > 0; v /= 10u)
            w->out[w->n + i] = (uint8_t)('0' + (unsigned)(v % 10u));
    w->n += k;
}

MSD_HD void msd_vrs_put_u32(msd_vrs_w *w, uint32_t v, unsigned width) /* %u: the same in 32-bit arithmetic */
{
    unsigned k = 1;
    for (uint32_t x = v; x >= 10u; x /= 10u)
        ++k;
    if (k < width)
        k = width;
    if (w->out)
        for (unsigned i = k; i-- > 0; v /= 10u)
            w->out[w->n + i] = (uint8_t)('0' + v % 10u);
    w->n += k;
}

MSD_HD void msd_vrs_put_int(msd_vrs_w *w, int32_t v) /* %d */
{
    uint32_t u = (uint32_t)v;
    if (v < 0) {
        msd_vrs_putc(w, '-');
        u = 0u - u;
    }
    msd_vrs_put_u32(w, u, 0);
}

MSD_HD void msd_vrs_put_hex(msd_vrs_w *w, uint32_t v, unsigned digits, int upper) /* %0<digits>X / x of a value that fits */
{
    for (unsigned i = digits; i-- > 0;) {
        const unsigned h = (v >> (4u * i)) & 15u;
        msd_vrs_putc(w, (char)(h < 10 ? '0' + h : (upper ? 'A' : 'a') + (h - 10)));
    }
}

/* |x| x factor rounded to an integer, ties to even on the exact binary value, for a factor of at most 10^6 < 2^20 and a
 * finite |x| below 2^43:  x = m 2^-s with m < 2^53, so s >= 10; m x factor < 2^73 is kept in two words hi:lo with
 * hi < 2^9, the shift by s drops the fraction, which is compared with a half; the quotient is below 2^63.
 * The 128-bit arithmetic alone would hold |x| < 2^57 for a factor of 100, 2^47 for 10^5 (msd_sbs_scale5 stops at 2^46) and
 * 2^44 for 10^6 -- where the quotient still fits 64 bits --; one bound serves all.  Beyond it, NaN and infinity: 0; callers
 * keep such values away (msd_vrs_coord_printable, the range of nav_qnh_raw). */
MSD_HD uint64_t msd_vrs_scale(double x, uint32_t factor)
{
    uint64_t bits;
    memcpy(&bits, &x, sizeof bits);
    const unsigned ex = (unsigned)((bits >> 52) & 0x7FFu);
    uint64_t m = bits & 0xFFFFFFFFFFFFFull;
    unsigned s; /* x = m 2^-s */
    if (ex == 0) {
        s = 1074;
    } else {
        m |= 1ull << 52;
        s = 1075u - ex;
    }
    if (m == 0 || s >= 127u || ex > 1065u) /* below 2^-74 the product is under a half whatever the factor */
        return 0;
    /* hi:lo = m x factor */
    const uint64_t p0 = (m & 0xFFFFFFFFull) * factor, p1 = (m >> 32) * factor;
    const uint64_t lo = p0 + (p1 << 32);
    const uint64_t hi = (p1 >> 32) + (lo < p0 ? 1u : 0u);
    /* q = hi:lo >> s, the remainder against half = 2^(s - 1) */
    uint64_t q, rem_hi, rem_lo, half_hi, half_lo;
    if (s < 64) { /* 10 <= s: hi < 2^9 fits above lo's rest */
        q = (lo >> s) | (hi << (64 - s));
        rem_hi = 0;
        rem_lo = lo & ((1ull << s) - 1ull);
        half_hi = 0;
        half_lo = 1ull << (s - 1);
    } else if (s == 64) {
        q = hi;
        rem_hi = 0;
        rem_lo = lo;
        half_hi = 0;
        half_lo = 1ull << 63;
    } else { /* 65 <= s <= 126 */
        q = hi >> (s - 64);
        rem_hi = hi & ((1ull << (s - 64)) - 1ull);
        rem_lo = lo;
        half_hi = 1ull << (s - 65);
        half_lo = 0;
    }
    const int above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
    const int equal = rem_hi == half_hi && rem_lo == half_lo;
    if (above || (equal && (q & 1u)))
        ++q;
    return q;
}

/* %f (places = 6, factor = 10^6) and %.2f (2, 100) of a double with |x| < 2^32 */
MSD_HD void msd_vrs_put_fixed(msd_vrs_w *w, double x, unsigned places, uint32_t factor)
{
    uint64_t bits;
    memcpy(&bits, &x, sizeof bits);
    if (bits >> 63)
        msd_vrs_putc(w, '-');
    const uint64_t q = msd_vrs_scale(x, factor);
    msd_vrs_put_u32(w, (uint32_t)(q / factor), 0);
    msd_vrs_putc(w, '.');
    msd_vrs_put_u32(w, (uint32_t)(q % factor), places);
}

/* What the decoders deliver; anything else follows the rule modes_hip.h states, on the device and in the host object.
 * Sig: a value with the sign bit set (-0.0 and negative NaNs too), a NaN, or one at or above 2^32 is written as 0. */
MSD_HD int msd_vrs_sig_printable(double v)
{
    uint64_t bits;
    memcpy(&bits, &v, sizeof bits);
    return !(bits >> 63) && v < 4294967296.0;
}

MSD_HD double msd_vrs_sig(const double *s) /* net_io.c:3265-3267, summed in that order */
{
    return 255 * ((s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + s[6] + s[7] + 1e-5) / 8);
}

/* a latitude or longitude that is not finite or beyond +-360: the three position keys are left out */
MSD_HD int msd_vrs_coord_printable(double x)
{
    return fabs(x) <= 360.0;
}

/* what the position state holds of an aircraft (msd_pos_aircraft on the device, the exported entry's head in a test).
 * Named members, no arrays: a lane keeps the struct in registers */
typedef struct msd_vrs_head {
    uint64_t seen, messages;
    uint64_t gs_updated, ias_updated, tas_updated, position_updated;
    double lat, lon;
    uint32_t addr, gs, ias, tas;
    uint8_t gs_source, ias_source, tas_source, position_source;
    int8_t adsb_version;
} msd_vrs_head;

MSD_HD void msd_vrs_head_of_state(uint64_t key, const msd_pos_aircraft *p, msd_vrs_head *h)
{
    h->seen = p->seen;
    h->messages = p->messages;
    h->gs_updated = p->upd[MSD_PV_GS];
    h->ias_updated = p->upd[MSD_PV_IAS];
    h->tas_updated = p->upd[MSD_PV_TAS];
    h->position_updated = p->upd[MSD_PV_POSITION];
    h->lat = p->lat;
    h->lon = p->lon;
    h->addr = (uint32_t)(key & 0x1FFFFFFu);
    h->gs = p->gs;
    h->ias = p->ias;
    h->tas = p->tas;
    h->gs_source = p->src[MSD_PV_GS];
    h->ias_source = p->src[MSD_PV_IAS];
    h->tas_source = p->src[MSD_PV_TAS];
    h->position_source = p->src[MSD_PV_POSITION];
    h->adsb_version = p->version[0];
}

MSD_HD void msd_vrs_head_of_entry(const msd_aircraft *a, msd_vrs_head *h)
{
    h->seen = a->seen;
    h->messages = a->messages;
    h->gs_updated = a->updated[MSD_AC_GS];
    h->ias_updated = a->updated[MSD_AC_IAS];
    h->tas_updated = a->updated[MSD_AC_TAS];
    h->position_updated = a->updated[MSD_AC_POSITION];
    h->lat = a->lat;
    h->lon = a->lon;
    h->addr = a->addr & 0x1FFFFFFu;
    h->gs = a->gs;
    h->ias = a->ias;
    h->tas = a->tas;
    h->gs_source = a->source[MSD_AC_GS];
    h->ias_source = a->source[MSD_AC_IAS];
    h->tas_source = a->source[MSD_AC_TAS];
    h->position_source = a->source[MSD_AC_POSITION];
    h->adsb_version = a->adsb_version;
}

MSD_HD int msd_vrs_head_valid(unsigned source, uint64_t updated, uint64_t now) /* trackDataValid of gs, ias, tas, position */
{
    return source != 0 && now < updated + 70000u;
}

/* net_io.c:3246-3256 in integers: the aircraft is in the part (bucket addr % 2048, part_shift = 11 - log2(n_parts)) and
 * is written.  now - seen wraps as the reference's does: an aircraft seen after now_ms is not written */
MSD_HD int msd_vrs_selected(const msd_vrs_head *h, uint64_t now_ms, uint32_t part, uint32_t part_shift)
{
    return ((h->addr & 2047u) >> part_shift) == part && h->messages >= 2u && !(h->addr & MSD_NON_ICAO_ADDRESS) &&
           now_ms - h->seen <= 5000u;
}

MSD_HD void msd_vrs_put_escaped(msd_vrs_w *w, const char *s, unsigned most) /* jsonEscapeString */
{
    for (unsigned i = 0; i < most && s[i] != 0; ++i) {
        const unsigned ch = (unsigned char)s[i];
        if (ch == '"' || ch == '\\') {
            msd_vrs_putc(w, '\\');
            msd_vrs_putc(w, (char)ch);
        } else if (ch < 32 || ch > 127) {
            msd_vrs_putc(w, '\\');
            msd_vrs_putc(w, 'u');
            msd_vrs_put_hex(w, ch, 4, 0);
        } else {
            msd_vrs_putc(w, (char)ch);
        }
    }
}

MSD_HD void msd_vrs_put_bool(msd_vrs_w *w, int v)
{
    msd_vrs_puts(w, v ? "true" : "false");
}

/* One aircraft's object at now_ms, with a comma in front of it when `comma` -> its length (at most
 * MSD_VRS_AIRCRAFT_MAX).  out == NULL: the length alone. */
MSD_HD uint32_t msd_vrs_aircraft(const msd_vrs_head *h, const msd_trk_aircraft *t, uint64_t now, int comma,
                                 const uint16_t *track_table, uint8_t *out)
{
    msd_vrs_w w;
    w.out = out;
    w.n = 0;
    if (comma)
        msd_vrs_putc(&w, ',');
    msd_vrs_puts(&w, "{\"Sig\":");
    {
        const double v = msd_vrs_sig(t->signal_level);
        msd_vrs_put_u64(&w, msd_vrs_sig_printable(v) ? (uint64_t)rint(v) : 0u, 0);
    }
    msd_vrs_puts(&w, ",\"Icao\":\"");
    msd_vrs_put_hex(&w, h->addr & 0xFFFFFFu, 6, 1);
    msd_vrs_putc(&w, '"');
    if (msd_trk_valid(t, MSD_AC_ALTITUDE_BARO, now) && t->altitude_baro_reliable >= 3) {
        msd_vrs_puts(&w, ",\"Alt\":");
        msd_vrs_put_int(&w, t->alt_baro);
    }
    if (msd_trk_valid(t, MSD_AC_ALTITUDE_GEOM, now)) {
        msd_vrs_puts(&w, ",\"GAlt\":");
        msd_vrs_put_int(&w, t->alt_geom);
    }
    if (msd_trk_valid(t, MSD_AC_NAV_QNH, now)) {
        const float qnh = t->nav_qnh_commb ? (float)(800 + t->nav_qnh_raw * 0.1) : (float)(800.0 + (t->nav_qnh_raw - 1) * 0.8);
        msd_vrs_puts(&w, ",\"InHg\":");
        msd_vrs_put_fixed(&w, qnh * 0.02952998307, 2, 100u);
    }
    if (msd_trk_valid(t, MSD_AC_NAV_ALTITUDE_MCP, now)) {
        msd_vrs_puts(&w, ",\"TAlt\":");
        msd_vrs_put_int(&w, t->nav_altitude_mcp);
    } else if (msd_trk_valid(t, MSD_AC_NAV_ALTITUDE_FMS, now)) {
        msd_vrs_puts(&w, ",\"TAlt\":");
        msd_vrs_put_int(&w, t->nav_altitude_fms);
    }
    if (msd_trk_valid(t, MSD_AC_CALLSIGN, now)) {
        msd_vrs_puts(&w, ",\"Call\":\"");
        msd_vrs_put_escaped(&w, t->callsign, 8);
        msd_vrs_putc(&w, '"');
    }
    if (msd_vrs_head_valid(h->position_source, h->position_updated, now) && msd_vrs_coord_printable(h->lat) && msd_vrs_coord_printable(h->lon)) {
        msd_vrs_puts(&w, ",\"Lat\":");
        msd_vrs_put_fixed(&w, h->lat, 6, 1000000u);
        msd_vrs_puts(&w, ",\"Long\":");
        msd_vrs_put_fixed(&w, h->lon, 6, 1000000u);
        msd_vrs_puts(&w, ",\"PosTime\":");
        msd_vrs_put_u64(&w, h->position_updated, 0);
    }
    msd_vrs_puts(&w, ",\"Mlat\":");
    msd_vrs_put_bool(&w, h->position_source == 2u /* SOURCE_MLAT */);
    msd_vrs_puts(&w, ",\"Tisb\":");
    msd_vrs_put_bool(&w, h->position_source == 5u /* SOURCE_TISB */);
    if (msd_vrs_head_valid(h->gs_source, h->gs_updated, now)) {
        msd_vrs_puts(&w, ",\"Spd\":");
        msd_vrs_put_int(&w, (int32_t)h->gs); /* %d of a uint32_t */
        msd_vrs_puts(&w, ",\"SpdTyp\":0");
    } else if (msd_vrs_head_valid(h->ias_source, h->ias_updated, now)) {
        msd_vrs_puts(&w, ",\"Spd\":");
        msd_vrs_put_u32(&w, h->ias, 0);
        msd_vrs_puts(&w, ",\"SpdTyp\":2");
    } else if (msd_vrs_head_valid(h->tas_source, h->tas_updated, now)) {
        msd_vrs_puts(&w, ",\"Spd\":");
        msd_vrs_put_u32(&w, h->tas, 0);
        msd_vrs_puts(&w, ",\"SpdTyp\":3");
    }
    {
        const msd_aircraft_heading *hd = 0;
        int heading = 1;
        if (msd_trk_valid(t, MSD_AC_TRACK, now)) {
            hd = &t->track;
            heading = 0;
        } else if (msd_trk_valid(t, MSD_AC_MAG_HEADING, now)) {
            hd = &t->mag_heading;
        } else if (msd_trk_valid(t, MSD_AC_TRUE_HEADING, now)) {
            hd = &t->true_heading;
        }
        if (hd) {
            msd_vrs_puts(&w, ",\"Trak\":");
            msd_vrs_put_int(&w, msd_pb_heading(hd, track_table));
            msd_vrs_puts(&w, ",\"TrkH\":");
            msd_vrs_put_bool(&w, heading);
        }
    }
    if (msd_trk_valid(t, MSD_AC_NAV_HEADING, now)) {
        msd_vrs_puts(&w, ",\"TTrk\":");
        msd_vrs_put_int(&w, (int32_t)(t->nav_heading_v2 ? (float)(t->nav_heading_raw * 180.0 / 256.0) : (float)t->nav_heading_raw));
    }
    if (msd_trk_valid(t, MSD_AC_SQUAWK, now)) {
        msd_vrs_puts(&w, ",\"Sqk\":\"");
        msd_vrs_put_hex(&w, t->squawk, 4, 0);
        msd_vrs_putc(&w, '"');
    }
    if (msd_trk_valid(t, MSD_AC_GEOM_RATE, now)) {
        msd_vrs_puts(&w, ",\"Vsi\":");
        msd_vrs_put_int(&w, t->geom_rate);
        msd_vrs_puts(&w, ",\"VsiT\":1");
    } else if (msd_trk_valid(t, MSD_AC_BARO_RATE, now)) {
        msd_vrs_puts(&w, ",\"Vsi\":");
        msd_vrs_put_int(&w, t->baro_rate);
        msd_vrs_puts(&w, ",\"VsiT\":0");
    }
    msd_vrs_puts(&w, ",\"Gnd\":");
    msd_vrs_put_bool(&w, msd_trk_valid(t, MSD_AC_AIRGROUND, now) && t->source[MSD_AC_AIRGROUND] >= 4u /* SOURCE_MODE_S_CHECKED */ &&
                             t->air_ground == 1u /* AG_GROUND */);
    msd_vrs_puts(&w, ",\"Trt\":");
    msd_vrs_put_int(&w, h->adsb_version >= 0 ? h->adsb_version + 3 : 1);
    msd_vrs_puts(&w, ",\"Cmsgs\":");
    msd_vrs_put_u64(&w, h->messages, 0);
    msd_vrs_putc(&w, '}');
    return w.n;
}

MSD_HD uint32_t msd_vrs_head_text(uint8_t *out) /* {"acList":[ */
{
    msd_vrs_w w;
    w.out = out;
    w.n = 0;
    msd_vrs_puts(&w, "{\"acList\":[");
    return w.n;
}

MSD_HD uint32_t msd_vrs_tail_text(uint8_t *out) /* ]}\n */
{
    msd_vrs_w w;
    w.out = out;
    w.n = 0;
    msd_vrs_puts(&w, "]}\n");
    return w.n;
}

/* what msd_pos_vrs accepts -> 11 - log2(n_parts), or -1 */
MSD_HD int msd_vrs_part_shift(const msd_vrs_options *opt)
{
    if (!opt || opt->flags != 0 || opt->reserved != 0)
        return -1;
    const uint32_t n = opt->n_parts;
    if (n == 0 || n > 2048u || (n & (n - 1u)) != 0 || opt->part >= n)
        return -1;
    int shift = 11;
    for (uint32_t x = n; x > 1u; x >>= 1)
        --shift;
    return shift;
}

#endif
