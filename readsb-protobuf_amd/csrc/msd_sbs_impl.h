/* msd_sbs_impl.h -- the text of readsb's SBS (BaseStation) output, one implementation for the writer's two kernels
 * (msd_sbs_kernels.hip: the length kernel counts what the store kernel writes) and for a stand-alone host program that
 * holds the arithmetic against glibc (tests/c/sbs_units.c).  Restated from net_io.c: modesSendSBSOutput :1038-1241, the
 * conditions around it :1266-1270, mode_s.c:2164-2172; modes_hip.h "SBS output" has the contract.
 * The host twin's writer (host/msd_pos_host.c) does NOT use this file's number or date code: it prints with snprintf and
 * gmtime_r and is what the device is compared with.
 *
 * No printf here: every conversion is integer arithmetic whose result is glibc's byte for byte.
 *   %1.5f of a double   the exactly rounded decimal: mantissa x 100000 in 128 bits, shifted by the exponent, the
 *                       remainder compared with half, ties to even; the sign is kept (-0.00000)
 *   %.0f of a float     rintf: round half to even, one exact instruction
 *   the ground track    looked up: float(atan2(ew, ns) * 180 / pi) is the host libm's, evaluated once per argument pair
 *                       by msd_sbs_build_track_table; no atan2 on the device
 *   dates               days -> civil date by the era / year-of-era division (proleptic Gregorian), no leap seconds */
#ifndef MSD_SBS_IMPL_H
#define MSD_SBS_IMPL_H

#include <math.h>
#include <string.h>

#include "msd_pos_impl.h"

#define MSD_SBS_FLAGS (MSD_WIRE_VERBATIM | MSD_SBS_NET_ONLY | MSD_SBS_GNSS | MSD_SBS_NOW_IS_RECEIVED)
#define MSD_SBS_YEAR_10000_MS 253402300800000ll
#define MSD_SBS_TRACK_MAG 1023u /* magnitudes 0 .. 1022: ew_raw - 1, ns_raw - 1 (mode_s.c:823-828) */
#define MSD_SBS_TRACK_ENTRIES (4u * MSD_SBS_TRACK_MAG * MSD_SBS_TRACK_MAG)

/* out == NULL counts */
typedef struct msd_sbs_w {
    uint8_t *out;
    uint32_t n;
} msd_sbs_w;

MSD_HD void msd_sbs_putc(msd_sbs_w *w, char c)
{
    if (w->out)
        w->out[w->n] = (uint8_t)c;
    w->n++;
}

/* %0<width>u / %u */
MSD_HD void msd_sbs_put_uint(msd_sbs_w *w, uint32_t v, unsigned width)
{
    unsigned k = 1; /* digits; they are stored from the last one backwards: no array on a lane's stack */
    for (uint32_t x = v; x >= 10u; x /= 10u)
        ++k;
    if (k < width)
        k = width;
    if (w->out)
        for (unsigned i = k; i-- > 0; v /= 10u)
            w->out[w->n + i] = (uint8_t)('0' + v % 10u);
    w->n += k;
}

MSD_HD void msd_sbs_put_int(msd_sbs_w *w, int32_t v) /* %d */
{
    uint32_t u = (uint32_t)v;
    if (v < 0) {
        msd_sbs_putc(w, '-');
        u = 0u - u;
    }
    msd_sbs_put_uint(w, u, 0);
}

MSD_HD void msd_sbs_put_hex(msd_sbs_w *w, uint32_t v, unsigned digits, int upper) /* %0<digits>X / x of a value that fits */
{
    for (unsigned i = digits; i-- > 0;) {
        const unsigned h = (v >> (4u * i)) & 15u;
        msd_sbs_putc(w, (char)(h < 10 ? '0' + h : (upper ? 'A' : 'a') + (h - 10)));
    }
}

/* |x| x 100000 rounded to an integer, ties to even on the exact binary value, for a finite |x| below 2^46:
 * x = m 2^e with e <= -7; m x 100000 has at most 70 bits and is kept in two words, the shift by -e drops the fraction,
 * which is compared with a half */
MSD_HD uint64_t msd_sbs_scale5(double x)
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
    if (m == 0 || s >= 127u || ex > 1068u)
        return 0;
    /* hi:lo = m x 100000 */
    const uint64_t p0 = (m & 0xFFFFFFFFull) * 100000ull, p1 = (m >> 32) * 100000ull;
    const uint64_t lo = p0 + (p1 << 32);
    const uint64_t hi = (p1 >> 32) + (lo < p0 ? 1u : 0u);
    /* q = hi:lo >> s, the remainder against half = 2^(s - 1) */
    uint64_t q, rem_hi, rem_lo, half_hi, half_lo;
    if (s < 64) { /* 7 <= s: hi < 2^6 fits above lo's rest */
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

MSD_HD void msd_sbs_put_f5(msd_sbs_w *w, double x) /* %1.5f */
{
    uint64_t bits;
    memcpy(&bits, &x, sizeof bits);
    if (bits >> 63)
        msd_sbs_putc(w, '-');
    const uint64_t q = msd_sbs_scale5(x);
    msd_sbs_put_uint(w, (uint32_t)(q / 100000u), 0); /* callers keep |x| <= 360 */
    msd_sbs_putc(w, '.');
    msd_sbs_put_uint(w, (uint32_t)(q % 100000u), 5);
}

/* %.0f of a float in [0, 2^31): the integer printf writes */
MSD_HD uint32_t msd_sbs_round0(float x)
{
    return (uint32_t)rintf(x);
}

/* what the decoders deliver; anything else is printed as an empty field (modes_hip.h) */
MSD_HD int msd_sbs_gs_printable(float gs)
{
    uint32_t bits;
    memcpy(&bits, &gs, sizeof bits);
    return !(bits >> 31) && gs < 100000.0f;
}

MSD_HD int msd_sbs_coord_printable(double x)
{
    return fabs(x) <= 360.0;
}

/* POSIX milliseconds -> civil date and time; t >= 0 */
typedef struct msd_sbs_time {
    uint64_t year;
    unsigned month, day, hour, min, sec, ms;
} msd_sbs_time;

MSD_HD void msd_sbs_civil(uint64_t t, msd_sbs_time *o)
{
    const uint64_t days = t / 86400000ull;
    const unsigned rest = (unsigned)(t % 86400000ull);
    const uint64_t z = days + 719468u; /* from 0000-03-01 */
    const uint64_t era = z / 146097u;
    const unsigned doe = (unsigned)(z - era * 146097u);
    const unsigned yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    const unsigned doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
    const unsigned mp = (5u * doy + 2u) / 153u;
    o->day = doy - (153u * mp + 2u) / 5u + 1u;
    o->month = mp < 10u ? mp + 3u : mp - 9u;
    o->year = yoe + era * 400u + (o->month <= 2u ? 1u : 0u);
    o->hour = rest / 3600000u;
    o->min = rest / 60000u % 60u;
    o->sec = rest / 1000u % 60u;
    o->ms = rest % 1000u;
}

/* `%04d/%02d/%02d,%02d:%02d:%02d.%03u` of ms + offset: a negative sum as 0, the year modulo 10000 */
MSD_HD void msd_sbs_put_time(msd_sbs_w *w, uint64_t ms, int64_t utc_offset_ms)
{
    int64_t s = (int64_t)(ms + (uint64_t)utc_offset_ms);
    if (s < 0)
        s = 0;
    msd_sbs_time c;
    msd_sbs_civil((uint64_t)s, &c);
    msd_sbs_put_uint(w, (uint32_t)(c.year % 10000u), 4);
    msd_sbs_putc(w, '/');
    msd_sbs_put_uint(w, c.month, 2);
    msd_sbs_putc(w, '/');
    msd_sbs_put_uint(w, c.day, 2);
    msd_sbs_putc(w, ',');
    msd_sbs_put_uint(w, c.hour, 2);
    msd_sbs_putc(w, ':');
    msd_sbs_put_uint(w, c.min, 2);
    msd_sbs_putc(w, ':');
    msd_sbs_put_uint(w, c.sec, 2);
    msd_sbs_putc(w, '.');
    msd_sbs_put_uint(w, c.ms, 3);
}

MSD_HD int msd_sbs_options_ok(const msd_sbs_options *opt)
{
    if (!opt || (opt->flags & ~MSD_SBS_FLAGS) || opt->reserved != 0)
        return 0;
    const uint64_t limit = (uint64_t)MSD_SBS_YEAR_10000_MS; /* 0 <= now_ms + utc_offset_ms < limit, without wrapping */
    if (opt->utc_offset_ms >= 0)
        return opt->now_ms < limit && (uint64_t)opt->utc_offset_ms < limit - opt->now_ms;
    const uint64_t back = (uint64_t)0 - (uint64_t)opt->utc_offset_ms;
    return opt->now_ms >= back && opt->now_ms - back < limit;
}

/* the SBS message type, 0: the message writes nothing (net_io.c:1058-1096) */
MSD_HD unsigned msd_sbs_type(unsigned msgtype, unsigned metype)
{
    switch (msgtype) {
    case 4: case 20: return 5;
    case 5: case 21: return 6;
    case 0: case 16: return 7;
    case 11: return 8;
    case 17: case 18:
        if (metype >= 1 && metype <= 4) return 1;
        if (metype >= 5 && metype <= 8) return 2;
        if (metype >= 9 && metype <= 18) return 3;
        if (metype == 19) return 4;
        return 0;
    default: return 0;
    }
}

/* mode_s.c:2164-2172, net_io.c:1266 and :1043, and the type */
MSD_HD unsigned msd_sbs_delivered(const msd_message *m, const msd_fields *f, const msd_sbs_track *t, uint32_t flags)
{
    if (!(t->flags & MSD_SBS_TRACKED) || m->correctedbits >= 2 || (f->addr & MSD_NON_ICAO_ADDRESS))
        return 0;
    if (!(flags & (MSD_WIRE_VERBATIM | MSD_SBS_NET_ONLY)) && !(t->flags & MSD_SBS_SEEN_TWICE))
        return 0;
    return msd_sbs_type(m->msgtype, f->metype);
}

/* the index of a velocity's ground track in the table, -1: not what ES type 19 subtype 1 / 2 can carry */
MSD_HD int32_t msd_sbs_track_index(int ew, int ns, unsigned mesub)
{
    unsigned a = (unsigned)(ew < 0 ? -ew : ew), b = (unsigned)(ns < 0 ? -ns : ns);
    if (mesub == 2) {
        if ((a | b) & 3u)
            return -1;
        a >>= 2;
        b >>= 2;
    }
    if (a >= MSD_SBS_TRACK_MAG || b >= MSD_SBS_TRACK_MAG)
        return -1;
    const unsigned sign = (ew < 0 ? 2u : 0u) | (ns < 0 ? 1u : 0u);
    return (int32_t)((sign * MSD_SBS_TRACK_MAG + a) * MSD_SBS_TRACK_MAG + b);
}

/* mm->heading of a record whose own heading is valid and a ground track, as %.0f prints it; -1: field 14 stays empty.
 * msd_fields_to_float's order: the velocity's track where gs.selected > 0, then the raw heading's value in its place
 * (mode_s.c:835-853, :922, comm_b.c:485-490,623-628) */
MSD_HD int32_t msd_sbs_heading(const msd_fields *f, float gs_selected, const uint16_t *track_table)
{
    int valid = f->heading_valid;
    unsigned type = f->heading_type;
    int32_t v = -1;
    if (f->velocity_valid && gs_selected > 0) {
        const int32_t k = msd_sbs_track_index(f->ew_vel, f->ns_vel, f->mesub);
        if (k < 0)
            return -1;
        v = track_table[k];
        type = 1; /* HEADING_GROUND_TRACK */
        valid = 1;
    }
    if (f->heading_valid) {
        float h;
        if (f->commb_format == 8 || f->commb_format == 9) {
            h = (float)((f->heading_raw & 1023u) * 90.0 / 512.0);
            if (f->heading_raw & 1024u)
                h = (float)(h + 180.0);
        } else if (f->metype == 19) {
            h = (float)((f->heading_raw & 1023u) * 360.0 / 1024.0); /* the ten bits ME carries */
        } else {
            h = (float)((f->heading_raw & 127u) * 360.0 / 128.0); /* seven */
        }
        v = (int32_t)msd_sbs_round0(h);
    }
    return valid && type == 1 ? v : -1;
}

MSD_HD void msd_sbs_put_flag(msd_sbs_w *w, int valid, int set) /* `,-1` / `,0` / `,` */
{
    msd_sbs_putc(w, ',');
    if (valid) {
        if (set)
            msd_sbs_putc(w, '-');
        msd_sbs_putc(w, set ? '1' : '0');
    }
}

/* One record's line into out (MSD_SBS_MAX bytes at least; NULL: nothing is stored) -> its length, 0: no line. */
MSD_HD uint32_t msd_sbs_line(const msd_message *m, const msd_fields *f, const msd_sbs_track *t, uint32_t flags,
                             uint64_t now_ms, int64_t utc_offset_ms, const uint16_t *track_table, uint8_t *out)
{
    const unsigned type = msd_sbs_delivered(m, f, t, flags);
    if (!type)
        return 0;
    msd_sbs_w w;
    w.out = out;
    w.n = 0;
    const int gnss = (flags & MSD_SBS_GNSS) != 0;
    const int delta_valid = (t->flags & MSD_SBS_GEOM_DELTA_VALID) != 0;
    /* 1-6 */
    msd_sbs_putc(&w, 'M'), msd_sbs_putc(&w, 'S'), msd_sbs_putc(&w, 'G'), msd_sbs_putc(&w, ',');
    msd_sbs_putc(&w, (char)('0' + type));
    msd_sbs_putc(&w, ','), msd_sbs_putc(&w, '1'), msd_sbs_putc(&w, ','), msd_sbs_putc(&w, '1'), msd_sbs_putc(&w, ',');
    msd_sbs_put_hex(&w, f->addr & 0xFFFFFFu, 6, 1);
    msd_sbs_putc(&w, ','), msd_sbs_putc(&w, '1'), msd_sbs_putc(&w, ',');
    /* 7-10 */
    msd_sbs_put_time(&w, m->sysTimestampMsg, utc_offset_ms);
    msd_sbs_putc(&w, ',');
    msd_sbs_put_time(&w, (flags & MSD_SBS_NOW_IS_RECEIVED) ? m->sysTimestampMsg : now_ms, utc_offset_ms);
    /* 11: %s of the callsign */
    msd_sbs_putc(&w, ',');
    if (f->callsign_valid)
        for (int i = 0; i < 8 && f->callsign[i]; ++i)
            msd_sbs_putc(&w, f->callsign[i]);
    /* 12 */
    msd_sbs_putc(&w, ',');
    if (gnss) {
        if (f->altitude_geom_valid) {
            msd_sbs_put_int(&w, f->altitude_geom);
            msd_sbs_putc(&w, 'H');
        } else if (f->altitude_baro_valid && delta_valid) {
            msd_sbs_put_int(&w, (int32_t)((uint32_t)f->altitude_baro + (uint32_t)t->geom_delta));
            msd_sbs_putc(&w, 'H');
        } else if (f->altitude_baro_valid) {
            msd_sbs_put_int(&w, f->altitude_baro);
        }
    } else {
        if (f->altitude_baro_valid)
            msd_sbs_put_int(&w, f->altitude_baro);
        else if (f->altitude_geom_valid && delta_valid)
            msd_sbs_put_int(&w, (int32_t)((uint32_t)f->altitude_geom - (uint32_t)t->geom_delta));
    }
    /* 13 */
    msd_sbs_putc(&w, ',');
    if ((t->flags & MSD_SBS_GS_VALID) && msd_sbs_gs_printable(t->gs_selected))
        msd_sbs_put_uint(&w, msd_sbs_round0(t->gs_selected), 0);
    /* 14 */
    msd_sbs_putc(&w, ',');
    {
        const int32_t h = msd_sbs_heading(f, t->gs_selected, track_table);
        if (h >= 0)
            msd_sbs_put_uint(&w, (uint32_t)h, 0);
    }
    /* 15-16 */
    msd_sbs_putc(&w, ',');
    if ((t->flags & MSD_SBS_CPR_DECODED) && msd_sbs_coord_printable(t->lat) && msd_sbs_coord_printable(t->lon)) {
        msd_sbs_put_f5(&w, t->lat);
        msd_sbs_putc(&w, ',');
        msd_sbs_put_f5(&w, t->lon);
    } else {
        msd_sbs_putc(&w, ',');
    }
    /* 17 */
    msd_sbs_putc(&w, ',');
    if (gnss) {
        if (f->geom_rate_valid) {
            msd_sbs_put_int(&w, f->geom_rate);
            msd_sbs_putc(&w, 'H');
        } else if (f->baro_rate_valid) {
            msd_sbs_put_int(&w, f->baro_rate);
        }
    } else {
        if (f->baro_rate_valid)
            msd_sbs_put_int(&w, f->baro_rate);
        else if (f->geom_rate_valid)
            msd_sbs_put_int(&w, f->geom_rate);
    }
    /* 18 */
    msd_sbs_putc(&w, ',');
    if (f->squawk_valid)
        msd_sbs_put_hex(&w, f->squawk, 4, 0);
    /* 19-22 */
    msd_sbs_put_flag(&w, f->alert_valid, f->alert);
    msd_sbs_put_flag(&w, f->squawk_valid, f->squawk == 0x7500 || f->squawk == 0x7600 || f->squawk == 0x7700);
    msd_sbs_put_flag(&w, f->spi_valid, f->spi);
    msd_sbs_put_flag(&w, f->airground == 1 || f->airground == 2, f->airground == 1);
    msd_sbs_putc(&w, '\r');
    msd_sbs_putc(&w, '\n');
    return w.n;
}

/* Host only.  The velocity's ground track (mode_s.c:835-839) as %.0f prints it, for every sign pair and magnitude pair:
 * MSD_SBS_TRACK_ENTRIES entries, index msd_sbs_track_index.  rintf is what printf does to a float (tests/c/sbs_units.c
 * holds both against snprintf). */
static inline void msd_sbs_build_track_table(uint16_t *table)
{
    for (unsigned sign = 0; sign < 4; ++sign)
        for (unsigned a = 0; a < MSD_SBS_TRACK_MAG; ++a)
            for (unsigned b = 0; b < MSD_SBS_TRACK_MAG; ++b) {
                const int ew = (sign & 2u) ? -(int)a : (int)a, ns = (sign & 1u) ? -(int)b : (int)b;
                float ground_track = (float)(atan2(ew, ns) * 180.0 / MSD_POS_PI);
                if (ground_track < 0)
                    ground_track += 360;
                table[(sign * MSD_SBS_TRACK_MAG + a) * MSD_SBS_TRACK_MAG + b] = (uint16_t)rintf(ground_track);
            }
}

#endif
