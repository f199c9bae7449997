/* msd_pb_impl.h -- the bytes of readsb's aircraft.pb (the AircraftsUpdate message of readsb.proto as protobuf-c 1.3's
 * aircrafts_update__pack writes it, generateAircraftProtoBuf net_io.c:1977-2080), one implementation for the writer's two
 * kernels (msd_pb_kernels.hip: the length kernel counts what the store kernel writes) and for a stand-alone host program
 * (tests/c/pb_units.c); modes_hip.h "aircraft.pb" has the contract.
 * The host twin's writer (host/msd_pos_host.c) does NOT use this file: it is a plain sequential encoder of its own and is
 * what the device is compared with.
 *
 * Every value is a varint or a bit copy of a float or a double.  The floats are msd_aircraft_to_float's expressions --
 * IEEE multiply, divide and add on doubles, narrowed once; compile with contraction off --, the velocity's ground track
 * comes out of a table made with the host's libm (msd_pb_build_track_table), and rssi's log10 is the one libm call, the
 * device library's on the device (DESIGN.md 4.10 has its margin). */
#ifndef MSD_PB_IMPL_H
#define MSD_PB_IMPL_H

#include <math.h>

#include "msd_trk_impl.h"

#define MSD_PB_TRACK_MAG 1023u /* magnitudes 0 .. 1022: ew_raw - 1, ns_raw - 1 (mode_s.c:823-828) */
#define MSD_PB_TRACK_ENTRIES (4u * MSD_PB_TRACK_MAG * MSD_PB_TRACK_MAG)
#define MSD_PB_HEADER_MAX 22u  /* `now` and `messages`: a tag and a varint of at most 10 bytes each */
/* the written state of a slot: the last seen_pos in the low word, the attached bits above it */
#define MSD_PB_FLIGHT_ATTACHED ((uint64_t)1 << 32)
#define MSD_PB_NAV_MODES_ATTACHED ((uint64_t)1 << 33)

/* out == NULL counts */
typedef struct msd_pb_w {
    uint8_t *out;
    uint32_t n;
} msd_pb_w;

MSD_HD void msd_pb_byte(msd_pb_w *w, uint32_t b)
{
    if (w->out)
        w->out[w->n] = (uint8_t)b;
    w->n++;
}

MSD_HD void msd_pb_varint(msd_pb_w *w, uint64_t v)
{
    while (v >= 128u) {
        msd_pb_byte(w, (uint32_t)(v & 127u) | 128u);
        v >>= 7;
    }
    msd_pb_byte(w, (uint32_t)v);
}

MSD_HD void msd_pb_tag(msd_pb_w *w, uint32_t field, uint32_t wire_type)
{
    msd_pb_varint(w, (uint64_t)(field << 3 | wire_type));
}

/* proto3 scalars: nothing for a zero */
MSD_HD void msd_pb_uint(msd_pb_w *w, uint32_t field, uint64_t v)
{
    if (v) {
        msd_pb_tag(w, field, 0);
        msd_pb_varint(w, v);
    }
}

MSD_HD void msd_pb_int32(msd_pb_w *w, uint32_t field, int32_t v) /* int32 and enums: a negative value is sign-extended */
{
    msd_pb_uint(w, field, (uint64_t)(int64_t)v);
}

MSD_HD void msd_pb_fixed(msd_pb_w *w, uint64_t bits, unsigned nbytes)
{
    for (unsigned i = 0; i < nbytes; ++i)
        msd_pb_byte(w, (uint32_t)(bits >> (8u * i)) & 255u);
}

MSD_HD void msd_pb_float(msd_pb_w *w, uint32_t field, float v)
{
    if (!(0 == v)) { /* field_is_zeroish: -0.0 goes, NaN stays */
        union { float f; uint32_t u; } b;
        b.f = v;
        msd_pb_tag(w, field, 5);
        msd_pb_fixed(w, b.u, 4);
    }
}

MSD_HD void msd_pb_double(msd_pb_w *w, uint32_t field, double v)
{
    if (!(0 == v)) {
        union { double f; uint64_t u; } b;
        b.f = v;
        msd_pb_tag(w, field, 1);
        msd_pb_fixed(w, b.u, 8);
    }
}

/* the index of a velocity's components in the ground-track table; -1: a pair no subtype 1 / 2 message carries.  An entry
 * keeps no subtype: components beyond 1022 are subtype 2's multiples of 4, whose angle is the quarter pair's */
MSD_HD int32_t msd_pb_track_index(int ew, int ns)
{
    unsigned a = (unsigned)(ew < 0 ? -ew : ew), b = (unsigned)(ns < 0 ? -ns : ns);
    if (a >= MSD_PB_TRACK_MAG || b >= MSD_PB_TRACK_MAG) {
        if ((a | b) & 3u)
            return -1;
        a >>= 2;
        b >>= 2;
        if (a >= MSD_PB_TRACK_MAG || b >= MSD_PB_TRACK_MAG)
            return -1;
    }
    const unsigned sign = (ew < 0 ? 2u : 0u) | (ns < 0 ? 1u : 0u);
    return (int32_t)((sign * MSD_PB_TRACK_MAG + a) * MSD_PB_TRACK_MAG + b);
}

/* a->meta.track = mm->heading and its kin: the float of msd_aircraft_to_float converted to int32_t */
MSD_HD int32_t msd_pb_heading(const msd_aircraft_heading *h, const uint16_t *track_table)
{
    const unsigned raw = h->raw;
    switch (h->kind) {
    case MSD_HDG_COMMB: {
        float v = (float)((raw & 1023u) * 90.0 / 512.0);
        if (raw & 1024u)
            v = (float)(v + 180.0);
        return (int32_t)v;
    }
    case MSD_HDG_ES19:
        return (int32_t)(float)(raw * 360.0 / 1024.0);
    case MSD_HDG_SURFACE:
        return (int32_t)(float)(raw * 360.0 / 128.0);
    case MSD_HDG_VELOCITY: {
        const int32_t k = msd_pb_track_index(h->ew, h->ns);
        return k < 0 ? 0 : (int32_t)track_table[k];
    }
    default:
        return 0;
    }
}

/* what the position state holds of an aircraft (msd_pos_aircraft on the device, the exported entry's head in a test) */
typedef struct msd_pb_head {
    uint64_t seen, messages, position_updated;
    double lat, lon;
    uint32_t addr, gs, ias, tas;
    uint8_t gs_source, ias_source, tas_source, position_source;
    int8_t adsb_version;
    uint32_t distance; /* a->meta.distance of a tracker that keeps the receiver range; 0 of any other: whoever has one sets it */
} msd_pb_head;

MSD_HD void msd_pb_head_of_state(uint64_t key, const msd_pos_aircraft *p, msd_pb_head *h)
{
    h->seen = p->seen;
    h->messages = p->messages;
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
    h->distance = 0;
}

MSD_HD void msd_pb_head_of_entry(const msd_aircraft *a, msd_pb_head *h)
{
    h->seen = a->seen;
    h->messages = a->messages;
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
    h->distance = 0;
}

/* net_io.c:2011 in integers: the aircraft is written */
MSD_HD int msd_pb_selected(const msd_pb_head *h, uint64_t now_ms)
{
    return h->messages >= 2u && !(now_ms > h->seen && now_ms - h->seen > 90000u);
}

MSD_HD int msd_pb_position_valid(const msd_pb_head *h, uint64_t now_ms)
{
    return h->position_source != 0 && now_ms < h->position_updated + 70000u;
}

/* the written state after a write at now_ms (net_io.c:2025-2034): t's callsign and nav_modes validities, h's position */
MSD_HD uint64_t msd_pb_next_state(uint64_t state, const msd_pb_head *h, const msd_trk_aircraft *t, uint64_t now_ms)
{
    if (t->source[MSD_AC_CALLSIGN] != 0 && now_ms < t->updated[MSD_AC_CALLSIGN] + 70000u)
        state |= MSD_PB_FLIGHT_ATTACHED;
    if (t->source[MSD_AC_NAV_MODES] != 0 && now_ms < t->updated[MSD_AC_NAV_MODES] + 70000u)
        state |= MSD_PB_NAV_MODES_ATTACHED;
    if (msd_pb_position_valid(h, now_ms)) {
        const uint64_t s = (now_ms - h->position_updated) / 1000u; /* the wrapped difference, saturated */
        state = (state & ~(uint64_t)0xFFFFFFFFu) | (s > 0xFFFFFFFFu ? 0xFFFFFFFFu : s);
    }
    return state;
}

MSD_HD float msd_pb_rssi(const msd_trk_aircraft *t) /* net_io.c:2052 */
{
    const double *s = t->signal_level;
    return (float)(10 * log10((s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + s[6] + s[7] + 1e-5) / 8));
}

MSD_HD void msd_pb_source(msd_pb_w *w, uint32_t field, const msd_trk_aircraft *t, int member)
{
    msd_pb_uint(w, field, t->source[member]);
}

/* ValidSource's members (generateValidSourceMessage, net_io.c:1896-1929); `wind` (132) is not written */
MSD_HD void msd_pb_valid_source(msd_pb_w *w, const msd_pb_head *h, const msd_trk_aircraft *t)
{
    msd_pb_source(w, 100, t, MSD_AC_CALLSIGN);
    msd_pb_source(w, 101, t, MSD_AC_ALTITUDE_BARO);
    msd_pb_source(w, 102, t, MSD_AC_ALTITUDE_GEOM);
    msd_pb_uint(w, 103, h->gs_source);
    msd_pb_uint(w, 104, h->ias_source);
    msd_pb_uint(w, 105, h->tas_source);
    msd_pb_source(w, 106, t, MSD_AC_MACH);
    msd_pb_source(w, 107, t, MSD_AC_TRACK);
    msd_pb_source(w, 108, t, MSD_AC_TRACK_RATE);
    msd_pb_source(w, 109, t, MSD_AC_ROLL);
    msd_pb_source(w, 110, t, MSD_AC_MAG_HEADING);
    msd_pb_source(w, 111, t, MSD_AC_TRUE_HEADING);
    msd_pb_source(w, 112, t, MSD_AC_BARO_RATE);
    msd_pb_source(w, 113, t, MSD_AC_GEOM_RATE);
    msd_pb_source(w, 114, t, MSD_AC_SQUAWK);
    msd_pb_source(w, 115, t, MSD_AC_EMERGENCY);
    msd_pb_source(w, 116, t, MSD_AC_NAV_QNH);
    msd_pb_source(w, 117, t, MSD_AC_NAV_ALTITUDE_MCP);
    msd_pb_source(w, 118, t, MSD_AC_NAV_ALTITUDE_FMS);
    msd_pb_source(w, 119, t, MSD_AC_NAV_HEADING);
    msd_pb_source(w, 120, t, MSD_AC_NAV_MODES);
    for (uint32_t field = 121; field <= 124; ++field) /* lat, lon, nic, rc */
        msd_pb_uint(w, field, h->position_source);
    msd_pb_source(w, 125, t, MSD_AC_NIC_BARO);
    msd_pb_source(w, 126, t, MSD_AC_NAC_P);
    msd_pb_source(w, 127, t, MSD_AC_NAC_V);
    msd_pb_source(w, 128, t, MSD_AC_SIL);
    msd_pb_source(w, 129, t, MSD_AC_SIL); /* sil_type */
    msd_pb_source(w, 130, t, MSD_AC_GVA);
    msd_pb_source(w, 131, t, MSD_AC_SDA);
}

MSD_HD int msd_pb_member_set(const msd_trk_aircraft *t, int member) /* msd_aircraft_to_float's "was ever set" */
{
    return t->updated[member] != 0 || t->source[member] != 0;
}

/* AircraftMeta's body in ascending field number; `state` is the written state after this write */
MSD_HD void msd_pb_body(msd_pb_w *w, const msd_pb_head *h, const msd_trk_aircraft *t, uint64_t state, const uint16_t *track_table)
{
    msd_pb_uint(w, 1, h->addr);
    if (state & MSD_PB_FLIGHT_ATTACHED) {
        uint32_t k = 0;
        while (k < 8 && t->callsign[k] != 0)
            ++k;
        if (k) {
            msd_pb_tag(w, 2, 2);
            msd_pb_byte(w, k);
            for (uint32_t i = 0; i < k; ++i)
                msd_pb_byte(w, (uint8_t)t->callsign[i]);
        }
    }
    msd_pb_uint(w, 3, t->squawk);
    msd_pb_uint(w, 4, t->category);
    msd_pb_int32(w, 5, t->alt_baro);
    msd_pb_int32(w, 6, msd_pb_heading(&t->mag_heading, track_table));
    msd_pb_uint(w, 7, h->ias);
    msd_pb_double(w, 8, h->lat);
    msd_pb_double(w, 9, h->lon);
    msd_pb_uint(w, 10, h->messages);
    msd_pb_uint(w, 11, h->seen);
    msd_pb_float(w, 12, msd_pb_rssi(t));
    msd_pb_uint(w, 13, h->distance);
    msd_pb_int32(w, 15, t->air_ground);
    msd_pb_int32(w, 20, t->alt_geom);
    msd_pb_int32(w, 21, t->baro_rate);
    msd_pb_int32(w, 22, t->geom_rate);
    msd_pb_uint(w, 23, h->gs);
    msd_pb_uint(w, 24, h->tas);
    if (msd_pb_member_set(t, MSD_AC_MACH))
        msd_pb_float(w, 25, (float)(t->mach_raw * 2.048 / 512));
    msd_pb_int32(w, 26, msd_pb_heading(&t->true_heading, track_table));
    msd_pb_int32(w, 27, msd_pb_heading(&t->track, track_table));
    if (msd_pb_member_set(t, MSD_AC_TRACK_RATE)) {
        float r = (float)((unsigned)(t->track_rate_q & 511) * 8.0 / 256.0);
        if (t->track_rate_q < 0)
            r = r - 16;
        msd_pb_float(w, 28, r);
    }
    if (msd_pb_member_set(t, MSD_AC_ROLL)) {
        float roll = (float)((unsigned)(t->roll_q & 511) * 45.0 / 256.0);
        if (t->roll_q < 0)
            roll = (float)(roll - 90.0);
        msd_pb_float(w, 29, roll);
    }
    if (msd_pb_member_set(t, MSD_AC_NAV_QNH))
        msd_pb_float(w, 30, t->nav_qnh_commb ? (float)(800 + t->nav_qnh_raw * 0.1) : (float)(800.0 + (t->nav_qnh_raw - 1) * 0.8));
    msd_pb_int32(w, 31, t->nav_altitude_mcp);
    msd_pb_int32(w, 32, t->nav_altitude_fms);
    if (msd_pb_member_set(t, MSD_AC_NAV_HEADING))
        msd_pb_int32(w, 33, (int32_t)(t->nav_heading_v2 ? (float)(t->nav_heading_raw * 180.0 / 256.0) : (float)t->nav_heading_raw));
    msd_pb_uint(w, 34, t->nic);
    msd_pb_uint(w, 35, t->rc);
    msd_pb_int32(w, 36, h->adsb_version >= 0 ? h->adsb_version : 0);
    msd_pb_uint(w, 37, t->nic_baro);
    msd_pb_uint(w, 38, t->nac_p);
    msd_pb_uint(w, 39, t->nac_v);
    msd_pb_uint(w, 40, t->sil);
    msd_pb_uint(w, 41, state & 0xFFFFFFFFu);
    msd_pb_uint(w, 42, t->alert != 0);
    msd_pb_uint(w, 43, t->spi != 0);
    msd_pb_uint(w, 44, t->gva);
    msd_pb_uint(w, 45, t->sda);
    /* 46 declination, 47 wind_speed, 48 wind_direction: not written */
    msd_pb_int32(w, 100, t->addr_type);
    msd_pb_int32(w, 101, t->emergency);
    msd_pb_int32(w, 102, t->sil_type);
    if (state & MSD_PB_NAV_MODES_ATTACHED) { /* a set pointer: written even when empty */
        uint32_t k = 0;
        for (uint32_t b = 0; b < 6; ++b)
            k += (t->nav_modes >> b) & 1u;
        msd_pb_tag(w, 150, 2);
        msd_pb_byte(w, 2u * k);
        for (uint32_t b = 0; b < 6; ++b)
            msd_pb_uint(w, b + 1u, (t->nav_modes >> b) & 1u);
    }
    {
        msd_pb_w c = {0, 0};
        msd_pb_valid_source(&c, h, t);
        msd_pb_tag(w, 151, 2);
        msd_pb_varint(w, c.n);
        msd_pb_valid_source(w, h, t);
    }
}

/* One `aircraft` (15) entry of AircraftsUpdate: tag, length, body -> its length.  out == NULL: the length alone. */
MSD_HD uint32_t msd_pb_aircraft(const msd_pb_head *h, const msd_trk_aircraft *t, uint64_t state, const uint16_t *track_table,
                                uint8_t *out)
{
    msd_pb_w c = {0, 0}, w = {out, 0};
    msd_pb_body(&c, h, t, state, track_table);
    msd_pb_byte(&w, 0x7A);
    msd_pb_varint(&w, c.n);
    if (!out)
        return w.n + c.n;
    msd_pb_body(&w, h, t, state, track_table);
    return w.n;
}

/* One entry of Statistics.polar_range (modes_hip.h "Receiver range", msd_pos_range_pb): tag 0x32, length, key and value,
 * either left out when 0 -> its length, at most MSD_RANGE_PB_ENTRY_MAX.  out == NULL: the length alone. */
MSD_HD uint32_t msd_range_pb_entry(uint32_t bucket, uint32_t metres, uint8_t *out)
{
    msd_pb_w c = {0, 0}, w = {out, 0};
    msd_pb_uint(&c, 1, bucket);
    msd_pb_uint(&c, 2, metres);
    msd_pb_byte(&w, 0x32);
    msd_pb_byte(&w, c.n); /* at most 8 */
    msd_pb_uint(&w, 1, bucket);
    msd_pb_uint(&w, 2, metres);
    return w.n;
}

/* a file's head: `now` (1) and `messages` (2) */
MSD_HD uint32_t msd_pb_header(uint64_t now_ms, uint64_t messages_total, uint8_t *out)
{
    msd_pb_w w = {out, 0};
    msd_pb_uint(&w, 1, now_ms / 1000u);
    msd_pb_uint(&w, 2, messages_total);
    return w.n;
}

/* what msd_pos_aircraft_pb accepts */
MSD_HD int msd_pb_options_ok(const msd_pb_options *opt)
{
    return opt && opt->flags == 0 && opt->reserved == 0;
}

/* Host only.  The velocity's ground track (mode_s.c:835-839) as the conversion to int32_t leaves it in meta.track, for
 * every sign pair and magnitude pair: MSD_PB_TRACK_ENTRIES entries, index msd_pb_track_index.  msd_sbs_build_track_table's
 * shape with the truncation in place of rintf. */
static inline void msd_pb_build_track_table(uint16_t *table)
{
    for (unsigned sign = 0; sign < 4; ++sign)
        for (unsigned a = 0; a < MSD_PB_TRACK_MAG; ++a)
            for (unsigned b = 0; b < MSD_PB_TRACK_MAG; ++b) {
                const int ew = (sign & 2u) ? -(int)a : (int)a, ns = (sign & 1u) ? -(int)b : (int)b;
                float ground_track = (float)(atan2(ew, ns) * 180.0 / MSD_POS_PI);
                if (ground_track < 0)
                    ground_track += 360;
                table[(sign * MSD_PB_TRACK_MAG + a) * MSD_PB_TRACK_MAG + b] = (uint16_t)(int32_t)ground_track;
            }
}

#endif
