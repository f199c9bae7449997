/* msd_history_impl.h -- the bytes of readsb's history_N.pb (the AircraftsUpdate message of readsb.proto with `history`
 * entries alone, as protobuf-c 1.3's aircrafts_update__pack writes what generateHistoryProtoBuf builds, net_io.c:2086-2177),
 * one implementation for the writer's two kernels (msd_history_kernels.hip: the length kernel counts what the store kernel
 * writes) and for a stand-alone host program (tests/c/history_units.c); modes_hip.h "history_N.pb" has the contract.
 * The host twin's writer (host/msd_pos_host.c) does NOT use this file: it is a plain sequential encoder of its own and is
 * what the device is compared with.
 *
 * Every value is a varint or a bit copy of a double: no float is computed, no libm function is called.  The primitives
 * are aircraft.pb's (msd_pb_impl.h); so are the two halves of the selection, msd_pb_selected and msd_pb_position_valid,
 * over the same msd_pb_head -- of which an entry needs seen, messages, the position with its validity and the address, and
 * a lane loads no more than those: the head is a local whose other members nobody reads. */
#ifndef MSD_HISTORY_IMPL_H
#define MSD_HISTORY_IMPL_H

#include "msd_pb_impl.h"

#define MSD_HISTORY_HEADER_MAX 11u /* `now`: a tag and a varint of at most 10 bytes */

/* net_io.c:2115-2124 in integers, at messageNow() = now_ms: aircraft.pb's rule, and the position is valid */
MSD_HD int msd_history_selected(const msd_pb_head *h, uint64_t now_ms)
{
    return msd_pb_selected(h, now_ms) && msd_pb_position_valid(h, now_ms);
}

/* what `alt_baro` (5) carries (net_io.c:2138-2146): INVALID_ALTITUDE on the ground, the barometric altitude while it is
 * reliable, else the geometric one, else nothing.  Of the table entry it reads, where they lie: airground's, altitude_baro's
 * and altitude_geom's source, the first two's `updated`, altitude_geom_expires, air_ground, altitude_baro_reliable and the
 * two altitudes */
MSD_HD int32_t msd_history_altitude(const msd_trk_aircraft *t, uint64_t now_ms)
{
    if (msd_trk_valid(t, MSD_AC_AIRGROUND, now_ms) && t->source[MSD_AC_AIRGROUND] >= 4 /* SOURCE_MODE_S_CHECKED */ &&
        t->air_ground == 1 /* AG_GROUND */)
        return -9999;
    if (msd_trk_valid(t, MSD_AC_ALTITUDE_BARO, now_ms) && t->altitude_baro_reliable >= 3)
        return t->alt_baro;
    if (msd_trk_valid(t, MSD_AC_ALTITUDE_GEOM, now_ms))
        return t->alt_geom;
    return 0;
}

/* AircraftHistory's body in ascending field number: addr (1), alt_baro (5), lat (8), lon (9) */
MSD_HD void msd_history_body(msd_pb_w *w, const msd_pb_head *h, int32_t altitude)
{
    msd_pb_uint(w, 1, h->addr);
    msd_pb_int32(w, 5, altitude);
    msd_pb_double(w, 8, h->lat);
    msd_pb_double(w, 9, h->lon);
}

/* One `history` (14) entry of AircraftsUpdate: tag 0x72, a one-byte length, the body -> its length, at most
 * MSD_HISTORY_ENTRY_MAX.  out == NULL: the length alone. */
MSD_HD uint32_t msd_history_entry(const msd_pb_head *h, int32_t altitude, uint8_t *out)
{
    msd_pb_w c = {0, 0}, w = {out, 0};
    msd_history_body(&c, h, altitude);
    msd_pb_byte(&w, 0x72);
    msd_pb_byte(&w, c.n); /* at most 34 */
    msd_history_body(&w, h, altitude);
    return w.n;
}

/* a file's head: `now` (1); `messages` is never set */
MSD_HD uint32_t msd_history_header(uint64_t now_ms, uint8_t *out)
{
    msd_pb_w w = {out, 0};
    msd_pb_uint(&w, 1, now_ms / 1000u);
    return w.n;
}

/* what msd_pos_history_pb accepts */
MSD_HD int msd_history_options_ok(const msd_history_options *opt)
{
    return opt && opt->flags == 0 && opt->reserved == 0;
}

#endif
