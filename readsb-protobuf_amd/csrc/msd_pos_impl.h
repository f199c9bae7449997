/* msd_pos_impl.h -- the position path of the reference's tracker, one implementation for the position kernels
 * (device) and the host twin (libmsd_host.so): the per-aircraft state and the function that feeds it one record.
 * Restated from track.c / track.h:
 *   accept_data :170-196 (its reduce_forward half is msd_trk_impl.h's: msd_pos_acc.accepted tells it which of the six
 *   members a record's feed accepted), trackDataValid track.h:217-219, trackDataAge :229-235,
 *   getBearing :238-250, greatcircle :260-279, update_polar_range :281-308, speed_check :313-369, doGlobalCPR :371-446,
 *   doLocalCPR :448-542, updatePosition :551-688 (the declination, :676-681, left out; :683-686 is "the receiver range" at
 *   the end of this file), the part of trackUpdateFromMessage that reaches them -- seen / messages
 *   :1024-1025, the per-source versions :1032-1075, the gs / ias / tas stores :1222-1235, the CPR stores :1313-1329,
 *   :1381-1383 -- and the part of trackRemoveStaleAircraft :1494-1570 that concerns these members.
 * Not here: geomag_calc, SBS and MLAT input (the SBS output's text is msd_sbs_impl.h).  NIC / Rc and the other members of
 * struct aircraft are msd_trk_impl.h's, for a tracker with the aircraft table.
 *
 * Every validity of the six kept members has stale_interval 60 s and expire_interval 70 s (track.c:113-115,132-134), so
 * the state keeps `source` and `updated` and derives stale = updated + 60000, expires = updated + 70000: accept_data is
 * the only place that sets a source other than SOURCE_INVALID, and it sets all three together.
 *
 * The coordinates are msd_cpr_impl.h's and exact.  greatcircle's sin / cos / acos / atan2 are the libm of whoever
 * compiles this: its distances feed three comparisons (--max-range, the local range limit, the speed check), and
 * msd_pos_acc.margin keeps the smallest |distance - limit| seen so that a caller can tell whether a stream came close
 * enough to a gate for two libms to decide it differently (modes_hip.h, msd_pos_update).  The receiver range delivers a
 * distance truncated to metres and a bearing rounded to a bucket, and keeps two margins of its own for the same purpose
 * (modes_hip.h, "Receiver range"). */
#ifndef MSD_POS_IMPL_H
#define MSD_POS_IMPL_H

#include "modes_hip.h"
#include "msd_cpr_impl.h"

#define MSD_POS_PI 3.14159265358979323846 /* M_PI */
enum { MSD_PV_GS = 0, MSD_PV_IAS, MSD_PV_TAS, MSD_PV_CPR_ODD, MSD_PV_CPR_EVEN, MSD_PV_POSITION, MSD_PV_N };
/* msd_pos_stats' counters in its order */
enum {
    MSD_PC_SURFACE = 0, MSD_PC_AIRBORNE, MSD_PC_GLOBAL_OK, MSD_PC_GLOBAL_BAD, MSD_PC_GLOBAL_SKIPPED, MSD_PC_GLOBAL_RANGE,
    MSD_PC_GLOBAL_SPEED, MSD_PC_LOCAL_OK, MSD_PC_LOCAL_AIRCRAFT, MSD_PC_LOCAL_RECEIVER, MSD_PC_LOCAL_SKIPPED,
    MSD_PC_LOCAL_RANGE, MSD_PC_LOCAL_SPEED, MSD_PC_N
};
#define MSD_POS_TTL 600000u       /* TRACK_AIRCRAFT_TTL, track.h:58 */
#define MSD_POS_ONEHIT_TTL 60000u /* TRACK_AIRCRAFT_ONEHIT_TTL, track.h:61 */
#define MSD_POS_EMPTY (~(uint64_t)0)

typedef struct msd_pos_aircraft { /* 136 bytes: what struct aircraft (track.h) keeps for the position path */
    uint64_t seen, messages;
    uint64_t upd[MSD_PV_N];       /* data_validity.updated */
    double lat, lon;              /* meta.lat / meta.lon */
    uint32_t gs, ias, tas;        /* meta.gs / .ias / .tas: uint32 (readsb.pb-c.h:208,249,253) */
    float gs_last_pos;
    uint32_t even_lat, even_lon, odd_lat, odd_lon;
    int32_t reliable_odd, reliable_even;
    uint8_t src[MSD_PV_N];        /* data_validity.source */
    uint8_t even_type, odd_type;
    int8_t version[3];            /* adsb_version, tisb_version, adsr_version; -1 until seen (track.c:88) */
    uint8_t pad[5];
} msd_pos_aircraft;

typedef struct msd_pos_acc {
    uint64_t c[MSD_PC_N];
    double margin;
    uint32_t accepted; /* bit MSD_PV_x: accept_data took member x; only ever set here, whoever reads it clears it per record */
    uint32_t gs_valid; /* of the record fed last: mm->gs_valid and mm->gs.selected as :1223 leaves it (0 when not valid), */
    float gs_selected; /* for the SBS row (modes_hip.h "SBS output"); nobody else reads them */
} msd_pos_acc;

MSD_HD uint64_t msd_pos_key(uint32_t receiver, uint32_t addr)
{
    return ((uint64_t)receiver << 25) | (addr & 0x1FFFFFFu);
}
/* home slot of a key in a table of 2^k slots: msd_pos_hash(key) & (slots - 1), then linear probing */
MSD_HD uint32_t msd_pos_hash(uint64_t key)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32);
}

/* what msd_pos_create and msd_pos_host_create accept */
MSD_HD int msd_pos_config_ok(const msd_pos_config *cfg)
{
    return cfg && cfg->capacity >= 64u && cfg->capacity <= (1u << 24) && (cfg->capacity & (cfg->capacity - 1u)) == 0 &&
           cfg->receivers >= 1u && cfg->receivers <= 65536u && cfg->filter_persistence >= 0;
}

MSD_HD void msd_pos_aircraft_init(msd_pos_aircraft *a)
{
    const msd_pos_aircraft z = {0};
    *a = z;
    a->version[0] = a->version[1] = a->version[2] = -1;
}

MSD_HD int msd_pos_valid(const msd_pos_aircraft *a, int k, uint64_t now) /* trackDataValid */
{
    return a->src[k] != 0 && now < a->upd[k] + 70000u;
}

MSD_HD uint64_t msd_pos_age(const msd_pos_aircraft *a, int k, uint64_t now) /* trackDataAge */
{
    if (a->src[k] == 0)
        return ~(uint64_t)0;
    if (a->upd[k] >= now)
        return 0;
    return now - a->upd[k];
}

MSD_HD int msd_pos_accept(msd_pos_aircraft *a, int k, unsigned source, uint64_t now) /* accept_data */
{
    if (now < a->upd[k])
        return 0;
    if (source < a->src[k] && now < a->upd[k] + 60000u)
        return 0;
    a->src[k] = (uint8_t)source;
    a->upd[k] = now;
    return 1;
}

MSD_HD double msd_pos_greatcircle(double lat0, double lon0, double lat1, double lon1) /* track.c:260-279 */
{
    lat0 = lat0 * MSD_POS_PI / 180.0;
    lon0 = lon0 * MSD_POS_PI / 180.0;
    lat1 = lat1 * MSD_POS_PI / 180.0;
    lon1 = lon1 * MSD_POS_PI / 180.0;
    const double dlat = fabs(lat1 - lat0), dlon = fabs(lon1 - lon0);
    if (dlat < 0.001 && dlon < 0.001) { /* haversine for small distances */
        const double h = sin(dlat / 2) * sin(dlat / 2) + cos(lat0) * cos(lat1) * sin(dlon / 2) * sin(dlon / 2);
        return 6371e3 * 2 * atan2(sqrt(h), sqrt(1.0 - h));
    }
    return 6371e3 * acos(sin(lat0) * sin(lat1) + cos(lat0) * cos(lat1) * cos(dlon));
}

MSD_HD void msd_pos_gate(msd_pos_acc *acc, double distance, double limit)
{
    const double m = fabs(distance - limit);
    if (m < acc->margin)
        acc->margin = m;
}

/* speed_check, track.c:313-369: may the aircraft have got from its last position to (lat, lon) by now? */
MSD_HD int msd_pos_speed_check(const msd_pos_aircraft *a, uint64_t now, double lat, double lon, int surface, msd_pos_acc *acc)
{
    int speed;
    if (!msd_pos_valid(a, MSD_PV_POSITION, now))
        return 1;
    const uint64_t elapsed = msd_pos_age(a, MSD_PV_POSITION, now);
    if (msd_pos_valid(a, MSD_PV_GS, now)) {
        const float g = (float)a->gs; /* the comparison and the choice are in float: float against uint32 */
        speed = (int)((a->gs_last_pos > g) ? a->gs_last_pos : g);
        speed = (int)(speed + (2 * msd_pos_age(a, MSD_PV_GS, now) / 1000.0)); /* 2 knots per second of not knowing */
    } else if (msd_pos_valid(a, MSD_PV_TAS, now)) {
        speed = (int)(a->tas * 4u / 3u);
    } else if (msd_pos_valid(a, MSD_PV_IAS, now)) {
        speed = (int)(a->ias * 2u);
    } else {
        speed = surface ? 100 : 700;
    }
    speed = speed * 4 / 3;
    if (surface) {
        if (speed < 20)
            speed = 20;
        if (speed > 150)
            speed = 150;
    } else if (speed < 200) {
        speed = 200;
    }
    const double range = (surface ? 0.1e3 : 0.5e3) + ((elapsed + 1000.0) / 1000.0) * (speed * 1852.0 / 3600.0);
    const double distance = msd_pos_greatcircle(a->lat, a->lon, lat, lon);
    msd_pos_gate(acc, distance, range);
    return distance <= range;
}

/* doGlobalCPR, track.c:371-446 */
MSD_HD int msd_pos_global(const msd_pos_aircraft *a, const msd_pos_receiver *rx, uint64_t now, unsigned source, int fflag,
                          int surface, double *lat, double *lon, msd_pos_acc *acc)
{
    int result;
    if (surface) {
        double reflat, reflon;
        if (msd_pos_valid(a, MSD_PV_POSITION, now)) {
            reflat = a->lat;
            reflon = a->lon;
        } else if (rx->latlon_valid) {
            reflat = rx->lat;
            reflon = rx->lon;
        } else {
            return -1;
        }
        result = msd_cpr_surface(reflat, reflon, (int)a->even_lat, (int)a->even_lon, (int)a->odd_lat, (int)a->odd_lon, fflag,
                                 lat, lon);
    } else {
        result = msd_cpr_airborne((int)a->even_lat, (int)a->even_lon, (int)a->odd_lat, (int)a->odd_lon, fflag, lat, lon);
    }
    if (result < 0)
        return result;
    if (rx->max_range_m > 0 && rx->latlon_valid) {
        const double range = msd_pos_greatcircle(rx->lat, rx->lon, *lat, *lon);
        msd_pos_gate(acc, range, rx->max_range_m);
        if (range > rx->max_range_m) {
            acc->c[MSD_PC_GLOBAL_RANGE]++;
            return -2;
        }
    }
    if (msd_pos_valid(a, MSD_PV_POSITION, now) && source <= a->src[MSD_PV_POSITION] &&
        !msd_pos_speed_check(a, now, *lat, *lon, surface, acc)) {
        acc->c[MSD_PC_GLOBAL_SPEED]++;
        return -2;
    }
    return result;
}

/* doLocalCPR, track.c:448-542: 1 aircraft-relative, 2 receiver-relative, -1 */
MSD_HD int msd_pos_local(const msd_pos_aircraft *a, const msd_pos_receiver *rx, uint64_t now, unsigned source, int fflag,
                         int surface, uint32_t cpr_lat, uint32_t cpr_lon, double *lat, double *lon, msd_pos_acc *acc)
{
    double reflat, reflon, range_limit = 0;
    int relative_to;
    if (now - a->upd[MSD_PV_POSITION] < (10 * 60 * 1000)) { /* unsigned, whatever the source says (:466) */
        reflat = a->lat;
        reflon = a->lon;
        range_limit = 1852 * 100;
        relative_to = 1;
    } else if (!surface && rx->latlon_valid) {
        reflat = rx->lat;
        reflon = rx->lon;
        if (rx->max_range_m == 0)
            return -1;
        else if (rx->max_range_m <= 1852 * 180)
            range_limit = rx->max_range_m;
        else if (rx->max_range_m < 1852 * 360)
            range_limit = (1852 * 360) - rx->max_range_m;
        else
            return -1;
        relative_to = 2;
    } else {
        return -1;
    }
    if (msd_cpr_relative(reflat, reflon, (int)cpr_lat, (int)cpr_lon, fflag, surface, lat, lon) < 0)
        return -1;
    if (range_limit > 0) {
        const double range = msd_pos_greatcircle(reflat, reflon, *lat, *lon);
        msd_pos_gate(acc, range, range_limit);
        if (range > range_limit) {
            acc->c[MSD_PC_LOCAL_RANGE]++;
            return -1;
        }
    }
    if (msd_pos_valid(a, MSD_PV_POSITION, now) && source <= a->src[MSD_PV_POSITION] &&
        !msd_pos_speed_check(a, now, *lat, *lon, surface, acc)) {
        acc->c[MSD_PC_LOCAL_SPEED]++;
        return -1;
    }
    return relative_to;
}

/* decodeMovementFieldV0 / V2 (mode_s.c:216-259), as msd_fields.c states them for msd_fields_to_float */
MSD_HD float msd_pos_movement(unsigned m, int v2)
{
    if (m >= 125) return 0;
    if (m == 124) return 180;
    if (m >= 109) return (float)(100 + (m - 109 + 0.5) * 5);
    if (m >= 94) return (float)(70 + (m - 94 + 0.5) * 2);
    if (m >= 39) return (float)(15 + (m - 39 + 0.5) * 1);
    if (m >= 13) return (float)(2 + (m - 13 + 0.5) * 0.50);
    if (m >= 9) return (float)(1 + (m - 9 + 0.5) * 0.25);
    if (v2) {
        if (m >= 3) return (float)(0.125 + (m - 3 + 0.5) * 0.875 / 6);
        if (m >= 2) return (float)(0.125 / 2);
        return 0;
    }
    if (m >= 2) return (float)(0.125 + (m - 2 + 0.5) * 0.125);
    return 0;
}

/* gs_valid and gs.v0 / gs.v2 of a record, by the expressions of msd_fields_to_float: the airborne velocity's
 * sqrtf(ns^2 + ew^2 + 0.5) (mode_s.c:831; sqrtf is the correctly rounded IEEE square root on the device too,
 * tests/test_gpu_sqrt_check.py), the surface movement tables, the BDS 5,0 ground speed */
MSD_HD int msd_pos_record_gs(const msd_fields *f, float *v0, float *v2)
{
    if (f->velocity_valid) {
        const int ew = f->ew_vel, ns = f->ns_vel;
        *v0 = *v2 = sqrtf((float)((ns * ns) + (ew * ew) + 0.5));
        return 1;
    }
    if (f->movement) {
        *v0 = msd_pos_movement(f->movement, 0);
        *v2 = msd_pos_movement(f->movement, 1);
        return 1;
    }
    if (f->commb_valid & MSD_COMMB_GS) {
        *v0 = *v2 = (float)(unsigned)f->gs;
        return 1;
    }
    return 0;
}

/* updatePosition, track.c:551-688; returns location_result */
MSD_HD int msd_pos_update_position(msd_pos_aircraft *a, const msd_pos_receiver *rx, int filter_persistence, uint64_t now,
                                   const msd_fields *f, int gs_valid, float gs_selected, double *new_lat, double *new_lon,
                                   msd_pos_acc *acc)
{
    const int surface = f->cpr_type == 0, fflag = f->cpr_odd;
    const unsigned source = f->source;
    int location_result = -1;
    uint64_t max_elapsed;
    if (surface) {
        acc->c[MSD_PC_SURFACE]++;
        max_elapsed = (gs_valid && gs_selected <= 25) ? 50000 : 25000;
    } else {
        acc->c[MSD_PC_AIRBORNE]++;
        max_elapsed = 10000;
    }
    const uint64_t uo = a->upd[MSD_PV_CPR_ODD], ue = a->upd[MSD_PV_CPR_EVEN];
    if (msd_pos_valid(a, MSD_PV_CPR_ODD, now) && msd_pos_valid(a, MSD_PV_CPR_EVEN, now) &&
        a->src[MSD_PV_CPR_ODD] == a->src[MSD_PV_CPR_EVEN] && a->odd_type == a->even_type &&
        (uo >= ue ? uo - ue : ue - uo) <= max_elapsed) {
        location_result = msd_pos_global(a, rx, now, source, fflag, surface, new_lat, new_lon, acc);
        if (location_result == -2) {
            /* bad data: both halves go, and the position with them once it is not trusted any more */
            acc->c[MSD_PC_GLOBAL_BAD]++;
            a->src[MSD_PV_CPR_ODD] = 0;
            a->src[MSD_PV_CPR_EVEN] = 0;
            a->reliable_odd--;
            a->reliable_even--;
            if (a->reliable_odd <= 0 || a->reliable_even <= 0) {
                a->src[MSD_PV_POSITION] = 0;
                a->reliable_odd = 0;
                a->reliable_even = 0;
            }
            return -2;
        } else if (location_result == -1) {
            acc->c[MSD_PC_GLOBAL_SKIPPED]++;
        } else if (msd_pos_accept(a, MSD_PV_POSITION, source, now)) {
            acc->accepted |= 1u << MSD_PV_POSITION;
            acc->c[MSD_PC_GLOBAL_OK]++;
            if (a->reliable_odd <= 0 || a->reliable_even <= 0) {
                a->reliable_odd = 1;
                a->reliable_even = 1;
            } else if (fflag) {
                a->reliable_odd = a->reliable_odd + 1 < filter_persistence ? a->reliable_odd + 1 : filter_persistence;
            } else {
                a->reliable_even = a->reliable_even + 1 < filter_persistence ? a->reliable_even + 1 : filter_persistence;
            }
            if (msd_pos_valid(a, MSD_PV_GS, now))
                a->gs_last_pos = (float)a->gs;
        } else {
            acc->c[MSD_PC_GLOBAL_SKIPPED]++;
            location_result = -2;
        }
    }
    if (location_result == -1) {
        location_result = msd_pos_local(a, rx, now, source, fflag, surface, f->cpr_lat, f->cpr_lon, new_lat, new_lon, acc);
        if (location_result >= 0 && msd_pos_accept(a, MSD_PV_POSITION, source, now)) {
            acc->accepted |= 1u << MSD_PV_POSITION;
            acc->c[MSD_PC_LOCAL_OK]++;
            if (msd_pos_valid(a, MSD_PV_GS, now))
                a->gs_last_pos = (float)a->gs;
            if (location_result == 1)
                acc->c[MSD_PC_LOCAL_AIRCRAFT]++;
            if (location_result == 2)
                acc->c[MSD_PC_LOCAL_RECEIVER]++;
        } else {
            acc->c[MSD_PC_LOCAL_SKIPPED]++;
            location_result = -1;
        }
    }
    if (location_result >= 0) {
        a->lat = *new_lat;
        a->lon = *new_lon;
    }
    return location_result;
}

/* One record of an aircraft that is neither Mode A/C nor address 0 (track.c:999-1008: the caller skips those), with
 * messageNow() = now = the record's sysTimestampMsg (:1010). */
MSD_HD void msd_pos_feed(msd_pos_aircraft *a, const msd_pos_receiver *rx, int filter_persistence, uint64_t now,
                         const msd_fields *f, msd_position *out, msd_pos_acc *acc)
{
    const unsigned source = f->source;
    int cpr_new = 0;
    out->lat = 0;
    out->lon = 0;
    out->decoded = 0;
    out->relative = 0;
    out->surface = (uint8_t)(f->cpr_valid && f->cpr_type == 0);
    out->result = MSD_POS_NOT_TRIED;
    a->seen = now;
    a->messages++;
    acc->gs_valid = 0;
    acc->gs_selected = 0;

    /* the version of this message's source (:1032-1075); -1 for everything that is not ADS-B, TIS-B or ADS-R */
    const int vi = source == 7 ? 0 : source == 5 ? 1 : source == 6 ? 2 : -1;
    int version = vi >= 0 ? a->version[vi] : -1;
    if (version < 0)
        version = 0;
    if (f->opstatus & MSD_OPS_VALID)
        version = (int)MSD_OPS_VERSION(f->opstatus);
    if (vi >= 0)
        a->version[vi] = (int8_t)version;

    float v0 = 0, v2 = 0, gs_selected = 0;
    const int gs_valid = msd_pos_record_gs(f, &v0, &v2);
    if (gs_valid) { /* :1222-1227 */
        gs_selected = version == 2 ? v2 : v0;
        acc->gs_selected = gs_selected;
        acc->gs_valid = 1;
        if (msd_pos_accept(a, MSD_PV_GS, source, now)) {
            acc->accepted |= 1u << MSD_PV_GS;
            a->gs = (uint32_t)gs_selected;
        }
    }
    if (f->ias_valid && msd_pos_accept(a, MSD_PV_IAS, source, now)) {
        acc->accepted |= 1u << MSD_PV_IAS;
        a->ias = f->ias;
    }
    if (f->tas_valid && msd_pos_accept(a, MSD_PV_TAS, source, now)) {
        acc->accepted |= 1u << MSD_PV_TAS;
        a->tas = f->tas;
    }
    if (f->cpr_valid && !f->cpr_odd && msd_pos_accept(a, MSD_PV_CPR_EVEN, source, now)) { /* :1313-1320 */
        acc->accepted |= 1u << MSD_PV_CPR_EVEN;
        a->even_type = f->cpr_type;
        a->even_lat = f->cpr_lat;
        a->even_lon = f->cpr_lon;
        cpr_new = 1;
    }
    if (f->cpr_valid && f->cpr_odd && msd_pos_accept(a, MSD_PV_CPR_ODD, source, now)) { /* :1322-1329 */
        acc->accepted |= 1u << MSD_PV_CPR_ODD;
        a->odd_type = f->cpr_type;
        a->odd_lat = f->cpr_lat;
        a->odd_lon = f->cpr_lon;
        cpr_new = 1;
    }
    if (cpr_new) {
        double lat = 0, lon = 0;
        const int r = msd_pos_update_position(a, rx, filter_persistence, now, f, gs_valid, gs_selected, &lat, &lon, acc);
        out->result = (int8_t)r;
        if (r >= 0) {
            out->decoded = 1;
            out->relative = (uint8_t)r;
            out->lat = lat;
            out->lon = lon;
        }
    }
}

/* trackRemoveStaleAircraft for one aircraft (track.c:1500-1501, :1520-1560): 1 = remove it */
MSD_HD int msd_pos_expire_one(msd_pos_aircraft *a, uint64_t now)
{
    if ((now - a->seen) > MSD_POS_TTL || (a->messages == 1 && (now - a->seen) > MSD_POS_ONEHIT_TTL))
        return 1;
    for (int k = 0; k < MSD_PV_N; ++k)
        if (a->src[k] != 0 && now >= a->upd[k] + 70000u)
            a->src[k] = 0;
    if (a->src[MSD_PV_POSITION] == 0) {
        a->reliable_odd = 0;
        a->reliable_even = 0;
    }
    return 0;
}

/* ---- the receiver range: the last lines of updatePosition (track.c:683-686) with update_polar_range (:281-308) and
 * getBearing (:238-250).  For a record whose msd_pos_update_position returned location_result >= 0, after lat / lon and
 * the pos_reliable counters are updated:
 *     a->meta.distance = 0                                                              :683
 *     if pos_reliable_odd >= 1 && pos_reliable_even >= 1 && mm->source == SOURCE_ADSB   :684
 *         a->meta.distance = update_polar_range(new_lat, new_lon)                       :685
 * update_polar_range: 0 without a receiver location (:285); range = greatcircle(receiver, position) (:288);
 * longest_distance = range where range is within --max-range (or there is none) and longer (:290-292); with
 * --stats-range, bucket = (int)round(getBearing / 5), 72 and more -> 0 (:296-300), polar_range[bucket] = (uint32_t)range
 * where polar_range[bucket] < range (:302-304); -> (uint32_t)range (:307).
 * The serial walk does none of the trigonometry: it leaves msd_pos_range_code per record, and msd_pos_range_one is
 * evaluated by one lane per record afterwards (msd_pos_range_kernel), by the host object in stream order.  Both results are
 * maxima -- of (uint32_t)range, which is monotone in range, and of non-negative doubles -- so the order does not matter. */
#define MSD_RANGE_CODE_DECODED 1u /* location_result >= 0: the record sets a->meta.distance (:683) */
#define MSD_RANGE_CODE_EVAL 2u    /* and :684 holds: update_polar_range is called */
#define MSD_RANGE_CODE_LAST 4u    /* the aircraft's last decoded record of the call (of the piece): it leaves the distance */

/* a: the aircraft after msd_pos_feed took the record, o: what the feed delivered for it.  A receiver-relative decode can
 * succeed at pos_reliable 0 / 0 (after an expiry): decoded, not evaluated. */
MSD_HD uint32_t msd_pos_range_code(const msd_pos_aircraft *a, const msd_fields *f, const msd_position *o)
{
    if (!o->decoded)
        return 0;
    return MSD_RANGE_CODE_DECODED | (a->reliable_odd >= 1 && a->reliable_even >= 1 && f->source == 7 ? MSD_RANGE_CODE_EVAL : 0u);
}

MSD_HD double msd_pos_bearing(double lat0, double lon0, double lat1, double lon1) /* getBearing, track.c:238-250: [0, 360] */
{
    lat0 = lat0 * MSD_POS_PI / 180.0;
    lon0 = lon0 * MSD_POS_PI / 180.0;
    lat1 = lat1 * MSD_POS_PI / 180.0;
    lon1 = lon1 * MSD_POS_PI / 180.0;
    const double dlon = lon1 - lon0;
    const double x = cos(lat0) * sin(dlon);
    const double y = cos(lat1) * sin(lat0) - sin(lat1) * cos(lat0) * cos(dlon);
    const double b = atan2(x, y);
    const double bearing = 180 / MSD_POS_PI * b;
    return bearing + 180;
}

typedef struct msd_range_one {
    double range;          /* greatcircle(receiver, position) */
    double range_margin;   /* min(|range - nearest integer|, |range - max_range_m| with a limit) */
    double bearing_margin; /* with the polar range: the bearing's distance from the nearest edge 2.5 + 5k; 0 below 1 m */
    uint32_t metres;       /* (uint32_t)range: update_polar_range's return value */
    uint32_t bucket;       /* with the polar range: 0 .. 71 */
    uint32_t counts;       /* range is a number: it takes part in the maxima (a NaN compares false in :290 and :302) */
    uint32_t longest;      /* :290's first half: within --max-range, or there is none */
} msd_range_one;

/* update_polar_range's arithmetic for one position and a receiver with a location */
MSD_HD void msd_pos_range_one(const msd_pos_receiver *rx, double lat, double lon, int polar, msd_range_one *e)
{
    const double range = msd_pos_greatcircle(rx->lat, rx->lon, lat, lon);
    e->range = range;
    e->counts = range >= 0;
    e->metres = e->counts ? (uint32_t)range : 0u;
    e->longest = e->counts && (range <= rx->max_range_m || rx->max_range_m == 0);
    e->range_margin = e->counts ? fabs(range - floor(range + 0.5)) : 0;
    if (rx->max_range_m != 0 && !(fabs(range - rx->max_range_m) >= e->range_margin))
        e->range_margin = fabs(range - rx->max_range_m);
    e->bucket = 0;
    e->bearing_margin = INFINITY;
    if (polar) {
        const double q = msd_pos_bearing(rx->lat, rx->lon, lat, lon) / 5;
        int bucket = (int)round(q);
        if (bucket >= (int)MSD_RANGE_BUCKETS || bucket < 0)
            bucket = 0;
        e->bucket = (uint32_t)bucket;
        e->bearing_margin = range >= 1 ? 5 * fabs(q - floor(q) - 0.5) : 0;
    }
}

#endif
