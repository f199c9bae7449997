/* msd_trk_impl.h -- the rest of trackUpdateFromMessage, one implementation for the table kernels (device) and the host
 * twin (libmsd_host.so): the per-aircraft table entry and the function that feeds it one record.  Restated from
 * track.c / track.h, in the reference's order:
 *   trackCreateAircraft's defaults :83-90, accept_data :170-196 with the per-member stale intervals of :108-143 and, for a
 *   tracker that reduces, its reduce_forward half with the DF11 timer of :1396-1400 (msd_trk_reduce below), combine_validity :200-215, compare_validity :217-228, trackDataValid / Fresh / Age
 *   track.h:217-235, compute_nic :690-776, compute_rc :778-892, compute_v0_nacp :897-924, compute_v0_sil :929-967,
 *   compute_nic_rc_from_message :969-976, altitude_to_feet :978-987, trackUpdateFromMessage :1020-1378 minus what
 *   msd_pos_feed does (seen / messages, gs / ias / tas, the CPR halves and updatePosition), the NIC / Rc of doGlobalCPR
 *   :378-379 and doLocalCPR :458-473 with updatePosition's stores :667-674, and trackRemoveStaleAircraft's EXPIRE list
 *   :1520-1563 for these members.
 * Not here: FATSV state, geomag_calc, SBS and MLAT input (a->meta.distance and update_polar_range are msd_pos_impl.h's,
 * "the receiver range", kept beside the table, not in it).  The SBS output takes the aircraft's
 * geom_delta and its validity from the entry after a record's feed (msd_trk_sbs below); its text is msd_sbs_impl.h.
 * trackMatchAC is msd_modeac_impl.h; of modeA_hit / modeC_hit this file has the two resets (:1096-1102, :1154-1156).
 *
 * The entry is the public msd_aircraft (modes_hip.h); its head -- receiver .. pos_reliable_even -- and the validities
 * of gs, ias, tas, the CPR halves and the position belong to the position state and are filled in by msd_trk_export.
 * What updatePosition decided for a record comes in as the msd_position the position walk wrote: `result` says whether
 * the record's CPR half was accepted (anything but MSD_POS_NOT_TRIED) and which decode delivered the position.
 *
 * Integer logic and copies of doubles only, apart from one double division in altitude_to_feet (IEEE, the same on both
 * sides) and msd_pos_record_gs's correctly rounded square root: the device and the host agree bit for bit. */
#ifndef MSD_TRK_IMPL_H
#define MSD_TRK_IMPL_H

#include "msd_pos_impl.h"

typedef msd_aircraft msd_trk_aircraft;

#define MSD_TRK_RELIABLE_MAX 20 /* ALTITUDE_BARO_RELIABLE_MAX, track.h:71 */
#define MSD_REDUCE_TIMERS (MSD_AC_N + 1) /* per slot of a tracker that reduces: the members' timers, then the DF11 timer */
#define MSD_REDUCE_MAX_INTERVAL 15000u   /* --net-beast-reduce-interval is capped at 15 s (readsb.c) */
/* what the position walk leaves in a record's verdict byte for the table walk: msd_pos_acc.accepted in bits 0-5 and */
#define MSD_REDUCE_WALK_SEEN_TWICE 64u   /* the aircraft's messages > 1 after the record */

MSD_HD void msd_trk_init(msd_trk_aircraft *a) /* trackCreateAircraft */
{
    unsigned char *b = (unsigned char *)a;
    for (unsigned i = 0; i < sizeof *a; ++i)
        b[i] = 0;
    for (int i = 0; i < 8; ++i)
        a->signal_level[i] = 1e-5;
    a->addr_type = 255; /* the first message's addrtype is below it (:82, :1028) */
    a->adsb_version = a->tisb_version = a->adsr_version = -1;
    a->adsb_hrd = 3; /* HEADING_MAGNETIC */
    a->adsb_tah = 1; /* HEADING_GROUND_TRACK */
}

MSD_HD uint64_t msd_trk_stale(const msd_trk_aircraft *a, int k)
{
    if (k == MSD_AC_ALTITUDE_GEOM)
        return a->altitude_geom_stale;
    return a->updated[k] + ((k == MSD_AC_ALTITUDE_BARO || k == MSD_AC_SQUAWK || k == MSD_AC_AIRGROUND) ? 15000u : 60000u);
}

MSD_HD uint64_t msd_trk_expires(const msd_trk_aircraft *a, int k)
{
    return k == MSD_AC_ALTITUDE_GEOM ? a->altitude_geom_expires : a->updated[k] + 70000u;
}

MSD_HD int msd_trk_valid(const msd_trk_aircraft *a, int k, uint64_t now) /* trackDataValid */
{
    return a->source[k] != 0 && now < msd_trk_expires(a, k);
}

MSD_HD int msd_trk_fresh(const msd_trk_aircraft *a, int k, uint64_t now) /* trackDataFresh */
{
    return a->source[k] != 0 && now < msd_trk_stale(a, k);
}

MSD_HD uint64_t msd_trk_age(const msd_trk_aircraft *a, int k, uint64_t now) /* trackDataAge */
{
    if (a->source[k] == 0)
        return ~(uint64_t)0;
    if (a->updated[k] >= now)
        return 0;
    return now - a->updated[k];
}

/* The reduce_forward half of accept_data (:182-193) for one record of a tracker that reduces (modes_hip.h "Reduced Beast
 * output"): next[k] is data_validity.next_reduce_forward of member k, next[MSD_AC_N] the aircraft's
 * next_reduce_forward_DF11; they sit beside the entry, as the hit bytes do, start at 0 and are not touched by EXPIRE.
 * `forward` is mm->reduce_forward.  A timer depends on its own member's accepts only, so the order in which a record's
 * members come by does not matter.  mm->sbs_in is never set here. */
typedef struct msd_trk_reduce {
    uint64_t *next;
    uint32_t interval; /* Modes.net_output_beast_reduce_interval, ms */
    uint8_t df17;      /* mm->msgtype == 17 */
    uint8_t cpr;       /* mm->cpr_valid */
    uint8_t forward;
} msd_trk_reduce;

MSD_HD void msd_trk_reduce_member(msd_trk_reduce *r, int k, uint64_t now, int reduce_often)
{
    if (now > r->next[k]) {
        r->next[k] = now + ((r->df17 || reduce_often) ? (uint64_t)r->interval : (uint64_t)r->interval * 4u);
        if (r->interval > 7000u && r->cpr) /* global CPR stays possible at a long interval */
            r->next[k] = now + 7000u;
        r->forward = 1;
    }
}

/* r: NULL for a tracker that does not reduce */
MSD_HD int msd_trk_accept(msd_trk_aircraft *a, int k, unsigned source, uint64_t now, int reduce_often, msd_trk_reduce *r) /* accept_data */
{
    if (now < a->updated[k])
        return 0;
    if (source < a->source[k] && now < msd_trk_stale(a, k))
        return 0;
    a->source[k] = (uint8_t)source;
    a->updated[k] = now;
    if (k == MSD_AC_ALTITUDE_GEOM) {
        a->altitude_geom_stale = now + (a->altitude_geom_stale_15s ? 15000u : 60000u);
        a->altitude_geom_expires = now + 70000u;
    }
    if (r)
        msd_trk_reduce_member(r, k, now, reduce_often);
    return 1;
}

MSD_HD int msd_trk_compare(const msd_trk_aircraft *a, int lhs, int rhs, uint64_t now) /* compare_validity */
{
    if (now < msd_trk_stale(a, lhs) && a->source[lhs] > a->source[rhs])
        return 1;
    else if (now < msd_trk_stale(a, rhs) && a->source[lhs] < a->source[rhs])
        return -1;
    else if (a->updated[lhs] > a->updated[rhs])
        return 1;
    else if (a->updated[lhs] < a->updated[rhs])
        return -1;
    return 0;
}

MSD_HD unsigned msd_trk_compute_nic(unsigned metype, int version, int nic_a, int nic_b, int nic_c) /* :690-776 */
{
    switch (metype) {
    case 5: case 9: case 20: return 11;
    case 6: case 10: case 21: return 10;
    case 7:
        if (version == 2)
            return (nic_a && !nic_c) ? 9 : 8;
        else if (version == 1)
            return nic_a ? 9 : 8;
        return 8;
    case 8:
        if (version == 2) {
            if (nic_a && nic_c) return 7;
            else if (nic_a && !nic_c) return 6;
            else if (!nic_a && nic_c) return 6;
            return 0;
        }
        return 0;
    case 11:
        if (version == 2)
            return (nic_a && nic_b) ? 9 : 8;
        else if (version == 1)
            return nic_a ? 9 : 8;
        return 8;
    case 12: return 7;
    case 13: return 6;
    case 14: return 5;
    case 15: return 4;
    case 16: return (nic_a && nic_b) ? 3 : 2;
    case 17: return 1;
    default: return 0;
    }
}

MSD_HD unsigned msd_trk_compute_rc(unsigned metype, int version, int nic_a, int nic_b, int nic_c) /* :778-892 */
{
    switch (metype) {
    case 5: case 9: case 20: return 8;
    case 6: case 10: case 21: return 25;
    case 7:
        if (version == 2)
            return (nic_a && !nic_c) ? 75 : 186;
        else if (version == 1)
            return nic_a ? 75 : 186;
        return 186;
    case 8:
        if (version == 2) {
            if (nic_a && nic_c) return 371;
            else if (nic_a && !nic_c) return 556;
            else if (!nic_a && nic_c) return 926;
            return 0; /* RC_UNKNOWN */
        }
        return 0;
    case 11:
        if (version == 2)
            return (nic_a && nic_b) ? 75 : 186;
        else if (version == 1)
            return nic_a ? 75 : 186;
        return 186;
    case 12: return 371;
    case 13:
        if (version == 2) {
            if (!nic_a && nic_b) return 556;
            else if (!nic_a && !nic_b) return 926;
            else if (nic_a && nic_b) return 1112;
            return 0;
        } else if (version == 1) {
            return nic_a ? 1112 : 926;
        }
        return 926;
    case 14: return 1852;
    case 15: return 3704;
    case 16:
        if (version == 2)
            return (nic_a && nic_b) ? 7408 : 14816;
        else if (version == 1)
            return nic_a ? 7408 : 14816;
        return 18520;
    case 17: return 37040;
    default: return 0;
    }
}

MSD_HD int msd_trk_v0_nacp(unsigned msgtype, unsigned metype) /* compute_v0_nacp, ED-102A table N-7 */
{
    if (msgtype != 17 && msgtype != 18)
        return -1;
    switch (metype) {
    case 0: return 0;
    case 5: return 11;
    case 6: return 10;
    case 7: return 8;
    case 8: return 0;
    case 9: return 11;
    case 10: return 10;
    case 11: return 8;
    case 12: return 7;
    case 13: return 6;
    case 14: return 5;
    case 15: return 4;
    case 16: return 1;
    case 17: return 1;
    case 18: return 0;
    case 20: return 11;
    case 21: return 10;
    case 22: return 0;
    default: return -1;
    }
}

MSD_HD int msd_trk_v0_sil(unsigned msgtype, unsigned metype) /* compute_v0_sil, ED-102A table N-8 */
{
    if (msgtype != 17 && msgtype != 18)
        return -1;
    if (metype == 0 || metype == 18 || metype == 22)
        return 0;
    if ((metype >= 5 && metype <= 17) || metype == 20 || metype == 21)
        return 2;
    return -1;
}

MSD_HD int msd_trk_to_feet(int raw, unsigned unit) /* altitude_to_feet */
{
    if (unit == 1)
        return (int)(raw / 0.3048);
    if (unit == 0)
        return raw;
    return 0;
}

MSD_HD int msd_trk_min(int a, int b)
{
    return a < b ? a : b;
}

/* One record of an aircraft, after msd_pos_feed has had it: pos is what that wrote for the record.  nicrc: decoded_nic /
 * decoded_rc of the record.  hits: the aircraft's {modeA_hit, modeC_hit} bytes of a tracker that matches Mode A/C
 * replies (msd_modeac_impl.h), else NULL.  next_reduce: the aircraft's MSD_AC_N + 1 timers of a tracker that reduces,
 * else NULL; with them, interval is the reduce interval, pos_accepted msd_pos_acc.accepted as msd_pos_feed left it for
 * this record, and the return value is mm->reduce_forward.  Without them it is 0. */
MSD_HD int msd_trk_feed(msd_trk_aircraft *a, uint64_t now, const msd_message *m, const msd_fields *f,
                        const msd_position *pos, msd_pos_nicrc *nicrc, uint8_t *hits, uint64_t *next_reduce,
                        uint32_t interval, unsigned pos_accepted)
{
    const unsigned source = f->source;
    msd_trk_reduce red, *const r = next_reduce ? &red : 0;
    red.next = next_reduce;
    red.interval = interval;
    red.df17 = m->msgtype == 17;
    red.cpr = f->cpr_valid != 0;
    red.forward = 0;
    if (r) { /* the six members msd_pos_feed accepted: gs, the CPR halves and the position are reduce_often (:617 .. :1323) */
        if (pos_accepted & (1u << MSD_PV_GS))
            msd_trk_reduce_member(r, MSD_AC_GS, now, 1);
        if (pos_accepted & (1u << MSD_PV_IAS))
            msd_trk_reduce_member(r, MSD_AC_IAS, now, 0);
        if (pos_accepted & (1u << MSD_PV_TAS))
            msd_trk_reduce_member(r, MSD_AC_TAS, now, 0);
        if (pos_accepted & (1u << MSD_PV_CPR_ODD))
            msd_trk_reduce_member(r, MSD_AC_CPR_ODD, now, 1);
        if (pos_accepted & (1u << MSD_PV_CPR_EVEN))
            msd_trk_reduce_member(r, MSD_AC_CPR_EVEN, now, 1);
        if (pos_accepted & (1u << MSD_PV_POSITION))
            msd_trk_reduce_member(r, MSD_AC_POSITION, now, 1);
    }
    nicrc->rc = 0;
    nicrc->nic = 0;
    nicrc->set = 0;

    if (m->signalLevel > 0) { /* :1020-1023 */
        a->signal_level[a->signal_next & 7] = m->signalLevel;
        a->signal_next = (uint8_t)((a->signal_next + 1) & 7);
    }
    if (f->addrtype < a->addr_type) /* :1028 */
        a->addr_type = f->addrtype;

    /* the version of this message's source (:1032-1054), as msd_pos_feed keeps it */
    int8_t *const vp = source == 7 ? &a->adsb_version : source == 5 ? &a->tisb_version : source == 6 ? &a->adsr_version : 0;
    int version = vp ? *vp : -1;
    if (version < 0)
        version = 0;
    if (f->category_valid)
        a->category = f->category;
    if (f->opstatus & MSD_OPS_VALID) { /* :1063-1072 */
        version = (int)MSD_OPS_VERSION(f->opstatus);
        if (MSD_OPS_HRD(f->opstatus) != 0)
            a->adsb_hrd = (uint8_t)MSD_OPS_HRD(f->opstatus);
        if (MSD_OPS_TAH(f->opstatus) != 0)
            a->adsb_tah = (uint8_t)MSD_OPS_TAH(f->opstatus);
    }
    if (vp)
        *vp = (int8_t)version;

    /* ADS-B v0: NACp and SIL from the position message type (:1074-1089) */
    int nac_p_valid = (f->acc_valid & MSD_ACC_NAC_P) != 0;
    unsigned nac_p = f->nac_p, sil = f->sil, sil_type = f->sil_type;
    if (version == 0 && !nac_p_valid) {
        const int c = msd_trk_v0_nacp(m->msgtype, f->metype);
        if (c != -1) {
            nac_p_valid = 1;
            nac_p = (unsigned)c;
        }
    }
    if (version == 0 && sil_type == 0) {
        const int c = msd_trk_v0_sil(m->msgtype, f->metype);
        if (c != -1) {
            sil_type = 1; /* SIL_UNKNOWN */
            sil = (unsigned)c;
        }
    }

    /* the barometric altitude and its plausibility gate (:1091-1151) */
    if (f->altitude_baro_valid &&
        (source >= a->source[MSD_AC_ALTITUDE_BARO] || msd_trk_age(a, MSD_AC_ALTITUDE_BARO, now) > 15 * 1000)) {
        const int alt = msd_trk_to_feet(f->altitude_baro, f->altitude_baro_unit);
        /* :1096-1102, before the gate: an altitude the gate refuses below clears the hit too */
        if (hits && hits[1] && (a->alt_baro + 49) / 100 != (alt + 49) / 100)
            hits[1] = 0;
        const int delta = alt - a->alt_baro;
        const int adelta = delta < 0 ? -delta : delta;
        int fpm = 0, max_fpm = 12500, min_fpm = -12500;
        if (adelta >= 300) {
            const uint64_t age = msd_trk_age(a, MSD_AC_ALTITUDE_BARO, now);
            int q = (int32_t)(uint32_t)age / 100; /* (int) trackDataAge(...) / 100 */
            if (q < 0)
                q = -q;
            fpm = delta * 60 * 10 / (q + 10);
            if (msd_trk_valid(a, MSD_AC_GEOM_RATE, now) &&
                msd_trk_age(a, MSD_AC_GEOM_RATE, now) < msd_trk_age(a, MSD_AC_BARO_RATE, now)) {
                const int w = msd_trk_min(11000, (int32_t)(uint32_t)msd_trk_age(a, MSD_AC_GEOM_RATE, now) / 2);
                min_fpm = a->geom_rate - 1500 - w;
                max_fpm = a->geom_rate + 1500 + w;
            } else if (msd_trk_valid(a, MSD_AC_BARO_RATE, now)) {
                const int w = msd_trk_min(11000, (int32_t)(uint32_t)msd_trk_age(a, MSD_AC_BARO_RATE, now) / 2);
                min_fpm = a->baro_rate - 1500 - w;
                max_fpm = a->baro_rate + 1500 + w;
            }
            if (msd_trk_valid(a, MSD_AC_ALTITUDE_BARO, now) && age < 30000) {
                const uint64_t lim = MSD_TRK_RELIABLE_MAX - (MSD_TRK_RELIABLE_MAX * age / 30000);
                /* min() of a uint64 and an int compares as uint64 */
                if (lim < (uint64_t)(int64_t)a->altitude_baro_reliable)
                    a->altitude_baro_reliable = (int32_t)lim;
            } else {
                a->altitude_baro_reliable = 0;
            }
        }
        const int good_crc = (m->crc == 0 && source != 2) ? (MSD_TRK_RELIABLE_MAX / 2 - 1) : 0;
        if (a->altitude_baro_reliable <= 0 || adelta < 300 || (fpm < max_fpm && fpm > min_fpm) ||
            (good_crc && a->altitude_baro_reliable <= (MSD_TRK_RELIABLE_MAX / 2 + 2))) {
            if (msd_trk_accept(a, MSD_AC_ALTITUDE_BARO, source, now, 1, r)) {
                a->altitude_baro_reliable = msd_trk_min(MSD_TRK_RELIABLE_MAX, a->altitude_baro_reliable + (good_crc + 1));
                a->alt_baro = alt;
            }
        } else {
            a->altitude_baro_reliable = a->altitude_baro_reliable - (good_crc + 1);
            if (a->altitude_baro_reliable <= 0) {
                a->altitude_baro_reliable = 0;
                a->source[MSD_AC_ALTITUDE_BARO] = 0;
            }
        }
    }

    if (f->squawk_valid && msd_trk_accept(a, MSD_AC_SQUAWK, source, now, 0, r)) {
        if (hits && f->squawk != a->squawk) /* :1154-1156 */
            hits[0] = 0;
        a->squawk = f->squawk;
    }
    if (f->emergency_valid && msd_trk_accept(a, MSD_AC_EMERGENCY, source, now, 0, r))
        a->emergency = f->emergency;
    if (f->altitude_geom_valid && msd_trk_accept(a, MSD_AC_ALTITUDE_GEOM, source, now, 1, r))
        a->alt_geom = msd_trk_to_feet(f->altitude_geom, f->altitude_geom_unit);
    if (f->geom_delta_valid && msd_trk_accept(a, MSD_AC_GEOM_DELTA, source, now, 1, r))
        a->geom_delta = f->geom_delta;

    /* the record's heading, valid and typed as msd_fields_to_float says (:1197-1212) */
    {
        int hv = f->heading_valid;
        unsigned htype = f->heading_type;
        msd_aircraft_heading h;
        h.raw = f->heading_raw;
        h.ew = 0;
        h.ns = 0;
        h.kind = MSD_HDG_NONE;
        h.pad = 0;
        if (f->velocity_valid) {
            float v0 = 0, v2 = 0;
            (void)msd_pos_record_gs(f, &v0, &v2);
            if (v0 > 0) {
                htype = 1; /* HEADING_GROUND_TRACK */
                hv = 1;
                h.kind = MSD_HDG_VELOCITY;
                h.ew = f->ew_vel;
                h.ns = f->ns_vel;
            }
        }
        if (f->heading_valid) { /* the raw heading replaces the ground track's value, not its type */
            h.kind = (f->commb_format == 8 || f->commb_format == 9) ? MSD_HDG_COMMB : f->metype == 19 ? MSD_HDG_ES19 : MSD_HDG_SURFACE;
            h.ew = 0;
            h.ns = 0;
        } else {
            h.raw = 0;
        }
        if (hv) {
            a->heading_type = (uint8_t)htype;
            if (a->heading_type == 4) /* HEADING_MAGNETIC_OR_TRUE */
                a->heading_type = a->adsb_hrd;
            else if (a->heading_type == 5) /* HEADING_TRACK_OR_HEADING */
                a->heading_type = a->adsb_tah;
            if (a->heading_type == 1 && msd_trk_accept(a, MSD_AC_TRACK, source, now, 1, r))
                a->track = h;
            else if (a->heading_type == 3 && msd_trk_accept(a, MSD_AC_MAG_HEADING, source, now, 1, r))
                a->mag_heading = h;
            else if (a->heading_type == 2 && msd_trk_accept(a, MSD_AC_TRUE_HEADING, source, now, 1, r))
                a->true_heading = h;
        }
    }

    if ((f->commb_valid & MSD_COMMB_TRACK_RATE) && msd_trk_accept(a, MSD_AC_TRACK_RATE, source, now, 1, r))
        a->track_rate_q = f->track_rate_q;
    if ((f->commb_valid & MSD_COMMB_ROLL) && msd_trk_accept(a, MSD_AC_ROLL, source, now, 1, r))
        a->roll_q = f->roll_q;
    /* gs, ias, tas: msd_pos_feed (:1222-1235) */
    if ((f->commb_valid & MSD_COMMB_MACH) && msd_trk_accept(a, MSD_AC_MACH, source, now, 0, r))
        a->mach_raw = f->mach_raw;
    if (f->baro_rate_valid && msd_trk_accept(a, MSD_AC_BARO_RATE, source, now, 1, r))
        a->baro_rate = f->baro_rate;
    if (f->geom_rate_valid && msd_trk_accept(a, MSD_AC_GEOM_RATE, source, now, 1, r))
        a->geom_rate = f->geom_rate;

    if (f->airground != 0) { /* :1249-1258: an uncertain state does not replace fresh certain data */
        if (f->airground != 3 || !msd_trk_fresh(a, MSD_AC_AIRGROUND, now)) {
            if (msd_trk_accept(a, MSD_AC_AIRGROUND, source, now, 0, r))
                a->air_ground = f->airground;
        }
    }
    if (f->callsign_valid && msd_trk_accept(a, MSD_AC_CALLSIGN, source, now, 0, r))
        for (int i = 0; i < 8; ++i)
            a->callsign[i] = f->callsign[i];
    if ((f->nav_valid & MSD_NAV_MCP_ALTITUDE) && msd_trk_accept(a, MSD_AC_NAV_ALTITUDE_MCP, source, now, 0, r))
        a->nav_altitude_mcp = f->nav_mcp_altitude;
    if ((f->nav_valid & MSD_NAV_FMS_ALTITUDE) && msd_trk_accept(a, MSD_AC_NAV_ALTITUDE_FMS, source, now, 0, r))
        a->nav_altitude_fms = f->nav_fms_altitude;
    if (f->nav_altitude_source != 0 && msd_trk_accept(a, MSD_AC_NAV_ALTITUDE_SRC, source, now, 0, r))
        a->nav_altitude_src = f->nav_altitude_source;
    if ((f->nav_valid & MSD_NAV_HEADING) && msd_trk_accept(a, MSD_AC_NAV_HEADING, source, now, 0, r)) {
        a->nav_heading_raw = f->nav_heading_raw;
        a->nav_heading_v2 = (f->nav_valid & MSD_NAV_HEADING_V2) != 0;
    }
    if ((f->nav_valid & MSD_NAV_MODES) && msd_trk_accept(a, MSD_AC_NAV_MODES, source, now, 0, r))
        a->nav_modes |= f->nav_modes; /* :1281-1298 only ever set the flags */
    if ((f->nav_valid & MSD_NAV_QNH) && msd_trk_accept(a, MSD_AC_NAV_QNH, source, now, 0, r)) {
        a->nav_qnh_raw = f->nav_qnh_raw;
        a->nav_qnh_commb = (f->nav_valid & MSD_NAV_QNH_COMMB) != 0;
    }
    if (f->alert_valid && msd_trk_accept(a, MSD_AC_ALERT, source, now, 0, r))
        a->alert = f->alert;
    if (f->spi_valid && msd_trk_accept(a, MSD_AC_SPI, source, now, 0, r))
        a->spi = f->spi;

    /* :1313-1329: NIC / Rc of the CPR half this record stored (msd_pos_feed accepted it: updatePosition ran) */
    unsigned own_nic = 0, own_rc = 0;
    const int cpr_new = f->cpr_valid && pos->result != MSD_POS_NOT_TRIED;
    if (cpr_new) {
        const int nic_a = msd_trk_valid(a, MSD_AC_NIC_A, now) && a->nic_a;
        const int nic_b = f->nic_b_valid && f->nic_b;
        const int nic_c = msd_trk_valid(a, MSD_AC_NIC_C, now) && a->nic_c;
        own_nic = msd_trk_compute_nic(f->metype, a->adsb_version, nic_a, nic_b, nic_c);
        own_rc = msd_trk_compute_rc(f->metype, a->adsb_version, nic_a, nic_b, nic_c);
        if (f->cpr_odd) {
            a->cpr_odd_nic = (uint8_t)own_nic;
            a->cpr_odd_rc = (uint16_t)own_rc;
        } else {
            a->cpr_even_nic = (uint8_t)own_nic;
            a->cpr_even_rc = (uint16_t)own_rc;
        }
    }

    if ((f->acc_valid & MSD_ACC_SDA) && msd_trk_accept(a, MSD_AC_SDA, source, now, 0, r))
        a->sda = f->sda;
    if ((f->acc_valid & MSD_ACC_NIC_A) && msd_trk_accept(a, MSD_AC_NIC_A, source, now, 0, r))
        a->nic_a = f->nic_a & 1u;
    if ((f->acc_valid & MSD_ACC_NIC_C) && msd_trk_accept(a, MSD_AC_NIC_C, source, now, 0, r))
        a->nic_c = f->nic_c & 1u;
    if ((f->acc_valid & MSD_ACC_NIC_BARO) && msd_trk_accept(a, MSD_AC_NIC_BARO, source, now, 0, r))
        a->nic_baro = f->nic_baro;
    if (nac_p_valid && msd_trk_accept(a, MSD_AC_NAC_P, source, now, 0, r))
        a->nac_p = (uint8_t)nac_p;
    if (f->nac_v_valid && msd_trk_accept(a, MSD_AC_NAC_V, source, now, 0, r))
        a->nac_v = f->nac_v;
    if (sil_type != 0 && msd_trk_accept(a, MSD_AC_SIL, source, now, 0, r)) { /* :1355-1360 */
        a->sil = (uint8_t)sil;
        if (a->sil_type == 0 || sil_type != 1)
            a->sil_type = (uint8_t)sil_type;
    }
    if ((f->acc_valid & MSD_ACC_GVA) && msd_trk_accept(a, MSD_AC_GVA, source, now, 0, r))
        a->gva = f->gva;
    /* :1366 accepts sda a second time: the same stores again */

    /* the geometric altitude derived from baro + delta (:1373-1378) */
    if (a->altitude_baro_reliable >= 3 && msd_trk_compare(a, MSD_AC_ALTITUDE_BARO, MSD_AC_ALTITUDE_GEOM, now) > 0 &&
        msd_trk_compare(a, MSD_AC_GEOM_DELTA, MSD_AC_ALTITUDE_GEOM, now) > 0) {
        a->alt_geom = a->alt_baro + a->geom_delta;
        /* combine_validity(&altitude_geom_valid, &altitude_baro_valid, &geom_delta_valid) */
        const int b = MSD_AC_ALTITUDE_BARO, d = MSD_AC_GEOM_DELTA, g = MSD_AC_ALTITUDE_GEOM;
        const int from = a->source[b] == 0 ? d : a->source[d] == 0 ? b : -1;
        if (from >= 0) {
            const uint64_t st = msd_trk_stale(a, from), ex = msd_trk_expires(a, from);
            a->source[g] = a->source[from];
            a->updated[g] = a->updated[from];
            a->altitude_geom_stale = st;
            a->altitude_geom_expires = ex;
            a->altitude_geom_stale_15s = from == b; /* `*to = *from` copies the stale interval too */
            if (r) /* and next_reduce_forward; the two-source branch leaves it alone */
                r->next[g] = r->next[from];
        } else {
            const uint64_t sb = msd_trk_stale(a, b), sd = msd_trk_stale(a, d);
            const uint64_t eb = msd_trk_expires(a, b), ed = msd_trk_expires(a, d);
            a->source[g] = a->source[b] < a->source[d] ? a->source[b] : a->source[d];
            a->updated[g] = a->updated[b] > a->updated[d] ? a->updated[b] : a->updated[d];
            a->altitude_geom_stale = sb < sd ? sb : sd;
            a->altitude_geom_expires = eb < ed ? eb : ed;
        }
    }

    /* updatePosition's NIC / Rc (:378-379, :458-473, :662-674) */
    if (cpr_new && pos->result >= 0) {
        unsigned nic, rc;
        if (pos->result == 0) { /* global: the worse of the two halves */
            nic = a->cpr_even_nic < a->cpr_odd_nic ? a->cpr_even_nic : a->cpr_odd_nic;
            rc = a->cpr_even_rc > a->cpr_odd_rc ? a->cpr_even_rc : a->cpr_odd_rc;
        } else {
            nic = own_nic;
            rc = own_rc;
            if (pos->result == 1) { /* relative to the aircraft's last position */
                if (a->nic < nic)
                    nic = a->nic;
                if (a->rc < rc)
                    rc = a->rc;
            }
        }
        a->nic = (uint8_t)nic;
        a->rc = (uint16_t)rc;
        nicrc->nic = (uint8_t)nic;
        nicrc->rc = (uint16_t)rc;
        nicrc->set = 1;
    }

    if (r && m->msgtype == 11 && m->iid == 0 && m->correctedbits == 0 && now > r->next[MSD_AC_N]) { /* :1396-1400 */
        r->next[MSD_AC_N] = now + (uint64_t)interval * 4u;
        r->forward = 1;
    }
    return r ? red.forward : 0;
}

/* The SBS row of a record (modes_hip.h "SBS output"), in two halves as the record is fed in two: what the position feed
 * knows -- acc is msd_pos_feed's after this record, messages the aircraft's -- and what the table entry holds after
 * msd_trk_feed. */
MSD_HD void msd_pos_sbs(const msd_position *pos, const msd_pos_acc *acc, uint64_t messages, msd_sbs_track *row)
{
    const msd_sbs_track z = {0};
    *row = z;
    row->flags = (uint8_t)(MSD_SBS_TRACKED | (messages > 1 ? MSD_SBS_SEEN_TWICE : 0u) | (acc->gs_valid ? MSD_SBS_GS_VALID : 0u) |
                           (pos->decoded ? MSD_SBS_CPR_DECODED : 0u));
    row->lat = pos->lat;
    row->lon = pos->lon;
    row->gs_selected = acc->gs_selected;
}

MSD_HD void msd_trk_sbs(const msd_trk_aircraft *a, uint64_t now, msd_sbs_track *row)
{
    row->geom_delta = a->geom_delta;
    if (msd_trk_valid(a, MSD_AC_GEOM_DELTA, now))
        row->flags |= MSD_SBS_GEOM_DELTA_VALID;
}

/* trackRemoveStaleAircraft's EXPIRE list for an aircraft that stays (:1520-1563).  No line for nac_v, emergency, alert
 * and spi: their source is never cleared. */
MSD_HD void msd_trk_expire_one(msd_trk_aircraft *a, uint64_t now)
{
    for (int k = 0; k < MSD_AC_N; ++k) {
        if (k == MSD_AC_NAC_V || k == MSD_AC_EMERGENCY || k == MSD_AC_ALERT || k == MSD_AC_SPI)
            continue;
        if (a->source[k] != 0 && now >= msd_trk_expires(a, k))
            a->source[k] = 0;
    }
    if (a->source[MSD_AC_ALTITUDE_BARO] == 0)
        a->altitude_baro_reliable = 0;
}

/* a table entry as msd_pos_snapshot delivers it: the key, the position state's members, the rest from the table */
MSD_HD void msd_trk_export(uint64_t key, const msd_pos_aircraft *p, const msd_trk_aircraft *t, msd_aircraft *out)
{
    const unsigned char from[MSD_PV_N] = {MSD_AC_GS, MSD_AC_IAS, MSD_AC_TAS, MSD_AC_CPR_ODD, MSD_AC_CPR_EVEN, MSD_AC_POSITION};
    *out = *t;
    out->receiver = (uint32_t)(key >> 25);
    out->addr = (uint32_t)(key & 0x1FFFFFFu);
    out->seen = p->seen;
    out->messages = p->messages;
    out->lat = p->lat;
    out->lon = p->lon;
    out->gs = p->gs;
    out->ias = p->ias;
    out->tas = p->tas;
    out->pos_reliable_odd = p->reliable_odd;
    out->pos_reliable_even = p->reliable_even;
    for (int k = 0; k < MSD_PV_N; ++k) {
        out->source[from[k]] = p->src[k];
        out->updated[from[k]] = p->upd[k];
    }
    out->adsb_version = p->version[0];
    out->tisb_version = p->version[1];
    out->adsr_version = p->version[2];
}

#endif
