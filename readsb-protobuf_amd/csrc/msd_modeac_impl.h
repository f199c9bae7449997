/* msd_modeac_impl.h -- trackMatchAC, one implementation for the table kernels (device) and the host twin
 * (libmsd_host.so): which Mode A/C replies belong to an aircraft the table tracks.  Restated from the reference:
 *   modeAToIndex / indexToModeA track.h:246-256, modeACInit's modeCToATable and modeCToModeA mode_ac.c:63-98,
 *   the count of trackUpdateFromMessage track.c:999-1003, trackMatchAC track.c:1411-1485.
 * The two resets of the hits inside trackUpdateFromMessage (:1096-1102, :1154-1156) are in msd_trk_feed.
 *
 * The reference keeps one set of modeAC_count / _lastcount / _match / _age[4096] (track.c:59-62); here every receiver
 * has its own, laid out as four arrays of 4096 words one after the other (64 KiB per receiver), and an aircraft is matched
 * against its own receiver's.  modeA_hit / modeC_hit are two bytes per slot beside the table entry, not in it.
 * Integer logic only: the device and the host agree bit for bit. */
#ifndef MSD_MODEAC_IMPL_H
#define MSD_MODEAC_IMPL_H

#include "msd_fields_impl.h" /* msd_mode_a_to_c */
#include "msd_trk_impl.h"

#define MSD_MODEAC_CODES 4096u
#define MSD_MODEAC_MIN_MESSAGES 4u /* TRACK_MODEAC_MIN_MESSAGES, track.h:66 */
/* the four arrays of a receiver, in words from the receiver's base */
enum { MSD_MODEAC_COUNT = 0, MSD_MODEAC_LASTCOUNT = 4096, MSD_MODEAC_MATCH = 8192, MSD_MODEAC_AGE = 12288, MSD_MODEAC_WORDS = 16384 };

MSD_HD unsigned msd_mode_a_to_index(unsigned mode_a) /* modeAToIndex */
{
    return (mode_a & 0x0007u) | ((mode_a & 0x0070u) >> 1) | ((mode_a & 0x0700u) >> 2) | ((mode_a & 0x7000u) >> 3);
}

MSD_HD unsigned msd_index_to_mode_a(unsigned index) /* indexToModeA */
{
    return (index & 00007u) | ((index & 00070u) << 1) | ((index & 00700u) << 2) | ((index & 07000u) << 3);
}

/* modeACInit's modeCToATable: table[C + 13] = the Mode A code whose Gillham altitude is C hundreds of feet, 0 where
 * there is none.  No two codes share a C (the reference asserts it; tests/test_modeac_model.py checks it). */
MSD_HD void msd_modeac_build_c_to_a(uint16_t *table)
{
    for (unsigned i = 0; i < MSD_MODEAC_CODES; ++i)
        table[i] = 0;
    for (unsigned i = 0; i < MSD_MODEAC_CODES; ++i) {
        const unsigned mode_a = msd_index_to_mode_a(i);
        const int32_t c = msd_mode_a_to_c(mode_a);
        if (c == MSD_INVALID_ALTITUDE)
            continue;
        if (c + 13 >= 0 && c + 13 < (int32_t)MSD_MODEAC_CODES)
            table[c + 13] = (uint16_t)mode_a;
    }
}

MSD_HD unsigned msd_modeac_c_to_a(const uint16_t *table, int mode_c) /* modeCToModeA */
{
    if (mode_c < -13 || mode_c >= (int)MSD_MODEAC_CODES - 13) /* before the sum: any int may come in */
        return 0;
    return table[mode_c + 13];
}

/* (alt + 49) / 100 of :1097-1098 and :1435: C's division, towards zero */
MSD_HD int msd_modeac_mode_c(int alt_baro)
{
    return (alt_baro + 49) / 100;
}

/* modeAC_match[i] = modeAC_match[i] ? 0xFFFFFFFF : addr.  On the device aircraft arrive in any order: the first
 * compare-and-swap finds 0 and leaves its address, every later one finds a value and stores all ones -- the same word
 * whatever the order.  addr is never 0 (a record with address 0 is not tracked). */
MSD_HD void msd_modeac_mark(uint32_t *match, uint32_t addr)
{
#ifdef __HIP_DEVICE_COMPILE__
    if (atomicCAS(match, 0u, addr) != 0u)
        __hip_atomic_store(match, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *match = *match ? 0xFFFFFFFFu : addr;
#endif
}

MSD_HD int msd_modeac_live(const uint32_t *rx, unsigned i) /* heard often enough since the last match, :1427 */
{
    return (uint32_t)(rx[MSD_MODEAC_COUNT + i] - rx[MSD_MODEAC_LASTCOUNT + i]) >= MSD_MODEAC_MIN_MESSAGES;
}

/* One aircraft of trackMatchAC's scan (:1420-1457): `a` its table entry, `seen` its meta.seen, `rx` its receiver's four
 * arrays, hits its two bytes {modeA_hit, modeC_hit}.  now is trackMatchAC's argument, message_now what messageNow()
 * returns inside trackDataValid. */
MSD_HD void msd_modeac_match_one(const msd_trk_aircraft *a, uint64_t seen, uint32_t addr, uint64_t now, uint64_t message_now,
                                 const uint16_t *c_to_a, uint32_t *rx, uint8_t *hits)
{
    if ((uint64_t)(now - seen) > 5000u) /* unsigned: an aircraft seen after `now` is skipped too */
        return;
    if (msd_trk_valid(a, MSD_AC_SQUAWK, message_now)) {
        const unsigned i = msd_mode_a_to_index(a->squawk);
        if (msd_modeac_live(rx, i)) {
            hits[0] = 1;
            msd_modeac_mark(&rx[MSD_MODEAC_MATCH + i], addr);
        }
    }
    if (msd_trk_valid(a, MSD_AC_ALTITUDE_BARO, message_now)) {
        const int mode_c = msd_modeac_mode_c(a->alt_baro);
        for (int d = 0; d < 3; ++d) { /* C, C + 1, C - 1 */
            const unsigned mode_a = msd_modeac_c_to_a(c_to_a, mode_c + (d == 2 ? -1 : d));
            const unsigned i = msd_mode_a_to_index(mode_a);
            if (mode_a && msd_modeac_live(rx, i)) {
                hits[1] = 1;
                msd_modeac_mark(&rx[MSD_MODEAC_MATCH + i], addr);
            }
        }
    }
}

/* One code of the ageing loop (:1462-1484), after every aircraft has been matched */
MSD_HD void msd_modeac_age_one(uint32_t *rx, unsigned i)
{
    const uint32_t count = rx[MSD_MODEAC_COUNT + i];
    if (!count)
        return;
    if (!msd_modeac_live(rx, i)) {
        const uint32_t age = rx[MSD_MODEAC_AGE + i] + 1u;
        rx[MSD_MODEAC_AGE + i] = age;
        if (age > 15u) { /* not heard from for a while */
            rx[MSD_MODEAC_COUNT + i] = 0;
            rx[MSD_MODEAC_AGE + i] = 0;
            rx[MSD_MODEAC_LASTCOUNT + i] = 0; /* :1483 copies the cleared count */
            return;
        }
    } else {
        rx[MSD_MODEAC_AGE + i] = rx[MSD_MODEAC_MATCH + i] ? 10u : 0u;
    }
    rx[MSD_MODEAC_LASTCOUNT + i] = count;
}

MSD_HD void msd_modeac_export_code(const uint32_t *rx, unsigned i, msd_modeac_code *out)
{
    out->count = rx[MSD_MODEAC_COUNT + i];
    out->lastcount = rx[MSD_MODEAC_LASTCOUNT + i];
    out->match = rx[MSD_MODEAC_MATCH + i];
    out->age = rx[MSD_MODEAC_AGE + i];
}

MSD_HD void msd_modeac_export_hit(uint64_t key, const uint8_t *hits, msd_modeac_hit *out)
{
    out->receiver = (uint32_t)(key >> 25);
    out->addr = (uint32_t)(key & 0x1FFFFFFu);
    out->mode_a_hit = hits[0];
    out->mode_c_hit = hits[1];
    for (int k = 0; k < 6; ++k)
        out->pad[k] = 0;
}

#endif
