/* msd_pos.h -- what msd_pos.cpp (the C-ABI of the position tracker) launches from msd_pos_kernels.hip and from its six
 * writers (msd_reduce_kernels.hip, msd_sbs_kernels.hip, msd_pb_kernels.hip, msd_vrs_kernels.hip, msd_range_kernels.hip,
 * msd_history_kernels.hip).  Every function queues
 * kernels on `stream` and returns; all pointers are device memory.  The tables and the call structs are raw pointers
 * because kernels take them by value; msd_pos.cpp owns what they point into. */
#ifndef MSD_POS_H
#define MSD_POS_H

#include <hip/hip_runtime.h>

#include "msd_modeac_impl.h"

#define MSD_POS_TILE 256u          /* records per workgroup of a counting pass */
#define MSD_POS_PIECE (1u << 20)   /* records grouped and walked at a time; a call of more is cut into pieces */
#define MSD_POS_MAX_N (1u << 24)   /* records per call */
/* ctl words of a call */
enum { MSD_POS_CTL_FULL = 0, MSD_POS_CTL_BAD_RECEIVER = 1, MSD_POS_CTL_INSERTED = 2, MSD_POS_CTL_REMOVED = 3, MSD_POS_CTL_N = 4 };
/* device counters: MSD_PC_N sums, then the bits of the smallest gate margin (a non-negative double orders as its bits) */
#define MSD_POS_DSTATS (MSD_PC_N + 1)

typedef struct msd_pos_table {
    uint64_t *keys;        /* cap entries; MSD_POS_EMPTY = free */
    msd_pos_aircraft *st;  /* cap entries */
    msd_trk_aircraft *trk; /* cap entries of a table tracker (msd_pos_create_table), else NULL */
    uint8_t *hits;         /* 2 * cap bytes {modeA_hit, modeC_hit} of a tracker that matches Mode A/C replies, else NULL */
    uint64_t *next_reduce; /* MSD_REDUCE_TIMERS * cap timers of a tracker that reduces (msd_trk_reduce), else NULL */
    uint32_t *dist;        /* cap distances (a->meta.distance) of a tracker with the receiver range, else NULL */
    uint32_t cap;          /* a power of two */
} msd_pos_table;

void msd_pos_launch_fill(hipStream_t stream, uint64_t *keys, uint32_t cap);
/* step 1: slot[i] of every record (cap for a skipped one, whose out[i] is written here), fresh[i] = 1 where this record
 * inserted its aircraft; ctl says whether the table overflowed or a receiver index was out of range */
void msd_pos_launch_find(hipStream_t stream, msd_pos_table t, const msd_message *msgs, const msd_fields *fields,
                         const uint32_t *receiver, uint32_t nrx, uint32_t n, uint32_t *slot, uint8_t *fresh, msd_position *out,
                         uint32_t *ctl);
void msd_pos_launch_rollback(hipStream_t stream, msd_pos_table t, const uint32_t *slot, const uint8_t *fresh, uint32_t n);
/* steps 2 to 4 for records base .. base + n (n <= MSD_POS_PIECE): idx_a / idx_b hold n words each, hist
 * 256 * ceil(n / MSD_POS_TILE) words.  With t.trk, step 5: the table walk over the same grouped order, which reads the
 * out[] of step 3 and writes nicrc[] (n entries from base).  With t.next_reduce, the reduce instantiations of both walks:
 * forward[] (as out[], zeroed by the caller) gets every walked record's verdict byte, reduce_interval is in ms.  With sbs
 * (as out[], zeroed by the caller; a table tracker), the SBS instantiations: every walked record's row.  With rcode (as
 * out[], zeroed by the caller; a tracker with the receiver range), the range instantiation of the position walk: every
 * walked record's msd_pos_range_code, MSD_RANGE_CODE_LAST on each aircraft's last decoded record of the piece */
void msd_pos_launch_piece(hipStream_t stream, msd_pos_table t, const msd_message *msgs, const msd_fields *fields,
                          const uint32_t *receiver, const msd_pos_receiver *rx, int filter_persistence, uint32_t base,
                          uint32_t n, const uint32_t *slot, uint32_t *idx_a, uint32_t *idx_b, uint32_t *hist,
                          msd_position *out, unsigned long long *dstats, msd_pos_nicrc *nicrc, uint32_t reduce_interval,
                          uint8_t *forward, msd_sbs_track *sbs, uint8_t *rcode);
/* The receiver range (msd_pos_impl.h, "the receiver range").  Per receiver, 304 bytes that are msd_range_receiver's with
 * the double's bits where longest_m / longest_nm will be; margins: the bits of the two smallest margins.
 * range: one lane per record of the piece base .. base + n, behind the piece's walk: the maxima into rng[receiver],
 * combined per wavefront first when `combine`, and t.dist[slot] from the records that carry MSD_RANGE_CODE_LAST.
 * read: rows first .. first + count as msd_range_receiver into out, `take` zeroing longest behind it.
 * distances: the snapshot's ordering passes, then out[j] = the distance of the aircraft in the j-th slot */
typedef struct msd_range_state {
    uint32_t polar[MSD_RANGE_BUCKETS];
    unsigned long long longest_bits, evaluated;
} msd_range_state;
void msd_pos_launch_range(hipStream_t stream, msd_pos_table t, const msd_position *out, const uint32_t *receiver,
                          const msd_pos_receiver *rx, const uint32_t *slot, const uint8_t *rcode, uint32_t base, uint32_t n,
                          int polar, int combine, msd_range_state *rng, unsigned long long *margins);
void msd_pos_launch_range_read(hipStream_t stream, msd_range_state *rng, uint32_t first, uint32_t count, int take,
                               msd_range_receiver *out);
void msd_pos_launch_range_distances(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits, uint32_t *idx_a,
                                    uint32_t *idx_b, uint32_t *hist, uint32_t *out);
#ifdef __cplusplus
extern "C" {
#endif
int msd_pos_range_measure(msd_pos *p, int combine, int timing); /* msd_pos.cpp; for scripts/range_rate.py */
int msd_pos_range_kernel_ms(const msd_pos *p, float *ms);
#ifdef __cplusplus
}
#endif
/* expiry: marks and counts the aircraft to remove (ctl[MSD_POS_CTL_REMOVED]); rebuild inserts the others into `to` */
void msd_pos_launch_expire(hipStream_t stream, msd_pos_table t, uint64_t now_ms, uint32_t *ctl);
void msd_pos_launch_rebuild(hipStream_t stream, msd_pos_table from, msd_pos_table to);
/* snapshot of a table tracker: the slots of the `live` aircraft in ascending key order end up in one of idx_a / idx_b
 * (cap words each; hist: 256 * ceil(cap / MSD_POS_TILE) words), from where their entries are gathered into out[0 .. live).
 * key_bits: no key has a bit set at or above it */
void msd_pos_launch_snapshot(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits, uint32_t *idx_a,
                             uint32_t *idx_b, uint32_t *hist, msd_aircraft *out);
/* Mode A/C matching (msd_modeac_impl.h).  ac: the receivers' arrays, MSD_MODEAC_WORDS words each.
 * count: one for every record with msgtype 32 of a call that has passed its checks (every receiver index below nrx) */
void msd_pos_launch_modeac_count(hipStream_t stream, const msd_message *msgs, const msd_fields *fields,
                                 const uint32_t *receiver, uint32_t nrx, uint32_t n, uint32_t *ac);
/* trackMatchAC: match cleared, one lane per slot, one lane per (receiver, code) */
void msd_pos_launch_modeac_match(hipStream_t stream, msd_pos_table t, uint32_t nrx, uint64_t now_ms, uint64_t message_now_ms,
                                 const uint16_t *c_to_a, uint32_t *ac);
void msd_pos_launch_modeac_codes(hipStream_t stream, const uint32_t *rx_ac, msd_modeac_code *out);
/* the hits in the snapshot's order; buffers as msd_pos_launch_snapshot's */
void msd_pos_launch_modeac_hits(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits, uint32_t *idx_a,
                                uint32_t *idx_b, uint32_t *hist, msd_modeac_hit *out);
/* Reduced Beast output (msd_reduce_kernels.hip): the Beast frames of the records whose verdict byte passes the delivery
 * conditions, dense and in record order.  lengths: lens[i] and block_sums[0 .. ceil(n / 256)] -- the workgroups' offsets,
 * then the stream's length.  store: the bytes to out (device memory, as many as block_sums' last word says) and ends[i] */
void msd_reduce_launch_lengths(hipStream_t stream, const msd_message *msgs, const uint8_t *forward, uint32_t n, uint32_t flags,
                               uint8_t *lens, uint32_t *block_sums);
void msd_reduce_launch_store(hipStream_t stream, const msd_message *msgs, uint32_t n, uint32_t flags, const uint8_t *lens,
                             const uint32_t *block_off, uint8_t *out, uint32_t *ends);
/* SBS output (msd_sbs_kernels.hip): the lines of the records that pass the delivery conditions, dense and in record
 * order; lengths and store as the reduced output's.  track_table: msd_sbs_build_track_table's entries in device memory */
void msd_sbs_launch_lengths(hipStream_t stream, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk,
                            uint32_t n, msd_sbs_options opt, const uint16_t *track_table, uint8_t *lens, uint32_t *block_sums);
void msd_sbs_launch_store(hipStream_t stream, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk,
                          uint32_t n, msd_sbs_options opt, const uint16_t *track_table, const uint8_t *lens,
                          const uint32_t *block_off, uint8_t *out, uint32_t *ends);
/* the snapshot's ordering passes alone: the slots of the `live` aircraft in ascending key order -> the one of idx_a /
 * idx_b that holds them (buffers as msd_pos_launch_snapshot's; live > 0) */
const uint32_t *msd_pos_launch_ordered_slots(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits,
                                             uint32_t *idx_a, uint32_t *idx_b, uint32_t *hist);
/* aircraft.pb (msd_pb_kernels.hip).  state: the written state, 8 bytes per slot beside the table (msd_pb_impl.h).
 * fresh: a call's new aircraft start at 0 (slot / fresh as msd_pos_launch_find left them).  move: after
 * msd_pos_launch_rebuild(from, to), every survivor's state follows it */
#define MSD_PB_TILE 128u /* items per LDS image of the store kernel; tests/test_gpu_aircraft_pb.py sizes its receivers
                            around this value (its TILE): change both together */
void msd_pb_launch_fresh(hipStream_t stream, const uint32_t *slot, const uint8_t *fresh, uint32_t n, uint32_t cap, uint64_t *state);
void msd_pb_launch_move(hipStream_t stream, msd_pos_table from, const uint64_t *from_state, msd_pos_table to, uint64_t *to_state);
/* The items of a call are the nrx file heads and the live aircraft in stream order (live + nrx of them; idx: the ordered
 * slots).  lengths: first[0 .. nrx], items[], and per item shadow (the next written state), lens, within / cwithin (the
 * exclusive prefixes inside its workgroup of 256: bytes; the three counts, packed); block_sums: four arrays of
 * ceil(items / 256) + 1 words -- bytes, written, with position, TIS-B --, the workgroups' offsets and then the total; rx:
 * nrx rows.  store: the bytes to out (device memory, as many as block_sums' first total says), and every written
 * aircraft's shadow into state */
typedef struct msd_pb_call {
    msd_pos_table t;
    uint64_t *state;                /* the written state, per slot */
    const uint32_t *dist;           /* the distances of a tracker that keeps the receiver range, per slot; else NULL */
    const uint32_t *idx;            /* the ordered slots */
    const uint32_t *items;
    const uint64_t *messages_total; /* per receiver, or NULL */
    const uint16_t *track_table;
    uint64_t now_ms;
    uint32_t nitems, nrx;
} msd_pb_call;
void msd_pb_launch_lengths(hipStream_t stream, msd_pb_call c, uint32_t live, uint32_t *first, uint32_t *items, uint64_t *shadow,
                           uint16_t *lens, uint32_t *within, uint32_t *cwithin, uint32_t *block_sums, msd_pb_receiver *rx);
void msd_pb_launch_store(hipStream_t stream, msd_pb_call c, const uint64_t *shadow, const uint16_t *lens, const uint32_t *block_off,
                         uint8_t *out);
/* Statistics.polar_range (msd_range_kernels.hip): the 72 entries of receivers 0 .. nrx - 1, dense and in order; lengths
 * and store as the reduced output's over the nrx * 72 entries; end[r]: receiver r's end offset */
void msd_range_pb_launch_lengths(hipStream_t stream, const msd_range_state *rng, uint32_t nrx, uint8_t *lens, uint32_t *block_sums);
void msd_range_pb_launch_store(hipStream_t stream, const msd_range_state *rng, uint32_t nrx, const uint8_t *lens,
                               const uint32_t *block_off, uint8_t *out, unsigned long long *end);
/* VRS output (msd_vrs_kernels.hip).  The items of a call are, per receiver, a head, its live aircraft and a tail, in
 * stream order (live + 2 * nrx of them; idx: the ordered slots).  select: first[0 .. nrx], items[], and per item lens
 * (an aircraft's without its comma; 0: not selected) and swithin (the selected aircraft before it inside its workgroup of
 * 256); sel_sums: ceil(items / 256) + 1 words, the workgroups' offsets and then the total.  lengths: the comma goes into
 * lens, within (the bytes before the item inside its workgroup) and byte_sums follow, rx: nrx rows.  store: the bytes to
 * out (device memory, as many as byte_sums' total says) */
#define MSD_VRS_TILE 128u /* items per LDS image of the store kernel; tests/vrs_streams.py sizes its receivers around
                             this value (its TILE): change both together */
typedef struct msd_vrs_call {
    msd_pos_table t;
    const uint32_t *idx, *items, *first;
    const uint16_t *track_table;
    uint64_t now_ms;
    uint32_t nitems, nrx, part, part_shift;
} msd_vrs_call;
void msd_vrs_launch_lengths(hipStream_t stream, msd_vrs_call c, uint32_t live, uint32_t *first, uint32_t *items, uint16_t *lens,
                            uint16_t *swithin, uint32_t *within, uint32_t *sel_sums, uint32_t *byte_sums, msd_vrs_receiver *rx);
void msd_vrs_launch_store(hipStream_t stream, msd_vrs_call c, const uint16_t *lens, const uint32_t *block_off, uint8_t *out);
/* history_N.pb (msd_history_kernels.hip).  The items of a call are aircraft.pb's: the nrx file heads and the live aircraft
 * in stream order (live + nrx of them; idx: the ordered slots).  lengths: first[0 .. nrx], items[], and per item lens (0:
 * not written), within / cwithin (the exclusive prefixes inside its workgroup of 256: bytes, written aircraft);
 * block_sums: two arrays of ceil(items / 256) + 1 words -- bytes, written --, the workgroups' offsets and then the total;
 * rx: nrx rows.  store: the bytes to out (device memory, as many as block_sums' first total says).  Neither changes the
 * table */
typedef struct msd_history_call {
    msd_pos_table t;
    const uint32_t *idx; /* the ordered slots */
    const uint32_t *items;
    uint64_t now_ms;
    uint32_t nitems, nrx;
} msd_history_call;
void msd_history_launch_lengths(hipStream_t stream, msd_history_call c, uint32_t live, uint32_t *first, uint32_t *items,
                                uint8_t *lens, uint16_t *within, uint16_t *cwithin, uint32_t *block_sums, msd_history_receiver *rx);
void msd_history_launch_store(hipStream_t stream, msd_history_call c, const uint8_t *lens, const uint32_t *block_off, uint8_t *out);

#endif
