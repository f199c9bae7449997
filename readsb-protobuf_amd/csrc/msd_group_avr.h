/*
 * msd_group_avr.h -- AVR raw text input per receiver of a group (msd_group_accept_avr): what
 * msd_group.cpp (the entry, its checks), msd_group_remote.cpp (pieces, scratch, the receivers' kept lines) and
 * msd_group_avr_kernels.hip share.
 *
 * The layout is the Beast input's (msd_group_beast.h): a call is cut into pieces of whole entries, and in a piece every
 * entry has a segment [s0, s1) -- its kept incomplete line (at most MSD_AVR_LINE_MAX bytes) followed by its new bytes
 * --, s0 a multiple of MSD_AVR_SPAN = MSD_FR_TILE, so that the '\n' of a span belong to one receiver and the span ->
 * entry map is the filter stage's tile_ent.  The entries are msd_gb_entry records (tl: the bytes of kept line), with two
 * more bits in `opt`; the filter stage is the Beast input's own (msd_gb_launch_filter_records).
 */
#ifndef MSD_GROUP_AVR_H
#define MSD_GROUP_AVR_H

#include "msd_avr.h"
#include "msd_group_beast.h"

#if MSD_AVR_SPAN != MSD_FR_TILE
#error "a span of the line framing must be a tile of the filter stage"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* msd_gb_entry.opt, beside MSD_GB_OPT_NFIX and MSD_GB_OPT_MODEAC */
#define MSD_GA_OPT_KEEP_TS 0x200u /* the entry's MSD_AVR_KEEP_TIMESTAMP */
#define MSD_GA_OPT_DISCARD 0x400u /* its segment begins inside an overlong line (and tl is 0) */

/* per-entry counters in the spare words of the MSD_FR_CTR_* row (MSD_FR_CTR_NODES: the lines that became a record;
 * MSD_GB_CTR_REC_FIRST, MSD_GB_CTR_NEW_FIRST as for Beast; MSD_GB_CTR_NTL: the bytes of incomplete line it leaves in
 * `lines_out`) */
enum {
    MSD_GA_CTR_LINES = 20,   /* complete lines */
    MSD_GA_CTR_DROPPED = 21, /* ... that msd_avr_parse_line refuses */
    MSD_GA_CTR_LONG = 22,    /* ... of more than MSD_AVR_LINE_MAX bytes */
    MSD_GA_CTR_DISCARD = 23  /* 1: it ends inside an overlong line */
};

typedef struct msd_ga_scratch {
    /* n, ntiles (spans), len, ent, tile_ent (span -> entry), buf (the piece), cnt ([spans + 1] records per span, then
     * the spans' first records), nodes (the records' '\n'), cls, addr, ctr, tot (MSD_GB_TOT_NODES: the records), and
     * what only the filter stage touches */
    msd_gb_scratch f;
    const uint8_t *lines_in; /* [n][MSD_AVR_LINE_MAX] the kept lines */
    uint8_t *lines_out;      /* [n][MSD_AVR_LINE_MAX] the lines to keep */
    msd_message *rec;        /* [records] as msd_avr_launch_store leaves them, entry after entry in stream order */
} msd_ga_scratch;

/* Layout (src: the call's bytes), line framing per span, the spans' offsets, the parsed records, the end of every
 * segment and the class of every record.  Leaves the totals in f.tot and the per-entry counters in f.ctr. */
int msd_ga_launch_frame_decode(const uint8_t *src, const msd_fr_tables *t, const msd_ga_scratch *s, void *stream);

/* the driver is the Beast input's: msd_gr_accept (msd_group_beast.h, msd_group_remote.cpp) */

#ifdef __cplusplus
}
#endif
#endif
