/*
 * msd_group_beast.h -- Beast input per receiver of a group (msd_group_accept_beast): what
 * msd_group.cpp (the entry, its checks), msd_group_remote.cpp (pieces, scratch, the receivers' framing state) and
 * msd_group_beast_kernels.hip share.
 *
 * A call is laid out as pieces of whole entries.  In a piece every entry has a segment [s0, s1): its kept incomplete
 * frame followed by its new bytes, s0 a multiple of MSD_FR_TILE, so that no tile of the chain walk holds bytes of two
 * receivers.  Byte positions are piece-relative 32-bit numbers; "none" is the segment's own end s1.
 */
#ifndef MSD_GROUP_BEAST_H
#define MSD_GROUP_BEAST_H

#include <stddef.h>
#include <stdint.h>

#include "modes_hip.h"
#include "msd_frames.h"
#include "msd_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one entry of a piece, as the kernels read it */
typedef struct msd_gb_entry {
    uint64_t src;         /* where its new bytes start in the call's byte array (device memory) */
    uint64_t pending_gap; /* bytes behind its last frame that no 0x1A has charged yet */
    uint64_t now_ms;
    uint32_t s0, s1;      /* its segment of the piece */
    uint32_t tl;          /* bytes of kept frame at s0 */
    uint32_t tile0, ntiles; /* its tiles: ceil((s1 - s0) / MSD_FR_TILE) from s0 / MSD_FR_TILE on */
    uint32_t snap;        /* its filter snapshot: snaps + snap * MSD_SNAP_WORDS */
    uint32_t opt;         /* MSD_GB_OPT_*: its repair level and Mode A/C switch */
    uint32_t pad;
} msd_gb_entry;
#define MSD_GB_OPT_NFIX(o) ((o)&0xffu)
#define MSD_GB_OPT_MODEAC 0x100u

/* per-entry counters: MSD_FR_CTR_* of msd_frames.h (MSD_FR_CTR_WORDS uint64 each; NODES, NEW and RECORDS are the
 * entry's own counts, LAST_END is relative to s0), and in the spare words: */
enum {
    MSD_GB_CTR_REC_FIRST = 17, /* its first record in `out` */
    MSD_GB_CTR_NEW_FIRST = 18, /* its first address in `newaddr` */
    MSD_GB_CTR_NTL = 19        /* bytes of incomplete frame it leaves in `tails_out` (more than MSD_FR_TAIL_MAX: an error) */
};
/* totals of a piece */
enum { MSD_GB_TOT_NODES = 0, MSD_GB_TOT_ADDS, MSD_GB_TOT_CAND, MSD_GB_TOT_WORDS = 4 };

typedef struct msd_gb_scratch {
    uint32_t n;              /* entries of the piece */
    uint32_t ntiles, len;    /* tiles of the piece; len = ntiles * MSD_FR_TILE */
    const msd_gb_entry *ent; /* [n] */
    const uint32_t *tile_ent; /* [ntiles] the entry a tile belongs to */
    const uint8_t *tails_in; /* [n][MSD_FR_TAIL_MAX] the kept frames */
    uint8_t *tails_out;      /* [n][MSD_FR_TAIL_MAX] the frames to keep */
    uint8_t *buf;            /* [len] the piece */
    uint32_t *first;         /* [ntiles] first 0x1A at or after the tile's start, in its segment (s1: none) */
    uint32_t *nxt;           /* [ntiles] the same from the tile's end on */
    uint32_t *succ;          /* [len] as msd_fr_scratch */
    uint16_t *info;          /* [len] */
    uint8_t *mark;           /* [len] */
    uint32_t *exitl, *entry; /* [ntiles] */
    uint8_t *good;           /* [ntiles] */
    uint32_t *cnt;           /* [ntiles + 1] nodes per tile, then the tiles' first nodes */
    uint32_t *nodes;         /* [nodes] positions of the true chains, entry after entry */
    uint8_t *cls;            /* [nodes] MSD_FR_C_* */
    uint32_t *addr;          /* [nodes] */
    uint32_t *flags;         /* [nodes] compaction */
    uint32_t *off;           /* [nodes + 1] offsets of new adds, then of records */
    uint32_t *scan_tmp;
    uint32_t *newlist;       /* [adds] */
    uint32_t *newaddr;       /* [adds] every entry's new addresses in order of first add, entry after entry */
    unsigned long long *hash; /* [2 * hslots] entry << 32 | address; first add | member-from stamp << 32 */
    uint32_t hslots;
    uint32_t *snaps;         /* the receivers' filter snapshots */
    uint32_t *add_first;     /* [n + 1] the entries' ranges in newaddr, for msd_group_filter_apply_kernel */
    msd_message *out;        /* [records] entry after entry, stream order within one */
    uint8_t *errbits;        /* [records][2] the repaired bit positions of out[k] (0xff: none), for a verbatim wire call;
                                NULL in every other call */
    unsigned long long *ctr; /* [n][MSD_FR_CTR_WORDS] */
    unsigned long long *tot; /* [MSD_GB_TOT_WORDS] */
} msd_gb_scratch;

/* Stages 1 and 2 of a piece: lay it out (src: the call's bytes), successor graph, tile chains, one wavefront per entry
 * for the in-order reconciliation, the node list, the end of every segment and the class of every node.  Leaves the
 * totals in tot and the per-entry counters in ctr. */
int msd_gb_launch_chain_decode(const uint8_t *src, const msd_fr_tables *t, const msd_gb_scratch *s, void *stream);
/* Stage 3: first adds per (entry, address), the ordered inserts one workgroup per entry, verdicts and records.
 * hslots a power of two >= 2 * nadds when nadds > 0. */
int msd_gb_launch_filter(uint32_t nnodes, uint32_t nadds, const msd_fr_tables *t, const msd_gb_scratch *s, void *stream);
/* The same stage over records that are framed already (the AVR text input, msd_group_avr.h): record k is in[k], parsed
 * as msd_avr_parse_line leaves it; nodes[k] is any position of its entry's segment (its line's '\n'), cnt[] the
 * tiles' first records.  The records are written from `in`; buf, info and the chain arrays are not read. */
int msd_gb_launch_filter_records(const msd_message *in, uint32_t nnodes, uint32_t nadds, const msd_fr_tables *t,
                                 const msd_gb_scratch *s, void *stream);

/* ---- the output stage of both remote inputs (msd_group_remote_out_kernels.hip) ---- */
/* The records of a piece are out[0 .. *count), *count <= bound: `count` is the last word of the filter stage's scan
 * (off + nnodes), device memory; `bound` what the host knows after the first synchronisation (MSD_GB_TOT_CAND).
 * fields[k] = msd_decode_fields(out[k], NULL). */
int msd_gro_launch_fields(const msd_message *out, const uint32_t *count, uint32_t bound, msd_fields *fields, void *stream);
/* The records as one dense stream of Beast frames or AVR lines in `bytes` (page-locked host memory, at least
 * MSD_GRO_WIRE_MAX * bound bytes), and every entry's part of it from its counter row: ranges[2 e] its first byte,
 * ranges[2 e + 1] its bytes (0xffffffff: its records are not among the piece's); ranges is page-locked memory as well.
 * errbits: NULL, or for verbatim output the repaired positions beside the records (msd_gb_scratch.errbits).
 * lens [bound], block_sums [bound / 256 + 2] and starts [bound] are device scratch. */
#define MSD_GRO_WIRE_MAX 44u /* MSD_WIRE_MAX of msd_wire_impl.h */
int msd_gro_launch_wire(const msd_message *out, const uint32_t *count, uint32_t bound, const unsigned long long *ctr,
                        uint32_t n, int format, const uint8_t *errbits, uint8_t *lens, uint32_t *block_sums, uint32_t *starts,
                        uint8_t *bytes, uint32_t *ranges, void *stream);

/* what a call delivers instead of bare records: msd_group_accept_*_fields (want_fields) or _wire (want_wire); a sink
 * may be NULL */
typedef struct msd_gb_out {
    int want_fields, want_wire;
    msd_group_fields_fn fsink;
    msd_group_wire_fn wsink;
    int format;   /* MSD_WIRE_* */
    int verbatim; /* MSD_WIRE_VERBATIM */
} msd_gb_out;

/* ---- the driver of both remote inputs (msd_group_remote.cpp) ---- */
enum { MSD_GR_BEAST = 0, MSD_GR_AVR = 1 };

typedef struct msd_gr_input { /* one entry of a call, checked by the caller */
    uint32_t receiver;
    uint32_t nbytes;
    uint32_t flags; /* AVR: MSD_AVR_KEEP_TIMESTAMP; Beast: 0 */
    uint64_t offset;
    uint64_t now_ms;
    msd_filter *filter; /* the receiver's host filter */
    int nfix;           /* its repair level */
    int mode_ac;        /* its Mode A/C switch */
} msd_gr_input;

typedef struct msd_gb_view { /* what the driver needs of a group */
    int format; /* MSD_GR_* */
    void *stream;
    int device;
    uint32_t max_receivers;
    msd_fr_tables tables;
    uint32_t *d_snaps; /* the receivers' resident snapshots ([max_receivers][MSD_SNAP_WORDS]); NULL: a group that
                          resolves on the host, the call then uploads the snapshots of its own receivers */
    msd_remote_stats *remote; /* [max_receivers] the receivers' remote counters, which both inputs add to */
    void **state;      /* the driver's own of this format (scratch and the receivers' carries), created by its first call */
    char *err;
    size_t errlen;
} msd_gb_view;

/* 0, or a negative errno with the text in v->err; -EIO leaves the receivers' state undefined.  out: NULL for the plain
 * call (records to `sink`), else the fields or wire call (`sink` is not used) */
int msd_gr_accept(const msd_gb_view *v, const void *bytes, int on_device, const msd_gr_input *in, uint32_t n,
                  msd_group_message_fn sink, const msd_gb_out *out, void *user);
/* state: NULL, or what a call left in *v->state (it knows its format); avr_state: of MSD_GR_AVR calls */
void msd_gr_reset_receiver(void *state, uint32_t receiver);
void msd_gr_get_avr_stats(const void *avr_state, uint32_t receiver, msd_avr_stats *st);
void msd_gr_free(void *state); /* with the group's device current: releases the scratch */

#ifdef __cplusplus
}
#endif
#endif
