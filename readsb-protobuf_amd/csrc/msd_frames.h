/*
 * msd_frames.h -- Beast / AVR input on the GPU (msd_accept_beast, msd_accept_frames): what the kernels of
 * msd_frames_kernels.hip and the host side in msd_frames.cpp share.  DESIGN.md section 4.8 has the algorithm.
 *
 * One call is cut into pieces of at most MSD_FR_PIECE bytes; a piece is the incomplete frame the previous one left
 * (at most MSD_FR_TAIL_MAX bytes, `tail`) followed by new bytes (`data`), both in device memory.  Byte positions are
 * piece-relative 32-bit numbers.
 */
#ifndef MSD_FRAMES_H
#define MSD_FRAMES_H

#include <stddef.h>
#include <stdint.h>

#include "modes_hip.h"
#include "msd_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSD_FR_PIECE (1u << 23)   /* new bytes per piece: about 30 bytes of device scratch each */
#define MSD_FR_TAIL_MAX 64u       /* an incomplete frame: at most 2 + 2 * 26 bytes */
#define MSD_FR_TILE 4096u         /* bytes per tile of the chain walk */
#define MSD_FR_INC 0x80000000u    /* chain value: an incomplete frame starts at (value & ~MSD_FR_INC) */
#define MSD_FR_NEVER 0xFFFFFFFFu

/* node kinds (info & 0xff); info >> 8 = bytes from the 0x1A to the next scan point (eom, or + 1 for a skip) */
enum { MSD_FR_K_NONE = 0, MSD_FR_K_SKIP = 1, MSD_FR_K_INC = 2 }; /* frames carry their type byte: '1'..'5', 'H' */

/* per-node class after the decode stage */
enum {
    MSD_FR_C_NONE = 0,   /* not a message: skip, '4', '5', 'H', or '1' with mode_ac off */
    MSD_FR_C_ACC = 1,    /* accepted without the filter */
    MSD_FR_C_ADD = 2,    /* accepted without the filter, and icaoFilterAdd(addr) (clean DF17, DF11 with zero syndrome) */
    MSD_FR_C_TEST = 3,   /* accepted iff icaoFilterTest(addr) */
    MSD_FR_C_BAD = 4,    /* decodeModesMessage returns -2 */
    MSD_FR_C_UNKNOWN = 5, /* after the verdict: -1 */
    MSD_FR_C_MODEAC = 6  /* a type '1' frame delivered as a Mode A/C record */
};

/* device counters of a piece (uint64 each) */
enum {
    MSD_FR_CTR_NODES = 0, MSD_FR_CTR_MODES, MSD_FR_CTR_MODEAC, MSD_FR_CTR_BAD, MSD_FR_CTR_UNKNOWN, MSD_FR_CTR_ACC0,
    MSD_FR_CTR_ACC1, MSD_FR_CTR_ACC2, MSD_FR_CTR_FRAMES, MSD_FR_CTR_OTHER, MSD_FR_CTR_GARBAGE, MSD_FR_CTR_ADDS,
    MSD_FR_CTR_NEW, MSD_FR_CTR_RECORDS, MSD_FR_CTR_EXIT, MSD_FR_CTR_REWALKS, MSD_FR_CTR_LAST_END, MSD_FR_CTR_WORDS = 24
};

typedef struct msd_fr_tables {
    const uint32_t *crc_byte; /* msd_tables.crc_byte */
    const uint32_t *synhash;  /* msd_tables.synhash; NULL with --no-fix */
    uint32_t synh_mul56, synh_mul112;
    const uint64_t *fix2[2];  /* --aggressive: the (2, 4) tables for 56 / 112 bits */
    uint32_t fix2_lg[2];
    int nfix;
    int mode_ac;
} msd_fr_tables;

typedef struct msd_fr_scratch {
    uint32_t *succ;    /* [n] the next node of a node (a 0x1A position), n for none, or MSD_FR_INC | p */
    uint16_t *info;    /* [n] kind | scan length << 8, at 0x1A positions */
    uint8_t *mark;     /* [n] on the tile's own chain */
    uint32_t *first;   /* [ntiles + 1] first 0x1A at or after the tile's start (n: none) */
    uint32_t *exitl;   /* [ntiles] where the tile's own chain leaves it */
    uint32_t *entry;   /* [ntiles] where the true chain enters it */
    uint8_t *good;     /* [ntiles] entered at exitl[t - 1], the true chain follows the tile's own chain */
    uint32_t *cnt;     /* [n + 1] nodes per tile, then offsets (of tiles, new adds, records) */
    uint32_t *nodes;   /* [nodes] positions of the true chain */
    uint8_t *cls;      /* [nodes] MSD_FR_C_* */
    uint32_t *addr;    /* [nodes] the address added or tested */
    uint32_t *flags;   /* [nodes + 1] compaction */
    uint32_t *scan_tmp; /* block sums of the scans */
    uint32_t *newlist; /* [adds] nodes that insert a new address, in order */
    uint32_t *newaddr; /* [adds] ... and their addresses, for the host's copy of the filter */
    uint32_t *hash;    /* [4 * hslots] key, first add, member-from stamp, pad */
    uint32_t hslots;
    const uint32_t *snap; /* MSD_SNAP_WORDS: the filter as the piece begins */
    msd_message *out;  /* [records] */
    unsigned long long *ctr; /* MSD_FR_CTR_WORDS */
} msd_fr_scratch;

/* words of scan_tmp the prefix sums over n elements need */
size_t msd_fr_scan_tmp_words(uint32_t n);

/* Stage 1: successor graph, tile chains, the in-order reconciliation and the node list.  Leaves the node count, the
 * final chain value and the rewalk count in ctr. */
int msd_fr_launch_chain(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, const msd_fr_scratch *s,
                        void *stream);
/* Stage 2: decode and class of every node (needs the node count on the host: nnodes); counters. */
int msd_fr_launch_decode(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, uint32_t nnodes,
                         uint64_t pending_gap, const msd_fr_tables *t, const msd_fr_scratch *s, void *stream);
/* Stage 3: first adds, ordered insertion, verdicts, records.  hslots must be a power of two >= 2 * adds. */
int msd_fr_launch_filter(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, uint32_t nnodes,
                         uint32_t nadds, uint64_t now_ms, const msd_fr_tables *t, const msd_fr_scratch *s,
                         void *stream);
/* Pre-framed records (msd_accept_frames): class every record the way stage 2 classes a frame. */
int msd_fr_launch_records_decode(const msd_message *in, uint32_t n, const msd_fr_tables *t, const msd_fr_scratch *s,
                                 void *stream);
int msd_fr_launch_records_filter(const msd_message *in, uint32_t n, uint32_t nadds, uint64_t now_ms,
                                 const msd_fr_tables *t, const msd_fr_scratch *s, void *stream);

/* What msd_frames.cpp needs of a context (msd_capi.cpp owns struct msd_ctx). */
typedef struct msd_frames_view {
    void *stream;
    int device;
    int busy;              /* batches outstanding */
    int failed;            /* only msd_reset / msd_destroy are accepted */
    msd_fr_tables tables;
    msd_filter *filter;    /* the live ICAO filter */
    void **state;          /* the context's msd_frames_state, created on first use */
    char *err;             /* msd_last_error text */
    size_t errlen;
} msd_frames_view;
int msd_frames_get_view(msd_ctx *ctx, msd_frames_view *v);
void msd_frames_free(void *state);
void msd_frames_reset(void *state);

#ifdef __cplusplus
}
#endif
#endif
