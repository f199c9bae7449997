/*
 * msd_avr.h -- AVR raw text input on the GPU (msd_accept_avr): what the kernels of msd_avr_kernels.hip and the host
 * side in msd_frames.cpp share.  DESIGN.md section 4.8 has the framing rule.
 *
 * A piece is the incomplete line the previous one left (at most MSD_AVR_LINE_MAX bytes, `tail`) followed by new bytes
 * (`data`), both in device memory; byte positions are piece-relative 32-bit numbers, as in msd_frames.h.  With
 * `discard` set the piece begins inside an overlong line (and tl is 0).
 */
#ifndef MSD_AVR_H
#define MSD_AVR_H

#include <stddef.h>
#include <stdint.h>

#include "modes_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSD_AVR_SPAN 4096u    /* bytes whose '\n' one workgroup owns */
#define MSD_AVR_LOOKBACK 320u /* bytes in front of its span a workgroup also classifies: >= MSD_AVR_LINE_MAX + 1, in 64s */

/* device counters of a piece, in the counter block of msd_frames.h (uint64 each; the framing runs before the decision
 * stage clears the block for its own counters) */
enum {
    MSD_AVR_CTR_RECORDS = 0, /* lines that yield a record */
    MSD_AVR_CTR_LINES,
    MSD_AVR_CTR_DROPPED,
    MSD_AVR_CTR_LONG,
    MSD_AVR_CTR_LAST_NL /* 1 + the position of the piece's last '\n'; 0: none */
};

/* Counts per workgroup, their offsets and the totals.  wg: [spans + 1] words, spans = ceil(n / MSD_AVR_SPAN); ctr: the
 * counter block, cleared here.  n = tl + the new bytes. */
int msd_avr_launch_count(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, int discard, int mode_ac,
                         uint32_t *wg, unsigned long long *ctr, void *stream);
/* The records, dense and in stream order: msg, msgbits, timestampMsg, signalLevel as msd_avr_parse_line leaves them,
 * every other field zero (msd_fr_launch_records_decode decides them again).  out: ctr[MSD_AVR_CTR_RECORDS] records. */
int msd_avr_launch_store(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, int discard, int mode_ac,
                         int keep_timestamp, const uint32_t *wg, msd_message *out, void *stream);

/* the constants above, for tests that place lines across the kernels' boundaries */
uint32_t msd_avr_span_bytes(void);
uint32_t msd_avr_lookback_bytes(void);
uint32_t msd_avr_piece_bytes(void);

#ifdef __cplusplus
}
#endif
#endif
