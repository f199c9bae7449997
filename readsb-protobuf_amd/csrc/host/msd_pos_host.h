/* msd_pos_host.h -- the host twin of the position tracker (modes_hip.h, "positions"): the same object compiled for the
 * host from msd_cpr_impl.h and msd_pos_impl.h, fed record by record in stream order.  Same signatures as msd_pos_*
 * without the device; msd_pos_stats.min_gate_margin_m is the margin the contract in modes_hip.h speaks of. */
#ifndef MSD_POS_HOST_H
#define MSD_POS_HOST_H

#include "modes_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msd_pos_host msd_pos_host;
int msd_pos_host_create(const msd_pos_config *cfg, msd_pos_host **out); /* cfg->device is ignored */
void msd_pos_host_destroy(msd_pos_host *p);
int msd_pos_host_reset(msd_pos_host *p);
int msd_pos_host_set_receiver(msd_pos_host *p, uint32_t receiver, const msd_pos_receiver *rx);
int msd_pos_host_update(msd_pos_host *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver,
                        size_t n, msd_position *out);
int msd_pos_host_expire(msd_pos_host *p, uint64_t now_ms);
/* the aircraft table (modes_hip.h, "the aircraft table"): msd_pos_create_table, msd_pos_update_nicrc and
 * msd_pos_snapshot on the host, from msd_trk_impl.h; the same bytes */
int msd_pos_host_create_table(const msd_pos_config *cfg, msd_pos_host **out);
int msd_pos_host_update_nicrc(msd_pos_host *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver,
                              size_t n, msd_position *out, msd_pos_nicrc *nicrc);
int msd_pos_host_snapshot(msd_pos_host *p, msd_aircraft *out, size_t cap, size_t *n);
/* Mode A/C matching (modes_hip.h, "Mode A/C matching"): msd_pos_modeac_* on the host, from msd_modeac_impl.h; the same bytes */
int msd_pos_host_modeac_enable(msd_pos_host *p);
int msd_pos_host_modeac_match(msd_pos_host *p, uint64_t now_ms, uint64_t message_now_ms);
int msd_pos_host_modeac_codes(msd_pos_host *p, uint32_t receiver, msd_modeac_code *out);
int msd_pos_host_modeac_hits(msd_pos_host *p, msd_modeac_hit *out, size_t cap, size_t *n);
/* reduced Beast output (modes_hip.h, "Reduced Beast output"): msd_pos_reduce_enable, msd_pos_update_reduce and
 * msd_pos_reduce_wire on the host; the rule from msd_trk_impl.h, the frames from msd_beast_frame_out; the same bytes */
int msd_pos_host_reduce_enable(msd_pos_host *p, uint32_t interval_ms);
int msd_pos_host_update_reduce(msd_pos_host *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver,
                               size_t n, msd_position *out, msd_pos_nicrc *nicrc, uint8_t *forward);
int msd_pos_host_reduce_wire(msd_pos_host *p, const msd_message *msgs, const uint8_t *forward, size_t n, uint32_t flags,
                             uint8_t *out, size_t cap, size_t *out_len, uint32_t *ends);
/* SBS output (modes_hip.h, "SBS output"): msd_pos_sbs_enable, msd_pos_update_sbs and msd_pos_sbs_wire on the host; the
 * rows from the same walk, the text from snprintf, gmtime_r and the libm -- the yardstick of the device's writer */
int msd_pos_host_sbs_enable(msd_pos_host *p);
int msd_pos_host_update_sbs(msd_pos_host *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver,
                            size_t n, msd_position *out, msd_pos_nicrc *nicrc, uint8_t *forward, msd_sbs_track *trk);
int msd_pos_host_sbs_wire(msd_pos_host *p, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk, size_t n,
                          const msd_sbs_options *opt, uint8_t *out, size_t cap, size_t *out_len, uint32_t *ends);
/* aircraft.pb (modes_hip.h, "aircraft.pb"): msd_pos_pb_enable and msd_pos_aircraft_pb on the host -- a plain sequential
 * encoder over msd_pos_host_snapshot's entries with msd_aircraft_to_float and the libm's log10, the yardstick of the
 * device's writer.  min_rssi_margin_ulps (or NULL): the smallest distance, over every aircraft the call wrote, between the
 * double 10 * log10(...) and the nearest midpoint of two adjacent floats, in ulps of that double; +infinity without one */
int msd_pos_host_pb_enable(msd_pos_host *p);
int msd_pos_host_aircraft_pb(msd_pos_host *p, const msd_pb_options *opt, uint8_t *out, size_t cap, size_t *out_len,
                             msd_pb_receiver *rx, double *min_rssi_margin_ulps);
/* VRS output (modes_hip.h, "VRS output"): msd_pos_vrs_enable and msd_pos_vrs on the host -- a plain sequential writer
 * over msd_pos_host_snapshot's entries, snprintf with the reference's format strings, the yardstick of the device's
 * writer.  msd_pos_host_vrs_object: one entry's object at now_ms, with a comma in front when `comma`, into out
 * (MSD_VRS_AIRCRAFT_MAX + 1 bytes at least; NUL-terminated) -> its length; it does not look at selection */
int msd_pos_host_vrs_enable(msd_pos_host *p);
int msd_pos_host_vrs(msd_pos_host *p, const msd_vrs_options *opt, uint8_t *out, size_t cap, size_t *out_len, msd_vrs_receiver *rx);
size_t msd_pos_host_vrs_object(const msd_aircraft *a, uint64_t now_ms, int comma, char *out);
/* history_N.pb (modes_hip.h, "history_N.pb"): msd_pos_history_pb on the host -- a plain sequential encoder over
 * msd_pos_host_snapshot's entries that shares no code with the device's (msd_history_impl.h), the yardstick of the device's
 * writer.  No enable and no state, as on the device; -EINVAL without a table.  CONTRACT: the device and this object deliver
 * the same stream and the same rows on every table on which they hold the same msd_aircraft bytes; no libm function is
 * called on either side, so there is no margin.  msd_pos_host_history_entry: one entry's `history` element at now_ms into
 * out (MSD_HISTORY_ENTRY_MAX bytes at least, or NULL) -> its length; it does not look at selection */
int msd_pos_host_history_pb(msd_pos_host *p, const msd_history_options *opt, uint8_t *out, size_t cap, size_t *out_len,
                            msd_history_receiver *rx);
size_t msd_pos_host_history_entry(const msd_aircraft *a, uint64_t now_ms, uint8_t *out);
/* the receiver range (modes_hip.h, "Receiver range"): msd_pos_range_* on the host -- msd_pos_impl.h's per-record function
 * with the host's libm, record after record in stream order.  Its margins are the contract's */
int msd_pos_host_range_enable(msd_pos_host *p, uint32_t flags);
int msd_pos_host_range_read(msd_pos_host *p, uint32_t first, uint32_t count, msd_range_receiver *out, uint32_t flags);
int msd_pos_host_range_distances(msd_pos_host *p, uint32_t *out, size_t cap, size_t *n);
int msd_pos_host_range_margins(const msd_pos_host *p, msd_range_margins *m);
int msd_pos_host_range_pb(msd_pos_host *p, uint8_t *out, size_t cap, size_t *out_len, uint64_t *end);
/* for tests: the MSD_AC_N + 1 timers of one aircraft (the members' in MSD_AC_* order, then the DF11 timer) into out;
 * -ENOENT: no such aircraft */
int msd_pos_host_reduce_timers(const msd_pos_host *p, uint32_t receiver, uint32_t addr, uint64_t *out);
int msd_pos_host_get_stats(const msd_pos_host *p, msd_pos_stats *st);
/* the home slot of (receiver, addr) in a table of `capacity` slots (tests build collisions with it) */
uint32_t msd_pos_host_home_slot(uint32_t receiver, uint32_t addr, uint32_t capacity);
/* cpr.c's three decoders as msd_cpr_impl.h states them */
int msd_cpr_host_airborne(int even_lat, int even_lon, int odd_lat, int odd_lon, int fflag, double *lat, double *lon);
int msd_cpr_host_surface(double reflat, double reflon, int even_lat, int even_lon, int odd_lat, int odd_lon, int fflag,
                         double *lat, double *lon);
int msd_cpr_host_relative(double reflat, double reflon, int cprlat, int cprlon, int fflag, int surface, double *lat,
                          double *lon);

#ifdef __cplusplus
}
#endif
#endif
