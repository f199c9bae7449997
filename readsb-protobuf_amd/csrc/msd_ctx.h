/*
 * msd_ctx.h -- what the files of the stream driver share, with each other and with the receiver-group driver
 * (msd_group.cpp): the pipeline slot, the context itself, and the steps of the stream pipeline that are called across
 * a file boundary.  The driver is cut by stage:
 *   msd_capi.cpp     context lifetime and the exported functions
 *   msd_batch.cpp    everything that puts a batch on the GPU (the slot's buffers, enqueue, rescans, launch)
 *   msd_collect.cpp  everything that takes a batch off the GPU (the GPU resolve chain, the host fallback, delivery)
 * Private to the library.
 */
#ifndef MSD_CTX_H
#define MSD_CTX_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "modes_hip.h"
#include "msd_internal.h"
#include "msd_kernels.h"

namespace msd_impl {

constexpr uint64_t MIN_HIT_ARENA = 131072;      /* every position of one buffer */
constexpr uint64_t MIN_TRY_ARENA = 131072 * 5;  /* every phase of every position of one buffer */
constexpr int TAIL_SAMPLES = MSD_HALO_FRONT;    /* what a batch leaves for its successor's look-behind */
constexpr uint32_t SNAP_CAP = 64;               /* filter membership versions of one batch kept on the device */

/* One helper thread per context for the per-message part of finishing a batch (signal level, power
 * statistics, the copy into the caller's arrays), so that it overlaps with the calling thread queueing
 * the next batch's resolve.  At most one job at a time; run() returns at once, wait() joins it. */
struct Helper {
    /* one worker thread, jobs in order.  A job may call mark_delivered() when the part its poster waits for is
     * done; what it does after that is background work that the next job queues up behind.  Both sides spin for
     * a few hundred microseconds before they sleep: in a running stream the next event is never further away,
     * and a sleeping thread on a busy host comes back late. */
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<void()>> jobs;
    std::atomic<uint64_t> posted{0}, delivered{0}, finished{0}; /* jobs posted / past their delivery point / complete */
    bool stop = false;
    int device = 0;
    static void relax()
    {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
    template <typename Pred>
    static bool spin_for(Pred pred, int microseconds)
    {
        const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(microseconds);
        for (;;) {
            for (int i = 0; i < 64; ++i) {
                if (pred())
                    return true;
                relax();
            }
            if (std::chrono::steady_clock::now() >= until)
                return false;
        }
    }
    void loop()
    {
        (void)hipSetDevice(device);
        uint64_t taken = 0;
        for (;;) {
            (void)spin_for([&] { return posted.load(std::memory_order_acquire) > taken; }, 2000);
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !jobs.empty() || stop; });
            if (jobs.empty())
                return; /* stop, and nothing left to do */
            std::function<void()> job = std::move(jobs.front());
            jobs.pop_front();
            ++taken;
            lk.unlock();
            job();
            lk.lock();
            finished.store(taken, std::memory_order_release);
            if (delivered.load(std::memory_order_relaxed) < taken)
                delivered.store(taken, std::memory_order_release);
            cv.notify_all();
        }
    }
    void run(std::function<void()> f) /* does not wait: the job starts when the ones before it are complete */
    {
        std::unique_lock<std::mutex> lk(mu);
        if (!th.joinable())
            th = std::thread([this] { loop(); });
        jobs.push_back(std::move(f));
        posted.fetch_add(1, std::memory_order_release);
        cv.notify_all();
    }
    void mark_delivered() /* from the running job */
    {
        std::unique_lock<std::mutex> lk(mu);
        delivered.store(finished.load(std::memory_order_relaxed) + 1, std::memory_order_release);
        cv.notify_all();
    }
    void wait_delivered() /* the last job posted has passed its delivery point */
    {
        const uint64_t want = posted.load(std::memory_order_acquire);
        if (spin_for([&] { return delivered.load(std::memory_order_acquire) >= want; }, 2000))
            return;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return delivered.load(std::memory_order_acquire) >= want; });
    }
    void wait() /* everything posted is complete */
    {
        const uint64_t want = posted.load(std::memory_order_acquire);
        if (spin_for([&] { return finished.load(std::memory_order_acquire) >= want; }, 200))
            return;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return finished.load(std::memory_order_acquire) >= want; });
    }
    void shutdown()
    {
        wait();
        {
            std::unique_lock<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        if (th.joinable())
            th.join();
    }
};

/* A receiver group's call as the stream pipeline runs it (Slot::group): every buffer's look-behind comes from its
 * receiver's tail slot, its options from its receiver.  The arrays are indexed by buffer of the whole call; a slot's
 * batch starts batch_first / MSD_CHUNK_SAMPLES buffers into it (fill_params). */
struct GroupCall {
    const uint8_t *tails = nullptr; /* MsdScanParams.group_tails */
    const uint32_t *lb = nullptr;   /* every buffer's look-behind slot (MsdScanParams.group_lb) */
    const uint32_t *opt = nullptr;  /* every buffer's receiver options (MsdScanParams.group_opt) */
    /* the call's buffers whose receiver has Mode A/C on: ascending buffer indices, on the device (the group's control
     * rows) and on the host; nac 0: no Mode A/C in this call */
    const uint32_t *ac = nullptr;
    const uint32_t *ac_host = nullptr;
    uint32_t nac = 0;
    bool fix2 = false; /* some buffer of the call is at repair level 2: the two-bit tables, the FIX2 instantiation */
};

struct Slot {
    bool busy = false;
    bool download_started = false;
    bool gpu_resolve = false; /* the candidate lists stay in HBM: resolved there (msd_resolve_kernels.hip) */
    bool resolve_inflight = false; /* its first resolve pass (and the speculative message records) are queued */
    int threshold = 0;             /* Modes.preambleThreshold when the batch was launched */
    bool timed = false;            /* ev_start / ev_scan / ev_kernels were recorded for this batch */
    bool state_reset_done = false; /* ... and filter and clocks have been reset already (its chain was queued early) */
    bool reset_before = false;     /* msd_restart(): first batch of a new capture -- filter, clock and counters start
                                      over when its turn comes */
    bool dc = false;               /* --dcfilter: d_iq points at d_dcmag, the float sums come from d_magsq */
    uint16_t *d_dcmag = nullptr;   /* DC-blocked magnitudes of the batch (what the scan kernel reads) */
    float *d_magsq = nullptr;      /* their clamped squares, for the per-buffer float sums */
    uint64_t dropped_before = 0;   /* msd_note_dropped(): samples missing in front of this batch, not yet on the clock */
    uint32_t resolve_ntodo = 0;
    msd_rbuf *h_rbuf = nullptr;    /* pinned; the resolve kernel reports straight into it */
    msd_acc *d_acc = nullptr;
    uint32_t *d_adds = nullptr, *d_nmsgs = nullptr, *d_acc_ac = nullptr, *d_nac = nullptr;
    uint32_t *d_pred = nullptr; /* the batch's prediction table (msd_internal.h: MSD_PRED_WORDS), filled by its scan */
    uint32_t pred_gen = 0, pred_uses = 0; /* its generation for the batch in the slot; batches it has served */
    /* lean layout (UC8 / magnitudes, Mode S only, chain in order, resolve on the GPU): no gather kernel -- the
     * candidate lists stay in this slot's own region arenas until the batch's records are out, the resolve
     * workgroups read their buffer's region slices, the first resolve pass publishes sums and totals */
    bool lean = false;
    bool power_done = false; /* the batch's signal power kernel has been queued (d_powr, d_rec_off) */
    bool ahead_done = false; /* its resolve passes are through and its filter changes committed (by the msd_collect of
                                the batch before it); counters and delivery wait for its own msd_collect */
    int ahead_verdict = 0;   /* 1 / 2: the msd_collect before this batch's already found that the host resolver has to take
                                it / that its arenas overflowed (resolve_passes); nothing was committed */
    bool records_current = true; /* no further resolve pass ran after the one whose records were written */
    uint32_t npass = 0;
    uint64_t sample_counter0 = 0; /* the sample clock at the batch's first sample (gpu_begin) */
    msd_hit *d_rhits = nullptr;
    msd_try *d_rtries = nullptr;
    msd_region_counts *d_rcounts = nullptr;
    msd_wg_totals *d_rwgt = nullptr;
    uint32_t lean_k = 0, lean_hcap = 0, lean_tcap = 0, lean_nreg = 0; /* regions per buffer, slice capacities, regions */
    /* the slot's own arena sizes: the context's (msd_config) to begin with; grow_and_rescan() enlarges the region slices of
     * a slot whose batch overflowed them, lean_gather_now() the dense lists if somebody on the host wants such a batch */
    uint64_t rhit_arena = 0, rtry_arena = 0, dense_hits = 0, dense_tries = 0;
    uint64_t *d_powr = nullptr; /* [buffer][MSD_RB_MSG_CAP] signal power of the accepted messages */
    uint8_t *h_ctl = nullptr; /* pinned, read by the kernels in place: ts[2n] u64 | valid[n] | snap_idx[n] | todo[n] */
    msd_wire *h_wire = nullptr;                    /* pinned: the message records, written there by the kernels */
    unsigned long long *h_side = nullptr;          /* per record: power sum | signal_len << 48, for the statistics */
    msd_fields *h_fields = nullptr; /* pinned: header fields next to the records (MSD_CFG_DECODE_FIELDS) */
    hipEvent_t ev_resolve = nullptr, ev_records = nullptr, ev_power = nullptr;
    hipEvent_t ev_scanned = nullptr; /* side-stream layout: this batch's scan + gather are done (its float sums / Mode A/C kernels follow) */
    uint64_t launch_seq = 0;         /* running number of the launch that filled the slot */
    /* batch description */
    const uint8_t *d_iq = nullptr;
    const uint8_t *d_prev = nullptr;
    int have_prev = 0;
    uint64_t batch_first = 0; /* absolute sample index */
    uint64_t nsamples = 0;
    uint32_t nbuffers = 0;
    int last = 0;
    const GroupCall *group = nullptr; /* a receiver group's call (msd_group.cpp), null for a stream batch */
    /* device */
    msd_hit *d_hits = nullptr;
    msd_try *d_tries = nullptr;
    uint64_t *d_totals = nullptr;
    float *d_tile_sums = nullptr;    /* SC16 / SC16Q11: the scan's per-tile float sums, for the float-sum kernel's predictions */
    void *d_fm_work = nullptr;       /* 16-bit IQ, --dcfilter: the float-sum kernels' hand-over (msd_fm_work_bytes) */
    msd_ac_hit *d_ac_regions = nullptr; /* Mode A/C: the candidate kernel's region slices and counts, gathered into d_ac */
    msd_wg_counts *d_ac_counts = nullptr;
    uint32_t *d_rec_off = nullptr;   /* [max_buffers + 2] records in front of each buffer's (power kernel) */
    uint32_t *d_buf_first = nullptr; /* [max_buffers + 2] start of each buffer's hits in d_hits (gather kernel) */
    bool buf_first_valid = false;
    uint64_t *d_sums = nullptr;
    uint16_t *d_mag = nullptr;        /* Mode A/C: the batch's magnitudes as the scan computed them (MsdScanParams.mag_out) */
    const uint16_t *d_mag_prev = nullptr; /* ... and the last MSD_HALO_FRONT of the batch before, in that batch's own array */
    bool mag_pass = false;            /* this batch's Mode A/C candidate kernel reads d_mag */
    float *d_fmeans = nullptr;
    /* pinned host */
    uint64_t *h_totals = nullptr;
    uint64_t *h_sums = nullptr;
    float *h_fmeans = nullptr;
    msd_hit *h_hits = nullptr;
    size_t h_hits_cap = 0;
    msd_try *h_tries = nullptr;
    size_t h_tries_cap = 0;
    uint8_t *d_ragged = nullptr; /* zero-padded copy of a partially filled last 8-sample group */
    uint8_t *tail_dst = nullptr; /* where the gather kernel leaves the batch's last samples for its successor */
    uint8_t *d_upload = nullptr; /* msd_launch_host: this slot's copy of the batch in HBM */
    hipEvent_t ev_upload = nullptr;
    /* Mode A/C candidates */
    msd_ac_hit *d_ac = nullptr;
    uint64_t *d_ac_totals = nullptr, *h_ac_totals = nullptr;
    msd_ac_hit *h_ac = nullptr;
    size_t h_ac_cap = 0;
    /* deferred signal power of the accepted messages */
    uint64_t *d_req = nullptr, *d_pow = nullptr, *h_req = nullptr, *h_pow = nullptr;
    size_t req_cap = 0;
    hipEvent_t ev_start = nullptr, ev_scan = nullptr, ev_kernels = nullptr, ev_totals = nullptr,
               ev_copy0 = nullptr, ev_copy1 = nullptr;
};

} /* namespace msd_impl */

struct msd_ctx {
    msd_config cfg{};
    hipStream_t stream = nullptr, copy_stream = nullptr, aux_stream = nullptr, emit_stream = nullptr;
    bool own_stream = false;
    int bps = 2;
    msd_tables *tables = nullptr;
    uint16_t *d_lut = nullptr;
    uint32_t *d_crc = nullptr, *d_syn56 = nullptr, *d_syn112 = nullptr, *d_slicer = nullptr, *d_synhash = nullptr;
    uint64_t *d_fix2[2] = {nullptr, nullptr}; /* two-bit correction tables for 56 / 112 bits (nfix_crc == 2) */
    uint32_t fix2_lg[2] = {0, 0};
    /* per-workgroup candidate regions (shared by all batches: stream order serialises them) */
    msd_hit *d_region_hits = nullptr;
    msd_try *d_region_tries = nullptr;
    uint64_t hit_arena = 0, try_arena = 0;
    uint64_t *h_conv = nullptr; /* msd_convert_begin / _end: the sums of the conversion in flight (page-locked) */
    bool conv_pending = false;
    unsigned conv_n = 0;
    const msd_magbuf_view *magbuf_views = nullptr; /* msd_demodulate_magbufs: the caller's buffers while its finish() runs */
    const uint32_t *magbuf_noise = nullptr;        /* ... and their Mode A/C noise levels (demod_2400.c:530-531 from the caller's
                                                      means), for a batch that has to be scanned again in pieces */
    unsigned magbuf_nviews = 0;
    double want_hits_per_sample = 0, want_tries_per_sample = 0; /* region slices a slot should have at its next launch (grow_and_rescan) */
    msd_region_counts *d_counts = nullptr; /* per region (wavefront) of the scan kernel */
    msd_wg_totals *d_wg_totals = nullptr;  /* per workgroup of the scan kernel */
    uint32_t max_wg = 0, max_buffers = 0;  /* max_wg: most regions a scan is split into */
    /* Mode A/C candidate regions */
    uint64_t ac_arena = 0;
    uint64_t *d_ac_offsets = nullptr;
    uint32_t *d_noise = nullptr;
    void *d_fm_work = nullptr;       /* 16-bit IQ, --dcfilter: the float-sum kernels' hand-over (msd_fm_work_bytes) */
    uint32_t ac_max_wg = 0;
    unsigned long long *d_timers = nullptr; /* MSD_KERNEL_TIMING experiments */
    /* GPU resolve stage: per-buffer reports, accepted-message records, filter snapshots, control arrays */
    bool gpu_resolve = false;
    uint32_t *d_snaps = nullptr, *h_snaps = nullptr;
    uint32_t snaps_uploaded = 0;
    uint32_t inline_adds = MSD_RB_ADD_INLINE; /* msd_config.test_inline_adds lowers it */
    bool want_fields = false;       /* MSD_CFG_DECODE_FIELDS */
    msd_fields_fn fsink = nullptr;  /* set while msd_collect_fields runs: messages go here with their fields */
    void *fuser = nullptr;
    std::vector<msd_fields> out_fields; /* host-resolve path */
    hipEvent_t ev_aux = nullptr, ev_inputs = nullptr;
    msd_pred_entry *h_pred = nullptr;
    uint32_t *h_pred_count = nullptr;
    msd_pred_patch *h_patches = nullptr;
    uint32_t npatches = 0;
    /* the last MSD_HALO_FRONT samples of the previous batch, one buffer per pipeline stage + 1 */
    uint8_t *d_tail[MSD_PIPELINE_DEPTH + 1] = {};
    int tail_cur = 0;
    bool have_prev = false;
    uint8_t *d_stage = nullptr; /* msd_submit_host / msd_convert / msd_demodulate_magbuf staging */
    uint16_t *d_mag = nullptr;
    msd_impl::Slot slots[MSD_PIPELINE_DEPTH];
    int head = 0, outstanding = 0;
    uint64_t next_sample = 0;
    bool finished = false;
    uint64_t pending_dropped = 0; /* msd_note_dropped() since the last launch */
    bool restart_pending = false; /* msd_restart() since the last launch */
    const uint16_t *mag_prev = nullptr; /* Mode A/C: where the previous batch's last magnitudes are (its slot's d_mag) */
    uint32_t timing_interval = 1; /* msd_set_timing_interval() */
    /* experiment knobs, read from the environment once in msd_create */
    bool trace = false;      /* MSD_RESOLVE_TRACE */
    /* In-order layout without field decoding: the record kernel of a batch is not launched; the wavefronts of the
     * next scan write the records on their way in (MsdScanParams.emit).  pending_emit: resolve chain and signal
     * power queued, records not yet.  MSD_EMIT_FUSED=0 turns it off. */
    std::vector<uint32_t> bg_valid, bg_buf; /* the statistics half of finishing a batch, on the helper thread */
    std::vector<double> bg_means;
    std::vector<uint64_t> bg_scaled; /* per message: power sum | signal_len << 48 (msd_emit_impl.h) */
    bool emit_fused = false;
    bool power_fused = true; /* no signal power kernel: the resolve workgroups sum it (MSD_POWER_FUSED=0 keeps the kernel) */
    msd_impl::Slot *pending_emit = nullptr;
    bool chain_inline = true; /* MSD_CHAIN_INLINE=0: resolve chain on side streams instead of in order on the scan stream */
    bool lean_ok = false;     /* the configuration allows the lean layout (Slot::lean; MSD_LEAN=0 turns it off) */
    bool wait_inputs_on_stream = false; /* MSD_WAIT_INPUTS_ON_STREAM=1: the resolve kernel's stream waits for the snapshot upload */
    bool resolve_ahead = true; /* msd_collect also takes the next batch through its resolve passes (MSD_RESOLVE_AHEAD=0: no) */
    int debug_flags = 0;     /* MSD_DEBUG_FLAGS */
    uint64_t enqueue_seq = 0;
    uint64_t launch_count = 0;
    bool dc = false;              /* MSD_CFG_DC_FILTER */
    int q11_bits = 0;             /* msd_config.sc16q11_table_bits in effect: the batches' IQ goes through d_q11_table first */
    uint16_t *d_q11_table = nullptr;
    float *d_conv_magsq = nullptr; /* msd_convert of a MSD_CFG_DC_FILTER context: the clamped squares of the call's samples */
    float dc_a = 0, dc_b = 1;     /* struct converter_state, convert.c:28-33,479-482 */
    float *d_dcstate = nullptr;   /* z1_I, z1_Q on the device, carried from batch to batch */
    void *d_dc_work = nullptr;    /* the parallel-in-time DC filter's blocks, tables and control word (msd_dcp_work_bytes) */
    bool dc_last_parallel = false; /* the most recent DC block went through the parallel kernels (msd_dc_filter_status) */
    uint32_t dc_last_blocks = 0;
    bool dc_fused = false;        /* MSD_CFG_DC_FUSED_LAUNCH: the passes in one cooperative launch (measured slower) */
    int dc_passes = 24;           /* passes queued per batch (MSD_CFG_DC_ONE_PASS: 1, so that the in-order kernel behind them runs) */
    int scan_format = 0;          /* what the scan and its follow-up kernels read: cfg.format, or MAG16 behind the DC filter */
    size_t scan_bps = 2;
    msd_resolver resolver{};
    msd_stats stats{};
    msd_timing timing{};
    std::vector<double> means;
    std::vector<uint32_t> valid;
    std::vector<msd_message> out_msgs;
    std::vector<uint64_t> out_req;
    std::vector<uint32_t> out_buf;
    int cu_count = 256;
    msd_impl::Helper helper;
    bool failed = false;    /* a batch could not be finished: only msd_reset() / msd_destroy() are accepted */
    bool scan_queued = false; /* enqueue(): its scan kernel is on the stream (a later failure cannot be undone) */
    bool no_helper = false; /* MSD_NO_HELPER: everything on the calling thread */
    void *frames = nullptr; /* Beast / AVR input (msd_frames.cpp) */
    char err[256] = {0};
};

#pragma GCC visibility push(hidden) /* shared by the library's files, not part of its interface */
namespace msd_impl {

/* the batch in the slot has a Mode A/C pass: the context's configuration, or a receiver group call with some receiver on */
inline bool ac_on(const msd_ctx *c, const Slot &s)
{
    return c->cfg.mode_ac || (s.group && s.group->nac);
}

/* the batch in the slot can be resolved on the GPU */
inline bool gpu_eligible(const msd_ctx *c, const Slot &s)
{
    return c->gpu_resolve && s.nbuffers >= 4;
}

inline size_t bps_of(int format) /* bytes per sample */
{
    return (format == MSD_FMT_UC8 || format == MSD_FMT_MAG16) ? 2 : 4;
}

/* the message in c->err; returns code */
int fail(msd_ctx *c, int code, const char *fmt, ...);

#define HIPCHK(c, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((c), -EIO, "%s failed: %s", #call, hipGetErrorString(e_));              \
    } while (0)

/* Enqueue the GPU stage of the batch in the slot: scan, lists, Mode A/C, sums. */
int enqueue(msd_ctx *c, Slot &s, int format, const uint32_t *host_noise, bool pipelined = false);
/* Stage 1 of finishing a batch: once its totals are known, start the download of its candidate lists (an arena overflow
 * is scanned again in pieces here). */
int start_download(msd_ctx *c, Slot &s, int format);
/* the slot's power request / record buffers, pinned candidate lists and Mode A/C list, grown to at least the size given */
int ensure_req(msd_ctx *c, Slot &s, size_t n);
int ensure_host(msd_ctx *c, Slot &s, size_t nh, size_t nt);
int ensure_ac_host(msd_ctx *c, Slot &s, size_t nac);
/* the scan parameters of the slot's batch (a group call's look-behind, options and two-bit tables included) */
void fill_params(const msd_ctx *c, const Slot &s, MsdScanParams &p);
/* an overflowed batch again: in pieces for the host resolver; a lean one into bigger region slices (0: rescanned, 1: not
 * possible); a lean batch's dense lists after all */
int rerun_in_pieces(msd_ctx *c, Slot &s, int format);
int grow_and_rescan(msd_ctx *c, Slot &s, int format);
int lean_gather_now(msd_ctx *c, Slot &s);
/* --dcfilter: the batch's IQ -> DC-blocked magnitudes and squares, in order on `stream` */
int launch_dc_block(msd_ctx *c, const void *d_iq, uint64_t nsamples, uint16_t *d_mag, float *d_magsq, hipStream_t stream);
/* msd_collect behind its argument checks: finish() of the oldest batch in flight */
int collect(msd_ctx *c, msd_message_fn sink, void *user);
/* Wait for a batch's lists, resolve in order, deliver messages. */
int finish(msd_ctx *c, Slot &s, int format, msd_message_fn sink, void *user, const uint64_t *ts_override,
           const double *means_override, uint64_t resolver_first_chunk);
/* hipEventSynchronize for events that are about to fire: polls first */
hipError_t event_wait(hipEvent_t ev);
/* the first resolve pass of the slot's batch (and its speculative records) behind its own kernels */
int gpu_begin(msd_ctx *c, Slot &s, int format);
/* the records of the batch whose chain was queued last, if no scan came along to carry them */
int flush_pending_emit(msd_ctx *c);

/* the slot's control arrays of the GPU resolve stage, in pinned host memory */
struct GpuCtl {
    uint64_t *h_ts;
    uint32_t *h_valid, *h_snap, *h_todo;
};
GpuCtl gpu_ctl(const msd_ctx *c, const Slot &s);
void gpu_params(const msd_ctx *c, const Slot &s, MsdResolveParams &rp);

/* The two-bit correction tables (--aggressive, crc.c:374-379) into c->d_fix2 / c->fix2_lg: both or, on failure, neither.
 * *host_oom: a table could not be built in host memory. */
hipError_t upload_fix2(msd_ctx *c, bool *host_oom);

} /* namespace msd_impl */
#pragma GCC visibility pop

#endif
