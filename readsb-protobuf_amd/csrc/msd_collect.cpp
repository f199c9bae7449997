/*
 * msd_collect.cpp -- the collect side of the stream driver: everything that takes a batch off the GPU.  finish() is one
 * batch from "kernels queued" to "messages delivered"; what puts it on the GPU is msd_batch.cpp, msd_ctx.h is shared.
 *
 * The resolve stage with the candidate lists left in HBM: one workgroup per buffer against a snapshot of the ICAO
 * filter; the host only replays the buffers' add lists to find the snapshot every buffer has to see (msd_resolve.c)
 * and re-launches the ones that saw another: gpu_begin -> resolve_passes -> commit -> begin_successor.  finish_gpu()
 * drives that chain one batch ahead of the delivery and leaves the per-message half to the helper thread; the host
 * resolver is the fallback.
 *
 * Queueing: the first pass over a batch, the message records and their signal power are queued on the scan stream (or,
 * DESIGN.md 4.6, the high-priority aux / emit streams) as soon as the previous batch is committed, often long before
 * anybody waits for them; everything they report lands in pinned host memory, the host waits for one event.  The aux
 * stream carries the rare further passes of the side-stream layout, the signal-power round trip and the list download
 * of a batch the host resolves.
 */
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "modes_hip.h"
#include "msd_ctx.h"
#include "msd_internal.h"
#include "msd_kernels.h"

#pragma GCC visibility push(hidden) /* internal, shared between the library's files through msd_ctx.h */
namespace msd_impl {

using Clock = std::chrono::steady_clock;

static double ms_between(Clock::time_point a, Clock::time_point b)
{
    return std::chrono::duration<double, std::milli>(b - a).count();
}

/* hipEventSynchronize for events that are about to fire: poll for two milliseconds first -- eight batch periods; the
 * runtime's wait may put the thread to sleep, and on a busy host it then comes back late, which the in-order chain
 * feels at once (the next resolve pass can only be queued when this one has reported) */
hipError_t event_wait(hipEvent_t ev)
{
    const auto until = Clock::now() + std::chrono::microseconds(2000);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady)
            return e;
        if (Clock::now() >= until)
            return hipEventSynchronize(ev);
        Helper::relax();
    }
}

static void emit_thunk(const msd_message *mm, const uint64_t *power_req, uint32_t count, uint32_t buffer, void *user)
{
    msd_ctx *c = static_cast<msd_ctx *>(user);
    c->out_msgs.insert(c->out_msgs.end(), mm, mm + count);
    c->out_req.insert(c->out_req.end(), power_req, power_req + count);
    c->out_buf.insert(c->out_buf.end(), count, buffer);
}

GpuCtl gpu_ctl(const msd_ctx *c, const Slot &s)
{
    const size_t N = c->max_buffers;
    GpuCtl g;
    g.h_ts = reinterpret_cast<uint64_t *>(s.h_ctl);
    g.h_valid = reinterpret_cast<uint32_t *>(s.h_ctl + 16 * N);
    g.h_snap = g.h_valid + N;
    g.h_todo = g.h_snap + N;
    return g;
}

void gpu_params(const msd_ctx *c, const Slot &s, MsdResolveParams &rp)
{
    const GpuCtl g = gpu_ctl(c, s);
    rp.hits = s.d_hits;
    rp.tries = s.d_tries;
    rp.totals = s.d_totals;
    rp.buf_first = s.buf_first_valid ? s.d_buf_first : nullptr;
    /* the control arrays are read where they are, in pinned host memory: a few words per workgroup,
     * and an upload of 14 KiB would run as a blit kernel that fights the scan for compute units */
    rp.valid = g.h_valid;
    rp.ts = g.h_ts;
    rp.snaps = c->d_snaps;
    rp.snap_idx = g.h_snap;
    rp.todo = g.h_todo;
    rp.rbuf = s.h_rbuf;
    rp.nmsgs = s.d_nmsgs;
    rp.acc = s.d_acc;
    rp.adds = s.d_adds;
    if (ac_on(c, s)) {
        rp.ac = s.d_ac;
        rp.ac_totals = s.d_ac_totals;
        rp.acc_ac = s.d_acc_ac;
        rp.nac = s.d_nac;
    }
    rp.pred = reinterpret_cast<const unsigned long long *>(s.d_pred);
    rp.pred_gen = s.pred_gen;
    if (c->power_fused) { /* the signal power of the accepted messages at the end of every resolve workgroup */
        MsdScanParams sp{};
        fill_params(c, s, sp);
        rp.power = reinterpret_cast<unsigned long long *>(s.d_powr);
        rp.iq = sp.iq;
        rp.prev_tail = sp.prev_tail;
        rp.have_prev = sp.have_prev;
        rp.batch_first = sp.batch_first;
        rp.nsamples = sp.nsamples;
        rp.lut = sp.lut;
        rp.format = c->scan_format;
    }
    if (s.lean) {
        rp.hits = s.d_rhits;
        rp.tries = s.d_rtries;
        rp.buf_first = nullptr;
        rp.region_counts = s.d_rcounts;
        rp.wg_totals = s.d_rwgt;
        rp.regions_per_buffer = s.lean_k;
        rp.hcap = s.lean_hcap;
        rp.nscan_wg = (s.lean_nreg + MSD_SCAN_WAVES - 1) / MSD_SCAN_WAVES;
        rp.nregions = s.lean_nreg;
        rp.sums = s.d_sums;
        rp.h_sums = s.h_sums;
        rp.h_totals = s.h_totals;
        if (c->scan_format == MSD_FMT_SC16 || c->scan_format == MSD_FMT_SC16Q11) {
            rp.fmeans = s.d_fmeans;
            rp.h_fmeans = s.h_fmeans;
        }
        rp.h_ac_totals = s.h_ac_totals;
    }
}

static uint32_t slot_valid(const Slot &s, uint32_t b)
{
    const uint64_t first = (uint64_t)b * MSD_CHUNK_SAMPLES;
    uint64_t n = s.nsamples > first ? s.nsamples - first : 0;
    return (uint32_t)(n > MSD_CHUNK_SAMPLES ? MSD_CHUNK_SAMPLES : n);
}

/* one resolve pass over the s.resolve_ntodo buffers of the to-do list, on `ks`.  Its inputs (new
 * filter snapshots, control arrays) go up on the aux stream right away -- `ks` is usually still busy
 * with a scan -- and the kernel waits for them through an event. */
static int gpu_queue_pass(msd_ctx *c, Slot &s, hipStream_t ks, bool first_pass)
{
    const uint32_t nsn = msd_gpu_resolve_nsnaps(&c->resolver);
    for (uint32_t i = c->snaps_uploaded; i < nsn; ++i) {
        uint32_t *stage = c->h_snaps + (size_t)i * MSD_SNAP_WORDS;
        uint32_t active = 0;
        const uint32_t *two = msd_gpu_resolve_snapshot(&c->resolver, i, &active); /* slot[2][8192] */
        for (uint32_t h = 0; h < 8192; ++h) { /* interleaved on the device: a probe's two first slots are one load */
            stage[2 * h] = two[h];
            stage[2 * h + 1] = two[8192 + h];
        }
        stage[16384] = active;
        HIPCHK(c, hipMemcpyAsync(c->d_snaps + (size_t)i * MSD_SNAP_WORDS, stage, sizeof(uint32_t) * MSD_SNAP_WORDS,
                                 hipMemcpyHostToDevice, c->aux_stream));
    }
    c->snaps_uploaded = nsn;
    if (ks != c->aux_stream) {
        HIPCHK(c, hipEventRecord(c->ev_inputs, c->aux_stream));
        if (ks == c->stream && c->chain_inline && !c->wait_inputs_on_stream) {
            /* In order on the scan stream: the caller waits the few microseconds the 64 KB take (the copy engine is
             * idle) instead of the stream -- a wait packet in front of the resolve kernel holds the stream for 10 us
             * behind every scan, however long ago the event fired. */
            HIPCHK(c, event_wait(c->ev_inputs));
        } else {
            HIPCHK(c, hipStreamWaitEvent(ks, c->ev_inputs, 0));
        }
    }
    MsdResolveParams rp{};
    gpu_params(c, s, rp);
    int rc = 0;
    rp.first_pass = first_pass ? 1 : 0;
    rp.ctl_implicit = 1;
    rp.sample_counter0 = s.sample_counter0;
    rp.batch_samples = s.nsamples;
    rp.h_pred = c->h_pred;
    rp.h_pred_count = c->h_pred_count;
    if (!first_pass) /* (the first pass finds the table as the batch's scan kernel left it) */
        rc = msd_launch_pred_patch(reinterpret_cast<unsigned long long *>(s.d_pred), c->h_patches, c->npatches, ks);
    if (rc)
        return fail(c, rc, "prediction patch kernel launch failed");
    rc = msd_launch_resolve(&rp, s.resolve_ntodo, ks);
    if (rc)
        return fail(c, rc, "resolve kernel launch failed");
    return 0;
}

/* message records (pinned host memory) and signal power of every buffer on `ks`; ev_records marks the end */
static int gpu_queue_emit(msd_ctx *c, Slot &s, int format, hipStream_t ps, hipStream_t ks, bool do_power = true,
                          bool do_emit = true)
{
    MsdResolveParams rp{};
    gpu_params(c, s, rp);
    MsdScanParams p{};
    fill_params(c, s, p);
    /* the signal power on `ps`, the records on `ks` behind it */
    if (c->power_fused && do_power) { /* the resolve workgroups left the sums; the emit kernel adds up its own offsets */
        do_power = false;
        s.power_done = false;
    }
    int rc = do_power ? msd_launch_power_buffers(&p, format, s.d_acc, s.d_tries, s.d_nmsgs, s.nbuffers, s.d_totals,
                                                 reinterpret_cast<unsigned long long *>(s.d_powr),
                                                 c->cfg.mode_ac ? s.d_nac : nullptr, s.d_rec_off, ps)
                      : 0;
    if (rc)
        return fail(c, rc, "power kernel launch failed");
    if (do_power)
        s.power_done = true;
    if (!do_emit)
        return 0;
    if (ps != ks) {
        HIPCHK(c, hipEventRecord(s.ev_power, ps));
        HIPCHK(c, hipStreamWaitEvent(ks, s.ev_power, 0));
    }
    rc = msd_launch_emit(&rp, s.nbuffers, reinterpret_cast<const unsigned long long *>(s.d_powr), s.h_side,
                         s.h_wire, c->want_fields ? s.h_fields : nullptr,
                         (uint32_t)s.req_cap, ks);
    if (rc)
        return fail(c, rc, "emit kernel launch failed");
    HIPCHK(c, hipEventRecord(s.ev_records, ks));
    return 0;
}

/* The records are in pinned memory when ev_records fires: the kernels wrote them there themselves (PCIe-bound, ~45 us per
 * 35 000 messages, in order behind the batch's other kernels; a copy out of HBM measured slower on this stack). */
static int fetch_records(msd_ctx *c, Slot &s)
{
    HIPCHK(c, event_wait(s.ev_records));
    return 0;
}

/* The records of the batch whose chain was queued last and whose records are still owed, by the stand-alone
 * kernel on the scan stream (no scan came along to carry them). */
int flush_pending_emit(msd_ctx *c)
{
    Slot *p = c->pending_emit;
    if (!p)
        return 0;
    c->pending_emit = nullptr;
    return gpu_queue_emit(c, *p, c->scan_format, c->stream, c->stream, !p->power_done, true);
}

/* the samples a live receiver dropped in front of this batch go onto the sample clock when the batch's
 * turn comes (every earlier batch has been committed by then), sdr_rtlsdr.c:284,299 */
static void apply_dropped(msd_ctx *c, Slot &s)
{
    c->resolver.sample_counter += s.dropped_before;
    c->stats.samples_dropped += s.dropped_before; /* readsb.c:836 */
    s.dropped_before = 0;
}

/* Clocks, snapshot 0 = the live filter, first pass over every buffer and the (speculative) message
 * records, all behind the batch's own kernels on the scan stream.  Every earlier batch must have
 * been committed: this is the earliest moment its successor can start. */
int gpu_begin(msd_ctx *c, Slot &s, int format)
{
    apply_dropped(c, s);
    s.power_done = false;
    const GpuCtl g = gpu_ctl(c, s);
    for (uint32_t b = 0; b < s.nbuffers; ++b)
        g.h_valid[b] = slot_valid(s, b);
    s.sample_counter0 = c->resolver.sample_counter;
    msd_gpu_resolve_begin(&c->resolver, s.nbuffers, g.h_valid, g.h_ts, g.h_snap, g.h_todo, &s.resolve_ntodo);
    c->snaps_uploaded = 0;
    /* The scan stream carries scans (and their gathers) only, back to back.  Prediction + resolve run on
     * the high-priority chain stream behind the batch's own scan (ev_totals), power + records on a third
     * one behind the resolve: they share the GPU with the next batch's scan instead of delaying it. */
    hipStream_t ks = c->chain_inline ? c->stream : c->aux_stream;
    hipStream_t es = c->chain_inline ? c->stream : c->emit_stream;
    hipStream_t pws = es; /* the signal power kernel */
    int rc = ensure_req(c, s, (size_t)s.nbuffers * 96 + 4096);
    if (rc)
        return rc;
    if (ks != c->stream) {
        HIPCHK(c, hipStreamWaitEvent(ks, s.ev_totals, 0));
        /* Side streams: a scan workgroup fills its compute unit (all registers, all LDS), so a chain kernel that
         * meets a scan waits for it; the latency-bound kernels behind the scan (float sums, Mode A/C) leave
         * room.  If the next batch is queued already, the chain starts when that batch's scan has retired. */
        Slot &nx = c->slots[((&s - c->slots) + 1) % MSD_PIPELINE_DEPTH];
        if (&nx != &s && nx.busy && nx.launch_seq == s.launch_seq + 1 && nx.ev_scanned && nx.nsamples >= MSD_CHUNK_SAMPLES)
            HIPCHK(c, hipStreamWaitEvent(ks, nx.ev_scanned, 0));
    }
    rc = gpu_queue_pass(c, s, ks, true);
    if (!rc) {
        HIPCHK(c, hipEventRecord(s.ev_resolve, ks));
        if (c->emit_fused) {
            rc = flush_pending_emit(c); /* an older one no scan came after */
            if (!rc && !c->power_fused)
                rc = gpu_queue_emit(c, s, format, ks, ks, true, false); /* signal power now, records with the next scan */
            if (!rc)
                c->pending_emit = &s; /* (power_fused: the next scan's wavefronts sum the signal power as well) */
        } else {
            if (pws != ks)
                HIPCHK(c, hipStreamWaitEvent(pws, s.ev_resolve, 0));
            rc = gpu_queue_emit(c, s, format, pws, es);
        }
    }
    if (rc)
        return rc;
    s.resolve_inflight = true;
    return 0;
}

/* per-buffer sample counts and means (mag_buf.validLength - overlap, .mean_level, .mean_power) into c->valid / c->means;
 * have_sums false: zeros (a lean batch's sums arrive with its first resolve pass) */
static void batch_means(msd_ctx *c, const Slot &s, int format, const double *means_override, bool have_sums = true)
{
    c->valid.assign(s.nbuffers, 0);
    c->means.assign(2 * (size_t)s.nbuffers, 0.0);
    for (uint32_t b = 0; b < s.nbuffers && have_sums; ++b) {
        const uint32_t n = slot_valid(s, b);
        c->valid[b] = n;
        if (means_override) {
            c->means[2 * b] = means_override[2 * b];
            c->means[2 * b + 1] = means_override[2 * b + 1];
        } else if (format == MSD_FMT_SC16 || format == MSD_FMT_SC16Q11 || s.dc) {
            /* convert.c:245-251: float sum / unsigned -> float division, widened to double */
            c->means[2 * b] = (double)(s.h_fmeans[2 * b] / (float)n);
            c->means[2 * b + 1] = (double)(s.h_fmeans[2 * b + 1] / (float)n);
        } else {
            /* convert.c:104-110 (note 65536 for the level, 65535^2 for the power) */
            c->means[2 * b] = (double)s.h_sums[2 * b] / 65536.0 / (double)n;
            c->means[2 * b + 1] = (double)s.h_sums[2 * b + 1] / 65535.0 / 65535.0 / (double)n;
        }
    }
}

/* The resolve passes of a batch whose first pass is queued: wait, replay the filter changes on the host, run the
 * buffers that saw the wrong filter again, until the replay agrees with what every buffer assumed.  0: done (nothing
 * is committed yet); 1: the host resolver has to take the batch; 2: its candidate arenas overflowed (lean layout:
 * only the first pass tells); < 0: error. */
static int resolve_passes(msd_ctx *c, Slot &s, double &t_wait, double &t_replay)
{
    const uint32_t n = s.nbuffers;
    const GpuCtl g = gpu_ctl(c, s);
    hipEvent_t wait_for = s.ev_resolve;
    s.records_current = true; /* the message records in host memory belong to the latest pass */
    s.npass = 0;
    for (uint32_t pass = 0;; ++pass) {
        const auto k0 = Clock::now();
        ++s.npass;
        HIPCHK(c, event_wait(wait_for));
        const auto k1 = Clock::now();
        if (s.lean && pass == 0 && (s.h_totals[2] || (c->cfg.mode_ac && s.h_ac_totals[2]))) /* what the gather
                                                                                                   kernels' totals used to say */
            return 2;
        int rc = msd_gpu_resolve_replay(&c->resolver, n, s.h_rbuf, nullptr, c->inline_adds, pass, SNAP_CAP, c->h_pred,
                                        *c->h_pred_count, c->h_patches, &c->npatches, g.h_snap, g.h_todo,
                                        &s.resolve_ntodo);
        if (rc == -2) { /* a flip, or very many new addresses in one buffer: the complete add lists are needed.
                           They are in pinned host memory already (the resolve kernel writes a buffer's ~60 addresses
                           there itself; fetching the [buffer][1024] array cost a 2 MB copy per flip) */
            c->timing.resolve_long_lists++;
            rc = msd_gpu_resolve_replay(&c->resolver, n, s.h_rbuf, s.d_adds, c->inline_adds, pass, SNAP_CAP, c->h_pred,
                                        *c->h_pred_count, c->h_patches, &c->npatches, g.h_snap, g.h_todo,
                                        &s.resolve_ntodo);
        }
        t_wait += ms_between(k0, k1);
        t_replay += ms_between(k1, Clock::now());
        if (rc == 0)
            return 0;
        if (rc < 0)
            return 1;
        /* some buffers saw the wrong filter: once more for those, ahead of the queued scans */
        hipStream_t ps = c->chain_inline ? c->stream : c->aux_stream;
        rc = gpu_queue_pass(c, s, ps, false);
        if (rc)
            return rc;
        HIPCHK(c, hipEventRecord(c->ev_aux, ps));
        wait_for = c->ev_aux;
        s.records_current = false;
    }
}

/* The successor of a batch whose filter changes have just been committed: its first resolve pass can be queued. */
static int begin_successor(msd_ctx *c, Slot &s)
{
    Slot &nx = c->slots[((&s - c->slots) + 1) % MSD_PIPELINE_DEPTH];
    /* Across a capture boundary too: the filter and the clocks start over now (this batch was the old capture's
     * last one), the counters when the new capture's first batch is collected -- the caller may still want
     * the old ones.  (Not if samples were dropped in front of the new capture: they count on its counters.) */
    if (&nx != &s && nx.busy && nx.launch_seq == s.launch_seq + 1 && nx.gpu_resolve && !nx.resolve_inflight && !nx.ahead_done &&
        (!nx.reset_before || nx.dropped_before == 0)) {
        if (nx.reset_before) {
            msd_resolver_reset_state(&c->resolver);
            nx.state_reset_done = true;
        }
        return gpu_begin(c, nx, c->scan_format);
    }
    return 0;
}

/* What the per-message half of finishing a batch needs of finish_gpu's frame, and what it reports back. */
struct Delivery {
    msd_ctx *c;
    Slot *s;
    uint32_t n, total; /* buffers, records */
    msd_message_fn sink;
    void *user;
    int fetch_rc = 0;
    double t_power = 0;
};

/* The per-message half -- wait for the records, signal level and the order-sensitive power statistics
 * (demod_2400.c:386-408,422-427), the copy into the caller's arrays -- runs on the helper thread; it touches this
 * batch's records and the power fields of the statistics only. */
static void deliver_records(Delivery &d)
{
    msd_ctx *const c = d.c;
    Slot &s = *d.s;
    const uint32_t total = d.total;
    static_assert(sizeof(msd_wire) == sizeof(msd_message), "the records are msd_message arrays");
    d.fetch_rc = fetch_records(c, s);
    if (d.fetch_rc)
        return;
    const auto p0 = Clock::now();
    /* what the statistics half below needs, in the context's own storage: the caller's next batch reuses
     * c->valid / c->means / c->out_buf and this batch's slot while it runs */
    c->bg_valid = c->valid;
    c->bg_means = c->means;
    c->bg_buf.swap(c->out_buf);
    c->bg_scaled.resize(total ? total : 1);
    memcpy(c->bg_scaled.data(), s.h_side, (size_t)total * sizeof(uint64_t));
    d.t_power = ms_between(p0, Clock::now());
    /* the library's own array sinks take the whole batch with one copy instead of 35 000 calls */
    if (c->fsink == msd_array_fields_sink) {
        msd_array_fields_sink_state *st = static_cast<msd_array_fields_sink_state *>(c->fuser);
        const size_t room = st->count < st->cap ? st->cap - st->count : 0, k = total < room ? total : room;
        memcpy(st->out + st->count, s.h_wire, k * sizeof(msd_message));
        memcpy(st->fields + st->count, s.h_fields, k * sizeof(msd_fields));
        st->count += total;
    } else if (!c->fsink && d.sink == msd_array_sink) {
        msd_array_sink_state *st = static_cast<msd_array_sink_state *>(d.user);
        const size_t room = st->count < st->cap ? st->cap - st->count : 0, k = total < room ? total : room;
        memcpy(st->out + st->count, s.h_wire, k * sizeof(msd_message));
        st->count += total;
    }
    /* ---- the caller has its messages; from here on nothing of finish_gpu's frame (d) or of the slot is touched ---- */
    const uint32_t nb = d.n;
    const uint64_t nm = total;
    c->helper.mark_delivered();
    msd_resolve_power_stats(&c->resolver, nb, c->bg_valid.data(), c->bg_means.data(), c->bg_buf.data(),
                            c->bg_scaled.data(), nm);
}

/* While this batch's records are on their way: the resolve half of the NEXT batch -- wait for its first pass
 * (queued when this batch's filter changes were committed, possibly by the msd_collect before this one), replay,
 * commit its filter changes and queue the first pass of the batch behind it.  The chain of resolve passes then
 * runs one batch ahead of the delivery: the caller, who can only launch the next scan once this call returns,
 * never finds the GPU waiting for a resolve pass it has not been able to queue yet.  The counters of the next
 * batch are added when it is collected, as before.  Returns begin_rc, or what went wrong here. */
static int resolve_ahead(msd_ctx *c, Slot &s, int begin_rc)
{
    if (!(c->outstanding > 1 && !begin_rc && c->resolve_ahead))
        return begin_rc;
    Slot &nx = c->slots[((&s - c->slots) + 1) % MSD_PIPELINE_DEPTH];
    if (!(&nx != &s && nx.busy && nx.launch_seq == s.launch_seq + 1 && nx.gpu_resolve && nx.resolve_inflight && !nx.ahead_done &&
          (!nx.reset_before || nx.state_reset_done))) /* (a new capture's first batch: only once filter and clocks have started over) */
        return begin_rc;
    const bool trace = c->trace;
    double tw = 0, tr = 0;
    const int arc = resolve_passes(c, nx, tw, tr);
    if (trace)
        fprintf(stderr, "ahead: next batch's passes: waits %.3f ms, replay %.3f ms, verdict %d\n", tw, tr, arc);
    if (arc < 0) {
        begin_rc = arc;
    } else if (arc == 0) {
        const GpuCtl gn = gpu_ctl(c, nx);
        const auto a0 = Clock::now();
        msd_gpu_resolve_commit_state(&c->resolver, nx.nbuffers, gn.h_valid, nx.h_rbuf);
        nx.ahead_done = true;
        nx.resolve_inflight = false;
        const auto a1 = Clock::now();
        if (c->outstanding > 2)
            begin_rc = begin_successor(c, nx);
        if (trace)
            fprintf(stderr, "ahead: commit %.3f ms, the batch behind it begun in %.3f ms\n", ms_between(a0, a1), ms_between(a1, Clock::now()));
    } else { /* the host resolver's case or an overflow: nothing is committed, that batch's msd_collect acts on it */
        nx.ahead_verdict = arc;
    }
    return begin_rc;
}

/* Returns 1 when the batch has to go through the host resolver instead (nothing committed); 2 when its candidate
 * arenas overflowed (lean layout: only the first resolve pass tells). */
static int finish_gpu(msd_ctx *c, Slot &s, int format, msd_message_fn sink, void *user)
{
    const uint32_t n = s.nbuffers;
    const GpuCtl g = gpu_ctl(c, s);
    double t_wait = 0, t_replay = 0;
    const bool early = s.resolve_inflight || s.ahead_done;
    int begin_rc = 0;
    if (s.ahead_verdict) { /* the msd_collect before this one has been through the passes already */
        const int v = s.ahead_verdict;
        s.ahead_verdict = 0;
        s.resolve_inflight = false;
        if (c->pending_emit == &s)
            c->pending_emit = nullptr; /* its speculative records are void */
        return v;
    }
    if (!s.ahead_done) { /* (an earlier msd_collect may have done this half already: resolve_ahead) */
        if (!s.resolve_inflight) {
            int rc = gpu_begin(c, s, format);
            if (rc)
                return rc;
        }
        s.resolve_inflight = false;
        if (c->pending_emit == &s) { /* no scan was launched since */
            int rc = flush_pending_emit(c);
            if (rc)
                return rc;
        }
        int rc = resolve_passes(c, s, t_wait, t_replay);
        if (rc)
            return rc;
        msd_gpu_resolve_commit_state(&c->resolver, n, g.h_valid, s.h_rbuf);
        /* the filter is final for this batch: its successor can start */
        if (c->outstanding > 1)
            begin_rc = begin_successor(c, s);
    }
    s.ahead_done = false;
    s.resolve_inflight = false;
    if (c->pending_emit == &s) { /* no scan was launched since its chain was queued: nobody carries its records */
        int rc = flush_pending_emit(c);
        if (rc)
            return rc;
    }
    const uint32_t npass = s.npass;
    bool records_current = s.records_current;
    hipEvent_t wait_for = c->ev_aux; /* (only looked at after a further pass, which recorded it) */
    c->timing.resolve_passes = npass;
    const auto e0 = Clock::now();
    if (s.lean)
        batch_means(c, s, c->scan_format, nullptr);
    msd_gpu_resolve_commit_stats(&c->resolver, n, g.h_valid, s.h_rbuf);

    uint32_t total = 0;
    c->out_buf.clear();
    for (uint32_t b = 0; b < n; ++b) {
        const uint32_t k = s.h_rbuf[b].nmsgs + (c->cfg.mode_ac ? s.h_rbuf[b].nac : 0u);
        total += k;
        c->out_buf.insert(c->out_buf.end(), k, b);
    }
    if (total > s.req_cap) { /* more messages than the arrays of the speculative records hold */
        HIPCHK(c, hipEventSynchronize(s.ev_records));
        int rc = ensure_req(c, s, total);
        if (rc)
            return rc;
        records_current = false;
    }
    hipStream_t rs = c->chain_inline ? c->stream : c->emit_stream;
    if (!records_current && total) {
        if (!c->chain_inline) /* behind the last pass (or, if only the arrays grew, behind nothing new) */
            HIPCHK(c, hipStreamWaitEvent(rs, wait_for, 0));
        int rc = gpu_queue_emit(c, s, format, rs, rs);
        if (rc)
            return rc;
    }
    /* the per-message half on the helper thread, the next batch's resolve passes on this one meanwhile */
    Delivery d{c, &s, n, total, sink, user};
    const bool threaded = !c->no_helper;
    if (threaded)
        c->helper.run([&d] { deliver_records(d); });
    begin_rc = resolve_ahead(c, s, begin_rc);
    const auto e1 = Clock::now();
    if (threaded)
        c->helper.wait_delivered();
    else
        deliver_records(d);
    if (begin_rc)
        return begin_rc;
    if (d.fetch_rc)
        return d.fetch_rc;
    if (c->trace) {
        double cyc[8] = {0};
        for (uint32_t b = 0; b < n; ++b)
            for (int k = 0; k < 8; ++k)
                cyc[k] += s.h_rbuf[b].cyc[k];
        if (cyc[0] > 0) /* built with -DMSD_RESOLVE_TIMING=1 */
            fprintf(stderr, "resolve kernel, mean us per buffer: setup %.1f segment %.1f stage %.1f eval %.1f walk %.1f count %.1f no-try hits %.1f power %.1f\n",
                    cyc[0] / n / 100, cyc[5] / n / 100, cyc[1] / n / 100, cyc[2] / n / 100, cyc[3] / n / 100, cyc[4] / n / 100, cyc[7] / n / 100,
                    cyc[6] / n / 100);
        fprintf(stderr, "gpu resolve: %u passes%s, waits %.3f ms, replay %.3f ms, commit + next batch's first pass %.3f ms, "
                "power stats %.3f ms (helper), then waited %.3f ms for it\n", npass, early ? " (first one queued early)" : "",
                t_wait, t_replay, ms_between(e0, e1), d.t_power, ms_between(e1, Clock::now()));
    }
    /* callback sinks run on the calling thread, in order */
    if (c->fsink && c->fsink != msd_array_fields_sink) {
        for (uint32_t i = 0; i < total; ++i)
            c->fsink(&s.h_wire[i].mm, &s.h_fields[i], c->fuser);
    } else if (!c->fsink && sink && sink != msd_array_sink) {
        for (uint32_t i = 0; i < total; ++i)
            sink(&s.h_wire[i].mm, user);
    }
    return 0;
}

/* msd_restart(): the batch is the first of a new capture, and every batch of the previous one has been delivered. */
static void begin_capture(msd_ctx *c, Slot &s)
{
    c->helper.wait(); /* ... and its statistics are complete */
    if (s.state_reset_done)
        msd_resolver_reset_stats(&c->resolver);
    else
        msd_resolver_reset(&c->resolver);
    s.state_reset_done = false;
    /* the counters start over with the capture; the kernel-time sampling (one batch in timing_interval) runs on */
    const uint64_t timed = c->timing.timed_batches;
    const float scan_ms = c->timing.scan_kernel_ms, other_ms = c->timing.other_kernels_ms;
    memset(&c->timing, 0, sizeof c->timing);
    c->timing.timed_batches = timed;
    c->timing.scan_kernel_ms = scan_ms;
    c->timing.other_kernels_ms = other_ms;
    s.reset_before = false;
}

/* Start the download of the lists of the batch behind `s`, if there is one.  only_if_scanned: only when that does not
 * block (its kernels are done, and it is not lean); otherwise: unless it has been started already. */
static int download_next(msd_ctx *c, Slot &s, bool only_if_scanned)
{
    Slot &nx = c->slots[(c->head + 1) % MSD_PIPELINE_DEPTH];
    if (c->outstanding <= 1 || &nx == &s || !nx.busy ||
        (only_if_scanned ? nx.lean || hipEventQuery(nx.ev_totals) != hipSuccess : nx.download_started))
        return 0;
    return start_download(c, nx, c->scan_format);
}

/* the batch's counters and kernel times for msd_get_timing; the slot is free afterwards */
static void note_timing(msd_ctx *c, Slot &s, uint64_t H, uint64_t Tn, Clock::time_point t0, Clock::time_point t1)
{
    float ms = 0;
    c->timing.hits = H;
    c->timing.tries = Tn;
    if (s.timed && hipEventElapsedTime(&ms, s.ev_start, s.ev_scan) == hipSuccess)
        c->timing.scan_kernel_ms = ms, c->timing.timed_batches++;
    if (s.timed && hipEventElapsedTime(&ms, s.ev_scan, s.ev_kernels) == hipSuccess)
        c->timing.other_kernels_ms = ms;
    if (hipEventElapsedTime(&ms, s.ev_copy0, s.ev_copy1) == hipSuccess)
        c->timing.d2h_ms = ms;
    c->timing.resolve_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    s.busy = false;
}

/* The host resolver takes a batch that was meant for the GPU resolve: it needs the lists after all.  overflowed: its
 * arenas overflowed (lean layout) -- scanned again in pieces, stitched on the host. */
static int fetch_lists_for_host(msd_ctx *c, Slot &s, int format, bool overflowed)
{
    int rc = 0;
    if (overflowed) {
        if (c->pending_emit == &s)
            c->pending_emit = nullptr; /* its speculative records are void */
        HIPCHK(c, hipStreamSynchronize(c->stream));
        s.lean = false;
        rc = rerun_in_pieces(c, s, format);
        if (rc)
            return rc;
        batch_means(c, s, c->scan_format, nullptr); /* the pieces' gather / publish kernels published the sums again */
        s.gpu_resolve = false;
    } else if (s.lean) {
        batch_means(c, s, c->scan_format, nullptr); /* (published by the first resolve pass, which did run) */
        rc = lean_gather_now(c, s);
        if (rc)
            return rc;
    }
    const uint64_t H = s.h_totals[0], Tn = s.h_totals[1];
    rc = overflowed ? 0 : ensure_host(c, s, H, Tn);
    if (rc)
        return rc;
    if (H && !overflowed)
        HIPCHK(c, hipMemcpyAsync(s.h_hits, s.d_hits, H * sizeof(msd_hit), hipMemcpyDeviceToHost, c->aux_stream));
    if (Tn && !overflowed)
        HIPCHK(c, hipMemcpyAsync(s.h_tries, s.d_tries, Tn * sizeof(msd_try), hipMemcpyDeviceToHost, c->aux_stream));
    if (c->cfg.mode_ac && !overflowed) { /* (rerun_in_pieces has stitched the pieces' Mode A/C lists on the host already; the
                                            device holds the last piece's only -- round 5's fuzzer, drawing arena sizes,
                                            found a reply six buffers early: this copy used to run in both cases) */
        const uint64_t nac = s.h_ac_totals[0];
        rc = ensure_ac_host(c, s, nac);
        if (rc)
            return rc;
        if (nac)
            HIPCHK(c, hipMemcpyAsync(s.h_ac, s.d_ac, nac * sizeof(msd_ac_hit), hipMemcpyDeviceToHost, c->aux_stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->aux_stream));
    c->timing.resolve_fallback++;
    return 0;
}

/* signal power of the nm accepted messages (requests in s.h_req) into s.h_pow: a small kernel's round trip on the aux
 * stream -- the copy stream may already be busy downloading the next batch's lists */
static int power_from_device(msd_ctx *c, Slot &s, int format, size_t nm)
{
    HIPCHK(c, hipMemcpyAsync(s.d_req, s.h_req, nm * sizeof(uint64_t), hipMemcpyHostToDevice, c->aux_stream));
    MsdScanParams p{};
    fill_params(c, s, p);
    const int rc = msd_launch_power(&p, format, s.d_req, (uint32_t)nm, reinterpret_cast<unsigned long long *>(s.d_pow),
                                    c->aux_stream);
    if (rc)
        return fail(c, rc, "power kernel launch failed");
    HIPCHK(c, hipMemcpyAsync(s.h_pow, s.d_pow, nm * sizeof(uint64_t), hipMemcpyDeviceToHost, c->aux_stream));
    HIPCHK(c, hipStreamSynchronize(c->aux_stream));
    return 0;
}

/* Wait for a batch's lists, resolve in order, deliver messages. */
int finish(msd_ctx *c, Slot &s, int format, msd_message_fn sink, void *user,
           const uint64_t *ts_override, const double *means_override, uint64_t resolver_first_chunk)
{
    const auto ta = Clock::now();
    if (s.reset_before)
        begin_capture(c, s);
    int rc = start_download(c, s, format);
    if (rc)
        return rc;
    uint64_t H = s.lean ? 0 : s.h_totals[0], Tn = s.lean ? 0 : s.h_totals[1];
    HIPCHK(c, hipEventSynchronize(s.ev_copy1));
    const auto tb = Clock::now();
    s.download_started = false;
    /* the following batch's lists can come down while this one is resolved on the host */
    rc = download_next(c, s, true); /* (only if its kernels are done: does not block) */
    if (rc)
        return rc;
    batch_means(c, s, format, means_override, !s.lean);

    const auto t0 = Clock::now();
    const bool skip_resolve = (c->debug_flags & 0x1c) != 0; /* perf experiments with incomplete candidates */
    if (s.gpu_resolve) {
        rc = (ts_override || skip_resolve) ? 1 : finish_gpu(c, s, format, sink, user);
        s.resolve_inflight = false;
        if (rc == 2 && s.lean) { /* the region slices overflowed: bigger ones, one more scan, and the GPU resolve again */
            const int g = grow_and_rescan(c, s, format);
            if (g < 0)
                return g;
            if (g == 0) {
                s.ahead_done = false;
                s.ahead_verdict = 0;
                rc = finish_gpu(c, s, format, sink, user);
                s.resolve_inflight = false;
            }
        }
        if (rc < 0)
            return rc;
        if (s.lean) {
            H = s.h_totals[0];
            Tn = s.h_totals[1];
        }
        if (rc == 0) {
            const auto t1 = Clock::now();
            rc = download_next(c, s, false);
            if (rc)
                return rc;
            if (c->trace)
                fprintf(stderr, "finish: wait-download %.3f  means %.3f  gpu resolve+power+sink %.3f ms\n", ms_between(ta, tb),
                        ms_between(tb, t0), ms_between(t0, t1));
            note_timing(c, s, H, Tn, t0, t1);
            return 0;
        }
        rc = fetch_lists_for_host(c, s, format, rc == 2);
        if (rc)
            return rc;
        H = s.h_totals[0];
        Tn = s.h_totals[1];
    }
    c->helper.wait(); /* the statistics of the previous batch, if they are still being summed */
    c->timing.resolve_passes = 0;
    c->out_msgs.clear();
    c->out_req.clear();
    c->out_buf.clear();
    apply_dropped(c, s);
    if (!skip_resolve)
        msd_resolve_batch(&c->resolver, resolver_first_chunk, s.nbuffers, c->valid.data(), s.h_hits, H, s.h_tries, Tn,
                      c->cfg.mode_ac ? s.h_ac : nullptr, c->cfg.mode_ac ? s.h_ac_totals[0] : 0, ts_override,
                      emit_thunk, c);
    const auto t1 = Clock::now();
    rc = download_next(c, s, false); /* if the next batch was still running before the resolve, fetch it now */
    if (rc)
        return rc;

    /* signal power of the accepted messages: summed here out of the caller's mag_bufs, or by a small follow-up kernel */
    const size_t nm = c->out_msgs.size();
    if (nm) {
        rc = ensure_req(c, s, nm);
        if (rc)
            return rc;
        memcpy(s.h_req, c->out_req.data(), nm * sizeof(uint64_t));
        if (c->magbuf_views)
            msd_magbuf_power(c->magbuf_views, c->magbuf_nviews, c->out_req.data(), nm, s.h_pow);
        else
            rc = power_from_device(c, s, format, nm);
        if (rc)
            return rc;
    }
    msd_resolve_power(&c->resolver, s.nbuffers, c->valid.data(), c->means.data(), c->out_msgs.data(), sizeof(msd_message),
                      c->out_req.data(), c->out_buf.data(), s.h_pow, sizeof(uint64_t), nm);
    const auto t2 = Clock::now();
    if (c->fsink) { /* header fields on the host for the batches resolved here */
        c->out_fields.resize(nm ? nm : 1);
        msd_fields_batch(c->out_msgs.data(), sizeof(msd_message), c->out_buf.data(), nm, c->out_fields.data());
        for (size_t i = 0; i < nm; ++i)
            c->fsink(&c->out_msgs[i], &c->out_fields[i], c->fuser);
    } else if (sink)
        for (size_t i = 0; i < nm; ++i)
            sink(&c->out_msgs[i], user);
    if (c->trace)
        fprintf(stderr, "finish: wait-download %.3f  next-download+means %.3f  resolve %.3f  power %.3f  sink %.3f ms\n",
                ms_between(ta, tb), ms_between(tb, t0), ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, Clock::now()));
    note_timing(c, s, H, Tn, t0, t1);
    return 0;
}

int collect(msd_ctx *c, msd_message_fn sink, void *user)
{
    if (!c)
        return -EINVAL;
    if (c->failed)
        return -EIO; /* msd_last_error() still says why; msd_reset() starts over */
    if (c->outstanding == 0)
        return fail(c, -ENODATA, "no batch outstanding");
    Slot &s = c->slots[c->head];
    int rc = finish(c, s, c->scan_format, sink, user, nullptr, nullptr, s.batch_first / MSD_CHUNK_SAMPLES);
    if (rc < 0) { /* the batch is lost and the filter / clocks are in an unknown state: the context refuses further
                     batches until msd_reset() */
        c->failed = true;
        s.busy = false;
    }
    c->head = (c->head + 1) % MSD_PIPELINE_DEPTH;
    c->outstanding--;
    return rc;
}

} /* namespace msd_impl */
#pragma GCC visibility pop

/* ---- the exported entry points that collect a batch ---- */
using namespace msd_impl;

extern "C" {

int msd_collect(msd_ctx *c, msd_message_fn sink, void *user)
{
    if (!c)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return collect(c, sink, user);
}

int msd_collect_fields(msd_ctx *c, msd_fields_fn sink, void *user)
{
    if (!c)
        return -EINVAL;
    if (!c->want_fields)
        return fail(c, -EINVAL, "the context was created without MSD_CFG_DECODE_FIELDS");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->fsink = sink;
    c->fuser = user;
    const int rc = collect(c, nullptr, nullptr);
    c->fsink = nullptr;
    c->fuser = nullptr;
    return rc;
}

} /* extern "C" */
