/*
 * msd_batch.cpp -- the launch side of the stream driver: everything that puts a batch on the GPU.
 * The slot's buffers (ensure_*), enqueue() -- one batch's kernels on the compute stream: memset sums -> scan kernel ->
 * offsets+gather [-> float means] [-> Mode A/C] -> publish --, start_download() of the candidate lists on the copy stream,
 * the rescans of an overflowed batch (rerun_in_pieces, grow_and_rescan, lean_gather_now), and launch().
 * What takes a batch off the GPU again is msd_collect.cpp; msd_ctx.h is what the two share.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
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

int ensure_req(msd_ctx *c, Slot &s, size_t n)
{
    if (n <= s.req_cap)
        return 0;
    size_t cap = s.req_cap ? s.req_cap : (size_t)1 << 14;
    while (cap < n)
        cap *= 2;
    (void)hipFree(s.d_req); (void)hipFree(s.d_pow);
    if (s.h_req) (void)hipHostFree(s.h_req);
    if (s.h_pow) (void)hipHostFree(s.h_pow);
    if (s.h_wire) (void)hipHostFree(s.h_wire);
    if (s.h_side) (void)hipHostFree(s.h_side);
    if (s.h_fields) (void)hipHostFree(s.h_fields);
    s.d_req = s.d_pow = s.h_req = s.h_pow = nullptr;
    s.h_wire = nullptr;
    s.h_side = nullptr;
    s.h_fields = nullptr;
    s.req_cap = 0;
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&s.d_req), cap * sizeof(uint64_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&s.d_pow), cap * sizeof(uint64_t)));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_req), cap * sizeof(uint64_t)));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_pow), cap * sizeof(uint64_t)));
    if (c->gpu_resolve) {
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_wire), cap * sizeof(msd_wire)));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_side), cap * sizeof(unsigned long long)));
        if (c->want_fields)
            HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_fields), cap * sizeof(msd_fields)));
    }
    s.req_cap = cap;
    return 0;
}

void fill_params(const msd_ctx *c, const Slot &s, MsdScanParams &p)
{
    p.iq = s.d_iq;
    p.prev_tail = s.d_prev;
    p.ragged = s.d_ragged;
    p.have_prev = s.have_prev;
    p.threshold = s.threshold;
    p.batch_first = s.batch_first;
    p.nsamples = s.nsamples;
    p.lut = c->d_lut;
    p.crc_tab = c->d_crc;
    p.syn56 = c->d_syn56;
    p.slicer = c->d_slicer;
    p.syn112 = c->d_syn112;
    p.nsyn56 = c->tables->nsyn56;
    p.nsyn112 = c->tables->nsyn112;
    p.synhash = c->d_synhash;
    p.synh_mul56 = c->tables->synhash_mul[0];
    p.synh_mul112 = c->tables->synhash_mul[1];
    p.fix2_56 = c->d_fix2[0];
    p.fix2_112 = c->d_fix2[1];
    p.fix2_lg56 = c->fix2_lg[0];
    p.fix2_lg112 = c->fix2_lg[1];
    if (const GroupCall *g = s.group) { /* a receiver group: batch_first is a whole number of buffers into the call */
        const uint64_t b0 = s.batch_first / MSD_CHUNK_SAMPLES;
        p.group_tails = g->tails;
        p.group_lb = g->lb + b0;
        p.group_opt = g->opt + b0;
        p.prev_tail = nullptr;
        p.have_prev = 0;
        if (!g->fix2) { /* the two-bit tables may exist, but no buffer of this call is at level 2 */
            p.fix2_56 = nullptr;
            p.fix2_112 = nullptr;
        }
    }
}

int ensure_host(msd_ctx *c, Slot &s, size_t nh, size_t nt)
{
    if (nh > s.h_hits_cap) {
        size_t cap = s.h_hits_cap ? s.h_hits_cap : (size_t)1 << 16;
        while (cap < nh)
            cap *= 2;
        if (s.h_hits)
            (void)hipHostFree(s.h_hits);
        s.h_hits = nullptr;
        s.h_hits_cap = 0;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_hits), cap * sizeof(msd_hit)));
        s.h_hits_cap = cap;
    }
    if (nt > s.h_tries_cap) {
        size_t cap = s.h_tries_cap ? s.h_tries_cap : (size_t)1 << 15;
        while (cap < nt)
            cap *= 2;
        if (s.h_tries)
            (void)hipHostFree(s.h_tries);
        s.h_tries = nullptr;
        s.h_tries_cap = 0;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_tries), cap * sizeof(msd_try)));
        s.h_tries_cap = cap;
    }
    return 0;
}

/* The arenas of the layouts without region slices (a batch that is not lean: msd_submit_*-sized batches of fewer than four
 * buffers, the mag_buf entry, MSD_CFG_NO_LEAN / MSD_CFG_HOST_RESOLVE contexts, the pieces of rerun_in_pieces), made at
 * first use. */
int ensure_dense(msd_ctx *c, Slot &s)
{
    if (!c->d_region_hits)
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_region_hits), c->hit_arena * sizeof(msd_hit)));
    if (!c->d_region_tries)
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_region_tries), c->try_arena * sizeof(msd_try)));
    if (!s.d_hits || s.dense_hits < c->hit_arena) {
        if (s.d_hits) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            (void)hipFree(s.d_hits);
            s.d_hits = nullptr;
        }
        s.dense_hits = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&s.d_hits), c->hit_arena * sizeof(msd_hit)));
        s.dense_hits = c->hit_arena;
    }
    if (!s.d_tries || s.dense_tries < c->try_arena) {
        if (s.d_tries) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            (void)hipFree(s.d_tries);
            s.d_tries = nullptr;
        }
        s.dense_tries = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&s.d_tries), c->try_arena * sizeof(msd_try)));
        s.dense_tries = c->try_arena;
    }
    return 0;
}

/* Lean layout: k regions (one per scan wavefront) per buffer, none across a buffer boundary; nwg of them in all. */
static void plan_lean_regions(const msd_ctx *c, const Slot &s, uint64_t tile, uint32_t &lean_k, uint32_t &lean_tpr, uint32_t &nwg)
{
    const uint32_t tiles_per_buffer = (uint32_t)(MSD_CHUNK_SAMPLES / tile);
    /* (the buffers that hold samples: a capture's last batch ends with one more, empty or short, buffer --
     * counting it would cost a full batch of 512 buffers an eighth of its regions, 4096 / 513 = 7) */
    const uint32_t nb_data = (uint32_t)((s.nsamples + MSD_CHUNK_SAMPLES - 1) / MSD_CHUNK_SAMPLES);
    uint32_t k = c->max_wg / (nb_data ? nb_data : 1);
    if (k > 64)
        k = 64;
    if (k > tiles_per_buffer)
        k = tiles_per_buffer;
    lean_tpr = (tiles_per_buffer + k - 1) / k;
    lean_k = (tiles_per_buffer + lean_tpr - 1) / lean_tpr; /* no empty pieces */
    nwg = (nb_data ? nb_data : 1) * lean_k;
}

/* A slot's region arena with room for `want` entries: a new allocation, the old one freed (nobody may be using it).
 * false: no memory for it, the arena stays as it is. */
template <typename T>
static bool grow_arena(T *&arena, uint64_t &have, uint64_t want)
{
    if (want <= have)
        return true;
    T *bigger = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&bigger), want * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    (void)hipFree(arena);
    arena = bigger;
    have = want;
    return true;
}

/* Another slot's batch overflowed its region slices and got bigger ones (grow_and_rescan): this slot follows before
 * it meets the same traffic -- it is idle now, its last batch has been collected; a failed allocation leaves it as it is. */
static int follow_arena_growth(msd_ctx *c, Slot &s)
{
    const uint64_t want_h = (uint64_t)(c->want_hits_per_sample * (double)s.nsamples), want_t = (uint64_t)(c->want_tries_per_sample * (double)s.nsamples);
    if (!((want_h > s.rhit_arena + s.rhit_arena / 64 || want_t > s.rtry_arena + s.rtry_arena / 64) && want_t < (1ull << 30))) /* (not for a rounding's worth) */
        return 0;
    size_t free_b = 0, total_b = 0;
    const uint64_t grow_b = (want_h > s.rhit_arena ? (want_h - s.rhit_arena) * sizeof(msd_hit) : 0) +
                            (want_t > s.rtry_arena ? (want_t - s.rtry_arena) * sizeof(msd_try) : 0);
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || grow_b + (1ull << 30) > free_b)
        return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)grow_arena(s.d_rhits, s.rhit_arena, want_h);
    (void)grow_arena(s.d_rtries, s.rtry_arena, want_t);
    return 0;
}

/* The batch whose resolve chain is queued and whose records are still owed (c->pending_emit): if this scan has a
 * wavefront for each of its buffers, they write that batch's records -- p.emit is filled, *carried is the slot;
 * otherwise the stand-alone kernel writes them now. */
static int carry_pending_emit(msd_ctx *c, Slot &s, uint32_t nwg, MsdScanParams &p, Slot **carried)
{
    *carried = nullptr;
    if (!c->pending_emit || c->pending_emit == &s)
        return 0;
    Slot &a = *c->pending_emit;
    if (!(nwg >= a.nbuffers && a.nbuffers))
        return flush_pending_emit(c);
    MsdResolveParams rp{};
    gpu_params(c, a, rp);
    p.emit.nbuffers = a.nbuffers;
    p.emit.stride = nwg / a.nbuffers;
    p.emit.cap = (uint32_t)a.req_cap;
    p.emit.totals = rp.totals;
    p.emit.nmsgs = rp.nmsgs;
    p.emit.rec_off = a.power_done ? a.d_rec_off : nullptr;
    p.emit.acc = rp.acc;
    p.emit.tries = rp.tries;
    p.emit.ts = rp.ts;
    p.emit.power = reinterpret_cast<const unsigned long long *>(a.d_powr);
    p.emit.dense = a.h_wire;
    p.emit.side = a.h_side;
    p.emit.ac = rp.ac;
    p.emit.ac_totals = rp.ac_totals;
    p.emit.acc_ac = rp.acc_ac;
    p.emit.nac = rp.nac;
    *carried = &a;
    c->pending_emit = nullptr;
    return 0;
}

/* The Mode A/C candidate pass of the batch, behind its scan (s.nbuffers != 0): a receiver group's listed buffers, or
 * every buffer of a stream batch. */
static int queue_ac_pass(msd_ctx *c, Slot &s, int format, const uint32_t *host_noise, bool fm)
{
    if (s.group && s.group->nac) {
        /* a receiver group: the listed buffers of this batch (a whole call, or a piece of a rescanned one) */
        const GroupCall &g = *s.group;
        const uint32_t b0 = (uint32_t)(s.batch_first / MSD_CHUNK_SAMPLES);
        const uint32_t *lo = std::lower_bound(g.ac_host, g.ac_host + g.nac, b0);
        const uint32_t *hi = std::lower_bound(lo, g.ac_host + g.nac, b0 + s.nbuffers);
        MsdScanParams p{};
        fill_params(c, s, p);
        p.debug_flags = c->debug_flags;
        int rc = msd_launch_group_ac(&p, format, s.d_sums, s.d_fmeans, g.ac + (lo - g.ac_host), (uint32_t)(hi - lo),
                                     b0, s.d_ac_regions, c->ac_arena, s.d_ac_counts, s.d_ac_totals, s.d_ac, c->ac_arena,
                                     c->ac_max_wg, c->stream);
        if (rc)
            return fail(c, rc, "Mode A/C kernel launch failed");
        return 0;
    }
    if (host_noise)
        HIPCHK(c, hipMemcpyAsync(c->d_noise, host_noise, sizeof(uint32_t) * s.nbuffers, hipMemcpyHostToDevice,
                                 c->stream));
    MsdScanParams p{};
    fill_params(c, s, p);
    p.debug_flags = c->debug_flags;
    int ac_format = format;
    if (s.mag_pass) { /* the scan in front left the magnitudes: nothing is converted twice */
        ac_format = MSD_FMT_MAG16;
        p.iq = reinterpret_cast<const uint8_t *>(s.d_mag);
        p.prev_tail = reinterpret_cast<const uint8_t *>(s.d_mag_prev);
        p.have_prev = s.have_prev && s.d_mag_prev;
        p.ragged = reinterpret_cast<const uint8_t *>(s.d_mag + (s.nsamples & ~7ull)); /* zeros behind the last sample */
    }
    int rc = msd_launch_ac(&p, ac_format, s.d_sums, s.d_fmeans, s.nbuffers, c->d_noise,
                           host_noise != nullptr ? 1 : ((s.dc || (s.mag_pass && fm)) ? 2 : 0), /* (16-bit IQ: the float sums, whatever the pass reads) */
                           s.d_ac_regions, c->ac_arena, s.d_ac_counts, c->d_ac_offsets, s.d_ac_totals, s.d_ac,
                           c->ac_arena, c->ac_max_wg, 0, c->stream);
    if (rc)
        return fail(c, rc, "Mode A/C kernel launch failed");
    return 0;
}

/* Enqueue the GPU stage for the batch in the slot: s.nsamples samples at s.d_iq (absolute index s.batch_first). */
int enqueue(msd_ctx *c, Slot &s, int format, const uint32_t *host_noise, bool pipelined)
{
    const uint64_t tile = msd_scan_tile(format);
    const uint32_t ntiles = (uint32_t)((s.nsamples + tile - 1) / tile);
    /* one region per wavefront: MSD_SCAN_WAVES per CU */
    uint32_t tpw = ntiles ? (ntiles + c->max_wg - 1) / c->max_wg : 1;
    if (tpw == 0)
        tpw = 1;
    uint32_t nwg = ntiles ? (ntiles + tpw - 1) / tpw : 0;
    /* Lean layout: only for batches that come through msd_launch_* and will be resolved on the GPU in order on this
     * stream. */
    uint32_t lean_k = 0, lean_tpr = 0;
    s.lean = false;
    s.mag_pass = false; /* set by the scan block below; an empty batch has none and must not inherit the slot's last one */
    if (pipelined && c->lean_ok && nwg && gpu_eligible(c, s) && s.nbuffers <= c->max_wg && !(c->debug_flags & 0x1f)) {
        plan_lean_regions(c, s, tile, lean_k, lean_tpr, nwg);
        tpw = lean_tpr;
        s.lean = true;
        const int grc = follow_arena_growth(c, s);
        if (grc)
            return grc;
    }

    if (!s.lean && nwg) {
        const int erc = ensure_dense(c, s);
        if (erc)
            return erc;
    }
    if (s.nsamples & 7u) { /* the last, partially filled 8-sample group: a zero-padded private copy */
        const size_t bps = bps_of(format);
        HIPCHK(c, hipMemsetAsync(s.d_ragged, 0, 64, c->stream));
        HIPCHK(c, hipMemcpyAsync(s.d_ragged, s.d_iq + (s.nsamples & ~7ull) * bps, (s.nsamples & 7u) * bps,
                                 hipMemcpyDeviceToDevice, c->stream));
    }
    /* d_sums is zero: whoever published the slot's previous batch left it so.  The offsets kernel
     * overwrites the totals. */
    const bool fm = format == MSD_FMT_SC16 || format == MSD_FMT_SC16Q11 || s.dc;
    const bool gather_publishes = nwg && !ac_on(c, s) && !fm; /* totals and sums are published by the gather kernel */
    if (!nwg) {
        HIPCHK(c, hipMemsetAsync(s.d_totals, 0, sizeof(uint64_t) * 4, c->stream));
        s.buf_first_valid = false;
    }
    if (ac_on(c, s) && !(s.nbuffers && s.nsamples)) /* (msd_launch_ac's offsets kernel writes them otherwise) */
        HIPCHK(c, hipMemsetAsync(s.d_ac_totals, 0, sizeof(uint64_t) * 4, c->stream));
    /* the three timing events cost about 5 us of stream time each (a barrier packet per record): they are
     * recorded for one batch in every c->timing_interval */
    s.timed = c->timing_interval && (c->enqueue_seq++ % c->timing_interval) == 0;
    if (s.timed)
        HIPCHK(c, hipEventRecord(s.ev_start, c->stream));
    if (nwg) {
        MsdScanParams p{};
        fill_params(c, s, p);
        p.ntiles = ntiles;
        p.tiles_per_wg = tpw;
        p.hits = s.lean ? s.d_rhits : c->d_region_hits;
        p.tries = s.lean ? s.d_rtries : c->d_region_tries;
        /* a tile can never produce more than one hit per position and five tries per hit */
        uint64_t hcap = (s.lean ? s.rhit_arena : c->hit_arena) / nwg, tcap = (s.lean ? s.rtry_arena : c->try_arena) / nwg;
        if (hcap > (uint64_t)tpw * tile)
            hcap = (uint64_t)tpw * tile;
        if (tcap > (uint64_t)tpw * tile * 5)
            tcap = (uint64_t)tpw * tile * 5;
        p.hcap = (uint32_t)hcap;
        p.tcap = (uint32_t)tcap;
        s.lean_hcap = p.hcap;
        s.lean_tcap = p.tcap;
        p.counts = s.lean ? s.d_rcounts : c->d_counts;
        p.wg_totals = s.lean ? s.d_rwgt : c->d_wg_totals;
        if (s.d_pred && s.gpu_resolve) { /* the batch's prediction table: a generation of its own, no wipe */
            s.pred_gen = s.pred_uses % MSD_PRED_GENS;
            if (s.pred_uses && s.pred_gen == 0) /* the 8-bit generations have come round: old entries must go */
                HIPCHK(c, hipMemsetAsync(s.d_pred, 0xFF, sizeof(uint32_t) * MSD_PRED_WORDS, c->stream));
            s.pred_uses++;
            p.pred = reinterpret_cast<unsigned long long *>(s.d_pred);
            p.pred_gen = s.pred_gen;
        }
        const bool tail_here = s.tail_dst && s.nsamples >= (uint64_t)TAIL_SAMPLES &&
                               (((s.nsamples - TAIL_SAMPLES) * bps_of(format)) & 3u) == 0; /* copied as dwords */
        if (s.lean) {
            p.regions_per_buffer = lean_k;
            p.tiles_per_region = lean_tpr;
            p.overflow = reinterpret_cast<unsigned long long *>(s.d_totals + 2);
            if (tail_here) {
                p.tail_src = reinterpret_cast<const uint32_t *>(s.d_iq + (s.nsamples - TAIL_SAMPLES) * bps_of(format));
                p.tail_dst = reinterpret_cast<uint32_t *>(s.tail_dst);
                p.tail_words = (uint32_t)(TAIL_SAMPLES * bps_of(format) / 4);
            }
            s.lean_k = lean_k;
            s.lean_nreg = nwg;
        }
        p.chunk_sums = s.d_sums;
        s.mag_pass = c->cfg.mode_ac && s.d_mag && pipelined && nwg && !host_noise;
        p.mag_out = s.mag_pass ? s.d_mag : nullptr;
        p.tile_sums = (fm && !s.dc && tile == 1024) ? s.d_tile_sums : nullptr;
        p.timers = c->d_timers;
        p.debug_flags = c->debug_flags;
        Slot *carried = nullptr;
        int rc = carry_pending_emit(c, s, nwg, p, &carried);
        if (rc)
            return rc;
        c->scan_queued = false;
        rc = msd_launch_scan(&p, format, nwg, c->stream);
        if (rc) {
            /* nothing was queued: the older batch's records are still owed (finish_gpu / flush_pending_emit write
             * them), as the header promises for a failed launch */
            if (carried)
                c->pending_emit = carried;
            return fail(c, rc, "scan kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        }
        c->scan_queued = true;
        if (s.timed)
            HIPCHK(c, hipEventRecord(s.ev_scan, c->stream));
        if (carried) {
            /* the records are on their way with this scan; without the event nobody could tell when they are
             * complete, so a failure here poisons the context instead of delivering stale records */
            const hipError_t e = hipEventRecord(carried->ev_records, c->stream);
            if (e != hipSuccess) {
                c->failed = true;
                return fail(c, -EIO, "hipEventRecord(ev_records) failed: %s", hipGetErrorString(e));
            }
        }
        if (s.lean) {
            /* no gather: the resolve workgroups read the region slices, the first resolve pass publishes */
            s.buf_first_valid = false;
            if (tail_here)
                s.tail_dst = nullptr; /* the scan's first wavefront copies it */
        } else {
            rc = msd_launch_gather(c->d_counts, c->d_wg_totals, nwg, s.d_totals, c->d_region_hits, c->d_region_tries, p.hcap, p.tcap,
                                   s.d_hits, s.dense_hits, s.d_tries, s.dense_tries, s.d_sums, s.nbuffers,
                                   gather_publishes ? s.h_totals : nullptr, gather_publishes ? s.h_sums : nullptr, nullptr, 0,
                                   tail_here ? s.d_iq + (s.nsamples - TAIL_SAMPLES) * bps_of(format) : nullptr,
                                   tail_here ? s.tail_dst : nullptr, tail_here ? (uint32_t)(TAIL_SAMPLES * bps_of(format)) : 0,
                                   tpw * tile, s.d_buf_first, 0, c->stream);
            s.buf_first_valid = true;
            if (tail_here)
                s.tail_dst = nullptr; /* done */
            if (rc)
                return fail(c, rc, "gather kernel launch failed");
        }
        if (!c->chain_inline && s.ev_scanned) /* the previous batch's chain is queued to start here, beside what follows */
            HIPCHK(c, hipEventRecord(s.ev_scanned, c->stream));
    } else if (s.timed) {
        HIPCHK(c, hipEventRecord(s.ev_scan, c->stream));
    }
    if (fm && s.nbuffers) {
        /* (the apply walk and the Mode A/C gather stay on the scan stream: deferred to the head of the batch's resolve chain
         * they were 2 % slower, LABLOG R4.5; the variant is scripts/experiments/r4_defer_tails.patch) */
        int rc = s.dc ? msd_launch_dc_sums(s.d_magsq, s.nsamples, MSD_CHUNK_SAMPLES, s.nbuffers, s.d_fmeans, s.d_fm_work, 0, c->stream)
                      : msd_launch_float_means(format, s.d_iq, s.nsamples, MSD_CHUNK_SAMPLES, s.nbuffers, s.d_fmeans,
                                               nwg && msd_scan_tile(format) == 1024 ? s.d_tile_sums : nullptr,
                                               s.d_fm_work, 0, c->stream);
        if (rc)
            return fail(c, rc, "float means kernel launch failed");
    }
    if (ac_on(c, s) && s.nbuffers) {
        const int rc = queue_ac_pass(c, s, format, host_noise, fm);
        if (rc)
            return rc;
    }
    if (s.timed)
        HIPCHK(c, hipEventRecord(s.ev_kernels, c->stream));

    /* totals and per-buffer sums go to pinned host memory from this stream, right behind the kernels */
    if (!gather_publishes && !s.lean) {
        int rc = msd_launch_publish(s.d_totals, ac_on(c, s) ? s.d_ac_totals : nullptr, s.d_sums,
                                    fm ? s.d_fmeans : nullptr, s.nbuffers, s.h_totals, s.h_ac_totals, s.h_sums,
                                    s.h_fmeans, c->stream);
        if (rc)
            return fail(c, rc, "publish kernel launch failed");
    }
    if (!s.lean || !c->chain_inline) /* in order, a lean batch's totals and sums come with its first resolve pass (ev_resolve)
                                        and nobody waits for this event; on side streams the chain does */
        HIPCHK(c, hipEventRecord(s.ev_totals, c->stream));
    return 0;
}

/* the slot's pinned Mode A/C candidate list, grown to at least nac entries */
int ensure_ac_host(msd_ctx *c, Slot &s, size_t nac)
{
    if (nac <= s.h_ac_cap)
        return 0;
    size_t cap = s.h_ac_cap ? s.h_ac_cap : (size_t)1 << 14;
    while (cap < nac)
        cap *= 2;
    if (s.h_ac)
        (void)hipHostFree(s.h_ac);
    s.h_ac = nullptr;
    s.h_ac_cap = 0;
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&s.h_ac), cap * sizeof(msd_ac_hit)));
    s.h_ac_cap = cap;
    return 0;
}

/* A batch whose candidate lists did not fit its arenas (an interference storm: a large share of
 * all positions look like preambles) is scanned again in pieces -- halves, quarters, ... down to
 * single buffers, which always fit -- and the pieces' lists are stitched together on the host.
 * Synchronous and slow on purpose; nothing is ever dropped. */
int rerun_in_pieces(msd_ctx *c, Slot &s, int format)
{
    const int erc = ensure_dense(c, s); /* before the pieces copy the slot: they share its dense lists */
    if (erc)
        return erc;
    const uint64_t total_buffers = s.nbuffers;
    for (uint64_t pieces = 2;; pieces *= 2) {
        uint64_t piece = ((s.nsamples + pieces - 1) / pieces + MSD_CHUNK_SAMPLES - 1) / MSD_CHUNK_SAMPLES *
                         MSD_CHUNK_SAMPLES;
        if (piece < MSD_CHUNK_SAMPLES)
            piece = MSD_CHUNK_SAMPLES;
        std::vector<msd_hit> hits;
        std::vector<msd_try> tries;
        std::vector<msd_ac_hit> acs;
        bool again = false;
        for (uint64_t off = 0; off < s.nsamples || (off == 0 && s.nsamples == 0); off += piece) {
            Slot t = s; /* shares the device buffers and events of s */
            t.gpu_resolve = false; /* the host resolver takes the pieces: no predictions wanted (they would land in the
                                      slot's table under a generation its next batch uses) */
            const uint64_t n = s.nsamples - off < piece ? s.nsamples - off : piece;
            const bool is_last = off + n >= s.nsamples;
            const uint64_t b0 = off / MSD_CHUNK_SAMPLES;
            t.d_iq = s.d_iq + off * bps_of(format);
            if (s.d_magsq)
                t.d_magsq = s.d_magsq + off;
            if (off) {
                t.d_prev = s.d_iq + (off - TAIL_SAMPLES) * bps_of(format);
                t.have_prev = 1;
            }
            t.batch_first = s.batch_first + off;
            t.nsamples = n;
            t.nbuffers = (uint32_t)((is_last ? total_buffers : (off + n) / MSD_CHUNK_SAMPLES) - b0);
            t.d_sums = s.d_sums + 2 * b0;
            t.d_fmeans = s.d_fmeans + 2 * b0;
            t.h_sums = s.h_sums + 2 * b0;
            t.h_fmeans = s.h_fmeans + 2 * b0;
            t.mag_pass = false; /* the pieces' Mode A/C passes convert the IQ themselves */
            t.d_mag = nullptr;
            /* mag_buf batches: the pieces keep the noise levels the first pass was given -- from the caller's per-buffer
             * mean_level / mean_power, which for the float converters are not what the integer sums of a MAG16 scan give */
            int rc = enqueue(c, t, format, c->magbuf_noise ? c->magbuf_noise + b0 : nullptr);
            if (rc)
                return rc;
            HIPCHK(c, hipEventSynchronize(t.ev_totals));
            const uint64_t H = s.h_totals[0], Tn = s.h_totals[1];
            const uint64_t nac = ac_on(c, s) ? s.h_ac_totals[0] : 0;
            if (s.h_totals[2] || (ac_on(c, s) && s.h_ac_totals[2])) {
                if (piece == MSD_CHUNK_SAMPLES)
                    return fail(c, -EOVERFLOW, "candidate arena overflow on a single buffer");
                again = true;
                break;
            }
            rc = ensure_host(c, s, H, Tn);
            if (!rc)
                rc = ensure_ac_host(c, s, nac);
            if (rc)
                return rc;
            if (H)
                HIPCHK(c, hipMemcpyAsync(s.h_hits, s.d_hits, H * sizeof(msd_hit), hipMemcpyDeviceToHost, c->copy_stream));
            if (Tn)
                HIPCHK(c, hipMemcpyAsync(s.h_tries, s.d_tries, Tn * sizeof(msd_try), hipMemcpyDeviceToHost, c->copy_stream));
            if (nac)
                HIPCHK(c, hipMemcpyAsync(s.h_ac, s.d_ac, nac * sizeof(msd_ac_hit), hipMemcpyDeviceToHost, c->copy_stream));
            HIPCHK(c, hipStreamSynchronize(c->copy_stream));
            const uint64_t try0 = tries.size();
            for (uint64_t i = 0; i < H; ++i) {
                msd_hit h = s.h_hits[i] + off; /* position is the low field: no carry into the mask */
                if (MSD_HIT_NLIVE(h))
                    h += (msd_hit)try0 << 34;
                hits.push_back(h);
            }
            for (uint64_t i = 0; i < Tn; ++i) {
                msd_try tr = s.h_tries[i];
                tr.pos += (uint32_t)off;
                tries.push_back(tr);
            }
            for (uint64_t i = 0; i < nac; ++i) {
                msd_ac_hit a = s.h_ac[i];
                a.pos += off;
                acs.push_back(a);
            }
            if (s.nsamples == 0)
                break;
        }
        if (again)
            continue;
        int rc = ensure_host(c, s, hits.size(), tries.size());
        if (!rc)
            rc = ensure_ac_host(c, s, acs.size());
        if (rc)
            return rc;
        if (!hits.empty())
            memcpy(s.h_hits, hits.data(), hits.size() * sizeof(msd_hit));
        if (!tries.empty())
            memcpy(s.h_tries, tries.data(), tries.size() * sizeof(msd_try));
        if (!acs.empty())
            memcpy(s.h_ac, acs.data(), acs.size() * sizeof(msd_ac_hit));
        s.h_totals[0] = hits.size();
        s.h_totals[1] = tries.size();
        s.h_totals[2] = 0;
        if (ac_on(c, s)) {
            s.h_ac_totals[0] = acs.size();
            s.h_ac_totals[2] = 0;
        }
        c->timing.reruns++;
        return 0;
    }
}

/* (msd_ctx.h) Idempotent; blocks only until the batch's kernels are done. */
int start_download(msd_ctx *c, Slot &s, int format)
{
    if (s.download_started)
        return 0;
    if (s.lean) { /* totals, sums and the overflow flag arrive with the first resolve pass (finish_gpu) */
        HIPCHK(c, hipEventRecord(s.ev_copy0, c->copy_stream));
        HIPCHK(c, hipEventRecord(s.ev_copy1, c->copy_stream));
        s.download_started = true;
        return 0;
    }
    const bool trace = c->trace;
    auto td0 = std::chrono::steady_clock::now();
    HIPCHK(c, event_wait(s.ev_totals));
    if (trace && s.timed) {
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, s.ev_start, s.ev_scan);
        (void)hipEventElapsedTime(&b, s.ev_start, s.ev_kernels);
        fprintf(stderr, "start_download: waited %.3f ms for the totals; scan %.3f ms, all kernels %.3f ms after its start\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td0).count(), a, b);
    }
    const bool overflow = s.h_totals[2] || (ac_on(c, s) && s.h_ac_totals[2]);
    if (overflow) {
        int rc = rerun_in_pieces(c, s, format);
        if (rc)
            return rc;
    }
    const uint64_t H = s.h_totals[0], Tn = s.h_totals[1];
    HIPCHK(c, hipEventRecord(s.ev_copy0, c->copy_stream));
    if (overflow) { /* rescanned in pieces and stitched on the host: the host resolver takes it */
        s.gpu_resolve = false;
        s.resolve_inflight = false;
    }
    if (!overflow && !s.gpu_resolve) {
        int rc = ensure_host(c, s, H, Tn);
        if (rc)
            return rc;
        if (H)
            HIPCHK(c, hipMemcpyAsync(s.h_hits, s.d_hits, H * sizeof(msd_hit), hipMemcpyDeviceToHost, c->copy_stream));
        if (Tn)
            HIPCHK(c, hipMemcpyAsync(s.h_tries, s.d_tries, Tn * sizeof(msd_try), hipMemcpyDeviceToHost, c->copy_stream));
        if (ac_on(c, s)) {
            const uint64_t nac = s.h_ac_totals[0];
            rc = ensure_ac_host(c, s, nac);
            if (rc)
                return rc;
            if (nac)
                HIPCHK(c, hipMemcpyAsync(s.h_ac, s.d_ac, nac * sizeof(msd_ac_hit), hipMemcpyDeviceToHost, c->copy_stream));
        }
    }
    HIPCHK(c, hipEventRecord(s.ev_copy1, c->copy_stream));
    s.download_started = true;
    return 0;
}

/* Lean layout: the dense, ordered candidate lists after all (somebody on the host wants them): the gather kernel
 * over the slot's region slices, synchronously.  Totals land in h_totals; the sums were published already. */
int lean_gather_now(msd_ctx *c, Slot &s)
{
    /* the first resolve pass has published the batch's totals: a slot whose region slices were enlarged may hold more
     * than the dense lists were made for */
    const uint64_t H = s.h_totals[0] ? s.h_totals[0] : 1, Tn = s.h_totals[1] ? s.h_totals[1] : 1; /* (never a null list) */
    if (H > s.dense_hits || Tn > s.dense_tries) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (H > s.dense_hits) {
            (void)hipFree(s.d_hits);
            s.d_hits = nullptr;
            s.dense_hits = 0;
            HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&s.d_hits), (H + H / 8) * sizeof(msd_hit)));
            s.dense_hits = H + H / 8;
        }
        if (Tn > s.dense_tries) {
            (void)hipFree(s.d_tries);
            s.d_tries = nullptr;
            s.dense_tries = 0;
            HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&s.d_tries), (Tn + Tn / 8) * sizeof(msd_try)));
            s.dense_tries = Tn + Tn / 8;
        }
    }
    int rc = msd_launch_gather(s.d_rcounts, s.d_rwgt, s.lean_nreg, s.d_totals, s.d_rhits, s.d_rtries, s.lean_hcap, s.lean_tcap,
                               s.d_hits, s.dense_hits, s.d_tries, s.dense_tries, s.d_sums, s.nbuffers, s.h_totals, nullptr,
                               nullptr, 0, nullptr, nullptr, 0, 0, nullptr, 1, c->stream);
    if (rc)
        return fail(c, rc, "gather kernel launch failed");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* A lean batch overflowed the region slices of its slot (an interference storm, a pulse train: a large share of all
 * positions look like preambles).  The scan counts on past the end of a slice, so the region counts say exactly what
 * every region needed: the slot gets slices the densest region fits (plus an eighth), the batch is scanned again into
 * them and stays on the GPU resolve -- one extra scan instead of the whole batch in pieces through the host resolver
 * (rerun_in_pieces: 0.09-0.7 GS/s on such input).  The slot keeps the bigger slices; the other slots follow at their
 * next launch (enqueue: c->want_*).  0: rescanned, the first resolve pass has to be begun again; 1: not possible (no
 * device memory for it, or it was the Mode A/C arena): the old way; < 0: error. */
int grow_and_rescan(msd_ctx *c, Slot &s, int format)
{
    if (!s.lean || !s.lean_nreg || !s.d_rcounts || (c->cfg.flags & MSD_CFG_NO_ARENA_GROWTH))
        return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<msd_region_counts> rc(s.lean_nreg);
    HIPCHK(c, hipMemcpy(rc.data(), s.d_rcounts, rc.size() * sizeof(msd_region_counts), hipMemcpyDeviceToHost));
    uint64_t mh = 0, mt = 0;
    for (const msd_region_counts &r : rc) {
        mh = r.nhits > mh ? r.nhits : mh;
        mt = r.ntries > mt ? r.ntries : mt;
    }
    if (mh <= s.lean_hcap && mt <= s.lean_tcap)
        return 1; /* the Mode S slices held: it was the Mode A/C arena */
    uint64_t hcap = mh + mh / 8 + 64, tcap = mt + mt / 8 + 64;
    hcap = hcap > s.lean_hcap ? hcap : s.lean_hcap;
    tcap = tcap > s.lean_tcap ? tcap : s.lean_tcap;
    const uint64_t need_h = hcap * s.lean_nreg, need_t = tcap * s.lean_nreg;
    if (need_t >= (1ull << 30) || hcap >= (1ull << 32) || tcap >= (1ull << 32))
        return 1; /* try indices are 30 bits of the hit record */
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess)
        return 1;
    const uint64_t grow_b = (need_h > s.rhit_arena ? (need_h - s.rhit_arena) * sizeof(msd_hit) : 0) +
                            (need_t > s.rtry_arena ? (need_t - s.rtry_arena) * sizeof(msd_try) : 0);
    if (grow_b + (1ull << 30) > free_b)
        return 1;
    const bool grew_h = need_h > s.rhit_arena, grew_t = need_t > s.rtry_arena;
    if (!grow_arena(s.d_rhits, s.rhit_arena, need_h) || !grow_arena(s.d_rtries, s.rtry_arena, need_t))
        return 1;
    /* what the other slots should have before they meet the same traffic, per sample of a batch: from what THIS batch
     * needed (need_h / need_t entries for its nsamples -- not the slot's whole arena, which is sized for max_batch_samples
     * and would turn a short batch's overflow into several hits per sample for everybody), only for the arena that grew,
     * and never more than the kernels can produce -- one hit per position, five tries per hit -- plus the eighth of
     * head-room the slices are given above */
    const double ns = (double)(s.nsamples ? s.nsamples : 1);
    if (grew_h) {
        const double per_h = std::min(1.25, (double)need_h / ns);
        c->want_hits_per_sample = per_h > c->want_hits_per_sample ? per_h : c->want_hits_per_sample;
    }
    if (grew_t) {
        const double per_t = std::min(6.25, (double)need_t / ns);
        c->want_tries_per_sample = per_t > c->want_tries_per_sample ? per_t : c->want_tries_per_sample;
    }
    HIPCHK(c, hipMemsetAsync(s.d_totals, 0, 4 * sizeof(uint64_t), c->stream)); /* the overflow flag the first scan raised */
    s.h_totals[2] = 0;
    if (c->pending_emit == &s)
        c->pending_emit = nullptr;
    const int erc = enqueue(c, s, format, nullptr, true);
    if (erc)
        return erc < 0 ? erc : -EIO;
    if (!s.lean)
        return 1;
    c->timing.reruns++;
    return 0;
}

static int check_batch(msd_ctx *c, const void *p, uint64_t nsamples, int last)
{
    if (!c)
        return -EINVAL;
    if (c->failed)
        return -EIO;
    if (c->finished)
        return fail(c, -EINVAL, "capture already finished; call msd_reset()");
    if (nsamples > c->cfg.max_batch_samples || nsamples > MSD_MAX_BATCH_SAMPLES)
        return fail(c, -E2BIG, "batch of %llu samples exceeds max_batch_samples %llu",
                    (unsigned long long)nsamples, (unsigned long long)c->cfg.max_batch_samples);
    if (!last && (nsamples == 0 || nsamples % MSD_CHUNK_SAMPLES != 0))
        return fail(c, -EINVAL, "only the last batch may be a partial buffer");
    if (nsamples && (!p || (reinterpret_cast<uintptr_t>(p) & 15u)))
        return fail(c, -EINVAL, "IQ pointer must be non-null and 16-byte aligned");
    return 0;
}

/* --dcfilter: the batch's IQ -> DC-blocked magnitudes and squares, the converter state advanced; strictly in stream
 * order on `stream`.  The parallel-in-time kernels first, the in-order kernel behind them (it returns at once when they
 * came out exact -- they always have so far; MSD_CFG_DC_SEQUENTIAL: the in-order kernel alone). */
int launch_dc_block(msd_ctx *c, const void *d_iq, uint64_t nsamples, uint16_t *d_mag, float *d_magsq, hipStream_t stream)
{
    const void *skip_if = nullptr;
    c->dc_last_parallel = false;
    if (c->d_dc_work && nsamples && (reinterpret_cast<uintptr_t>(d_iq) & 15u) == 0) {
        const uint32_t L = msd_dcp_block_len(nsamples);
        /* a pass that is not needed is two launches that return at once, 12 us: a batch of a buffer or two (at most 128 blocks,
         * 5-10 passes measured, profiles/r06_dc_passes.txt) gets 12 queued, not 24 -- what the in-order kernel behind them
         * would cost such a batch if they ever ran out is a millisecond */
        const int passes = (nsamples + L - 1) / L <= 128u && c->dc_passes > 12 ? 12 : c->dc_passes;
        const int rc = msd_launch_dcfilter_parallel(c->cfg.format, d_iq, nsamples, c->dc_a, c->dc_b, c->d_dcstate, d_mag, d_magsq,
                                                    c->d_dc_work, L, passes, c->dc_fused ? 1 : 0, stream);
        if (rc)
            return rc;
        skip_if = c->d_dc_work;
        c->dc_last_parallel = true;
        c->dc_last_blocks = (uint32_t)((nsamples + L - 1) / L);
    }
    return msd_launch_dcfilter(c->cfg.format, d_iq, nsamples, c->dc_a, c->dc_b, c->d_dcstate, d_mag, d_magsq, skip_if, stream);
}

static int launch(msd_ctx *c, const void *d_iq, uint64_t nsamples, int last)
{
    int rc = check_batch(c, d_iq, nsamples, last);
    if (rc)
        return rc;
    if (c->outstanding >= MSD_PIPELINE_DEPTH)
        return fail(c, -EBUSY, "pipeline full: call msd_collect() first");
    Slot &s = c->slots[(c->head + c->outstanding) % MSD_PIPELINE_DEPTH];
    s.busy = true;
    s.launch_seq = ++c->launch_count;
    s.d_iq = static_cast<const uint8_t *>(d_iq);
    s.d_prev = c->d_tail[c->tail_cur];
    s.have_prev = c->have_prev ? 1 : 0;
    s.d_mag_prev = c->mag_prev;
    s.batch_first = c->next_sample;
    s.nsamples = nsamples;
    s.last = last;
    s.dropped_before = c->pending_dropped;
    c->pending_dropped = 0;
    s.reset_before = c->restart_pending;
    c->restart_pending = false;
    s.threshold = c->cfg.preamble_threshold;
    s.dc = c->dc;
    if (c->dc) { /* the converter proper: IQ -> DC-blocked magnitudes, strictly in stream order */
        rc = launch_dc_block(c, d_iq, nsamples, s.d_dcmag, s.d_magsq, c->stream);
        if (rc) {
            s.busy = false;
            return fail(c, rc, "DC filter kernel launch failed");
        }
        s.d_iq = reinterpret_cast<const uint8_t *>(s.d_dcmag);
    } else if (c->q11_bits) { /* convert_sc16q11_table: the scan runs on its magnitudes and its integer sums are the converter's */
        rc = msd_launch_q11_table(d_iq, nsamples, c->d_q11_table, c->q11_bits, s.d_dcmag, nullptr, c->cu_count, c->stream);
        if (rc) {
            s.busy = false;
            return fail(c, rc, "SC16Q11 table converter launch failed");
        }
        s.d_iq = reinterpret_cast<const uint8_t *>(s.d_dcmag);
    }
    /* a capture of N samples is floor(N/131072)+1 buffers, the last possibly empty
     * (sdr_ifile.c:192-216: EOF is only noticed by a short read) */
    s.nbuffers = (uint32_t)(nsamples / MSD_CHUNK_SAMPLES) + (last ? 1u : 0u);
    const int tail_nxt = (c->tail_cur + 1) % (MSD_PIPELINE_DEPTH + 1);
    s.tail_dst = nsamples >= (uint64_t)TAIL_SAMPLES ? c->d_tail[tail_nxt] : nullptr;
    auto tl0 = std::chrono::steady_clock::now();
    c->scan_queued = false;
    s.gpu_resolve = gpu_eligible(c, s);
    rc = enqueue(c, s, c->scan_format, nullptr, true);
    if (rc) { /* nothing was consumed: the dropped samples and a pending restart wait for the next launch */
        if (c->scan_queued) /* ... unless kernels of this batch are on the stream already: their follow-ups are missing,
                               the slot's lists and sums are half written -- only msd_reset() starts over */
            c->failed = true;
        s.busy = false;
        c->pending_dropped += s.dropped_before;
        c->restart_pending = c->restart_pending || s.reset_before;
        s.dropped_before = 0;
        s.reset_before = false;
        return rc;
    }
    if (c->trace) {
        static const auto t_origin = std::chrono::steady_clock::now();
        fprintf(stderr, "launch: at %.3f ms, enqueue %.3f ms\n",
                std::chrono::duration<double, std::milli>(tl0 - t_origin).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count());
    }
    s.resolve_inflight = false;
    s.ahead_done = false;
    s.ahead_verdict = 0;
    if (s.gpu_resolve && c->outstanding == 0) { /* no earlier batch to wait for: resolve right behind the scan */
        rc = gpu_begin(c, s, c->scan_format);
        if (rc) {
            s.busy = false;
            return rc;
        }
    }
    if (nsamples >= (uint64_t)TAIL_SAMPLES) {
        if (s.tail_dst) /* no gather kernel ran (cannot happen with that many samples) */
            HIPCHK(c, hipMemcpyAsync(s.tail_dst, s.d_iq + (nsamples - TAIL_SAMPLES) * c->scan_bps,
                                     (size_t)TAIL_SAMPLES * c->scan_bps, hipMemcpyDeviceToDevice, c->stream));
        s.tail_dst = nullptr;
        c->tail_cur = tail_nxt;
        c->have_prev = true;
        c->mag_prev = s.mag_pass ? s.d_mag + (nsamples - TAIL_SAMPLES) : nullptr;
    }
    c->next_sample += nsamples;
    c->outstanding++;
    if (last)
        c->finished = true;
    return 0;
}

} /* namespace msd_impl */
#pragma GCC visibility pop

/* ---- the exported entry points that launch a batch ---- */
using namespace msd_impl;

extern "C" {

int msd_launch_device(msd_ctx *c, const void *d_iq, uint64_t nsamples, int last)
{
    if (!c)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return launch(c, d_iq, nsamples, last);
}

int msd_submit_device(msd_ctx *c, const void *d_iq, uint64_t nsamples, int last, msd_message_fn sink,
                      void *user)
{
    if (!c)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    while (c->outstanding) {
        int rc = collect(c, sink, user);
        if (rc)
            return rc;
    }
    int rc = launch(c, d_iq, nsamples, last);
    if (rc)
        return rc;
    return collect(c, sink, user);
}

int msd_launch_host(msd_ctx *c, const void *h_iq, uint64_t nsamples, int last)
{
    if (!c)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (nsamples > c->cfg.max_batch_samples)
        return fail(c, -E2BIG, "batch exceeds max_batch_samples");
    if (c->outstanding >= MSD_PIPELINE_DEPTH)
        return fail(c, -EBUSY, "pipeline full: call msd_collect() first");
    if (nsamples && !h_iq)
        return fail(c, -EINVAL, "IQ pointer must be non-null");
    Slot &s = c->slots[(c->head + c->outstanding) % MSD_PIPELINE_DEPTH];
    if (!s.d_upload) {
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&s.d_upload), c->cfg.max_batch_samples * c->bps + 64));
        HIPCHK(c, hipEventCreateWithFlags(&s.ev_upload, hipEventDisableTiming));
    }
    /* upload on the copy stream (it runs ahead of the kernels of the batches in front), the batch's
     * kernels wait for it through an event */
    if (nsamples)
        HIPCHK(c, hipMemcpyAsync(s.d_upload, h_iq, nsamples * c->bps, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, hipEventRecord(s.ev_upload, c->copy_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, s.ev_upload, 0));
    return launch(c, s.d_upload, nsamples, last);
}

int msd_submit_host(msd_ctx *c, const void *h_iq, uint64_t nsamples, int last, msd_message_fn sink,
                    void *user)
{
    if (!c)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (nsamples > c->cfg.max_batch_samples)
        return fail(c, -E2BIG, "batch exceeds max_batch_samples");
    if (!c->d_stage)
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_stage), c->cfg.max_batch_samples * 4 + 64));
    while (c->outstanding) {
        int rc = collect(c, sink, user);
        if (rc)
            return rc;
    }
    if (nsamples)
        HIPCHK(c, hipMemcpyAsync(c->d_stage, h_iq, nsamples * c->bps, hipMemcpyHostToDevice, c->stream));
    return msd_submit_device(c, c->d_stage, nsamples, last, sink, user);
}

int msd_note_dropped(msd_ctx *c, uint64_t nsamples)
{
    if (!c)
        return -EINVAL;
    if (c->failed)
        return -EIO;
    if (c->finished)
        return fail(c, -EINVAL, "capture already finished; call msd_reset()");
    if (nsamples) {
        c->pending_dropped += nsamples;
        c->have_prev = false; /* MAGBUF_DISCONTINUOUS: fifo.c:178-181 zeroes the overlap */
    }
    return 0;
}

} /* extern "C" */
