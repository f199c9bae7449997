/*
 * msd_capi.cpp -- the C-ABI of include/modes_hip.h: a context's lifetime (msd_create, msd_destroy, msd_reset,
 * msd_restart), its setters and getters, and the exported entry points -- the batch pipeline (msd_launch_* /
 * msd_collect, three batches in flight; msd_submit_* is the depth-1 synchronous form), the converter and mag_buf
 * entries, field decoding and wire encoding of records the caller holds, and the two array sinks.
 *
 * What the entry points drive is in two files, cut by stage: msd_batch.cpp puts a batch on the GPU, msd_collect.cpp
 * takes it off again (the GPU resolve chain, the hand-off to the ordered host resolve stage msd_resolve.c, delivery).
 * Receiver groups (msd_group_*) are driven from msd_group.cpp.  msd_ctx.h is what they all share.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "modes_hip.h"
#include "msd_ctx.h"
#include "msd_internal.h"
#include "msd_frames.h"
#include "msd_kernels.h"

extern "C" int msd_tables_selftest(const msd_tables *t);

#pragma GCC visibility push(hidden) /* internal, some of it shared with the library's other files (msd_ctx.h) */
namespace msd_impl {

/* why the calling thread's last msd_create failed (there is no context to hold the text yet);
 * msd_last_error(NULL) returns it */
thread_local char g_create_err[256] = {0};

int fail(msd_ctx *c, int code, const char *fmt, ...)
{
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof c->err, fmt, ap);
        va_end(ap);
    }
    return code;
}

hipError_t upload_fix2(msd_ctx *c, bool *host_oom)
{
    uint64_t *d[2] = {nullptr, nullptr};
    uint32_t lg[2] = {0, 0};
    hipError_t e = hipSuccess;
    *host_oom = false;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        uint64_t *tab = msd_fix2_table(c->tables, k ? 112 : 56, &lg[k]);
        if (!tab) {
            *host_oom = true;
            e = hipErrorOutOfMemory;
            break;
        }
        const size_t bytes = sizeof(uint64_t) << lg[k];
        e = hipMalloc(reinterpret_cast<void **>(&d[k]), bytes);
        if (e == hipSuccess)
            e = hipMemcpy(d[k], tab, bytes, hipMemcpyHostToDevice);
        free(tab);
    }
    if (e != hipSuccess) {
        (void)hipFree(d[0]);
        (void)hipFree(d[1]);
        return e;
    }
    for (int k = 0; k < 2; ++k) {
        c->d_fix2[k] = d[k];
        c->fix2_lg[k] = lg[k];
    }
    return hipSuccess;
}

void destroy(msd_ctx *c)
{
    if (!c)
        return;
    c->helper.shutdown();
    (void)hipSetDevice(c->cfg.device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    msd_frames_free(c->frames);
    c->frames = nullptr;
    if (c->copy_stream)
        (void)hipStreamSynchronize(c->copy_stream);
    if (c->aux_stream)
        (void)hipStreamSynchronize(c->aux_stream);
    if (c->emit_stream)
        (void)hipStreamSynchronize(c->emit_stream);
    if (c->d_timers) {
        unsigned long long t[16];
        if (hipMemcpy(t, c->d_timers, sizeof t, hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "kernel section cycles (sum over wavefronts):");
            for (int k = 0; k < 12; ++k)
                fprintf(stderr, " [%d]=%llu", k, t[k]);
            fprintf(stderr, "\n");
        }
        (void)hipFree(c->d_timers);
    }
    for (Slot &s : c->slots) {
        (void)hipFree(s.d_hits); (void)hipFree(s.d_tries); (void)hipFree(s.d_totals); (void)hipFree(s.d_buf_first); (void)hipFree(s.d_rec_off); (void)hipFree(s.d_tile_sums); (void)hipFree(s.d_sums); (void)hipFree(s.d_fmeans);
        (void)hipFree(s.d_fm_work); (void)hipFree(s.d_ac_regions); (void)hipFree(s.d_ac_counts);
        if (s.h_totals) (void)hipHostFree(s.h_totals);
        if (s.h_sums) (void)hipHostFree(s.h_sums);
        if (s.h_fmeans) (void)hipHostFree(s.h_fmeans);
        if (s.h_hits) (void)hipHostFree(s.h_hits);
        if (s.h_tries) (void)hipHostFree(s.h_tries);
        (void)hipFree(s.d_req); (void)hipFree(s.d_pow);
        if (s.h_req) (void)hipHostFree(s.h_req);
        if (s.h_pow) (void)hipHostFree(s.h_pow);
        (void)hipFree(s.d_ac); (void)hipFree(s.d_ac_totals); (void)hipFree(s.d_mag); (void)hipFree(s.d_ragged);
        (void)hipFree(s.d_acc); if (s.d_adds) (void)hipHostFree(s.d_adds); (void)hipFree(s.d_nmsgs); (void)hipFree(s.d_powr); (void)hipFree(s.d_pred); (void)hipFree(s.d_rhits); (void)hipFree(s.d_rtries); (void)hipFree(s.d_rcounts); (void)hipFree(s.d_rwgt); (void)hipFree(s.d_acc_ac); (void)hipFree(s.d_nac);
        if (s.h_rbuf) (void)hipHostFree(s.h_rbuf);
        if (s.h_ctl) (void)hipHostFree(s.h_ctl);
        if (s.h_side) (void)hipHostFree(s.h_side);
        if (s.h_wire) (void)hipHostFree(s.h_wire);
        if (s.h_fields) (void)hipHostFree(s.h_fields);
        (void)hipFree(s.d_dcmag); (void)hipFree(s.d_magsq);
        if (s.ev_resolve) (void)hipEventDestroy(s.ev_resolve);
        if (s.ev_records) (void)hipEventDestroy(s.ev_records);
        if (s.ev_power) (void)hipEventDestroy(s.ev_power);
        if (s.ev_scanned) (void)hipEventDestroy(s.ev_scanned);
        if (s.ev_upload) (void)hipEventDestroy(s.ev_upload);
        (void)hipFree(s.d_upload);
        if (s.h_ac_totals) (void)hipHostFree(s.h_ac_totals);
        if (s.h_ac) (void)hipHostFree(s.h_ac);
        hipEvent_t *evs[] = {&s.ev_start, &s.ev_scan, &s.ev_kernels, &s.ev_totals, &s.ev_copy0, &s.ev_copy1};
        for (hipEvent_t *e : evs)
            if (*e)
                (void)hipEventDestroy(*e);
    }
    (void)hipFree(c->d_lut); (void)hipFree(c->d_crc); (void)hipFree(c->d_syn56); (void)hipFree(c->d_syn112); (void)hipFree(c->d_slicer); (void)hipFree(c->d_synhash);
    (void)hipFree(c->d_fix2[0]); (void)hipFree(c->d_fix2[1]);
    (void)hipFree(c->d_dcstate); (void)hipFree(c->d_dc_work); (void)hipFree(c->d_fm_work); (void)hipFree(c->d_q11_table); (void)hipFree(c->d_conv_magsq);
    if (c->h_conv)
        (void)hipHostFree(c->h_conv);
    (void)hipFree(c->d_region_hits); (void)hipFree(c->d_region_tries); (void)hipFree(c->d_counts); (void)hipFree(c->d_wg_totals);
    (void)hipFree(c->d_ac_offsets);
    (void)hipFree(c->d_noise);
    (void)hipFree(c->d_snaps);
    if (c->h_snaps) (void)hipHostFree(c->h_snaps);
    if (c->ev_aux) (void)hipEventDestroy(c->ev_aux);
    if (c->ev_inputs) (void)hipEventDestroy(c->ev_inputs);
    if (c->h_pred) (void)hipHostFree(c->h_pred);
    if (c->h_pred_count) (void)hipHostFree(c->h_pred_count);
    if (c->h_patches) (void)hipHostFree(c->h_patches);
    for (uint8_t *t : c->d_tail)
        (void)hipFree(t);
    (void)hipFree(c->d_stage);
    (void)hipFree(c->d_mag);
    if (c->copy_stream)
        (void)hipStreamDestroy(c->copy_stream);
    if (c->aux_stream)
        (void)hipStreamDestroy(c->aux_stream);
    if (c->emit_stream)
        (void)hipStreamDestroy(c->emit_stream);
    if (c->own_stream && c->stream)
        (void)hipStreamDestroy(c->stream);
    msd_resolver_free(&c->resolver);
    free(c->tables);
    delete c;
}

} /* namespace msd_impl */
#pragma GCC visibility pop

using namespace msd_impl;

extern "C" {

void msd_array_sink(const msd_message *mm, void *state)
{
    msd_array_sink_state *st = static_cast<msd_array_sink_state *>(state);
    if (st->count < st->cap)
        st->out[st->count] = *mm;
    st->count++;
}

static int create_context(const msd_config *cfg, msd_ctx **out, bool *out_of_memory)
{
    if (!cfg || !out)
        return -EINVAL;
    *out = nullptr;
    if (cfg->format < MSD_FMT_UC8 || cfg->format > MSD_FMT_MAG16 || cfg->nfix_crc < 0 || cfg->nfix_crc > 2 ||
        cfg->preamble_threshold < 1 || cfg->preamble_threshold > MSD_MAX_PREAMBLE_THRESHOLD ||
        ((cfg->flags & MSD_CFG_DC_FILTER) && cfg->format == MSD_FMT_MAG16) || cfg->sc16q11_table_bits < 0 ||
        cfg->sc16q11_table_bits > 11 || (cfg->sc16q11_table_bits && cfg->format != MSD_FMT_SC16Q11) ||
        !(cfg->sample_rate >= 0.0) || (cfg->sample_rate > 0.0 && cfg->sample_rate < 1.0)) {
        snprintf(g_create_err, sizeof g_create_err, "msd_create: invalid configuration");
        return -EINVAL;
    }
    g_create_err[0] = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
    {   /* no GPU: there is deliberately no CPU fallback */
        snprintf(g_create_err, sizeof g_create_err, "no usable HIP device (found %d, asked for device %d): this library has no CPU path", ndev, cfg->device);
        return -ENODEV;
    }
    msd_ctx *c = new (std::nothrow) msd_ctx;
    if (!c)
        return -ENOMEM;
    c->cfg = *cfg;
    if (c->cfg.max_batch_samples == 0)
        c->cfg.max_batch_samples = MSD_CHUNK_SAMPLES;
    if (c->cfg.max_batch_samples > MSD_MAX_BATCH_SAMPLES)
        c->cfg.max_batch_samples = MSD_MAX_BATCH_SAMPLES;
    c->bps = (cfg->format == MSD_FMT_UC8 || cfg->format == MSD_FMT_MAG16) ? 2 : 4;
    c->dc = (cfg->flags & MSD_CFG_DC_FILTER) != 0;
    c->q11_bits = (!c->dc && cfg->format == MSD_FMT_SC16Q11) ? cfg->sc16q11_table_bits : 0;
    c->scan_format = (c->dc || c->q11_bits) ? (int)MSD_FMT_MAG16 : cfg->format;
    c->scan_bps = bps_of(c->scan_format);
    if (c->dc) { /* init_converter's "DC block @ 1Hz", convert.c:479-482, at its sample_rate argument (Modes.sample_rate = 2.4 MHz) */
        c->dc_b = (float)exp(-2.0 * M_PI * 1.0 / (cfg->sample_rate > 0.0 ? cfg->sample_rate : 2400000.0));
        c->dc_a = (float)(1.0 - c->dc_b);
    }

#define CK(call)                                                              \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            snprintf(g_create_err, sizeof g_create_err, "msd_create: %s: %s", #call, hipGetErrorString(e_)); \
            if (e_ == hipErrorOutOfMemory)                                    \
                *out_of_memory = true;                                        \
            (void)hipGetLastError();                                          \
            destroy(c);                                                       \
            return -EIO;                                                      \
        }                                                                     \
    } while (0)

    CK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, cfg->device));
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (cfg->stream) {
        c->stream = static_cast<hipStream_t>(cfg->stream);
    } else {
        CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    CK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    { /* the resolve/power follow-ups are short and on the critical path: let them jump the queued scans */
        int least = 0, greatest = 0;
        CK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        CK(hipStreamCreateWithPriority(&c->aux_stream, hipStreamNonBlocking, greatest));
        CK(hipStreamCreateWithPriority(&c->emit_stream, hipStreamNonBlocking, greatest));
    }

    c->tables = static_cast<msd_tables *>(malloc(sizeof(msd_tables)));
    if (!c->tables) {
        destroy(c);
        return -ENOMEM;
    }
    msd_tables_build(c->tables, cfg->nfix_crc);
    if (msd_tables_selftest(c->tables) != 0) {
        destroy(c);
        return -EDOM; /* the folded UC8 table would not reproduce the reference's */
    }
    static_assert(offsetof(msd_tables, uc8_scan) == sizeof(((msd_tables *)nullptr)->uc8_folded) &&
                  sizeof(((msd_tables *)nullptr)->uc8_folded) == MSD_LUT_SCAN_OFFSET * sizeof(uint16_t),
                  "the scan kernel's table lies directly behind the folded one");
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_lut), sizeof c->tables->uc8_folded + sizeof c->tables->uc8_scan));
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_crc), sizeof c->tables->crc_byte));
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_syn56), sizeof c->tables->syn56 + 16));
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_syn112), sizeof c->tables->syn112 + 16));
    CK(hipMemcpy(c->d_lut, c->tables->uc8_folded, sizeof c->tables->uc8_folded + sizeof c->tables->uc8_scan, hipMemcpyHostToDevice));
    CK(hipMemcpy(c->d_crc, c->tables->crc_byte, sizeof c->tables->crc_byte, hipMemcpyHostToDevice));
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_slicer), sizeof c->tables->slicer));
    CK(hipMemcpy(c->d_slicer, c->tables->slicer, sizeof c->tables->slicer, hipMemcpyHostToDevice));
    CK(hipMemcpy(c->d_syn56, c->tables->syn56, sizeof c->tables->syn56, hipMemcpyHostToDevice));
    CK(hipMemcpy(c->d_syn112, c->tables->syn112, sizeof c->tables->syn112, hipMemcpyHostToDevice));
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_synhash), sizeof c->tables->synhash));
    CK(hipMemcpy(c->d_synhash, c->tables->synhash, sizeof c->tables->synhash, hipMemcpyHostToDevice));
    if (cfg->nfix_crc == 2) { /* --aggressive, crc.c:374-379 */
        bool host_oom = false;
        const hipError_t e = upload_fix2(c, &host_oom);
        if (host_oom) {
            destroy(c);
            return -ENOMEM;
        }
        CK(e);
    }

    const uint64_t B = c->cfg.max_batch_samples;
    /* Candidate arenas.  Base size: one hit per 8 samples, one live try per 16 -- eight times the benchmark capture's
     * density, and all that round 1's 8 GB budget allowed.  Default since round 4: four times the base, one hit per 2
     * samples and one try per 4 (14.5 GB per context at 128 Mi-sample batches, of 288): a burst of pulse trains that fills a
     * tenth of every buffer with preambles of five trial phases each stays on the fast path instead of sending the
     * whole batch through rerun_in_pieces (profiles/r04_density.txt: 74 against 1.2 GS/s).  What overflows even these is
     * rescanned in pieces as before -- nothing is ever truncated. */
    uint64_t hit_want = B / 8, try_want = B / 16;
    if (cfg->test_arena_permille > 0) { /* explicit size in thousandths of the base (tests: provoke the overflow path) */
        const uint64_t pm = (uint64_t)cfg->test_arena_permille;
        hit_want = hit_want * pm / 1000;
        try_want = try_want * pm / 1000;
    } else {
        hit_want *= 4;
        try_want *= 4;
    }
    c->hit_arena = hit_want > MIN_HIT_ARENA ? hit_want : MIN_HIT_ARENA;
    c->try_arena = try_want > MIN_TRY_ARENA ? try_want : MIN_TRY_ARENA;
    c->max_wg = (uint32_t)c->cu_count * MSD_SCAN_WAVES * MSD_SCAN_WGS_PER_CU;
    c->max_buffers = (uint32_t)(B / MSD_CHUNK_SAMPLES) + 2u;
    /* (the arenas of the layouts without region slices -- c->d_region_*, the slots' dense lists d_hits / d_tries: 60 of the
     * 108 bytes per sample -- are made when a batch first takes such a layout: ensure_dense(); a context that only ever
     * runs the lean pipelined path, the default, never allocates them) */
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_counts), c->max_wg * sizeof(msd_region_counts)));
    CK(hipMalloc(reinterpret_cast<void **>(&c->d_wg_totals), (size_t)c->cu_count * MSD_SCAN_WGS_PER_CU * sizeof(msd_wg_totals)));
    if (cfg->mode_ac) {
        c->ac_arena = B / 32 > MIN_HIT_ARENA ? B / 32 : MIN_HIT_ARENA;
        c->ac_max_wg = (uint32_t)c->cu_count * 28u; /* regions of the Mode A/C candidate kernel: one per wavefront, 28 resident per CU (54 registers, 5 KB of LDS each) */
        CK(hipMalloc(reinterpret_cast<void **>(&c->d_ac_offsets), c->ac_max_wg * 2 * sizeof(uint64_t)));
        CK(hipMalloc(reinterpret_cast<void **>(&c->d_noise), c->max_buffers * sizeof(uint32_t)));
    }
    if (cfg->format != MSD_FMT_UC8 || (cfg->flags & MSD_CFG_DC_FILTER))
        CK(hipMalloc(&c->d_fm_work, msd_fm_work_bytes(1))); /* the converter entry's one buffer; the batches have their slots' */
    for (uint8_t *&t : c->d_tail) {
        CK(hipMalloc(reinterpret_cast<void **>(&t), (size_t)TAIL_SAMPLES * 4));
        CK(hipMemset(t, 0, (size_t)TAIL_SAMPLES * 4));
    }
    for (Slot &s : c->slots) {
        CK(hipMalloc(reinterpret_cast<void **>(&s.d_totals), 4 * sizeof(uint64_t)));
        CK(hipMalloc(reinterpret_cast<void **>(&s.d_buf_first), (c->max_buffers + 2) * sizeof(uint32_t)));
        if (cfg->format != MSD_FMT_UC8 || (cfg->flags & MSD_CFG_DC_FILTER))
            CK(hipMalloc(&s.d_fm_work, msd_fm_work_bytes(c->max_buffers)));
        if (cfg->mode_ac) {
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_ac_regions), c->ac_arena * sizeof(msd_ac_hit)));
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_ac_counts), c->ac_max_wg * sizeof(msd_wg_counts)));
        }
        if (cfg->format == MSD_FMT_SC16 || cfg->format == MSD_FMT_SC16Q11)
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_tile_sums), ((size_t)c->max_buffers * (MSD_CHUNK_SAMPLES / 1024) + 2) * 2 * sizeof(float)));
        CK(hipMalloc(reinterpret_cast<void **>(&s.d_rec_off), (c->max_buffers + 2) * sizeof(uint32_t)));
        CK(hipMalloc(reinterpret_cast<void **>(&s.d_ragged), 64));
        CK(hipMemset(s.d_ragged, 0, 64));
        CK(hipMalloc(reinterpret_cast<void **>(&s.d_sums), 2 * sizeof(uint64_t) * c->max_buffers));
        CK(hipMemset(s.d_sums, 0, 2 * sizeof(uint64_t) * c->max_buffers));
        CK(hipMalloc(reinterpret_cast<void **>(&s.d_fmeans), 2 * sizeof(float) * c->max_buffers));
        CK(hipHostMalloc(reinterpret_cast<void **>(&s.h_totals), 4 * sizeof(uint64_t)));
        if (cfg->mode_ac) {
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_ac), c->ac_arena * sizeof(msd_ac_hit)));
            if (!c->dc && !c->q11_bits && cfg->format != MSD_FMT_MAG16) /* (those scan magnitudes already) */
                CK(hipMalloc(reinterpret_cast<void **>(&s.d_mag), (cfg->max_batch_samples + 4096) * sizeof(uint16_t)));
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_ac_totals), 4 * sizeof(uint64_t)));
            CK(hipHostMalloc(reinterpret_cast<void **>(&s.h_ac_totals), 4 * sizeof(uint64_t)));
        }
        CK(hipHostMalloc(reinterpret_cast<void **>(&s.h_sums), 2 * sizeof(uint64_t) * c->max_buffers));
        CK(hipHostMalloc(reinterpret_cast<void **>(&s.h_fmeans), 2 * sizeof(float) * c->max_buffers));
        if (c->dc) {
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_dcmag), c->cfg.max_batch_samples * sizeof(uint16_t) + 64));
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_magsq), c->cfg.max_batch_samples * sizeof(float) + 64));
        } else if (c->q11_bits) { /* the table converter's magnitudes: what the scan kernel reads */
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_dcmag), c->cfg.max_batch_samples * sizeof(uint16_t) + 64));
            CK(hipMemset(s.d_dcmag, 0, c->cfg.max_batch_samples * sizeof(uint16_t) + 64));
        }
        hipEvent_t *evs[] = {&s.ev_start, &s.ev_scan, &s.ev_kernels, &s.ev_totals, &s.ev_copy0, &s.ev_copy1};
        for (hipEvent_t *e : evs)
            CK(hipEventCreate(e));
    }
    if (c->q11_bits) {
        std::vector<uint16_t> tab((size_t)1 << (2 * c->q11_bits));
        msd_sc16q11_table_build(c->q11_bits, tab.data());
        CK(hipMalloc(reinterpret_cast<void **>(&c->d_q11_table), tab.size() * sizeof(uint16_t)));
        CK(hipMemcpy(c->d_q11_table, tab.data(), tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    if (c->dc) {
        CK(hipMalloc(reinterpret_cast<void **>(&c->d_dcstate), 2 * sizeof(float)));
        CK(hipMemset(c->d_dcstate, 0, 2 * sizeof(float))); /* convert.c:476-477 */
        if (!(cfg->flags & MSD_CFG_DC_SEQUENTIAL)) { /* 0.3 MB + 8 bytes per 64 samples of a batch */
            CK(hipMalloc(&c->d_dc_work, msd_dcp_work_bytes(c->cfg.max_batch_samples, 0)));
            c->dc_passes = (cfg->flags & MSD_CFG_DC_ONE_PASS) ? 1 : 24;
            c->dc_fused = (cfg->flags & MSD_CFG_DC_FUSED_LAUNCH) != 0;
        }
    }
    {
        c->trace = (cfg->flags & MSD_CFG_TRACE) != 0;
        c->resolver.trace = c->trace;
        c->resolver.threads = cfg->resolve_threads > 0 ? cfg->resolve_threads : 0;
        /* Where the resolve chain (prediction, resolve, power, records) runs.  In order on the
         * scan stream when that stream carries nothing but scans (UC8 / magnitudes, Mode S only): a kernel that
         * shares the GPU with a scan slows it by about its own duration, so side streams buy 2 % there and make
         * the scan launches 15 % longer.  On side streams (prediction + resolve on a high-priority one, power +
         * records on a third) when the scan stream also carries the latency-bound float-sum or Mode A/C
         * kernels, which the chain overlaps well: +13..17 % whole-job rate, measured.  MSD_CFG_CHAIN_IN_ORDER /
         * MSD_CFG_CHAIN_SIDE_STREAMS override. */
        {
            const bool follow_ups = cfg->mode_ac || cfg->format == MSD_FMT_SC16 || cfg->format == MSD_FMT_SC16Q11 ||
                                    (cfg->flags & MSD_CFG_DC_FILTER);
            c->chain_inline = (cfg->flags & MSD_CFG_CHAIN_IN_ORDER) ? true : (cfg->flags & MSD_CFG_CHAIN_SIDE_STREAMS) ? false : !follow_ups;
        }
        c->no_helper = (cfg->flags & MSD_CFG_NO_HELPER) != 0;
        c->emit_fused = c->chain_inline && !(cfg->flags & MSD_CFG_DECODE_FIELDS) && !(cfg->flags & MSD_CFG_EMIT_KERNEL);
        /* the signal power in the resolve workgroups (no kernel of its own): in the in-order layout it takes a kernel
         * and a gap off the stream; on side streams, where the resolve kernel shares the GPU with a scan, a longer
         * resolve kernel costs more than the small power kernel behind it (measured: SC16 121 -> 124.5, Mode A/C 149 ->
         * 156 GS/s with the kernel) */
        c->power_fused = (cfg->flags & MSD_CFG_POWER_IN_RESOLVE) ? true : (cfg->flags & MSD_CFG_POWER_KERNEL) ? false : c->chain_inline;
        c->resolve_ahead = !(cfg->flags & MSD_CFG_NO_RESOLVE_AHEAD);
        c->wait_inputs_on_stream = (cfg->flags & MSD_CFG_WAIT_INPUTS_ON_STREAM) != 0;
        c->helper.device = cfg->device;
        c->debug_flags = cfg->debug_flags;
        c->gpu_resolve = !(cfg->flags & MSD_CFG_HOST_RESOLVE);
        c->want_fields = (cfg->flags & MSD_CFG_DECODE_FIELDS) != 0;
        if (cfg->test_inline_adds > 0 && (uint32_t)cfg->test_inline_adds < MSD_RB_ADD_INLINE)
            c->inline_adds = (uint32_t)cfg->test_inline_adds;
        else if (cfg->test_inline_adds < 0)
            c->inline_adds = 0; /* every add through the long list */
    }
    /* (every layout: UC8 / magnitudes in order, 16-bit IQ and Mode A/C with the chain on side streams) */
    c->lean_ok = c->gpu_resolve && !c->dc && !(cfg->flags & MSD_CFG_NO_LEAN);
    if (c->lean_ok)
        for (Slot &s : c->slots) {
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_rhits), c->hit_arena * sizeof(msd_hit)));
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_rtries), c->try_arena * sizeof(msd_try)));
            s.rhit_arena = c->hit_arena;
            s.rtry_arena = c->try_arena;
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_rcounts), c->max_wg * sizeof(msd_region_counts)));
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_rwgt), (size_t)c->cu_count * MSD_SCAN_WGS_PER_CU * sizeof(msd_wg_totals)));
            CK(hipMemset(s.d_totals, 0, 4 * sizeof(uint64_t)));
        }
    if (c->gpu_resolve) {
        const size_t ctl_bytes = (size_t)28 * c->max_buffers;
        for (Slot &s : c->slots) {
            CK(hipHostMalloc(reinterpret_cast<void **>(&s.h_rbuf), sizeof(msd_rbuf) * c->max_buffers));
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_acc), sizeof(msd_acc) * MSD_RB_MSG_CAP * c->max_buffers));
            /* (page-locked host memory the kernels write into: see finish_gpu) */
            CK(hipHostMalloc(reinterpret_cast<void **>(&s.d_adds), sizeof(uint32_t) * MSD_RB_MSG_CAP * c->max_buffers));
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_nmsgs), sizeof(uint32_t) * c->max_buffers));
            if (cfg->mode_ac) {
                CK(hipMalloc(reinterpret_cast<void **>(&s.d_acc_ac), sizeof(uint32_t) * MSD_RB_AC_CAP * c->max_buffers));
                CK(hipMalloc(reinterpret_cast<void **>(&s.d_nac), sizeof(uint32_t) * c->max_buffers));
            }
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_pred), sizeof(uint32_t) * MSD_PRED_WORDS));
            CK(hipMemset(s.d_pred, 0xFF, sizeof(uint32_t) * MSD_PRED_WORDS)); /* every slot vacant (generation 0xff) */
            CK(hipMalloc(reinterpret_cast<void **>(&s.d_powr), sizeof(uint64_t) * MSD_RB_MSG_CAP * c->max_buffers));
            CK(hipHostMalloc(reinterpret_cast<void **>(&s.h_ctl), ctl_bytes));
            memset(s.h_ctl, 0, ctl_bytes);
            CK(hipEventCreateWithFlags(&s.ev_resolve, hipEventDisableTiming));
            CK(hipEventCreateWithFlags(&s.ev_records, hipEventDisableTiming));
            CK(hipEventCreateWithFlags(&s.ev_power, hipEventDisableTiming));
            CK(hipEventCreateWithFlags(&s.ev_scanned, hipEventDisableTiming));
        }
        CK(hipMalloc(reinterpret_cast<void **>(&c->d_snaps), sizeof(uint32_t) * MSD_SNAP_WORDS * (SNAP_CAP + 1)));
        CK(hipHostMalloc(reinterpret_cast<void **>(&c->h_snaps), sizeof(uint32_t) * MSD_SNAP_WORDS * (SNAP_CAP + 1)));
        CK(hipEventCreateWithFlags(&c->ev_aux, hipEventDisableTiming));
        CK(hipEventCreateWithFlags(&c->ev_inputs, hipEventDisableTiming));
        CK(hipHostMalloc(reinterpret_cast<void **>(&c->h_pred), sizeof(msd_pred_entry) * MSD_PRED_LIST));
        CK(hipHostMalloc(reinterpret_cast<void **>(&c->h_pred_count), 64));
        CK(hipHostMalloc(reinterpret_cast<void **>(&c->h_patches), sizeof(msd_pred_patch) * 2 * MSD_PRED_LIST));
        *c->h_pred_count = 0;
    } else {
        c->gpu_resolve = false;
    }
#undef CK
#ifdef MSD_KERNEL_TIMING /* -DMSD_KERNEL_TIMING builds only: the scan kernel's section clocks, printed by msd_destroy */
    {
        if (hipMalloc(reinterpret_cast<void **>(&c->d_timers), 16 * sizeof(unsigned long long)) == hipSuccess)
            (void)hipMemset(c->d_timers, 0, 16 * sizeof(unsigned long long));
    }
#endif
    c->resolver.stats = &c->stats;
    c->resolver.mode_ac = cfg->mode_ac;
    msd_resolver_reset(&c->resolver);
    *out = c;
    return 0;
}

int msd_create(const msd_config *cfg, msd_ctx **out)
{
    bool oom = false;
    int rc = create_context(cfg, out, &oom);
    if (rc && oom && cfg->test_arena_permille == 0) {
        /* The default candidate arenas are four times the base size (108 bytes per sample of max_batch_samples over
         * the four pipeline slots).  On a smaller or a shared GPU that may not fit where the base size does: one more
         * try at the base size -- the only price is an earlier arena overflow (a batch rescanned in pieces) on captures
         * that are mostly preamble -- and the context says so (msd_arena_permille). */
        msd_config smaller = *cfg;
        smaller.test_arena_permille = 1000;
        oom = false;
        rc = create_context(&smaller, out, &oom);
    }
    return rc;
}

int msd_arena_permille(const msd_ctx *ctx)
{
    if (!ctx)
        return -EINVAL;
    return ctx->cfg.test_arena_permille > 0 ? ctx->cfg.test_arena_permille : 4000;
}

void msd_destroy(msd_ctx *ctx)
{
    destroy(ctx);
}

const char *msd_last_error(const msd_ctx *ctx)
{
    return ctx ? ctx->err : g_create_err; /* NULL: why this thread's last msd_create failed */
}

int msd_reset(msd_ctx *c)
{
    if (!c)
        return -EINVAL;
    if (c->outstanding && !c->failed)
        return fail(c, -EBUSY, "batches outstanding");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->failed) { /* drop whatever was in flight when a batch failed */
        HIPCHK(c, hipDeviceSynchronize());
        for (Slot &s : c->slots) {
            s.busy = false;
            s.resolve_inflight = false;
            s.ahead_done = false;
            s.ahead_verdict = 0;
        }
        c->head = 0;
        c->outstanding = 0;
        c->pending_emit = nullptr;
        c->failed = false;
    }
    c->next_sample = 0;
    c->have_prev = false;
    c->finished = false;
    c->pending_dropped = 0;
    if (c->d_dcstate)
        HIPCHK(c, hipMemset(c->d_dcstate, 0, 2 * sizeof(float)));
    c->helper.wait();
    msd_resolver_reset(&c->resolver);
    msd_frames_reset(c->frames);
    memset(&c->timing, 0, sizeof c->timing);
    return 0;
}

int msd_frames_get_view(msd_ctx *c, msd_frames_view *v)
{
    if (!c || !v)
        return -EINVAL;
    memset(v, 0, sizeof *v);
    v->stream = c->stream;
    v->device = c->cfg.device;
    v->busy = c->outstanding != 0;
    v->failed = c->failed;
    v->tables.crc_byte = c->d_crc;
    v->tables.synhash = c->cfg.nfix_crc >= 1 ? c->d_synhash : nullptr;
    v->tables.synh_mul56 = c->tables->synhash_mul[0];
    v->tables.synh_mul112 = c->tables->synhash_mul[1];
    v->tables.fix2[0] = c->d_fix2[0];
    v->tables.fix2[1] = c->d_fix2[1];
    v->tables.fix2_lg[0] = c->fix2_lg[0];
    v->tables.fix2_lg[1] = c->fix2_lg[1];
    v->tables.nfix = c->cfg.nfix_crc;
    v->tables.mode_ac = c->cfg.mode_ac;
    v->filter = &c->resolver.filter;
    v->state = &c->frames;
    v->err = c->err;
    v->errlen = sizeof c->err;
    return 0;
}

int msd_decode_fields_device(msd_ctx *c, const msd_message *msgs, size_t n, msd_fields *out)
{
    if (!c || (n && (!msgs || !out)) || n > (1u << 24))
        return -EINVAL;
    if (n == 0)
        return 0;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    msd_message *d_in = nullptr;
    msd_fields *d_out = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_in), n * sizeof *d_in);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&d_out), n * sizeof *d_out);
    int rc = 0;
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_in, msgs, n * sizeof *d_in, hipMemcpyHostToDevice, c->aux_stream);
    if (e == hipSuccess)
        rc = msd_launch_fields(d_in, d_out, (uint32_t)n, c->aux_stream);
    if (e == hipSuccess && !rc)
        e = hipMemcpyAsync(out, d_out, n * sizeof *d_out, hipMemcpyDeviceToHost, c->aux_stream);
    if (e == hipSuccess && !rc)
        e = hipStreamSynchronize(c->aux_stream);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (e != hipSuccess)
        return fail(c, -EIO, "msd_decode_fields_device: %s", hipGetErrorString(e));
    return rc ? fail(c, rc, "field kernel launch failed") : 0;
}

/* Lengths and their scan, the stream's length to the host, then -- if it fits -- the store into a device array and two
 * copies into the caller's. */
int msd_wire_encode(msd_ctx *c, const msd_message *msgs, size_t n, int on_device, int format, uint32_t flags, uint8_t *out,
                    size_t cap, size_t *out_len, uint32_t *ends)
{
    if (!c || !out_len)
        return -EINVAL;
    if (format != MSD_WIRE_BEAST && format != MSD_WIRE_AVR && format != MSD_WIRE_AVR_MLAT)
        return fail(c, -EINVAL, "msd_wire_encode: unknown format %d", format);
    if (flags & ~MSD_WIRE_VERBATIM)
        return fail(c, -EINVAL, "msd_wire_encode: unknown flags 0x%x", flags);
    if ((n && !msgs) || n > (1u << 24))
        return fail(c, -EINVAL, "msd_wire_encode: no records, or more than 2^24");
    if (c->failed)
        return fail(c, -EIO, "an earlier call failed");
    if (c->outstanding)
        return fail(c, -EBUSY, "batches outstanding");
    *out_len = 0;
    if (n == 0)
        return 0;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int verbatim = (flags & MSD_WIRE_VERBATIM) ? 1 : 0;
    const uint32_t nblocks = (uint32_t)((n + 255) / 256);
    msd_message *d_in = nullptr;
    uint8_t *d_lens = nullptr, *d_out = nullptr;
    uint32_t *d_sums = nullptr, *d_ends = nullptr;
    uint32_t total = 0;
    int rc = 0;
    bool nospc = false;
    hipError_t e = hipSuccess;
    if (!on_device) {
        e = hipMalloc(reinterpret_cast<void **>(&d_in), n * sizeof *d_in);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_in, msgs, n * sizeof *d_in, hipMemcpyHostToDevice, c->aux_stream);
        msgs = d_in;
    }
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&d_lens), n);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void **>(&d_sums), sizeof(uint32_t) * ((size_t)nblocks + 1));
    if (e == hipSuccess)
        rc = msd_launch_wire_lengths(msgs, (uint32_t)n, format, verbatim, d_lens, d_sums, c->aux_stream);
    if (e == hipSuccess && !rc)
        e = hipMemcpyAsync(&total, d_sums + nblocks, sizeof total, hipMemcpyDeviceToHost, c->aux_stream);
    if (e == hipSuccess && !rc)
        e = hipStreamSynchronize(c->aux_stream);
    if (e == hipSuccess && !rc) {
        *out_len = total;
        nospc = total > cap || (total && !out);
    }
    if (e == hipSuccess && !rc && !nospc) {
        e = hipMalloc(reinterpret_cast<void **>(&d_out), (size_t)total + 16);
        if (e == hipSuccess && ends)
            e = hipMalloc(reinterpret_cast<void **>(&d_ends), n * sizeof(uint32_t));
        if (e == hipSuccess)
            rc = msd_launch_wire_store(msgs, (uint32_t)n, format, verbatim, d_lens, d_sums, d_out, d_ends, c->aux_stream);
        if (e == hipSuccess && !rc && total)
            e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, c->aux_stream);
        if (e == hipSuccess && !rc && ends)
            e = hipMemcpyAsync(ends, d_ends, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->aux_stream);
        if (e == hipSuccess && !rc)
            e = hipStreamSynchronize(c->aux_stream);
    }
    (void)hipFree(d_in);
    (void)hipFree(d_lens);
    (void)hipFree(d_sums);
    (void)hipFree(d_out);
    (void)hipFree(d_ends);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, e == hipErrorOutOfMemory ? -ENOMEM : -EIO, "msd_wire_encode: %s", hipGetErrorString(e));
    }
    if (rc)
        return fail(c, rc, "wire kernel launch failed");
    if (nospc)
        return fail(c, -ENOSPC, "msd_wire_encode: %u bytes needed, room for %zu", total, cap);
    return 0;
}

int msd_restart(msd_ctx *c)
{
    if (!c)
        return -EINVAL;
    if (!c->outstanding)
        return msd_reset(c);
    if (!c->finished)
        return fail(c, -EINVAL, "msd_restart: the running capture has not been closed (last != 0) yet");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->next_sample = 0;
    c->have_prev = false;
    c->finished = false;
    c->pending_dropped = 0;
    if (c->d_dcstate) /* behind the converter kernels of the capture that is still draining */
        HIPCHK(c, hipMemsetAsync(c->d_dcstate, 0, 2 * sizeof(float), c->stream));
    c->restart_pending = true;
    return 0;
}

int msd_set_timing_interval(msd_ctx *c, uint32_t every)
{
    if (!c)
        return -EINVAL;
    c->timing_interval = every;
    c->enqueue_seq = 0;
    return 0;
}

int msd_set_preamble_threshold(msd_ctx *c, int threshold)
{
    if (!c)
        return -EINVAL;
    if (threshold < 1 || threshold > MSD_MAX_PREAMBLE_THRESHOLD)
        return fail(c, -EINVAL, "preamble threshold %d outside 1..%d", threshold, MSD_MAX_PREAMBLE_THRESHOLD);
    c->cfg.preamble_threshold = threshold;
    return 0;
}

void msd_array_fields_sink(const msd_message *mm, const msd_fields *fields, void *state)
{
    msd_array_fields_sink_state *st = static_cast<msd_array_fields_sink_state *>(state);
    if (st->count < st->cap) {
        st->out[st->count] = *mm;
        st->fields[st->count] = *fields;
    }
    st->count++;
}

int msd_host_alloc(msd_ctx *c, size_t bytes, void **out)
{
    if (!c || !out)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    *out = nullptr;
    HIPCHK(c, hipHostMalloc(out, bytes ? bytes : 1));
    return 0;
}

void msd_host_free(msd_ctx *c, void *p)
{
    if (c && p) {
        (void)hipSetDevice(c->cfg.device);
        (void)hipHostFree(p);
    }
}

int msd_thread_attach(msd_ctx *c)
{
    if (!c)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    (void)hipStreamQuery(c->stream);
    (void)hipGetLastError();
    return 0;
}

int msd_host_register(msd_ctx *c, void *p, size_t bytes)
{
    if (!c || !p || !bytes)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipHostRegister(p, bytes, hipHostRegisterDefault));
    return 0;
}

void msd_host_unregister(msd_ctx *c, void *p)
{
    if (c && p) {
        (void)hipSetDevice(c->cfg.device);
        (void)hipHostUnregister(p);
    }
}

int msd_get_stats(const msd_ctx *c, msd_stats *st)
{
    if (!c || !st)
        return -EINVAL;
    const_cast<msd_ctx *>(c)->helper.wait(); /* the power statistics of the last batch are summed on the helper thread */
    *st = c->stats;
    return 0;
}

int msd_get_timing(const msd_ctx *c, msd_timing *t)
{
    if (!c || !t)
        return -EINVAL;
    *t = c->timing;
    return 0;
}

int msd_dc_filter_status(msd_ctx *c, uint32_t out[4])
{
    if (!c || !out || !c->dc)
        return -EINVAL;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!c->d_dc_work || !c->dc_last_parallel)
        return 0;
    uint32_t ctl[12] = {0};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(ctl, c->d_dc_work, sizeof ctl, hipMemcpyDeviceToHost));
    out[0] = ctl[0];  /* DcpCtl.done */
    out[1] = ctl[9] > ctl[10] ? ctl[9] : ctl[10]; /* .passes_ch */
    out[2] = ctl[11]; /* .guessed */
    out[3] = c->dc_last_blocks;
    return 0;
}

int msd_get_buffer_means(const msd_ctx *c, double *means, size_t cap)
{
    if (!c || !means)
        return -EINVAL;
    size_t n = c->means.size() / 2;
    for (size_t i = 0; i < n && i < cap; ++i) {
        means[2 * i] = c->means[2 * i];
        means[2 * i + 1] = c->means[2 * i + 1];
    }
    return (int)n;
}

int msd_convert_begin(msd_ctx *c, const void *iq_data, uint16_t *mag_data, unsigned nsamples)
{
    if (!c || c->cfg.format == MSD_FMT_MAG16)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (nsamples > c->cfg.max_batch_samples)
        return fail(c, -E2BIG, "nsamples exceeds max_batch_samples");
    if (c->conv_pending)
        return fail(c, -EBUSY, "a conversion is in flight: msd_convert_end() first");
    if (!c->d_stage)
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_stage), c->cfg.max_batch_samples * 4 + 64));
    if (!c->d_mag)
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_mag), c->cfg.max_batch_samples * 2 + 64));
    if (!c->h_conv) { /* where the sums come home: page-locked, so that nothing of this call waits for the device */
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&c->h_conv), 4 * sizeof(uint64_t)));
    }
    Slot &s = c->slots[0];
    if (c->outstanding)
        return fail(c, -EBUSY, "batches outstanding");
    memset(c->h_conv, 0, 4 * sizeof(uint64_t));
    float *h_fm = reinterpret_cast<float *>(c->h_conv + 2);
    HIPCHK(c, hipMemsetAsync(s.d_sums, 0, 2 * sizeof(uint64_t), c->stream));
    if (c->dc) {
        /* convert_*_generic (convert.c:113-213, 374-423): the DC estimate of the two channels lives in the context, as in
         * the reference's struct converter_state, and runs on from call to call -- a context that converts this way is a
         * converter and nothing else (msd_launch_* of the same context would advance the same state) */
        if (nsamples) {
            if (!c->d_conv_magsq)
                HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_conv_magsq), c->cfg.max_batch_samples * sizeof(float) + 64));
            HIPCHK(c, hipMemcpyAsync(c->d_stage, iq_data, (size_t)nsamples * c->bps, hipMemcpyHostToDevice, c->stream));
            int rc = launch_dc_block(c, c->d_stage, nsamples, c->d_mag, c->d_conv_magsq, c->stream);
            if (!rc)
                rc = msd_launch_dc_sums(c->d_conv_magsq, nsamples, nsamples, 1, s.d_fmeans, c->d_fm_work, 0, c->stream);
            if (rc)
                return fail(c, rc, "DC filter converter launch failed");
            HIPCHK(c, hipMemcpyAsync(mag_data, c->d_mag, (size_t)nsamples * 2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_fm, s.d_fmeans, 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        }
        c->conv_pending = true;
        c->conv_n = nsamples;
        return 0;
    }
    if (nsamples) {
        HIPCHK(c, hipMemcpyAsync(c->d_stage, iq_data, (size_t)nsamples * c->bps, hipMemcpyHostToDevice, c->stream));
        int rc = c->q11_bits ? msd_launch_q11_table(c->d_stage, nsamples, c->d_q11_table, c->q11_bits, c->d_mag,
                                                    reinterpret_cast<unsigned long long *>(s.d_sums), c->cu_count, c->stream)
                             : msd_launch_convert(c->cfg.format, c->d_stage, nsamples, c->d_lut, c->d_mag,
                                                  reinterpret_cast<unsigned long long *>(s.d_sums), c->stream);
        if (rc)
            return fail(c, rc, "convert kernel launch failed");
        if (c->cfg.format != MSD_FMT_UC8 && !c->q11_bits) {
            rc = msd_launch_float_means(c->cfg.format, c->d_stage, nsamples, nsamples, 1, s.d_fmeans, nullptr, c->d_fm_work, 0, c->stream);
            if (rc)
                return fail(c, rc, "float means kernel launch failed");
        }
        HIPCHK(c, hipMemcpyAsync(mag_data, c->d_mag, (size_t)nsamples * 2, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->h_conv, s.d_sums, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (c->cfg.format != MSD_FMT_UC8 && !c->q11_bits && nsamples)
        HIPCHK(c, hipMemcpyAsync(h_fm, s.d_fmeans, 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    c->conv_pending = true;
    c->conv_n = nsamples;
    return 0;
}

int msd_convert_end(msd_ctx *c, double *out_mean_level, double *out_mean_power)
{
    if (!c)
        return -EINVAL;
    if (!c->conv_pending)
        return fail(c, -EINVAL, "no conversion in flight");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->conv_pending = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned nsamples = c->conv_n;
    const uint64_t *sums = c->h_conv;
    const float *fm = reinterpret_cast<const float *>(c->h_conv + 2);
    if (!c->dc && (c->cfg.format == MSD_FMT_UC8 || c->q11_bits)) { /* integer sums: convert.c:104-110 and :318-326 */
        if (out_mean_level)
            *out_mean_level = (double)sums[0] / 65536.0 / (double)nsamples;
        if (out_mean_power)
            *out_mean_power = (double)sums[1] / 65535.0 / 65535.0 / (double)nsamples;
    } else {
        if (out_mean_level)
            *out_mean_level = (double)(fm[0] / (float)nsamples);
        if (out_mean_power)
            *out_mean_power = (double)(fm[1] / (float)nsamples);
    }
    return 0;
}

int msd_convert(msd_ctx *c, const void *iq_data, uint16_t *mag_data, unsigned nsamples,
                double *out_mean_level, double *out_mean_power)
{
    int rc = msd_convert_begin(c, iq_data, mag_data, nsamples);
    if (!rc)
        rc = msd_convert_end(c, out_mean_level, out_mean_power);
    return rc;
}

int msd_demodulate_magbufs(msd_ctx *c, const msd_magbuf_view *bufs, unsigned n, msd_message_fn sink, void *user)
{
    if (!c || !bufs || !n)
        return -EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((uint64_t)n * MSD_CHUNK_SAMPLES > c->cfg.max_batch_samples || n > c->max_buffers)
        return fail(c, -E2BIG, "more mag_bufs than max_batch_samples holds");
    for (unsigned k = 0; k < n; ++k) {
        const msd_magbuf_view &b = bufs[k];
        if (!b.data || b.overlap != MSD_OVERLAP || b.validLength < b.overlap || b.validLength - b.overlap > MSD_CHUNK_SAMPLES ||
            (k + 1 < n && b.validLength - b.overlap != MSD_CHUNK_SAMPLES))
            return fail(c, -EINVAL, "mag_buf geometry must be overlap=326, 131072 new samples (the last one: at most)");
    }
    if (c->outstanding)
        return fail(c, -EBUSY, "batches outstanding");
    if (!c->d_stage)
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_stage), c->cfg.max_batch_samples * 4 + 64));
    Slot &s = c->slots[0];
    /* the first buffer's data[0..326) -> the two-sample-padded "previous tail"; every buffer's data[326..) -> the batch */
    uint8_t *tail = c->d_tail[0];
    HIPCHK(c, hipMemsetAsync(tail, 0, (size_t)(TAIL_SAMPLES - MSD_OVERLAP) * 2, c->stream));
    HIPCHK(c, hipMemcpyAsync(tail + (size_t)(TAIL_SAMPLES - MSD_OVERLAP) * 2, bufs[0].data, (size_t)MSD_OVERLAP * 2,
                             hipMemcpyHostToDevice, c->stream));
    uint64_t total = 0;
    std::vector<uint64_t> ts(2 * (size_t)n);
    std::vector<double> means(2 * (size_t)n);
    std::vector<uint32_t> noise(n);
    for (unsigned k = 0; k < n; ++k) {
        const msd_magbuf_view &b = bufs[k];
        const unsigned mlen = b.validLength - b.overlap;
        if (mlen)
            HIPCHK(c, hipMemcpyAsync(c->d_stage + (size_t)k * MSD_CHUNK_SAMPLES * 2, b.data + b.overlap, (size_t)mlen * 2,
                                     hipMemcpyHostToDevice, c->stream));
        total += mlen;
        ts[2 * k] = b.sampleTimestamp;
        ts[2 * k + 1] = b.sysTimestamp;
        means[2 * k] = b.mean_level;
        means[2 * k + 1] = b.mean_power;
        /* demod_2400.c:530-531 from the caller's mag_buf.mean_level / .mean_power */
        const double noise_stddev = sqrt(b.mean_power - b.mean_level * b.mean_level);
        noise[k] = mlen ? (uint32_t)((b.mean_power + noise_stddev) * 65535 + 0.5) : 0u;
    }
    s.busy = true;
    s.d_iq = c->d_stage;
    s.d_prev = tail;
    s.have_prev = 1;
    s.threshold = c->cfg.preamble_threshold;
    s.dropped_before = 0;
    s.gpu_resolve = false; /* the caller's clocks and means: the host resolver */
    s.resolve_inflight = false;
    s.dc = false;
    s.batch_first = 0;
    s.nsamples = total;
    s.nbuffers = n;
    s.last = 1;
    int rc = enqueue(c, s, MSD_FMT_MAG16, c->cfg.mode_ac ? noise.data() : nullptr);
    if (rc) {
        s.busy = false;
        return rc;
    }
    c->magbuf_views = bufs;
    c->magbuf_nviews = n;
    c->magbuf_noise = c->cfg.mode_ac ? noise.data() : nullptr;
    rc = finish(c, s, MSD_FMT_MAG16, sink, user, ts.data(), means.data(), 0);
    c->magbuf_views = nullptr;
    c->magbuf_nviews = 0;
    c->magbuf_noise = nullptr;
    /* the stream interface's tail ring was borrowed: a following msd_submit_* starts afresh */
    c->have_prev = false;
    c->tail_cur = 0;
    return rc;
}

int msd_demodulate_magbuf(msd_ctx *c, const uint16_t *data, unsigned validLength, unsigned overlap,
                          uint64_t sampleTimestamp, uint64_t sysTimestamp, double mean_level,
                          double mean_power, msd_message_fn sink, void *user)
{
    const msd_magbuf_view one = {data, validLength, overlap, sampleTimestamp, sysTimestamp, mean_level, mean_power};
    return msd_demodulate_magbufs(c, &one, 1, sink, user);
}

} /* extern "C" */
