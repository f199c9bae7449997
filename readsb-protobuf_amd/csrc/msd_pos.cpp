/* msd_pos.cpp -- C-ABI of the position tracker (modes_hip.h "positions"): the object, its device memory and the order
 * in which a call queues the kernels of msd_pos_kernels.hip. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "msd_pos.h"
#include "msd_pb_impl.h"
#include "msd_vrs_impl.h"
#include "msd_sbs_impl.h"

struct msd_pos {
    int device = 0;
    hipStream_t stream = nullptr;
    msd_pos_table tab[2] = {}; /* tab[cur] is live; expiry rebuilds into the other */
    int cur = 0;
    uint32_t nrx = 0;
    int fp = 8;
    uint64_t live = 0;
    msd_pos_receiver *d_rx = nullptr;
    unsigned long long *d_stats = nullptr;
    uint32_t *d_ctl = nullptr;
    /* per-call buffers, grown to the largest call seen */
    size_t cap_n = 0, cap_in = 0;
    uint32_t *d_slot = nullptr;
    uint8_t *d_fresh = nullptr;
    msd_position *d_out = nullptr;
    /* a table tracker (msd_pos_create_table): tab[k].trk, the per-record NIC / Rc and the snapshot's buffers */
    bool table = false;
    msd_pos_nicrc *d_nicrc = nullptr;
    uint32_t *s_idx[2] = {nullptr, nullptr}, *s_hist = nullptr;
    msd_aircraft *d_snap = nullptr;
    size_t cap_snap = 0;
    uint32_t *d_idx[2] = {nullptr, nullptr}, *d_hist = nullptr;
    msd_message *d_msgs = nullptr;
    msd_fields *d_fields = nullptr;
    uint32_t *d_receiver = nullptr;
    /* Mode A/C matching (msd_pos_modeac_enable): tab[k].hits, the receivers' arrays, modeCToATable and the buffers the
     * two read-out calls hand to the host */
    uint32_t *d_ac = nullptr;
    uint16_t *d_c_to_a = nullptr;
    msd_modeac_code *d_codes = nullptr;
    msd_modeac_hit *d_hits_out = nullptr;
    size_t cap_hits_out = 0;
    /* reduced Beast output (msd_pos_reduce_enable): tab[k].next_reduce, the verdict byte per record of a call, and the
     * writer's buffers -- records and verdicts that came from the host, lengths, offsets, ends, the stream */
    bool reduce = false;
    uint32_t reduce_interval = 0;
    uint8_t *d_forward = nullptr;
    size_t cap_forward = 0, cap_w = 0, cap_w_in = 0, cap_w_out = 0;
    msd_message *d_w_msgs = nullptr;
    uint8_t *d_w_forward = nullptr, *d_w_lens = nullptr, *d_w_out = nullptr;
    uint32_t *d_w_block = nullptr, *d_w_ends = nullptr;
    /* SBS output (msd_pos_sbs_enable): the ground-track table, the row per record of a call, and the writer's buffers --
     * records, fields and rows that came from the host; lengths, offsets, ends and the stream are the reduced writer's */
    uint16_t *d_track_table = nullptr;
    msd_sbs_track *d_sbs = nullptr, *d_s_trk = nullptr;
    size_t cap_sbs = 0, cap_s_in = 0;
    msd_message *d_s_msgs = nullptr;
    msd_fields *d_s_fields = nullptr;
    /* aircraft.pb (msd_pos_pb_enable): the written state beside tab[k], the truncating ground-track table, and the
     * writer's buffers -- per receiver (made with the state), per item (grown to the largest call seen); the stream is the
     * reduced writer's */
    uint64_t *pb_state[2] = {nullptr, nullptr};
    uint16_t *d_pb_table = nullptr;
    uint32_t *d_pb_first = nullptr;
    uint64_t *d_pb_total = nullptr;
    msd_pb_receiver *d_pb_rx = nullptr;
    size_t cap_pb = 0;
    uint32_t *d_pb_items = nullptr, *d_pb_within = nullptr, *d_pb_cwithin = nullptr, *d_pb_block = nullptr;
    uint64_t *d_pb_shadow = nullptr;
    uint16_t *d_pb_lens = nullptr;
    /* the truncating ground-track table aircraft.pb and the VRS output share: built by whichever of msd_pos_pb_enable and
     * msd_pos_vrs_enable comes first, owned here; d_pb_table is the same pointer once pb is enabled */
    uint16_t *d_trunc_table = nullptr;
    /* VRS output (msd_pos_vrs_enable): the writer's buffers -- per receiver (made at the enable), per item (grown to the
     * largest call seen); the stream is the reduced writer's */
    bool vrs = false;
    uint32_t *d_vrs_first = nullptr;
    msd_vrs_receiver *d_vrs_rx = nullptr;
    size_t cap_vrs = 0;
    uint32_t *d_vrs_items = nullptr, *d_vrs_within = nullptr, *d_vrs_sel = nullptr, *d_vrs_block = nullptr;
    uint16_t *d_vrs_lens = nullptr, *d_vrs_swithin = nullptr;
    char err[256] = "";
};

namespace {

int fail(msd_pos *p, int code, const char *what, hipError_t e)
{
    snprintf(p->err, sizeof p->err, "%s: %s", what, hipGetErrorString(e));
    return code;
}

#define POS_HIP(p, call)                                                                                              \
    do {                                                                                                              \
        const hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess)                                                                                         \
            return fail(p, e_ == hipErrorOutOfMemory ? -ENOMEM : -EIO, #call, e_);                                    \
    } while (0)

int clear(msd_pos *p)
{
    unsigned long long init[MSD_POS_DSTATS] = {};
    const double inf = INFINITY;
    memcpy(&init[MSD_PC_N], &inf, sizeof inf);
    msd_pos_launch_fill(p->stream, p->tab[p->cur].keys, p->tab[p->cur].cap);
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(p->d_stats, init, sizeof init, hipMemcpyHostToDevice, p->stream));
    if (p->d_ac) {
        POS_HIP(p, hipMemsetAsync(p->d_ac, 0, sizeof(uint32_t) * MSD_MODEAC_WORDS * p->nrx, p->stream));
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hipMemsetAsync(p->tab[k].hits, 0, 2u * (size_t)p->tab[k].cap, p->stream));
    }
    if (p->reduce)
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hipMemsetAsync(p->tab[k].next_reduce, 0, sizeof(uint64_t) * MSD_REDUCE_TIMERS * p->tab[k].cap, p->stream));
    if (p->d_pb_table)
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hipMemsetAsync(p->pb_state[k], 0, sizeof(uint64_t) * p->tab[k].cap, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    p->live = 0;
    return 0;
}

template <typename T> void release(T *&ptr)
{
    if (ptr)
        (void)hipFree(ptr);
    ptr = nullptr;
}

/* room for a call of n records (and for its inputs, when they come from the host) */
int reserve(msd_pos *p, size_t n, bool host_input, bool want_sbs)
{
    if (n > p->cap_n) {
        release(p->d_slot), release(p->d_fresh), release(p->d_out), release(p->d_idx[0]), release(p->d_idx[1]), release(p->d_hist);
        release(p->d_nicrc);
        p->cap_n = 0;
        const size_t piece = n < MSD_POS_PIECE ? n : MSD_POS_PIECE;
        const size_t tiles = (piece + MSD_POS_TILE - 1) / MSD_POS_TILE;
        POS_HIP(p, hipMalloc(&p->d_slot, n * sizeof(uint32_t)));
        POS_HIP(p, hipMalloc(&p->d_fresh, n));
        POS_HIP(p, hipMalloc(&p->d_out, n * sizeof(msd_position)));
        POS_HIP(p, hipMalloc(&p->d_idx[0], piece * sizeof(uint32_t)));
        POS_HIP(p, hipMalloc(&p->d_idx[1], piece * sizeof(uint32_t)));
        POS_HIP(p, hipMalloc(&p->d_hist, 256 * tiles * sizeof(uint32_t)));
        if (p->table)
            POS_HIP(p, hipMalloc(&p->d_nicrc, n * sizeof(msd_pos_nicrc)));
        p->cap_n = n;
    }
    if (p->reduce && n > p->cap_forward) {
        release(p->d_forward);
        p->cap_forward = 0;
        POS_HIP(p, hipMalloc(&p->d_forward, n));
        p->cap_forward = n;
    }
    if (want_sbs && n > p->cap_sbs) {
        release(p->d_sbs);
        p->cap_sbs = 0;
        POS_HIP(p, hipMalloc(&p->d_sbs, n * sizeof(msd_sbs_track)));
        p->cap_sbs = n;
    }
    if (host_input && n > p->cap_in) {
        release(p->d_msgs), release(p->d_fields), release(p->d_receiver);
        p->cap_in = 0;
        POS_HIP(p, hipMalloc(&p->d_msgs, n * sizeof(msd_message)));
        POS_HIP(p, hipMalloc(&p->d_fields, n * sizeof(msd_fields)));
        POS_HIP(p, hipMalloc(&p->d_receiver, n * sizeof(uint32_t)));
        p->cap_in = n;
    }
    return 0;
}


/* the index and histogram buffers of the snapshot's ordering passes, made at the first use */
int snapshot_buffers(msd_pos *p)
{
    if (p->s_hist)
        return 0;
    const size_t cap = p->tab[p->cur].cap, tiles = (cap + MSD_POS_TILE - 1) / MSD_POS_TILE;
    POS_HIP(p, hipMalloc(&p->s_idx[0], cap * sizeof(uint32_t)));
    POS_HIP(p, hipMalloc(&p->s_idx[1], cap * sizeof(uint32_t)));
    POS_HIP(p, hipMalloc(&p->s_hist, 256 * tiles * sizeof(uint32_t)));
    return 0;
}

/* the key is receiver << 25 | address: the passes above the highest receiver index's top bit have nothing to order */
uint32_t snapshot_key_bits(const msd_pos *p)
{
    uint32_t key_bits = 25;
    while (key_bits < 64 && ((uint64_t)(p->nrx - 1u) >> (key_bits - 25)) != 0)
        ++key_bits;
    return key_bits;
}

int create(const msd_pos_config *cfg, msd_pos **out, bool table)
{
    if (!out || !msd_pos_config_ok(cfg))
        return -EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev)
        return -ENODEV;
    msd_pos *p = new (std::nothrow) msd_pos;
    if (!p)
        return -ENOMEM;
    p->device = cfg->device;
    p->table = table;
    p->nrx = cfg->receivers;
    p->fp = cfg->filter_persistence ? cfg->filter_persistence : 8;
    std::vector<msd_pos_receiver> rx(p->nrx);
    memset(rx.data(), 0, rx.size() * sizeof(msd_pos_receiver));
    if (cfg->receiver)
        memcpy(rx.data(), cfg->receiver, rx.size() * sizeof(msd_pos_receiver));
    const auto build = [&]() -> int {
        POS_HIP(p, hipSetDevice(p->device));
        POS_HIP(p, hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            p->tab[k].cap = cfg->capacity;
            POS_HIP(p, hipMalloc(&p->tab[k].keys, sizeof(uint64_t) * cfg->capacity));
            POS_HIP(p, hipMalloc(&p->tab[k].st, sizeof(msd_pos_aircraft) * cfg->capacity));
            if (table)
                POS_HIP(p, hipMalloc(&p->tab[k].trk, sizeof(msd_trk_aircraft) * cfg->capacity));
        }
        POS_HIP(p, hipMalloc(&p->d_rx, sizeof(msd_pos_receiver) * p->nrx));
        POS_HIP(p, hipMalloc(&p->d_stats, sizeof(unsigned long long) * MSD_POS_DSTATS));
        POS_HIP(p, hipMalloc(&p->d_ctl, sizeof(uint32_t) * MSD_POS_CTL_N));
        POS_HIP(p, hipMemcpy(p->d_rx, rx.data(), sizeof(msd_pos_receiver) * p->nrx, hipMemcpyHostToDevice));
        return clear(p);
    };
    const int rc = build();
    if (rc) {
        msd_pos_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

} // namespace

extern "C" {

int msd_pos_create(const msd_pos_config *cfg, msd_pos **out)
{
    return create(cfg, out, false);
}

int msd_pos_create_table(const msd_pos_config *cfg, msd_pos **out)
{
    return create(cfg, out, true);
}

void msd_pos_destroy(msd_pos *p)
{
    if (!p)
        return;
    (void)hipSetDevice(p->device);
    if (p->stream)
        (void)hipStreamSynchronize(p->stream);
    for (int k = 0; k < 2; ++k)
        release(p->tab[k].keys), release(p->tab[k].st), release(p->tab[k].trk), release(p->tab[k].hits),
            release(p->tab[k].next_reduce);
    release(p->d_forward), release(p->d_w_msgs), release(p->d_w_forward), release(p->d_w_lens), release(p->d_w_out);
    release(p->d_w_block), release(p->d_w_ends);
    release(p->d_track_table), release(p->d_sbs), release(p->d_s_trk), release(p->d_s_msgs), release(p->d_s_fields);
    release(p->pb_state[0]), release(p->pb_state[1]), release(p->d_trunc_table), release(p->d_pb_first), release(p->d_pb_total);
    release(p->d_pb_rx), release(p->d_pb_items), release(p->d_pb_within), release(p->d_pb_cwithin), release(p->d_pb_block);
    release(p->d_pb_shadow), release(p->d_pb_lens);
    release(p->d_vrs_first), release(p->d_vrs_rx), release(p->d_vrs_items), release(p->d_vrs_within), release(p->d_vrs_sel);
    release(p->d_vrs_block), release(p->d_vrs_lens), release(p->d_vrs_swithin);
    release(p->d_ac), release(p->d_c_to_a), release(p->d_codes), release(p->d_hits_out);
    release(p->d_nicrc), release(p->s_idx[0]), release(p->s_idx[1]), release(p->s_hist), release(p->d_snap);
    release(p->d_rx), release(p->d_stats), release(p->d_ctl), release(p->d_slot), release(p->d_fresh), release(p->d_out);
    release(p->d_idx[0]), release(p->d_idx[1]), release(p->d_hist), release(p->d_msgs), release(p->d_fields),
        release(p->d_receiver);
    if (p->stream)
        (void)hipStreamDestroy(p->stream);
    delete p;
}

const char *msd_pos_last_error(const msd_pos *p)
{
    return p ? p->err : "no tracker";
}

int msd_pos_reset(msd_pos *p)
{
    if (!p)
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    return clear(p);
}

int msd_pos_set_receiver(msd_pos *p, uint32_t receiver, const msd_pos_receiver *rx)
{
    if (!p || receiver >= p->nrx)
        return -EINVAL;
    msd_pos_receiver r;
    memset(&r, 0, sizeof r);
    if (rx)
        r = *rx;
    POS_HIP(p, hipSetDevice(p->device));
    POS_HIP(p, hipMemcpy(p->d_rx + receiver, &r, sizeof r, hipMemcpyHostToDevice));
    return 0;
}

static int update(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, size_t n,
                  int on_device, msd_position *out, msd_pos_nicrc *nicrc, bool want_nicrc, uint8_t *forward, bool want_forward,
                  msd_sbs_track *trk = nullptr, bool want_sbs = false)
{
    if (!p || (want_nicrc && !p->table) || (want_forward && !p->reduce) || (want_sbs && !p->d_track_table))
        return -EINVAL;
    if (n == 0)
        return 0;
    if (!msgs || !fields || !out || (want_nicrc && !nicrc) || (want_forward && !forward) || (want_sbs && !trk) ||
        n > MSD_POS_MAX_N)
        return -EINVAL;
    if (!on_device && receiver)
        for (size_t i = 0; i < n; ++i)
            if (receiver[i] >= p->nrx)
                return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    const int rc = reserve(p, n, !on_device, want_sbs);
    if (rc)
        return rc;
    if (!on_device) {
        POS_HIP(p, hipMemcpyAsync(p->d_msgs, msgs, n * sizeof(msd_message), hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipMemcpyAsync(p->d_fields, fields, n * sizeof(msd_fields), hipMemcpyHostToDevice, p->stream));
        if (receiver)
            POS_HIP(p, hipMemcpyAsync(p->d_receiver, receiver, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
        msgs = p->d_msgs;
        fields = p->d_fields;
        receiver = receiver ? p->d_receiver : nullptr;
    }
    const msd_pos_table t = p->tab[p->cur];
    uint32_t ctl[MSD_POS_CTL_N] = {};
    POS_HIP(p, hipMemsetAsync(p->d_ctl, 0, sizeof ctl, p->stream));
    msd_pos_launch_find(p->stream, t, msgs, fields, receiver, p->nrx, (uint32_t)n, p->d_slot, p->d_fresh, p->d_out, p->d_ctl);
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(ctl, p->d_ctl, sizeof ctl, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    if (ctl[MSD_POS_CTL_FULL] || ctl[MSD_POS_CTL_BAD_RECEIVER]) { /* nothing changes: this call's aircraft leave again */
        msd_pos_launch_rollback(p->stream, t, p->d_slot, p->d_fresh, (uint32_t)n);
        POS_HIP(p, hipGetLastError());
        POS_HIP(p, hipStreamSynchronize(p->stream));
        snprintf(p->err, sizeof p->err, "%s", ctl[MSD_POS_CTL_BAD_RECEIVER] ? "a receiver index is out of range"
                                                                           : "the aircraft table is full");
        return ctl[MSD_POS_CTL_BAD_RECEIVER] ? -EINVAL : -ENOSPC;
    }
    p->live += ctl[MSD_POS_CTL_INSERTED];
    if (p->d_pb_table && ctl[MSD_POS_CTL_INSERTED]) { /* the new aircraft have been written nowhere yet */
        msd_pb_launch_fresh(p->stream, p->d_slot, p->d_fresh, (uint32_t)n, t.cap, p->pb_state[p->cur]);
        POS_HIP(p, hipGetLastError());
    }
    if (p->d_ac) { /* the call has passed its checks: its Mode A/C replies count (track.c:1001) */
        msd_pos_launch_modeac_count(p->stream, msgs, fields, receiver, p->nrx, (uint32_t)n, p->d_ac);
        POS_HIP(p, hipGetLastError());
    }
    if (p->table) /* a skipped record's entry stays zero */
        POS_HIP(p, hipMemsetAsync(p->d_nicrc, 0, n * sizeof(msd_pos_nicrc), p->stream));
    if (p->reduce) /* and its verdict */
        POS_HIP(p, hipMemsetAsync(p->d_forward, 0, n, p->stream));
    if (want_sbs) /* and its row; no other call makes rows */
        POS_HIP(p, hipMemsetAsync(p->d_sbs, 0, n * sizeof(msd_sbs_track), p->stream));
    for (size_t base = 0; base < n; base += MSD_POS_PIECE) {
        const size_t m = n - base < MSD_POS_PIECE ? n - base : MSD_POS_PIECE;
        msd_pos_launch_piece(p->stream, t, msgs, fields, receiver, p->d_rx, p->fp, (uint32_t)base, (uint32_t)m, p->d_slot,
                             p->d_idx[0], p->d_idx[1], p->d_hist, p->d_out, p->d_stats, p->d_nicrc, p->reduce_interval,
                             p->d_forward, want_sbs ? p->d_sbs : nullptr);
        POS_HIP(p, hipGetLastError());
    }
    POS_HIP(p, hipMemcpyAsync(out, p->d_out, n * sizeof(msd_position), hipMemcpyDeviceToHost, p->stream));
    if (want_nicrc)
        POS_HIP(p, hipMemcpyAsync(nicrc, p->d_nicrc, n * sizeof(msd_pos_nicrc), hipMemcpyDeviceToHost, p->stream));
    if (want_forward)
        POS_HIP(p, hipMemcpyAsync(forward, p->d_forward, n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                  p->stream));
    if (want_sbs)
        POS_HIP(p, hipMemcpyAsync(trk, p->d_sbs, n * sizeof(msd_sbs_track),
                                  on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_update(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, size_t n,
                   int on_device, msd_position *out)
{
    return update(p, msgs, fields, receiver, n, on_device, out, nullptr, false, nullptr, false);
}

int msd_pos_update_nicrc(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, size_t n,
                         int on_device, msd_position *out, msd_pos_nicrc *nicrc)
{
    return update(p, msgs, fields, receiver, n, on_device, out, nicrc, true, nullptr, false);
}

int msd_pos_update_reduce(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, size_t n,
                          int on_device, msd_position *out, msd_pos_nicrc *nicrc, uint8_t *forward)
{
    return update(p, msgs, fields, receiver, n, on_device, out, nicrc, nicrc != nullptr, forward, true);
}

int msd_pos_update_sbs(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, size_t n,
                       int on_device, msd_position *out, msd_pos_nicrc *nicrc, uint8_t *forward, msd_sbs_track *trk)
{
    return update(p, msgs, fields, receiver, n, on_device, out, nicrc, nicrc != nullptr, forward, forward != nullptr, trk, true);
}

int msd_pos_sbs_enable(msd_pos *p)
{
    if (!p || !p->table)
        return -EINVAL;
    if (p->d_track_table)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    std::vector<uint16_t> table;
    try {
        table.resize(MSD_SBS_TRACK_ENTRIES);
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    msd_sbs_build_track_table(table.data());
    uint16_t *d_table = nullptr;
    const auto build = [&]() -> int {
        POS_HIP(p, hipMalloc(&d_table, sizeof(uint16_t) * MSD_SBS_TRACK_ENTRIES));
        POS_HIP(p, hipMemcpyAsync(d_table, table.data(), sizeof(uint16_t) * MSD_SBS_TRACK_ENTRIES, hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was */
        (void)hipGetLastError();
        release(d_table);
        return rc;
    }
    p->d_track_table = d_table; /* the rows' buffer grows with the calls, as the verdicts' does */
    return 0;
}

int msd_pos_sbs_wire(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk, size_t n,
                     int on_device, const msd_sbs_options *opt, uint8_t *out, size_t cap, size_t *out_len, uint32_t *ends)
{
    if (!p || !p->d_track_table || !out_len || !msd_sbs_options_ok(opt) || n > MSD_POS_MAX_N)
        return -EINVAL;
    *out_len = 0;
    if (n == 0)
        return 0;
    if (!msgs || !fields || !trk || (!out && cap > 0))
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    const uint32_t nblocks = (uint32_t)((n + 255u) / 256u);
    if (n > p->cap_w) {
        release(p->d_w_lens), release(p->d_w_block), release(p->d_w_ends);
        p->cap_w = 0;
        POS_HIP(p, hipMalloc(&p->d_w_lens, n));
        POS_HIP(p, hipMalloc(&p->d_w_block, sizeof(uint32_t) * (nblocks + 1u)));
        POS_HIP(p, hipMalloc(&p->d_w_ends, sizeof(uint32_t) * n));
        p->cap_w = n;
    }
    if (!on_device) {
        if (n > p->cap_s_in) {
            release(p->d_s_msgs), release(p->d_s_fields), release(p->d_s_trk);
            p->cap_s_in = 0;
            POS_HIP(p, hipMalloc(&p->d_s_msgs, n * sizeof(msd_message)));
            POS_HIP(p, hipMalloc(&p->d_s_fields, n * sizeof(msd_fields)));
            POS_HIP(p, hipMalloc(&p->d_s_trk, n * sizeof(msd_sbs_track)));
            p->cap_s_in = n;
        }
        POS_HIP(p, hipMemcpyAsync(p->d_s_msgs, msgs, n * sizeof(msd_message), hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipMemcpyAsync(p->d_s_fields, fields, n * sizeof(msd_fields), hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipMemcpyAsync(p->d_s_trk, trk, n * sizeof(msd_sbs_track), hipMemcpyHostToDevice, p->stream));
        msgs = p->d_s_msgs;
        fields = p->d_s_fields;
        trk = p->d_s_trk;
    }
    msd_sbs_launch_lengths(p->stream, msgs, fields, trk, (uint32_t)n, *opt, p->d_track_table, p->d_w_lens, p->d_w_block);
    POS_HIP(p, hipGetLastError());
    uint32_t need = 0; /* at most 2^24 * 147 */
    POS_HIP(p, hipMemcpyAsync(&need, p->d_w_block + nblocks, sizeof need, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    *out_len = need;
    if (need > cap) {
        snprintf(p->err, sizeof p->err, "the SBS stream takes %u bytes, %zu were offered", need, cap);
        return -ENOSPC;
    }
    if (need > p->cap_w_out) {
        release(p->d_w_out);
        p->cap_w_out = 0;
        POS_HIP(p, hipMalloc(&p->d_w_out, need));
        p->cap_w_out = need;
    }
    /* (with need == 0 the store kernel still runs: it writes the ends and no byte of the stream) */
    msd_sbs_launch_store(p->stream, msgs, fields, trk, (uint32_t)n, *opt, p->d_track_table, p->d_w_lens, p->d_w_block, p->d_w_out,
                         p->d_w_ends);
    POS_HIP(p, hipGetLastError());
    if (need)
        POS_HIP(p, hipMemcpyAsync(out, p->d_w_out, need, hipMemcpyDeviceToHost, p->stream));
    if (ends)
        POS_HIP(p, hipMemcpyAsync(ends, p->d_w_ends, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

namespace {

/* the truncating ground-track table on the device, built once for aircraft.pb and the VRS output */
int trunc_table(msd_pos *p)
{
    if (p->d_trunc_table)
        return 0;
    std::vector<uint16_t> table;
    try {
        table.resize(MSD_PB_TRACK_ENTRIES);
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    msd_pb_build_track_table(table.data());
    uint16_t *d_table = nullptr;
    const auto build = [&]() -> int {
        POS_HIP(p, hipMalloc(&d_table, sizeof(uint16_t) * MSD_PB_TRACK_ENTRIES));
        POS_HIP(p, hipMemcpyAsync(d_table, table.data(), sizeof(uint16_t) * MSD_PB_TRACK_ENTRIES, hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = build();
    if (rc) {
        (void)hipGetLastError();
        release(d_table);
        return rc;
    }
    p->d_trunc_table = d_table;
    return 0;
}

} // namespace

int msd_pos_pb_enable(msd_pos *p)
{
    if (!p || !p->table)
        return -EINVAL;
    if (p->d_pb_table)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    const bool had_table = p->d_trunc_table != nullptr;
    const int made = trunc_table(p);
    if (made)
        return made;
    uint64_t *state[2] = {nullptr, nullptr}, *total = nullptr;
    uint32_t *first = nullptr;
    msd_pb_receiver *rx = nullptr;
    const auto build = [&]() -> int {
        for (int k = 0; k < 2; ++k) { /* the aircraft the table already has have been written nowhere yet */
            POS_HIP(p, hipMalloc(&state[k], sizeof(uint64_t) * p->tab[k].cap));
            POS_HIP(p, hipMemsetAsync(state[k], 0, sizeof(uint64_t) * p->tab[k].cap, p->stream));
        }
        POS_HIP(p, hipMalloc(&first, sizeof(uint32_t) * ((size_t)p->nrx + 1u)));
        POS_HIP(p, hipMalloc(&total, sizeof(uint64_t) * p->nrx));
        POS_HIP(p, hipMalloc(&rx, sizeof(msd_pb_receiver) * p->nrx));
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return snapshot_buffers(p);
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was (the snapshot's buffers, if they were made, are the snapshot's) */
        (void)hipGetLastError();
        release(state[0]), release(state[1]), release(first), release(total), release(rx);
        if (!had_table)
            release(p->d_trunc_table);
        return rc;
    }
    p->pb_state[0] = state[0];
    p->pb_state[1] = state[1];
    p->d_pb_first = first;
    p->d_pb_total = total;
    p->d_pb_rx = rx;
    p->d_pb_table = p->d_trunc_table;
    return 0;
}

int msd_pos_vrs_enable(msd_pos *p)
{
    if (!p || !p->table)
        return -EINVAL;
    if (p->vrs)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    const bool had_table = p->d_trunc_table != nullptr;
    const int made = trunc_table(p);
    if (made)
        return made;
    uint32_t *first = nullptr;
    msd_vrs_receiver *rx = nullptr;
    const auto build = [&]() -> int {
        POS_HIP(p, hipMalloc(&first, sizeof(uint32_t) * ((size_t)p->nrx + 1u)));
        POS_HIP(p, hipMalloc(&rx, sizeof(msd_vrs_receiver) * p->nrx));
        return snapshot_buffers(p);
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was (the snapshot's buffers, if they were made, are the snapshot's) */
        (void)hipGetLastError();
        release(first), release(rx);
        if (!had_table)
            release(p->d_trunc_table);
        return rc;
    }
    p->d_vrs_first = first;
    p->d_vrs_rx = rx;
    p->vrs = true;
    return 0;
}

int msd_pos_vrs(msd_pos *p, const msd_vrs_options *opt, uint8_t *out, size_t cap, size_t *out_len, msd_vrs_receiver *rx)
{
    const int shift = msd_vrs_part_shift(opt);
    if (!p || !p->vrs || !out_len || shift < 0 || (!out && cap > 0))
        return -EINVAL;
    *out_len = 0;
    if (p->live * MSD_VRS_AIRCRAFT_MAX + (uint64_t)p->nrx * (MSD_VRS_HEAD_LEN + MSD_VRS_TAIL_LEN) > 0xFFFFFFFFull) {
        snprintf(p->err, sizeof p->err, "%llu aircraft could take more than 2^32 - 1 bytes", (unsigned long long)p->live);
        return -E2BIG;
    }
    POS_HIP(p, hipSetDevice(p->device));
    const msd_pos_table t = p->tab[p->cur];
    const uint32_t live = (uint32_t)p->live;
    const size_t nitems = (size_t)live + 2u * (size_t)p->nrx;
    const uint32_t nblocks = (uint32_t)((nitems + 255u) / 256u);
    if (nitems > p->cap_vrs) {
        release(p->d_vrs_items), release(p->d_vrs_within), release(p->d_vrs_sel), release(p->d_vrs_block);
        release(p->d_vrs_lens), release(p->d_vrs_swithin);
        p->cap_vrs = 0;
        POS_HIP(p, hipMalloc(&p->d_vrs_items, sizeof(uint32_t) * nitems));
        POS_HIP(p, hipMalloc(&p->d_vrs_within, sizeof(uint32_t) * nitems));
        POS_HIP(p, hipMalloc(&p->d_vrs_sel, sizeof(uint32_t) * ((size_t)nblocks + 1u)));
        POS_HIP(p, hipMalloc(&p->d_vrs_block, sizeof(uint32_t) * ((size_t)nblocks + 1u)));
        POS_HIP(p, hipMalloc(&p->d_vrs_lens, sizeof(uint16_t) * nitems));
        POS_HIP(p, hipMalloc(&p->d_vrs_swithin, sizeof(uint16_t) * nitems));
        p->cap_vrs = nitems;
    }
    const uint32_t *idx = p->s_idx[0]; /* (not read without aircraft) */
    if (live)
        idx = msd_pos_launch_ordered_slots(p->stream, t, live, snapshot_key_bits(p), p->s_idx[0], p->s_idx[1], p->s_hist);
    const msd_vrs_call c = {t, idx, p->d_vrs_items, p->d_vrs_first, p->d_trunc_table, opt->now_ms, (uint32_t)nitems, p->nrx,
                            opt->part, (uint32_t)shift};
    msd_vrs_launch_lengths(p->stream, c, live, p->d_vrs_first, p->d_vrs_items, p->d_vrs_lens, p->d_vrs_swithin, p->d_vrs_within,
                           p->d_vrs_sel, p->d_vrs_block, p->d_vrs_rx);
    POS_HIP(p, hipGetLastError());
    uint32_t need = 0;
    POS_HIP(p, hipMemcpyAsync(&need, p->d_vrs_block + nblocks, sizeof need, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    *out_len = need;
    if (need > cap) {
        snprintf(p->err, sizeof p->err, "the VRS stream takes %u bytes, %zu were offered", need, cap);
        return -ENOSPC;
    }
    if (need > p->cap_w_out) {
        release(p->d_w_out);
        p->cap_w_out = 0;
        POS_HIP(p, hipMalloc(&p->d_w_out, need));
        p->cap_w_out = need;
    }
    msd_vrs_launch_store(p->stream, c, p->d_vrs_lens, p->d_vrs_block, p->d_w_out); /* (need >= 14: a receiver's frame) */
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(out, p->d_w_out, need, hipMemcpyDeviceToHost, p->stream));
    if (rx)
        POS_HIP(p, hipMemcpyAsync(rx, p->d_vrs_rx, sizeof(msd_vrs_receiver) * p->nrx, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_aircraft_pb(msd_pos *p, const msd_pb_options *opt, uint8_t *out, size_t cap, size_t *out_len, msd_pb_receiver *rx)
{
    if (!p || !p->d_pb_table || !out_len || !msd_pb_options_ok(opt) || (!out && cap > 0))
        return -EINVAL;
    *out_len = 0;
    if (p->live * MSD_PB_AIRCRAFT_MAX + (uint64_t)p->nrx * MSD_PB_HEADER_MAX > 0xFFFFFFFFull) {
        snprintf(p->err, sizeof p->err, "%llu aircraft could take more than 2^32 - 1 bytes", (unsigned long long)p->live);
        return -E2BIG;
    }
    POS_HIP(p, hipSetDevice(p->device));
    const msd_pos_table t = p->tab[p->cur];
    const uint32_t live = (uint32_t)p->live;
    const size_t nitems = (size_t)live + p->nrx;
    const uint32_t nblocks = (uint32_t)((nitems + 255u) / 256u);
    if (nitems > p->cap_pb) {
        release(p->d_pb_items), release(p->d_pb_within), release(p->d_pb_cwithin), release(p->d_pb_block);
        release(p->d_pb_shadow), release(p->d_pb_lens);
        p->cap_pb = 0;
        POS_HIP(p, hipMalloc(&p->d_pb_items, sizeof(uint32_t) * nitems));
        POS_HIP(p, hipMalloc(&p->d_pb_within, sizeof(uint32_t) * nitems));
        POS_HIP(p, hipMalloc(&p->d_pb_cwithin, sizeof(uint32_t) * nitems));
        POS_HIP(p, hipMalloc(&p->d_pb_block, sizeof(uint32_t) * 4u * ((size_t)nblocks + 1u)));
        POS_HIP(p, hipMalloc(&p->d_pb_shadow, sizeof(uint64_t) * nitems));
        POS_HIP(p, hipMalloc(&p->d_pb_lens, sizeof(uint16_t) * nitems));
        p->cap_pb = nitems;
    }
    const uint64_t *d_total = nullptr;
    if (opt->messages_total) {
        POS_HIP(p, hipMemcpyAsync(p->d_pb_total, opt->messages_total, sizeof(uint64_t) * p->nrx, hipMemcpyHostToDevice, p->stream));
        d_total = p->d_pb_total;
    }
    const uint32_t *idx = p->s_idx[0]; /* (not read without aircraft) */
    if (live)
        idx = msd_pos_launch_ordered_slots(p->stream, t, live, snapshot_key_bits(p), p->s_idx[0], p->s_idx[1], p->s_hist);
    msd_pb_launch_lengths(p->stream, t, p->pb_state[p->cur], idx, live, p->nrx, opt->now_ms, d_total, p->d_pb_table,
                          p->d_pb_first, p->d_pb_items, p->d_pb_shadow, p->d_pb_lens, p->d_pb_within, p->d_pb_cwithin,
                          p->d_pb_block, p->d_pb_rx);
    POS_HIP(p, hipGetLastError());
    uint32_t need = 0;
    POS_HIP(p, hipMemcpyAsync(&need, p->d_pb_block + nblocks, sizeof need, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    *out_len = need;
    if (need > cap) { /* no written state has moved: only the store kernel commits the shadow copy */
        snprintf(p->err, sizeof p->err, "the aircraft.pb stream takes %u bytes, %zu were offered", need, cap);
        return -ENOSPC;
    }
    if (need > p->cap_w_out) {
        release(p->d_w_out);
        p->cap_w_out = 0;
        POS_HIP(p, hipMalloc(&p->d_w_out, need));
        p->cap_w_out = need;
    }
    if (need) { /* (no byte: no aircraft was written, so no state moves either) */
        msd_pb_launch_store(p->stream, t, p->pb_state[p->cur], idx, live, p->nrx, opt->now_ms, d_total, p->d_pb_table,
                            p->d_pb_items, p->d_pb_shadow, p->d_pb_lens, p->d_pb_block, p->d_w_out);
        POS_HIP(p, hipGetLastError());
        POS_HIP(p, hipMemcpyAsync(out, p->d_w_out, need, hipMemcpyDeviceToHost, p->stream));
    }
    if (rx)
        POS_HIP(p, hipMemcpyAsync(rx, p->d_pb_rx, sizeof(msd_pb_receiver) * p->nrx, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_reduce_enable(msd_pos *p, uint32_t interval_ms)
{
    if (!p || !p->table || interval_ms > MSD_REDUCE_MAX_INTERVAL)
        return -EINVAL;
    if (p->reduce)
        return interval_ms == p->reduce_interval ? 0 : -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    uint64_t *next[2] = {nullptr, nullptr};
    const auto build = [&]() -> int {
        for (int k = 0; k < 2; ++k) { /* the aircraft the table already has start at 0, as a new one does */
            const size_t bytes = sizeof(uint64_t) * MSD_REDUCE_TIMERS * p->tab[k].cap;
            POS_HIP(p, hipMalloc(&next[k], bytes));
            POS_HIP(p, hipMemsetAsync(next[k], 0, bytes, p->stream));
        }
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was */
        (void)hipGetLastError();
        release(next[0]), release(next[1]);
        return rc;
    }
    p->tab[0].next_reduce = next[0];
    p->tab[1].next_reduce = next[1];
    p->reduce_interval = interval_ms;
    p->reduce = true;
    return 0;
}

int msd_pos_reduce_wire(msd_pos *p, const msd_message *msgs, const uint8_t *forward, size_t n, int on_device, uint32_t flags,
                        uint8_t *out, size_t cap, size_t *out_len, uint32_t *ends)
{
    if (!p || !p->reduce || !out_len || (flags & ~(MSD_WIRE_VERBATIM | MSD_REDUCE_NET_ONLY)) || n > MSD_POS_MAX_N)
        return -EINVAL;
    *out_len = 0;
    if (n == 0)
        return 0;
    if (!msgs || !forward || (!out && cap > 0))
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    const uint32_t nblocks = (uint32_t)((n + 255u) / 256u);
    if (n > p->cap_w) {
        release(p->d_w_lens), release(p->d_w_block), release(p->d_w_ends);
        p->cap_w = 0;
        POS_HIP(p, hipMalloc(&p->d_w_lens, n));
        POS_HIP(p, hipMalloc(&p->d_w_block, sizeof(uint32_t) * (nblocks + 1u)));
        POS_HIP(p, hipMalloc(&p->d_w_ends, sizeof(uint32_t) * n));
        p->cap_w = n;
    }
    if (!on_device) {
        if (n > p->cap_w_in) {
            release(p->d_w_msgs), release(p->d_w_forward);
            p->cap_w_in = 0;
            POS_HIP(p, hipMalloc(&p->d_w_msgs, n * sizeof(msd_message)));
            POS_HIP(p, hipMalloc(&p->d_w_forward, n));
            p->cap_w_in = n;
        }
        POS_HIP(p, hipMemcpyAsync(p->d_w_msgs, msgs, n * sizeof(msd_message), hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipMemcpyAsync(p->d_w_forward, forward, n, hipMemcpyHostToDevice, p->stream));
        msgs = p->d_w_msgs;
        forward = p->d_w_forward;
    }
    msd_reduce_launch_lengths(p->stream, msgs, forward, (uint32_t)n, flags, p->d_w_lens, p->d_w_block);
    POS_HIP(p, hipGetLastError());
    uint32_t need = 0; /* at most 2^24 * 44 */
    POS_HIP(p, hipMemcpyAsync(&need, p->d_w_block + nblocks, sizeof need, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    *out_len = need;
    if (need > cap) {
        snprintf(p->err, sizeof p->err, "the reduced stream takes %u bytes, %zu were offered", need, cap);
        return -ENOSPC;
    }
    if (need > p->cap_w_out) {
        release(p->d_w_out);
        p->cap_w_out = 0;
        POS_HIP(p, hipMalloc(&p->d_w_out, need));
        p->cap_w_out = need;
    }
    /* (with need == 0 the store kernel still runs: it writes the ends and no byte of the stream) */
    msd_reduce_launch_store(p->stream, msgs, (uint32_t)n, flags, p->d_w_lens, p->d_w_block, p->d_w_out, p->d_w_ends);
    POS_HIP(p, hipGetLastError());
    if (need)
        POS_HIP(p, hipMemcpyAsync(out, p->d_w_out, need, hipMemcpyDeviceToHost, p->stream));
    if (ends)
        POS_HIP(p, hipMemcpyAsync(ends, p->d_w_ends, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_snapshot(msd_pos *p, msd_aircraft *out, size_t cap, int on_device, size_t *n)
{
    if (!p || !p->table || !n || (!out && cap > 0))
        return -EINVAL;
    *n = (size_t)p->live;
    if (p->live > cap) {
        snprintf(p->err, sizeof p->err, "%llu aircraft do not fit %zu entries", (unsigned long long)p->live, cap);
        return -ENOSPC;
    }
    if (p->live == 0)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    const msd_pos_table t = p->tab[p->cur];
    const int rc = snapshot_buffers(p);
    if (rc)
        return rc;
    if (!on_device && p->live > p->cap_snap) {
        release(p->d_snap);
        p->cap_snap = 0;
        POS_HIP(p, hipMalloc(&p->d_snap, p->live * sizeof(msd_aircraft)));
        p->cap_snap = (size_t)p->live;
    }
    msd_aircraft *dst = on_device ? out : p->d_snap;
    msd_pos_launch_snapshot(p->stream, t, (uint32_t)p->live, snapshot_key_bits(p), p->s_idx[0], p->s_idx[1], p->s_hist, dst);
    POS_HIP(p, hipGetLastError());
    if (!on_device)
        POS_HIP(p, hipMemcpyAsync(out, p->d_snap, p->live * sizeof(msd_aircraft), hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_modeac_enable(msd_pos *p)
{
    if (!p || !p->table)
        return -EINVAL;
    if (p->d_ac)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    uint16_t c_to_a[MSD_MODEAC_CODES];
    msd_modeac_build_c_to_a(c_to_a);
    const size_t ac_bytes = sizeof(uint32_t) * MSD_MODEAC_WORDS * p->nrx;
    uint32_t *ac = nullptr;
    uint16_t *d_c_to_a = nullptr;
    msd_modeac_code *codes = nullptr;
    uint8_t *hits[2] = {nullptr, nullptr};
    const auto build = [&]() -> int {
        POS_HIP(p, hipMalloc(&ac, ac_bytes));
        POS_HIP(p, hipMalloc(&d_c_to_a, sizeof c_to_a));
        POS_HIP(p, hipMalloc(&codes, sizeof(msd_modeac_code) * MSD_MODEAC_CODES));
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hipMalloc(&hits[k], 2u * (size_t)p->tab[k].cap));
        POS_HIP(p, hipMemsetAsync(ac, 0, ac_bytes, p->stream));
        for (int k = 0; k < 2; ++k) /* the aircraft the table has already start without hits */
            POS_HIP(p, hipMemsetAsync(hits[k], 0, 2u * (size_t)p->tab[k].cap, p->stream));
        POS_HIP(p, hipMemcpyAsync(d_c_to_a, c_to_a, sizeof c_to_a, hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was */
        (void)hipGetLastError();
        release(ac), release(d_c_to_a), release(codes), release(hits[0]), release(hits[1]);
        return rc;
    }
    p->d_ac = ac;
    p->d_c_to_a = d_c_to_a;
    p->d_codes = codes;
    p->tab[0].hits = hits[0];
    p->tab[1].hits = hits[1];
    return 0;
}

int msd_pos_modeac_match(msd_pos *p, uint64_t now_ms, uint64_t message_now_ms)
{
    if (!p || !p->d_ac)
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    msd_pos_launch_modeac_match(p->stream, p->tab[p->cur], p->nrx, now_ms, message_now_ms, p->d_c_to_a, p->d_ac);
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_modeac_codes(msd_pos *p, uint32_t receiver, msd_modeac_code *out, int on_device)
{
    if (!p || !p->d_ac || receiver >= p->nrx || !out)
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    msd_modeac_code *dst = on_device ? out : p->d_codes;
    msd_pos_launch_modeac_codes(p->stream, p->d_ac + (size_t)receiver * MSD_MODEAC_WORDS, dst);
    POS_HIP(p, hipGetLastError());
    if (!on_device)
        POS_HIP(p, hipMemcpyAsync(out, p->d_codes, sizeof(msd_modeac_code) * MSD_MODEAC_CODES, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_modeac_hits(msd_pos *p, msd_modeac_hit *out, size_t cap, int on_device, size_t *n)
{
    if (!p || !p->d_ac || !n || (!out && cap > 0))
        return -EINVAL;
    *n = (size_t)p->live;
    if (p->live > cap) {
        snprintf(p->err, sizeof p->err, "%llu aircraft do not fit %zu entries", (unsigned long long)p->live, cap);
        return -ENOSPC;
    }
    if (p->live == 0)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    const int rc = snapshot_buffers(p);
    if (rc)
        return rc;
    if (!on_device && p->live > p->cap_hits_out) {
        release(p->d_hits_out);
        p->cap_hits_out = 0;
        POS_HIP(p, hipMalloc(&p->d_hits_out, p->live * sizeof(msd_modeac_hit)));
        p->cap_hits_out = (size_t)p->live;
    }
    msd_modeac_hit *dst = on_device ? out : p->d_hits_out;
    msd_pos_launch_modeac_hits(p->stream, p->tab[p->cur], (uint32_t)p->live, snapshot_key_bits(p), p->s_idx[0], p->s_idx[1],
                               p->s_hist, dst);
    POS_HIP(p, hipGetLastError());
    if (!on_device)
        POS_HIP(p, hipMemcpyAsync(out, p->d_hits_out, p->live * sizeof(msd_modeac_hit), hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_aircraft_valid(const msd_aircraft *a, int member, uint64_t now_ms)
{
    return a && member >= 0 && member < MSD_AC_N && msd_trk_valid(a, member, now_ms);
}

int msd_pos_expire(msd_pos *p, uint64_t now_ms)
{
    if (!p)
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    uint32_t ctl[MSD_POS_CTL_N] = {};
    POS_HIP(p, hipMemsetAsync(p->d_ctl, 0, sizeof ctl, p->stream));
    msd_pos_launch_expire(p->stream, p->tab[p->cur], now_ms, p->d_ctl);
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(ctl, p->d_ctl, sizeof ctl, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    if (!ctl[MSD_POS_CTL_REMOVED])
        return 0;
    /* linear probing has no holes to leave: the survivors are inserted again into the other, empty table */
    const int other = p->cur ^ 1;
    msd_pos_launch_fill(p->stream, p->tab[other].keys, p->tab[other].cap);
    msd_pos_launch_rebuild(p->stream, p->tab[p->cur], p->tab[other]);
    POS_HIP(p, hipGetLastError());
    if (p->d_pb_table) {
        msd_pb_launch_move(p->stream, p->tab[p->cur], p->pb_state[p->cur], p->tab[other], p->pb_state[other]);
        POS_HIP(p, hipGetLastError());
    }
    POS_HIP(p, hipStreamSynchronize(p->stream));
    p->cur = other;
    p->live -= ctl[MSD_POS_CTL_REMOVED];
    return 0;
}

int msd_pos_get_stats(const msd_pos *p, msd_pos_stats *st)
{
    if (!p || !st)
        return -EINVAL;
    unsigned long long d[MSD_POS_DSTATS];
    if (hipSetDevice(p->device) != hipSuccess ||
        hipMemcpy(d, p->d_stats, sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
        return -EIO;
    memcpy(st, d, sizeof(uint64_t) * MSD_PC_N);
    st->aircraft = p->live;
    memcpy(&st->min_gate_margin_m, &d[MSD_PC_N], sizeof(double));
    return 0;
}

} // extern "C"
