/* msd_pos.cpp -- C-ABI of the position tracker (modes_hip.h "positions"): the object, its device memory (msd_devbuf.h:
 * every buffer is an owning array, freed with the object) and the order in which a call queues the kernels of
 * msd_pos_kernels.hip and of the six writers.  The writers share emit(), host input is staged by stage(), the two
 * read-outs of the table share read_out(). */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <utility>
#include <vector>

#include "msd_pos.h"
#include "msd_devbuf.h"
#include "msd_pb_impl.h"
#include "msd_vrs_impl.h"
#include "msd_history_impl.h"
#include "msd_sbs_impl.h"

template <typename T> using dev = msd_devbuf<T>;

struct msd_pos {
    int device = 0;
    hipStream_t stream = nullptr;
    /* tab[cur] is live; expiry rebuilds into the other.  The kernels take a table by value, so it is raw pointers:
     * point_tables() fills them from the arrays below */
    msd_pos_table tab[2] = {};
    dev<uint64_t> keys[2];
    dev<msd_pos_aircraft> st[2];
    int cur = 0;
    uint32_t nrx = 0;
    int fp = 8;
    uint64_t live = 0;
    dev<msd_pos_receiver> d_rx;
    dev<unsigned long long> d_stats;
    dev<uint32_t> d_ctl;
    /* per-call buffers, grown to the largest call seen */
    dev<uint32_t> d_slot;
    dev<uint8_t> d_fresh;
    dev<msd_position> d_out;
    /* a table tracker (msd_pos_create_table): tab[k].trk, the per-record NIC / Rc and the snapshot's buffers */
    bool table = false;
    dev<msd_trk_aircraft> trk[2];
    dev<msd_pos_nicrc> d_nicrc;
    dev<uint32_t> s_idx[2], s_hist;
    dev<msd_aircraft> d_snap;
    dev<uint32_t> d_idx[2], d_hist;
    dev<msd_message> d_msgs;
    dev<msd_fields> d_fields;
    dev<uint32_t> d_receiver;
    /* Mode A/C matching (msd_pos_modeac_enable): tab[k].hits, the receivers' arrays, modeCToATable and the buffers the
     * two read-out calls hand to the host */
    dev<uint8_t> hits[2];
    dev<uint32_t> d_ac;
    dev<uint16_t> d_c_to_a;
    dev<msd_modeac_code> d_codes;
    dev<msd_modeac_hit> d_hits_out;
    /* reduced Beast output (msd_pos_reduce_enable): tab[k].next_reduce, the verdict byte per record of a call, and the
     * writer's buffers -- records and verdicts that came from the host, lengths, offsets, ends, the stream */
    bool reduce = false;
    uint32_t reduce_interval = 0;
    dev<uint64_t> next_reduce[2];
    dev<uint8_t> d_forward;
    dev<msd_message> d_w_msgs;
    dev<uint8_t> d_w_forward, d_w_lens, d_w_out;
    dev<uint32_t> d_w_block, d_w_ends;
    /* SBS output (msd_pos_sbs_enable): the ground-track table, the row per record of a call, and the writer's buffers --
     * records, fields and rows that came from the host; lengths, offsets, ends and the stream are the reduced writer's */
    dev<uint16_t> d_track_table;
    dev<msd_sbs_track> d_sbs, d_s_trk;
    dev<msd_message> d_s_msgs;
    dev<msd_fields> d_s_fields;
    /* aircraft.pb (msd_pos_pb_enable): the written state beside tab[k], and the writer's buffers -- per receiver (made
     * with the state), per item (grown to the largest call seen); the stream is the reduced writer's */
    bool pb = false;
    dev<uint64_t> pb_state[2];
    dev<uint32_t> d_pb_first;
    dev<uint64_t> d_pb_total;
    dev<msd_pb_receiver> d_pb_rx;
    dev<uint32_t> d_pb_items, d_pb_within, d_pb_cwithin, d_pb_block;
    dev<uint64_t> d_pb_shadow;
    dev<uint16_t> d_pb_lens;
    /* the truncating ground-track table aircraft.pb and the VRS output share: built by whichever of msd_pos_pb_enable and
     * msd_pos_vrs_enable comes first */
    dev<uint16_t> d_trunc_table;
    /* VRS output (msd_pos_vrs_enable): the writer's buffers -- per receiver (made at the enable), per item (grown to the
     * largest call seen); the stream is the reduced writer's */
    bool vrs = false;
    dev<uint32_t> d_vrs_first;
    dev<msd_vrs_receiver> d_vrs_rx;
    dev<uint32_t> d_vrs_items, d_vrs_within, d_vrs_sel, d_vrs_block;
    dev<uint16_t> d_vrs_lens, d_vrs_swithin;
    /* history_N.pb (msd_pos_history_pb; no enable): the writer's buffers, made by the first call -- per receiver, per item
     * (grown to the largest call seen); the stream is the reduced writer's */
    dev<uint32_t> d_hist_first;
    dev<msd_history_receiver> d_hist_rx;
    dev<uint32_t> d_hist_items, d_hist_block;
    dev<uint16_t> d_hist_within, d_hist_cwithin;
    dev<uint8_t> d_hist_lens;
    /* the receiver range (msd_pos_range_enable): tab[k].dist, the receivers' rows, the two margins' bits, the code byte
     * per record of a call, and the buffers the two read-out calls hand to the host */
    bool range = false, range_polar = false, range_combine = true, range_timing = false;
    hipEvent_t range_ev[2] = {nullptr, nullptr}; /* with range_timing: around the range kernel (scripts/range_rate.py) */
    float range_ms = 0;
    dev<uint32_t> dist[2];
    dev<msd_range_state> d_rng;
    dev<unsigned long long> d_rmargins;
    dev<uint8_t> d_rcode;
    dev<msd_range_receiver> d_rng_out;
    dev<uint32_t> d_dist_out;
    dev<unsigned long long> d_rng_end;
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

/* the one place where the tables learn where their arrays are: after the create and after every enable that adds one */
void point_tables(msd_pos *p)
{
    for (int k = 0; k < 2; ++k) {
        p->tab[k].keys = p->keys[k].get();
        p->tab[k].st = p->st[k].get();
        p->tab[k].trk = p->trk[k].get();
        p->tab[k].hits = p->hits[k].get();
        p->tab[k].next_reduce = p->next_reduce[k].get();
        p->tab[k].dist = p->dist[k].get();
    }
}

/* the receiver range as a new tracker has it: no distance, empty rows, no margin */
int range_clear(msd_pos *p, uint32_t *const dist[2], msd_range_state *rng, unsigned long long *margins)
{
    unsigned long long inf[2];
    const double d = INFINITY;
    memcpy(&inf[0], &d, sizeof d);
    inf[1] = inf[0];
    for (int k = 0; k < 2; ++k)
        POS_HIP(p, hipMemsetAsync(dist[k], 0, sizeof(uint32_t) * p->tab[k].cap, p->stream));
    POS_HIP(p, hipMemsetAsync(rng, 0, sizeof(msd_range_state) * p->nrx, p->stream));
    POS_HIP(p, hipMemcpyAsync(margins, inf, sizeof inf, hipMemcpyHostToDevice, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream)); /* inf leaves the stack */
    return 0;
}

int clear(msd_pos *p)
{
    unsigned long long init[MSD_POS_DSTATS] = {};
    const double inf = INFINITY;
    memcpy(&init[MSD_PC_N], &inf, sizeof inf);
    msd_pos_launch_fill(p->stream, p->tab[p->cur].keys, p->tab[p->cur].cap);
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(p->d_stats.get(), init, sizeof init, hipMemcpyHostToDevice, p->stream));
    if (p->d_ac.get()) {
        POS_HIP(p, hipMemsetAsync(p->d_ac.get(), 0, sizeof(uint32_t) * MSD_MODEAC_WORDS * p->nrx, p->stream));
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hipMemsetAsync(p->tab[k].hits, 0, 2u * (size_t)p->tab[k].cap, p->stream));
    }
    if (p->reduce)
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hipMemsetAsync(p->tab[k].next_reduce, 0, sizeof(uint64_t) * MSD_REDUCE_TIMERS * p->tab[k].cap, p->stream));
    if (p->pb)
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hipMemsetAsync(p->pb_state[k].get(), 0, sizeof(uint64_t) * p->tab[k].cap, p->stream));
    if (p->range) {
        uint32_t *const dist[2] = {p->dist[0].get(), p->dist[1].get()};
        const int rc = range_clear(p, dist, p->d_rng.get(), p->d_rmargins.get());
        if (rc)
            return rc;
    }
    POS_HIP(p, hipStreamSynchronize(p->stream));
    p->live = 0;
    return 0;
}

/* room for a call of n records (its inputs, when they come from the host, are stage()'s) */
int reserve(msd_pos *p, size_t n, bool want_sbs)
{
    const size_t piece = n < MSD_POS_PIECE ? n : MSD_POS_PIECE;
    const size_t tiles = (piece + MSD_POS_TILE - 1) / MSD_POS_TILE;
    POS_HIP(p, p->d_slot.reserve(n));
    POS_HIP(p, p->d_fresh.reserve(n));
    POS_HIP(p, p->d_out.reserve(n));
    POS_HIP(p, p->d_idx[0].reserve(piece));
    POS_HIP(p, p->d_idx[1].reserve(piece));
    POS_HIP(p, p->d_hist.reserve(256 * tiles));
    if (p->table)
        POS_HIP(p, p->d_nicrc.reserve(n));
    if (p->reduce)
        POS_HIP(p, p->d_forward.reserve(n));
    if (want_sbs)
        POS_HIP(p, p->d_sbs.reserve(n));
    if (p->range)
        POS_HIP(p, p->d_rcode.reserve(n));
    return 0;
}

/* Host input of a call onto the device: n elements of src into buf, and src points at the copy.  An array the caller
 * left out keeps its room and stays left out. */
template <typename T> int stage(msd_pos *p, dev<T> &buf, const T *&src, size_t n)
{
    POS_HIP(p, buf.reserve(n));
    if (src) {
        POS_HIP(p, hipMemcpyAsync(buf.get(), src, n * sizeof(T), hipMemcpyHostToDevice, p->stream));
        src = buf.get();
    }
    return 0;
}

/* the lengths, the workgroups' offsets and the ends of a call of n records: the reduced writer's and the SBS writer's */
int record_writer_buffers(msd_pos *p, size_t n, uint32_t nblocks)
{
    POS_HIP(p, p->d_w_lens.reserve(n));
    POS_HIP(p, p->d_w_block.reserve(nblocks + 1u));
    POS_HIP(p, p->d_w_ends.reserve(n));
    return 0;
}

/* What every writer does once its lengths are queued: the stream's length (block_sums[nblocks]) comes back and is
 * *out_len from then on, also where the call is refused; a stream that does not fit cap is -ENOSPC and moves nothing;
 * otherwise d_w_out grows to it, store(need) queues the writer's store kernel -- or not: what a writer does with no byte
 * to write is its own and stays at its call --, the bytes go to out and the writer's side array (side_bytes from
 * side_src, where the caller asked for it) to side_dst. */
template <typename Store>
int emit(msd_pos *p, const uint32_t *block_sums, uint32_t nblocks, const char *noun, uint8_t *out, size_t cap, size_t *out_len,
         void *side_dst, const void *side_src, size_t side_bytes, Store store)
{
    uint32_t need = 0;
    POS_HIP(p, hipMemcpyAsync(&need, block_sums + nblocks, sizeof need, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    *out_len = need;
    if (need > cap) {
        snprintf(p->err, sizeof p->err, "the %s stream takes %u bytes, %zu were offered", noun, need, cap);
        return -ENOSPC;
    }
    POS_HIP(p, p->d_w_out.reserve(need));
    store(need);
    POS_HIP(p, hipGetLastError());
    if (need)
        POS_HIP(p, hipMemcpyAsync(out, p->d_w_out.get(), need, hipMemcpyDeviceToHost, p->stream));
    if (side_dst)
        POS_HIP(p, hipMemcpyAsync(side_dst, side_src, side_bytes, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

/* the index and histogram buffers of the snapshot's ordering passes, made at the first use */
int snapshot_buffers(msd_pos *p)
{
    const size_t cap = p->tab[p->cur].cap, tiles = (cap + MSD_POS_TILE - 1) / MSD_POS_TILE;
    POS_HIP(p, p->s_idx[0].reserve(cap));
    POS_HIP(p, p->s_idx[1].reserve(cap));
    POS_HIP(p, p->s_hist.reserve(256 * tiles));
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

/* the live slots in the snapshot's order, for a writer over items (idx is not read without aircraft) */
const uint32_t *ordered_slots(msd_pos *p, uint32_t live)
{
    if (!live)
        return p->s_idx[0].get();
    return msd_pos_launch_ordered_slots(p->stream, p->tab[p->cur], live, snapshot_key_bits(p), p->s_idx[0].get(),
                                        p->s_idx[1].get(), p->s_hist.get());
}

/* A read-out of one entry per live aircraft in the snapshot's order: *n is their number, also where they do not fit cap
 * entries; launch(idx_a, idx_b, hist, dst) queues the ordered gather, into out itself where that is device memory and
 * else into the staging array, which is copied out. */
template <typename T, typename Launch>
int read_out(msd_pos *p, dev<T> &staging, T *out, size_t cap, int on_device, size_t *n, Launch launch)
{
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
    if (!on_device)
        POS_HIP(p, staging.reserve((size_t)p->live));
    launch(p->s_idx[0].get(), p->s_idx[1].get(), p->s_hist.get(), on_device ? out : staging.get());
    POS_HIP(p, hipGetLastError());
    if (!on_device)
        POS_HIP(p, hipMemcpyAsync(out, staging.get(), p->live * sizeof(T), hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

/* A ground-track table on the device, built once: build's `entries` entries into dst.  On an error dst stays empty. */
int track_table(msd_pos *p, dev<uint16_t> &dst, void (*build)(uint16_t *), size_t entries)
{
    if (dst.get())
        return 0;
    std::vector<uint16_t> table;
    try {
        table.resize(entries);
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    build(table.data());
    dev<uint16_t> d_table;
    const auto upload = [&]() -> int {
        POS_HIP(p, d_table.reserve(entries));
        POS_HIP(p, hipMemcpyAsync(d_table.get(), table.data(), sizeof(uint16_t) * entries, hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = upload();
    if (rc) { /* the tracker stays as it was */
        (void)hipGetLastError();
        return rc;
    }
    dst = std::move(d_table);
    return 0;
}

/* What the two enables over the truncating ground-track table have in common: the table, the snapshot's buffers and
 * `mine`, the enable's own arrays.  On an error the tracker stays as it was: the table goes again if this very call made
 * it (the snapshot's buffers, if they were made, are the snapshot's). */
template <typename Mine> int items_writer_enable(msd_pos *p, Mine mine)
{
    const bool had_table = p->d_trunc_table.get() != nullptr;
    const int made = track_table(p, p->d_trunc_table, msd_pb_build_track_table, MSD_PB_TRACK_ENTRIES);
    if (made)
        return made;
    int rc = mine();
    if (!rc)
        rc = snapshot_buffers(p);
    if (rc) {
        (void)hipGetLastError();
        if (!had_table)
            p->d_trunc_table = dev<uint16_t>();
    }
    return rc;
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
            POS_HIP(p, p->keys[k].reserve(cfg->capacity));
            POS_HIP(p, p->st[k].reserve(cfg->capacity));
            if (table)
                POS_HIP(p, p->trk[k].reserve(cfg->capacity));
        }
        point_tables(p);
        POS_HIP(p, p->d_rx.reserve(p->nrx));
        POS_HIP(p, p->d_stats.reserve(MSD_POS_DSTATS));
        POS_HIP(p, p->d_ctl.reserve(MSD_POS_CTL_N));
        POS_HIP(p, hipMemcpy(p->d_rx.get(), rx.data(), sizeof(msd_pos_receiver) * p->nrx, hipMemcpyHostToDevice));
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
    const hipStream_t stream = p->stream;
    if (stream)
        (void)hipStreamSynchronize(stream);
    for (hipEvent_t e : p->range_ev)
        if (e)
            (void)hipEventDestroy(e);
    delete p; /* every buffer, behind the stream's last work and before the stream goes */
    if (stream)
        (void)hipStreamDestroy(stream);
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
    POS_HIP(p, hipMemcpy(p->d_rx.get() + receiver, &r, sizeof r, hipMemcpyHostToDevice));
    return 0;
}

static int update(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, size_t n,
                  int on_device, msd_position *out, msd_pos_nicrc *nicrc, bool want_nicrc, uint8_t *forward, bool want_forward,
                  msd_sbs_track *trk = nullptr, bool want_sbs = false)
{
    if (!p || (want_nicrc && !p->table) || (want_forward && !p->reduce) || (want_sbs && !p->d_track_table.get()))
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
    int rc = reserve(p, n, want_sbs);
    if (rc)
        return rc;
    if (!on_device && ((rc = stage(p, p->d_msgs, msgs, n)) || (rc = stage(p, p->d_fields, fields, n)) ||
                       (rc = stage(p, p->d_receiver, receiver, n))))
        return rc;
    const msd_pos_table t = p->tab[p->cur];
    uint32_t *const d_ctl = p->d_ctl.get(), *const d_slot = p->d_slot.get();
    uint8_t *const d_fresh = p->d_fresh.get(), *const d_forward = p->d_forward.get();
    msd_position *const d_out = p->d_out.get();
    msd_pos_nicrc *const d_nicrc = p->d_nicrc.get();
    msd_sbs_track *const d_sbs = p->d_sbs.get();
    uint8_t *const d_rcode = p->range ? p->d_rcode.get() : nullptr;
    uint32_t ctl[MSD_POS_CTL_N] = {};
    POS_HIP(p, hipMemsetAsync(d_ctl, 0, sizeof ctl, p->stream));
    msd_pos_launch_find(p->stream, t, msgs, fields, receiver, p->nrx, (uint32_t)n, d_slot, d_fresh, d_out, d_ctl);
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    if (ctl[MSD_POS_CTL_FULL] || ctl[MSD_POS_CTL_BAD_RECEIVER]) { /* nothing changes: this call's aircraft leave again */
        msd_pos_launch_rollback(p->stream, t, d_slot, d_fresh, (uint32_t)n);
        POS_HIP(p, hipGetLastError());
        POS_HIP(p, hipStreamSynchronize(p->stream));
        snprintf(p->err, sizeof p->err, "%s", ctl[MSD_POS_CTL_BAD_RECEIVER] ? "a receiver index is out of range"
                                                                           : "the aircraft table is full");
        return ctl[MSD_POS_CTL_BAD_RECEIVER] ? -EINVAL : -ENOSPC;
    }
    p->live += ctl[MSD_POS_CTL_INSERTED];
    if (p->pb && ctl[MSD_POS_CTL_INSERTED]) { /* the new aircraft have been written nowhere yet */
        msd_pb_launch_fresh(p->stream, d_slot, d_fresh, (uint32_t)n, t.cap, p->pb_state[p->cur].get());
        POS_HIP(p, hipGetLastError());
    }
    if (p->d_ac.get()) { /* the call has passed its checks: its Mode A/C replies count (track.c:1001) */
        msd_pos_launch_modeac_count(p->stream, msgs, fields, receiver, p->nrx, (uint32_t)n, p->d_ac.get());
        POS_HIP(p, hipGetLastError());
    }
    if (p->table) /* a skipped record's entry stays zero */
        POS_HIP(p, hipMemsetAsync(d_nicrc, 0, n * sizeof(msd_pos_nicrc), p->stream));
    if (p->reduce) /* and its verdict */
        POS_HIP(p, hipMemsetAsync(d_forward, 0, n, p->stream));
    if (want_sbs) /* and its row; no other call makes rows */
        POS_HIP(p, hipMemsetAsync(d_sbs, 0, n * sizeof(msd_sbs_track), p->stream));
    if (d_rcode) /* and its range code: the range kernel passes it by */
        POS_HIP(p, hipMemsetAsync(d_rcode, 0, n, p->stream));
    for (size_t base = 0; base < n; base += MSD_POS_PIECE) {
        const size_t m = n - base < MSD_POS_PIECE ? n - base : MSD_POS_PIECE;
        msd_pos_launch_piece(p->stream, t, msgs, fields, receiver, p->d_rx.get(), p->fp, (uint32_t)base, (uint32_t)m, d_slot,
                             p->d_idx[0].get(), p->d_idx[1].get(), p->d_hist.get(), d_out, p->d_stats.get(), d_nicrc,
                             p->reduce_interval, d_forward, want_sbs ? d_sbs : nullptr, d_rcode);
        POS_HIP(p, hipGetLastError());
        if (d_rcode) { /* behind the piece's walk, piece after piece: an aircraft's last decoded record of the call wins */
            if (p->range_timing)
                POS_HIP(p, hipEventRecord(p->range_ev[0], p->stream));
            msd_pos_launch_range(p->stream, t, d_out, receiver, p->d_rx.get(), d_slot, d_rcode, (uint32_t)base, (uint32_t)m,
                                 p->range_polar, p->range_combine, p->d_rng.get(), p->d_rmargins.get());
            POS_HIP(p, hipGetLastError());
            if (p->range_timing) { /* a measuring run: the piece's kernel alone, waited for */
                float ms = 0;
                POS_HIP(p, hipEventRecord(p->range_ev[1], p->stream));
                POS_HIP(p, hipEventSynchronize(p->range_ev[1]));
                POS_HIP(p, hipEventElapsedTime(&ms, p->range_ev[0], p->range_ev[1]));
                p->range_ms = base ? p->range_ms + ms : ms;
            }
        }
    }
    POS_HIP(p, hipMemcpyAsync(out, d_out, n * sizeof(msd_position), hipMemcpyDeviceToHost, p->stream));
    if (want_nicrc)
        POS_HIP(p, hipMemcpyAsync(nicrc, d_nicrc, n * sizeof(msd_pos_nicrc), hipMemcpyDeviceToHost, p->stream));
    if (want_forward)
        POS_HIP(p, hipMemcpyAsync(forward, d_forward, n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                  p->stream));
    if (want_sbs)
        POS_HIP(p, hipMemcpyAsync(trk, d_sbs, n * sizeof(msd_sbs_track),
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
    if (p->d_track_table.get())
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    /* (the rows' buffer grows with the calls, as the verdicts' does) */
    return track_table(p, p->d_track_table, msd_sbs_build_track_table, MSD_SBS_TRACK_ENTRIES);
}

int msd_pos_sbs_wire(msd_pos *p, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk, size_t n,
                     int on_device, const msd_sbs_options *opt, uint8_t *out, size_t cap, size_t *out_len, uint32_t *ends)
{
    if (!p || !p->d_track_table.get() || !out_len || !msd_sbs_options_ok(opt) || n > MSD_POS_MAX_N)
        return -EINVAL;
    *out_len = 0;
    if (n == 0)
        return 0;
    if (!msgs || !fields || !trk || (!out && cap > 0))
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    const uint32_t nblocks = (uint32_t)((n + 255u) / 256u);
    int rc = record_writer_buffers(p, n, nblocks);
    if (rc)
        return rc;
    if (!on_device && ((rc = stage(p, p->d_s_msgs, msgs, n)) || (rc = stage(p, p->d_s_fields, fields, n)) ||
                       (rc = stage(p, p->d_s_trk, trk, n))))
        return rc;
    const uint16_t *const table = p->d_track_table.get();
    msd_sbs_launch_lengths(p->stream, msgs, fields, trk, (uint32_t)n, *opt, table, p->d_w_lens.get(), p->d_w_block.get());
    POS_HIP(p, hipGetLastError());
    /* the stream takes at most 2^24 * 147 bytes.  (With none the store kernel still runs: it writes the ends and no byte
     * of the stream) */
    return emit(p, p->d_w_block.get(), nblocks, "SBS", out, cap, out_len, ends, p->d_w_ends.get(), sizeof(uint32_t) * n,
                [&](uint32_t) {
                    msd_sbs_launch_store(p->stream, msgs, fields, trk, (uint32_t)n, *opt, table, p->d_w_lens.get(),
                                         p->d_w_block.get(), p->d_w_out.get(), p->d_w_ends.get());
                });
}

int msd_pos_pb_enable(msd_pos *p)
{
    if (!p || !p->table)
        return -EINVAL;
    if (p->pb)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    dev<uint64_t> state[2], total;
    dev<uint32_t> first;
    dev<msd_pb_receiver> rx;
    const int rc = items_writer_enable(p, [&]() -> int {
        for (int k = 0; k < 2; ++k) { /* the aircraft the table already has have been written nowhere yet */
            POS_HIP(p, state[k].reserve(p->tab[k].cap));
            POS_HIP(p, hipMemsetAsync(state[k].get(), 0, sizeof(uint64_t) * p->tab[k].cap, p->stream));
        }
        POS_HIP(p, first.reserve((size_t)p->nrx + 1u));
        POS_HIP(p, total.reserve(p->nrx));
        POS_HIP(p, rx.reserve(p->nrx));
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    });
    if (rc)
        return rc;
    p->pb_state[0] = std::move(state[0]);
    p->pb_state[1] = std::move(state[1]);
    p->d_pb_first = std::move(first);
    p->d_pb_total = std::move(total);
    p->d_pb_rx = std::move(rx);
    p->pb = true;
    return 0;
}

int msd_pos_vrs_enable(msd_pos *p)
{
    if (!p || !p->table)
        return -EINVAL;
    if (p->vrs)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    dev<uint32_t> first;
    dev<msd_vrs_receiver> rx;
    const int rc = items_writer_enable(p, [&]() -> int {
        POS_HIP(p, first.reserve((size_t)p->nrx + 1u));
        POS_HIP(p, rx.reserve(p->nrx));
        return 0;
    });
    if (rc)
        return rc;
    p->d_vrs_first = std::move(first);
    p->d_vrs_rx = std::move(rx);
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
    const uint32_t live = (uint32_t)p->live;
    const size_t nitems = (size_t)live + 2u * (size_t)p->nrx;
    const uint32_t nblocks = (uint32_t)((nitems + 255u) / 256u);
    POS_HIP(p, p->d_vrs_items.reserve(nitems));
    POS_HIP(p, p->d_vrs_within.reserve(nitems));
    POS_HIP(p, p->d_vrs_sel.reserve((size_t)nblocks + 1u));
    POS_HIP(p, p->d_vrs_block.reserve((size_t)nblocks + 1u));
    POS_HIP(p, p->d_vrs_lens.reserve(nitems));
    POS_HIP(p, p->d_vrs_swithin.reserve(nitems));
    const msd_vrs_call c = {p->tab[p->cur], ordered_slots(p, live), p->d_vrs_items.get(), p->d_vrs_first.get(),
                            p->d_trunc_table.get(), opt->now_ms, (uint32_t)nitems, p->nrx, opt->part, (uint32_t)shift};
    msd_vrs_launch_lengths(p->stream, c, live, p->d_vrs_first.get(), p->d_vrs_items.get(), p->d_vrs_lens.get(),
                           p->d_vrs_swithin.get(), p->d_vrs_within.get(), p->d_vrs_sel.get(), p->d_vrs_block.get(),
                           p->d_vrs_rx.get());
    POS_HIP(p, hipGetLastError());
    /* the store kernel always runs (need >= 14: a receiver's frame) */
    return emit(p, p->d_vrs_block.get(), nblocks, "VRS", out, cap, out_len, rx, p->d_vrs_rx.get(),
                sizeof(msd_vrs_receiver) * p->nrx, [&](uint32_t) {
                    msd_vrs_launch_store(p->stream, c, p->d_vrs_lens.get(), p->d_vrs_block.get(), p->d_w_out.get());
                });
}

int msd_pos_history_pb(msd_pos *p, const msd_history_options *opt, uint8_t *out, size_t cap, size_t *out_len,
                       msd_history_receiver *rx)
{
    if (!p || !p->table || !out_len || !msd_history_options_ok(opt) || (!out && cap > 0))
        return -EINVAL;
    *out_len = 0;
    if (p->live * MSD_HISTORY_ENTRY_MAX + (uint64_t)p->nrx * MSD_HISTORY_HEADER_MAX > 0xFFFFFFFFull) {
        snprintf(p->err, sizeof p->err, "%llu aircraft could take more than 2^32 - 1 bytes", (unsigned long long)p->live);
        return -E2BIG;
    }
    POS_HIP(p, hipSetDevice(p->device));
    const uint32_t live = (uint32_t)p->live;
    const size_t nitems = (size_t)live + p->nrx;
    const uint32_t nblocks = (uint32_t)((nitems + 255u) / 256u);
    const int rc = snapshot_buffers(p); /* there is no enable: the first call makes what the writer needs */
    if (rc)
        return rc;
    POS_HIP(p, p->d_hist_first.reserve((size_t)p->nrx + 1u));
    POS_HIP(p, p->d_hist_rx.reserve(p->nrx));
    POS_HIP(p, p->d_hist_items.reserve(nitems));
    POS_HIP(p, p->d_hist_within.reserve(nitems));
    POS_HIP(p, p->d_hist_cwithin.reserve(nitems));
    POS_HIP(p, p->d_hist_block.reserve(2u * ((size_t)nblocks + 1u)));
    POS_HIP(p, p->d_hist_lens.reserve(nitems));
    const msd_history_call c = {p->tab[p->cur], ordered_slots(p, live), p->d_hist_items.get(), opt->now_ms, (uint32_t)nitems,
                                p->nrx};
    msd_history_launch_lengths(p->stream, c, live, p->d_hist_first.get(), p->d_hist_items.get(), p->d_hist_lens.get(),
                               p->d_hist_within.get(), p->d_hist_cwithin.get(), p->d_hist_block.get(), p->d_hist_rx.get());
    POS_HIP(p, hipGetLastError());
    return emit(p, p->d_hist_block.get(), nblocks, "history", out, cap, out_len, rx, p->d_hist_rx.get(),
                sizeof(msd_history_receiver) * p->nrx, [&](uint32_t need) {
                    if (need) /* (no byte: now_ms < 1000 and no aircraft was written) */
                        msd_history_launch_store(p->stream, c, p->d_hist_lens.get(), p->d_hist_block.get(), p->d_w_out.get());
                });
}

int msd_pos_aircraft_pb(msd_pos *p, const msd_pb_options *opt, uint8_t *out, size_t cap, size_t *out_len, msd_pb_receiver *rx)
{
    if (!p || !p->pb || !out_len || !msd_pb_options_ok(opt) || (!out && cap > 0))
        return -EINVAL;
    *out_len = 0;
    if (p->live * (p->range ? MSD_PB_AIRCRAFT_MAX_RANGE : MSD_PB_AIRCRAFT_MAX) + (uint64_t)p->nrx * MSD_PB_HEADER_MAX > 0xFFFFFFFFull) {
        snprintf(p->err, sizeof p->err, "%llu aircraft could take more than 2^32 - 1 bytes", (unsigned long long)p->live);
        return -E2BIG;
    }
    POS_HIP(p, hipSetDevice(p->device));
    const uint32_t live = (uint32_t)p->live;
    const size_t nitems = (size_t)live + p->nrx;
    const uint32_t nblocks = (uint32_t)((nitems + 255u) / 256u);
    POS_HIP(p, p->d_pb_items.reserve(nitems));
    POS_HIP(p, p->d_pb_within.reserve(nitems));
    POS_HIP(p, p->d_pb_cwithin.reserve(nitems));
    POS_HIP(p, p->d_pb_block.reserve(4u * ((size_t)nblocks + 1u)));
    POS_HIP(p, p->d_pb_shadow.reserve(nitems));
    POS_HIP(p, p->d_pb_lens.reserve(nitems));
    const uint64_t *d_total = nullptr;
    if (opt->messages_total) {
        POS_HIP(p, hipMemcpyAsync(p->d_pb_total.get(), opt->messages_total, sizeof(uint64_t) * p->nrx, hipMemcpyHostToDevice,
                                  p->stream));
        d_total = p->d_pb_total.get();
    }
    const msd_pb_call c = {p->tab[p->cur], p->pb_state[p->cur].get(), p->tab[p->cur].dist, ordered_slots(p, live),
                           p->d_pb_items.get(), d_total,
                           p->d_trunc_table.get(), opt->now_ms, (uint32_t)nitems, p->nrx};
    msd_pb_launch_lengths(p->stream, c, live, p->d_pb_first.get(), p->d_pb_items.get(), p->d_pb_shadow.get(), p->d_pb_lens.get(),
                          p->d_pb_within.get(), p->d_pb_cwithin.get(), p->d_pb_block.get(), p->d_pb_rx.get());
    POS_HIP(p, hipGetLastError());
    /* a refused call has moved no written state: only the store kernel commits the shadow copy */
    return emit(p, p->d_pb_block.get(), nblocks, "aircraft.pb", out, cap, out_len, rx, p->d_pb_rx.get(),
                sizeof(msd_pb_receiver) * p->nrx, [&](uint32_t need) {
                    if (need) /* (no byte: no aircraft was written, so no state moves either) */
                        msd_pb_launch_store(p->stream, c, p->d_pb_shadow.get(), p->d_pb_lens.get(), p->d_pb_block.get(),
                                            p->d_w_out.get());
                });
}

int msd_pos_reduce_enable(msd_pos *p, uint32_t interval_ms)
{
    if (!p || !p->table || interval_ms > MSD_REDUCE_MAX_INTERVAL)
        return -EINVAL;
    if (p->reduce)
        return interval_ms == p->reduce_interval ? 0 : -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    dev<uint64_t> next[2];
    const auto build = [&]() -> int {
        for (int k = 0; k < 2; ++k) { /* the aircraft the table already has start at 0, as a new one does */
            const size_t timers = (size_t)MSD_REDUCE_TIMERS * p->tab[k].cap;
            POS_HIP(p, next[k].reserve(timers));
            POS_HIP(p, hipMemsetAsync(next[k].get(), 0, sizeof(uint64_t) * timers, p->stream));
        }
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was */
        (void)hipGetLastError();
        return rc;
    }
    p->next_reduce[0] = std::move(next[0]);
    p->next_reduce[1] = std::move(next[1]);
    point_tables(p);
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
    int rc = record_writer_buffers(p, n, nblocks);
    if (rc)
        return rc;
    if (!on_device && ((rc = stage(p, p->d_w_msgs, msgs, n)) || (rc = stage(p, p->d_w_forward, forward, n))))
        return rc;
    msd_reduce_launch_lengths(p->stream, msgs, forward, (uint32_t)n, flags, p->d_w_lens.get(), p->d_w_block.get());
    POS_HIP(p, hipGetLastError());
    /* the stream takes at most 2^24 * 44 bytes.  (With none the store kernel still runs: it writes the ends and no byte
     * of the stream) */
    return emit(p, p->d_w_block.get(), nblocks, "reduced", out, cap, out_len, ends, p->d_w_ends.get(), sizeof(uint32_t) * n,
                [&](uint32_t) {
                    msd_reduce_launch_store(p->stream, msgs, (uint32_t)n, flags, p->d_w_lens.get(), p->d_w_block.get(),
                                            p->d_w_out.get(), p->d_w_ends.get());
                });
}

int msd_pos_snapshot(msd_pos *p, msd_aircraft *out, size_t cap, int on_device, size_t *n)
{
    if (!p || !p->table || !n || (!out && cap > 0))
        return -EINVAL;
    return read_out(p, p->d_snap, out, cap, on_device, n, [&](uint32_t *idx_a, uint32_t *idx_b, uint32_t *hist, msd_aircraft *dst) {
        msd_pos_launch_snapshot(p->stream, p->tab[p->cur], (uint32_t)p->live, snapshot_key_bits(p), idx_a, idx_b, hist, dst);
    });
}

int msd_pos_modeac_enable(msd_pos *p)
{
    if (!p || !p->table)
        return -EINVAL;
    if (p->d_ac.get())
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    uint16_t c_to_a[MSD_MODEAC_CODES];
    msd_modeac_build_c_to_a(c_to_a);
    const size_t ac_words = (size_t)MSD_MODEAC_WORDS * p->nrx;
    dev<uint32_t> ac;
    dev<uint16_t> d_c_to_a;
    dev<msd_modeac_code> codes;
    dev<uint8_t> hits[2];
    const auto build = [&]() -> int {
        POS_HIP(p, ac.reserve(ac_words));
        POS_HIP(p, d_c_to_a.reserve(MSD_MODEAC_CODES));
        POS_HIP(p, codes.reserve(MSD_MODEAC_CODES));
        for (int k = 0; k < 2; ++k)
            POS_HIP(p, hits[k].reserve(2u * (size_t)p->tab[k].cap));
        POS_HIP(p, hipMemsetAsync(ac.get(), 0, sizeof(uint32_t) * ac_words, p->stream));
        for (int k = 0; k < 2; ++k) /* the aircraft the table has already start without hits */
            POS_HIP(p, hipMemsetAsync(hits[k].get(), 0, 2u * (size_t)p->tab[k].cap, p->stream));
        POS_HIP(p, hipMemcpyAsync(d_c_to_a.get(), c_to_a, sizeof c_to_a, hipMemcpyHostToDevice, p->stream));
        POS_HIP(p, hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was */
        (void)hipGetLastError();
        return rc;
    }
    p->d_ac = std::move(ac);
    p->d_c_to_a = std::move(d_c_to_a);
    p->d_codes = std::move(codes);
    p->hits[0] = std::move(hits[0]);
    p->hits[1] = std::move(hits[1]);
    point_tables(p);
    return 0;
}

int msd_pos_modeac_match(msd_pos *p, uint64_t now_ms, uint64_t message_now_ms)
{
    if (!p || !p->d_ac.get())
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    msd_pos_launch_modeac_match(p->stream, p->tab[p->cur], p->nrx, now_ms, message_now_ms, p->d_c_to_a.get(), p->d_ac.get());
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_modeac_codes(msd_pos *p, uint32_t receiver, msd_modeac_code *out, int on_device)
{
    if (!p || !p->d_ac.get() || receiver >= p->nrx || !out)
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    msd_modeac_code *dst = on_device ? out : p->d_codes.get();
    msd_pos_launch_modeac_codes(p->stream, p->d_ac.get() + (size_t)receiver * MSD_MODEAC_WORDS, dst);
    POS_HIP(p, hipGetLastError());
    if (!on_device)
        POS_HIP(p, hipMemcpyAsync(out, dst, sizeof(msd_modeac_code) * MSD_MODEAC_CODES, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_modeac_hits(msd_pos *p, msd_modeac_hit *out, size_t cap, int on_device, size_t *n)
{
    if (!p || !p->d_ac.get() || !n || (!out && cap > 0))
        return -EINVAL;
    return read_out(p, p->d_hits_out, out, cap, on_device, n, [&](uint32_t *idx_a, uint32_t *idx_b, uint32_t *hist, msd_modeac_hit *dst) {
        msd_pos_launch_modeac_hits(p->stream, p->tab[p->cur], (uint32_t)p->live, snapshot_key_bits(p), idx_a, idx_b, hist, dst);
    });
}

int msd_pos_range_enable(msd_pos *p, uint32_t flags)
{
    if (!p || (flags & ~MSD_RANGE_POLAR))
        return -EINVAL;
    if (p->range)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    dev<uint32_t> dist[2];
    dev<msd_range_state> rng;
    dev<unsigned long long> margins;
    const auto build = [&]() -> int {
        for (int k = 0; k < 2; ++k) /* the aircraft the table already has start at distance 0 */
            POS_HIP(p, dist[k].reserve(p->tab[k].cap));
        POS_HIP(p, rng.reserve(p->nrx));
        POS_HIP(p, margins.reserve(2));
        uint32_t *const d[2] = {dist[0].get(), dist[1].get()};
        return range_clear(p, d, rng.get(), margins.get());
    };
    const int rc = build();
    if (rc) { /* the tracker stays as it was */
        (void)hipGetLastError();
        return rc;
    }
    p->dist[0] = std::move(dist[0]);
    p->dist[1] = std::move(dist[1]);
    p->d_rng = std::move(rng);
    p->d_rmargins = std::move(margins);
    point_tables(p);
    p->range_polar = (flags & MSD_RANGE_POLAR) != 0;
    p->range = true;
    return 0;
}

/* for scripts/range_rate.py (declared in msd_pos.h, not in modes_hip.h): the range kernel with (1, the default) or without
 * (0) the per-wavefront reduction in front of its atomics -- the results are the same --, and with events around it whose
 * interval msd_pos_range_kernel_ms hands over: the last call's range kernels, in ms */
int msd_pos_range_measure(msd_pos *p, int combine, int timing)
{
    if (!p || !p->range)
        return -EINVAL;
    POS_HIP(p, hipSetDevice(p->device));
    if (timing && !p->range_ev[0]) {
        POS_HIP(p, hipEventCreate(&p->range_ev[0]));
        POS_HIP(p, hipEventCreate(&p->range_ev[1]));
    }
    p->range_combine = combine != 0;
    p->range_timing = timing != 0;
    return 0;
}

int msd_pos_range_kernel_ms(const msd_pos *p, float *ms)
{
    if (!p || !p->range || !ms)
        return -EINVAL;
    *ms = p->range_ms;
    return 0;
}

int msd_pos_range_read(msd_pos *p, uint32_t first, uint32_t count, msd_range_receiver *out, uint32_t flags)
{
    if (!p || !p->range || (flags & ~MSD_RANGE_TAKE_LONGEST) || first > p->nrx || count > p->nrx - first || (!out && count > 0))
        return -EINVAL;
    if (count == 0)
        return 0;
    POS_HIP(p, hipSetDevice(p->device));
    POS_HIP(p, p->d_rng_out.reserve(count));
    msd_pos_launch_range_read(p->stream, p->d_rng.get(), first, count, (flags & MSD_RANGE_TAKE_LONGEST) != 0, p->d_rng_out.get());
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(out, p->d_rng_out.get(), sizeof(msd_range_receiver) * count, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    return 0;
}

int msd_pos_range_distances(msd_pos *p, uint32_t *out, size_t cap, int on_device, size_t *n)
{
    if (!p || !p->range || !n || (!out && cap > 0))
        return -EINVAL;
    return read_out(p, p->d_dist_out, out, cap, on_device, n, [&](uint32_t *idx_a, uint32_t *idx_b, uint32_t *hist, uint32_t *dst) {
        msd_pos_launch_range_distances(p->stream, p->tab[p->cur], (uint32_t)p->live, snapshot_key_bits(p), idx_a, idx_b, hist, dst);
    });
}

int msd_pos_range_pb(msd_pos *p, uint8_t *out, size_t cap, size_t *out_len, uint64_t *end)
{
    if (!p || !p->range || !p->range_polar || !out_len || (!out && cap > 0))
        return -EINVAL;
    *out_len = 0;
    POS_HIP(p, hipSetDevice(p->device));
    const size_t n = (size_t)p->nrx * MSD_RANGE_BUCKETS; /* at most 65536 * 72 entries of at most 10 bytes */
    const uint32_t nblocks = (uint32_t)((n + 255u) / 256u);
    POS_HIP(p, p->d_w_lens.reserve(n));
    POS_HIP(p, p->d_w_block.reserve(nblocks + 1u));
    POS_HIP(p, p->d_rng_end.reserve(p->nrx));
    msd_range_pb_launch_lengths(p->stream, p->d_rng.get(), p->nrx, p->d_w_lens.get(), p->d_w_block.get());
    POS_HIP(p, hipGetLastError());
    return emit(p, p->d_w_block.get(), nblocks, "polar range", out, cap, out_len, end, p->d_rng_end.get(),
                sizeof(uint64_t) * p->nrx, [&](uint32_t) {
                    msd_range_pb_launch_store(p->stream, p->d_rng.get(), p->nrx, p->d_w_lens.get(), p->d_w_block.get(),
                                              p->d_w_out.get(), p->d_rng_end.get());
                });
}

int msd_pos_range_margins(const msd_pos *p, msd_range_margins *m)
{
    if (!p || !p->range || !m)
        return -EINVAL;
    unsigned long long d[2];
    if (hipSetDevice(p->device) != hipSuccess ||
        hipMemcpy(d, p->d_rmargins.get(), sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
        return -EIO;
    memcpy(&m->min_range_margin_m, &d[0], sizeof(double));
    memcpy(&m->min_bearing_margin_deg, &d[1], sizeof(double));
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
    POS_HIP(p, hipMemsetAsync(p->d_ctl.get(), 0, sizeof ctl, p->stream));
    msd_pos_launch_expire(p->stream, p->tab[p->cur], now_ms, p->d_ctl.get());
    POS_HIP(p, hipGetLastError());
    POS_HIP(p, hipMemcpyAsync(ctl, p->d_ctl.get(), sizeof ctl, hipMemcpyDeviceToHost, p->stream));
    POS_HIP(p, hipStreamSynchronize(p->stream));
    if (!ctl[MSD_POS_CTL_REMOVED])
        return 0;
    /* linear probing has no holes to leave: the survivors are inserted again into the other, empty table */
    const int other = p->cur ^ 1;
    if (p->range) /* a removed aircraft's distance goes with it */
        POS_HIP(p, hipMemsetAsync(p->tab[other].dist, 0, sizeof(uint32_t) * p->tab[other].cap, p->stream));
    msd_pos_launch_fill(p->stream, p->tab[other].keys, p->tab[other].cap);
    msd_pos_launch_rebuild(p->stream, p->tab[p->cur], p->tab[other]);
    POS_HIP(p, hipGetLastError());
    if (p->pb) {
        msd_pb_launch_move(p->stream, p->tab[p->cur], p->pb_state[p->cur].get(), p->tab[other], p->pb_state[other].get());
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
        hipMemcpy(d, p->d_stats.get(), sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
        return -EIO;
    memcpy(st, d, sizeof(uint64_t) * MSD_PC_N);
    st->aircraft = p->live;
    memcpy(&st->min_gate_margin_m, &d[MSD_PC_N], sizeof(double));
    return 0;
}

} // extern "C"
