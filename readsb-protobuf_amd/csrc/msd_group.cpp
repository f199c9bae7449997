/*
 * msd_group.cpp -- receiver groups (modes_hip.h msd_group_*): one buffer from each of many live
 * receivers in one call of a wrapped context.  The call runs through the context's stream pipeline as a batch whose
 * slot carries a GroupCall (msd_ctx.h); every buffer is then resolved against its own receiver's state.
 */
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <thread>
#include <vector>

#include "msd_ctx.h" /* the context, and with it modes_hip.h, msd_internal.h and msd_kernels.h */
#include "host/msd_wire.h" /* the host writers, for the entries resolved on host threads */
#include "msd_group_avr.h" /* Beast and AVR input per receiver (with msd_group_beast.h): msd_group_accept_* */

using namespace msd_impl;

namespace {

struct GroupReceiver {
    msd_resolver resolver{}; /* filter, clock (sample_counter) and the counters it sums into `stats` */
    msd_stats stats{};
    bool have_tail = false; /* its tail slot holds the end of its previous buffer */
    bool history = false;   /* a buffer since creation or the last reset: the repair level is fixed */
    msd_group_receiver_options opt{}; /* kept across msd_group_reset_receiver */
    bool mode_ac = false;             /* Mode A/C on (readsb --modeac), likewise kept */
};

/* what the host resolver delivers for one entry of a call */
struct GroupEntryOut {
    std::vector<msd_message> msgs;
    std::vector<uint64_t> req;
    std::vector<msd_fields> fields; /* of msgs, for a fields call (msd_group_submit_*_fields) */
    std::vector<msd_hit> hits; /* the entry's hits, positions made buffer-relative */
    std::vector<msd_ac_hit> ac; /* its Mode A/C candidates, likewise */
    std::vector<uint8_t> wire;  /* msgs in wire format, for a wire call (msd_group_submit_*_wire) */
    uint32_t wire_msgs = 0;     /* the messages `wire` carries */
    double means[2] = {0, 0};
    uint32_t valid = MSD_CHUNK_SAMPLES;
};

void group_emit(const msd_message *mm, const uint64_t *power_req, uint32_t count, uint32_t, void *user)
{
    GroupEntryOut *o = static_cast<GroupEntryOut *>(user);
    o->msgs.insert(o->msgs.end(), mm, mm + count);
    o->req.insert(o->req.end(), power_req, power_req + count);
}

/* body(i) for i in [0, n) on up to `threads` host threads (the calling one included); the work of a thread that could
 * not be started is done by the others */
void parallel_for(uint32_t n, uint32_t threads, const std::function<void(uint32_t)> &body)
{
    if (threads > n)
        threads = n;
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
        for (uint32_t i; (i = next.fetch_add(1)) < n;)
            body(i);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; ++t) {
        try {
            pool.emplace_back(work);
        } catch (...) {
            break;
        }
    }
    work();
    for (std::thread &t : pool)
        t.join();
}

} /* namespace */

struct msd_group {
    msd_ctx *ctx = nullptr;
    uint32_t max_receivers = 0;
    uint32_t threads = 1; /* host threads of the per-receiver work */
    bool gpu = false;     /* resolve on the GPU against the receivers' device snapshots (not MSD_CFG_HOST_RESOLVE) */
    GroupReceiver *rx = nullptr;
    uint8_t *d_tails = nullptr;    /* [max_receivers][MSD_HALO_FRONT] raw samples */
    uint32_t *d_ctl = nullptr;     /* [4][max_receivers]: per buffer its look-behind slot, its receiver and its receiver's
                                      options (threshold | nfix_crc << 16); then the call's buffers with Mode A/C on */
    uint32_t *h_ctl = nullptr;     /* pinned copy */
    uint32_t *d_snaps = nullptr;   /* [max_receivers][MSD_SNAP_WORDS]: every receiver's ICAO filter on the device */
    uint32_t *h_apply = nullptr;   /* pinned, read in place by the filter kernel: slot[n] | add_first[n + 1] | flip[n] */
    uint32_t *h_adds = nullptr;    /* pinned: the entries' adds, max_receivers * MSD_RB_MSG_CAP */
    uint32_t *h_snap = nullptr;    /* pinned staging of one snapshot */
    uint64_t host_buffers = 0;     /* buffers resolved on the host (msd_timing.resolve_fallback) */
    std::vector<GroupEntryOut> out;
    std::vector<uint64_t> req_all;
    /* wire calls, made by the first of them (group_make_wire) */
    uint8_t *h_wire_out = nullptr; /* pinned: the entries' bytes of the buffers resolved on the GPU */
    size_t wire_cap = 0;
    uint32_t *h_wire_entries = nullptr; /* pinned [max_receivers][4]: offset, bytes, messages, 0 per buffer */
    uint32_t *d_wire_counts = nullptr;  /* [max_receivers][2]: bytes and messages per buffer, between the two kernels */
    void *beast = nullptr; /* Beast input (msd_group_remote.cpp): scratch and the receivers' framing state, made by the
                              first msd_group_accept_beast */
    void *avr = nullptr;   /* AVR text input, likewise, made by the first msd_group_accept_avr */
    msd_remote_stats *remote = nullptr; /* [max_receivers] the remote counters both inputs add to */
    char err[256] = {0};
};

namespace {

int gfail(msd_group *g, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g->err, sizeof g->err, fmt, ap);
    va_end(ap);
    return code;
}

#define GHIPCHK(g, call)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return gfail((g), -EIO, "%s failed: %s", #call, hipGetErrorString(e_));             \
    } while (0)

/* the receiver's host filter -> its device snapshot (at creation, reset and after a buffer resolved on the host) */
int group_upload_snapshot(msd_group *g, uint32_t receiver)
{
    if (!g->gpu)
        return 0;
    const msd_filter &f = g->rx[receiver].resolver.filter;
    for (uint32_t h = 0; h < 8192; ++h) {
        g->h_snap[2 * h] = f.slot[0][h];
        g->h_snap[2 * h + 1] = f.slot[1][h];
    }
    g->h_snap[16384] = (uint32_t)f.active;
    GHIPCHK(g, hipMemcpy(g->d_snaps + (size_t)receiver * MSD_SNAP_WORDS, g->h_snap, sizeof(uint32_t) * MSD_SNAP_WORDS,
                         hipMemcpyHostToDevice));
    return 0;
}

void group_receiver_reset(GroupReceiver &r)
{
    msd_resolver_reset(&r.resolver); /* filter, clock and the counters behind r.resolver.stats */
    memset(&r.stats, 0, sizeof r.stats);
    r.have_tail = false;
    r.history = false;
}

/* The two-bit correction tables (--aggressive, crc.c:374-379) of the group's context, made when the first receiver is
 * set to repair level 2 (msd_create makes them when the group's own configuration has nfix_crc 2). */
int group_make_fix2(msd_group *g)
{
    msd_ctx *c = g->ctx;
    if (c->d_fix2[1])
        return 0;
    GHIPCHK(g, hipSetDevice(c->cfg.device));
    bool host_oom = false;
    const hipError_t e = upload_fix2(c, &host_oom);
    if (host_oom)
        return gfail(g, -ENOMEM, "two-bit correction table: out of host memory");
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return gfail(g, e == hipErrorOutOfMemory ? -ENOMEM : -EIO, "two-bit correction table: %s", hipGetErrorString(e));
    }
    return 0;
}

/* The Mode A/C buffers of the group's context (slot 0, the only one a group uses): the candidate kernel's regions and
 * counts, the ordered list and its totals, and for the GPU resolve the accepted replies per buffer -- made when the first
 * receiver is switched on.  The arena holds a candidate per 32 samples of a full call, and never less than one per
 * sample of one buffer, so that a call rescanned in pieces always fits once the pieces are single buffers. */
int group_make_ac(msd_group *g)
{
    msd_ctx *c = g->ctx;
    Slot &s = c->slots[0];
    if (s.d_ac)
        return 0;
    GHIPCHK(g, hipSetDevice(c->cfg.device));
    const uint64_t B = c->cfg.max_batch_samples;
    const uint64_t arena = B / 32 > MIN_HIT_ARENA ? B / 32 : MIN_HIT_ARENA;
    const uint32_t max_wg = (uint32_t)c->cu_count * 28u; /* as msd_create: one region per resident wavefront */
    msd_ac_hit *regions = nullptr, *dense = nullptr;
    msd_wg_counts *counts = nullptr;
    uint64_t *totals = nullptr, *h_totals = nullptr;
    uint32_t *acc_ac = nullptr, *nac = nullptr;
    bool ok = hipMalloc(reinterpret_cast<void **>(&regions), arena * sizeof(msd_ac_hit)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&dense), arena * sizeof(msd_ac_hit)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&counts), max_wg * sizeof(msd_wg_counts)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&totals), 4 * sizeof(uint64_t)) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&h_totals), 4 * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess;
    if (ok && g->gpu)
        ok = hipMalloc(reinterpret_cast<void **>(&acc_ac), sizeof(uint32_t) * MSD_RB_AC_CAP * c->max_buffers) == hipSuccess &&
             hipMalloc(reinterpret_cast<void **>(&nac), sizeof(uint32_t) * c->max_buffers) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)hipFree(regions);
        (void)hipFree(dense);
        (void)hipFree(counts);
        (void)hipFree(totals);
        if (h_totals)
            (void)hipHostFree(h_totals);
        (void)hipFree(acc_ac);
        (void)hipFree(nac);
        return gfail(g, -ENOMEM, "Mode A/C buffers: out of memory");
    }
    memset(h_totals, 0, 4 * sizeof(uint64_t));
    s.d_ac_regions = regions;
    s.d_ac = dense;
    s.d_ac_counts = counts;
    s.d_ac_totals = totals;
    s.h_ac_totals = h_totals;
    s.d_acc_ac = acc_ac;
    s.d_nac = nac;
    c->ac_arena = arena;
    c->ac_max_wg = max_wg;
    return 0;
}

int group_check(const msd_group *g, const msd_group_entry *e, uint32_t n)
{
    if (n > g->max_receivers)
        return -EINVAL;
    if (n && !e)
        return -EINVAL;
    std::vector<bool> seen(g->max_receivers, false);
    for (uint32_t i = 0; i < n; ++i) {
        if (e[i].receiver >= g->max_receivers || e[i].flags != 0 || seen[e[i].receiver])
            return -EINVAL;
        seen[e[i].receiver] = true;
    }
    return 0;
}

/* where a call's messages go: `sink` for msd_group_submit_*, `fsink` with the decoded fields for
 * msd_group_submit_*_fields (want_fields: a fields call, whether or not it has a sink), `wsink` with every entry's
 * bytes in wire format for msd_group_submit_*_wire (want_wire, likewise) */
struct GroupSink {
    msd_group_message_fn sink = nullptr;
    msd_group_fields_fn fsink = nullptr;
    msd_group_wire_fn wsink = nullptr;
    void *user = nullptr;
    bool want_fields = false;
    bool want_wire = false;
    int wire_format = MSD_WIRE_BEAST;
    uint32_t wire_flags = 0;
};

/* The buffers of the wire calls: the pinned array the kernels write the entries' bytes to -- at least `bytes`, grown
 * when a call's worst case needs more --, the per-buffer results and the counts between the two kernels. */
int group_make_wire(msd_group *g, size_t bytes)
{
    GHIPCHK(g, hipSetDevice(g->ctx->cfg.device));
    if (!g->h_wire_entries) {
        uint32_t *entries = nullptr, *counts = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&entries), sizeof(uint32_t) * 4 * g->max_receivers, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&counts), sizeof(uint32_t) * 2 * g->max_receivers) != hipSuccess) {
            (void)hipGetLastError();
            if (entries)
                (void)hipHostFree(entries);
            return gfail(g, -ENOMEM, "wire output buffers: out of memory");
        }
        g->h_wire_entries = entries;
        g->d_wire_counts = counts;
    }
    if (bytes > g->wire_cap) { /* (nothing of an earlier call is in flight: every call ends synchronised) */
        const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 16);
        uint8_t *p = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return gfail(g, -ENOMEM, "wire output array: out of memory");
        }
        if (g->h_wire_out)
            (void)hipHostFree(g->h_wire_out);
        g->h_wire_out = p;
        g->wire_cap = want;
    }
    return 0;
}

constexpr uint32_t GROUP_FULL_GUARD = 6000u; /* occupied active slots above which a buffer is resolved on the host (as the
                                                context's replay does: a buffer adds at most 970 addresses, two slots each) */

/* The entries idx[] on the host: each buffer through the host resolver's sequential path against its receiver's filter,
 * hit positions made buffer-relative; then the signal power of their messages with the group look-behind.  The
 * candidate lists must be in s.h_hits / s.h_tries.  want_fields: the decoded fields of every entry's messages beside
 * them, an entry on its own so that the Mode A/C altitude carry stays inside its buffer.  to.want_wire: every entry's
 * messages through the host writers (host/msd_wire.c), on the entry's thread. */
int group_host_entries(msd_group *g, Slot &s, const msd_group_entry *e, const std::vector<uint32_t> &idx, const GroupSink &to)
{
    const bool want_fields = to.want_fields;
    msd_ctx *c = g->ctx;
    const int format = c->cfg.format;
    const uint64_t H = s.h_totals[0];
    const msd_hit *hits = s.h_hits;
    const uint32_t n = s.nbuffers;
    const uint64_t NA = ac_on(c, s) ? s.h_ac_totals[0] : 0; /* Mode A/C candidates of the call (s.h_ac), ordered */
    std::vector<uint64_t> first(n + 1), ac_first(n + 1);
    {
        uint64_t h = 0, a = 0;
        for (uint32_t i = 0; i <= n; ++i) {
            const uint64_t pos = (uint64_t)i * MSD_CHUNK_SAMPLES;
            while (h < H && MSD_HIT_POS(hits[h]) < pos)
                ++h;
            while (a < NA && s.h_ac[a].pos < pos)
                ++a;
            first[i] = h;
            ac_first[i] = a;
        }
    }
    parallel_for((uint32_t)idx.size(), g->threads, [&](uint32_t k) {
        const uint32_t i = idx[k];
        GroupEntryOut &o = g->out[i];
        GroupReceiver &r = g->rx[e[i].receiver];
        o.hits.assign(hits + first[i], hits + first[i + 1]);
        for (msd_hit &h : o.hits)
            h -= (msd_hit)i * MSD_CHUNK_SAMPLES; /* position is the low field */
        o.ac.assign(s.h_ac + ac_first[i], s.h_ac + ac_first[i + 1]); /* (none unless its receiver has Mode A/C on) */
        for (msd_ac_hit &a : o.ac)
            a.pos -= (uint64_t)i * MSD_CHUNK_SAMPLES;
        msd_resolve_batch(&r.resolver, 0, 1, &o.valid, o.hits.data(), o.hits.size(), s.h_tries, s.h_totals[1], o.ac.data(),
                          o.ac.size(), nullptr, group_emit, &o);
    });
    g->req_all.clear();
    for (uint32_t i : idx)
        for (uint64_t q : g->out[i].req)
            g->req_all.push_back(q + ((uint64_t)i * MSD_CHUNK_SAMPLES << 16));
    const size_t nm = g->req_all.size();
    if (nm) {
        MsdScanParams p{};
        fill_params(c, s, p);
        int rc = ensure_req(c, s, nm);
        if (rc)
            return gfail(g, rc, "power: %s", c->err);
        memcpy(s.h_req, g->req_all.data(), nm * sizeof(uint64_t));
        GHIPCHK(g, hipMemcpyAsync(s.d_req, s.h_req, nm * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        rc = msd_launch_power(&p, format, s.d_req, (uint32_t)nm, reinterpret_cast<unsigned long long *>(s.d_pow), c->stream);
        if (rc)
            return gfail(g, rc, "group power kernel launch failed");
        GHIPCHK(g, hipMemcpyAsync(s.h_pow, s.d_pow, nm * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        GHIPCHK(g, hipStreamSynchronize(c->stream));
    }
    std::vector<uint64_t> pow_first(idx.size() + 1, 0);
    for (size_t k = 0; k < idx.size(); ++k)
        pow_first[k + 1] = pow_first[k] + g->out[idx[k]].req.size();
    parallel_for((uint32_t)idx.size(), g->threads, [&](uint32_t k) {
        GroupEntryOut &o = g->out[idx[k]];
        GroupReceiver &r = g->rx[e[idx[k]].receiver];
        const std::vector<uint32_t> buf(o.msgs.size(), 0u);
        msd_resolve_power(&r.resolver, 1, &o.valid, o.means, o.msgs.data(), sizeof(msd_message), o.req.data(), buf.data(),
                          s.h_pow + pow_first[k], sizeof(uint64_t), o.msgs.size());
        if (want_fields) { /* one buffer index for the whole entry: the carry starts empty and never leaves it */
            o.fields.resize(o.msgs.size());
            msd_fields_batch(o.msgs.data(), sizeof(msd_message), buf.data(), o.msgs.size(), o.fields.data());
        }
        if (to.want_wire) {
            const int verbatim = (to.wire_flags & MSD_WIRE_VERBATIM) ? 1 : 0;
            o.wire.resize(o.msgs.size() * MSD_AVR_MAX); /* MSD_AVR_MAX > MSD_BEAST_MAX; the line's NUL is overwritten */
            size_t used = 0;
            o.wire_msgs = 0;
            for (const msd_message &mm : o.msgs) {
                const size_t len = to.wire_format == MSD_WIRE_BEAST
                                       ? msd_beast_frame_out(&mm, verbatim, o.wire.data() + used)
                                       : msd_avr_line_out(&mm, to.wire_format == MSD_WIRE_AVR_MLAT, verbatim,
                                                          reinterpret_cast<char *>(o.wire.data()) + used);
                used += len;
                o.wire_msgs += len ? 1u : 0u;
            }
            o.wire.resize(used);
        }
    });
    g->host_buffers += idx.size();
    for (uint32_t i : idx) { /* the device copies follow the host filters */
        const int rc = group_upload_snapshot(g, e[i].receiver);
        if (rc)
            return rc;
    }
    return 0;
}

/* The GPU resolve of one call: every buffer in one pass of msd_resolve_kernel against its own receiver's snapshot
 * (snap_idx = receiver), signal power and records on the device, then the receivers' filter changes applied to the host
 * filters and, by msd_group_filter_apply_kernel, to the device snapshots.  Buffers the kernel hands back (fallback) and
 * receivers whose active table is nearly full are returned in `host` for group_host_entries.  want_fields: the emit
 * kernel also writes the decoded fields, s.h_fields[k] beside s.h_wire[k].  to.want_wire: behind the emit kernel the two
 * wire kernels leave every such buffer's bytes in g->h_wire_out, as g->h_wire_entries says. */
int group_gpu_entries(msd_group *g, Slot &s, const msd_group_entry *e, std::vector<uint32_t> &gpu_idx,
                      std::vector<uint32_t> &host, std::vector<uint32_t> &rec_first, const GroupSink &to)
{
    const bool want_fields = to.want_fields;
    msd_ctx *c = g->ctx;
    const uint32_t n = s.nbuffers;
    const GpuCtl ctl = gpu_ctl(c, s);
    gpu_idx.clear();
    for (uint32_t i = 0; i < n; ++i) {
        GroupReceiver &r = g->rx[e[i].receiver];
        /* sdr_ifile.c:187-190 on the receiver's own clock (the drops are on it already) */
        const uint64_t sample_ts = (uint64_t)(r.resolver.sample_counter * 12e6 / 2400000.0);
        ctl.h_ts[2 * i] = sample_ts;
        ctl.h_ts[2 * i + 1] = sample_ts / 12000u;
        ctl.h_valid[i] = MSD_CHUNK_SAMPLES;
        ctl.h_snap[i] = e[i].receiver;
        if (r.resolver.filter.active_used > GROUP_FULL_GUARD) {
            host.push_back(i);
        } else {
            ctl.h_todo[gpu_idx.size()] = i;
            gpu_idx.push_back(i);
        }
    }
    const uint32_t ntodo = (uint32_t)gpu_idx.size();
    if (!ntodo)
        return 0;
    MsdResolveParams rp{};
    gpu_params(c, s, rp);
    rp.snaps = g->d_snaps;
    rp.pred = reinterpret_cast<const unsigned long long *>(s.d_pred); /* never written by a group scan: no predictions */
    rp.pred_gen = 0;
    rp.power = nullptr;   /* the fused power would read the batch's previous buffer as look-behind */
    rp.first_pass = 0;
    rp.ctl_implicit = 0;
    GHIPCHK(g, hipMemsetAsync(s.d_nmsgs, 0, sizeof(uint32_t) * n, c->stream)); /* host-resolved buffers emit nothing */
    if (rp.ac)
        GHIPCHK(g, hipMemsetAsync(s.d_nac, 0, sizeof(uint32_t) * n, c->stream));
    int rc = msd_launch_resolve(&rp, ntodo, c->stream);
    if (rc)
        return gfail(g, rc, "resolve kernel launch failed");
    MsdScanParams p{};
    fill_params(c, s, p);
    rc = msd_launch_group_power_buffers(&p, c->cfg.format, s.d_acc, s.d_nmsgs, rp.todo, ntodo,
                                        reinterpret_cast<unsigned long long *>(s.d_powr), c->stream);
    if (rc)
        return gfail(g, rc, "group power kernel launch failed");
    GHIPCHK(g, hipStreamSynchronize(c->stream));
    /* the kernel's verdicts: a buffer it could not finish goes to the host, its records must not be emitted */
    uint32_t total = 0;
    bool zeroed = false;
    rec_first.assign(n + 1, 0);
    for (uint32_t k = 0; k < ntodo; ++k) {
        const uint32_t i = gpu_idx[k];
        if (s.h_rbuf[i].fallback) {
            host.push_back(i);
            GHIPCHK(g, hipMemsetAsync(s.d_nmsgs + i, 0, sizeof(uint32_t), c->stream));
            if (rp.ac)
                GHIPCHK(g, hipMemsetAsync(s.d_nac + i, 0, sizeof(uint32_t), c->stream));
            zeroed = true;
        }
    }
    if (zeroed) {
        std::vector<uint32_t> keep;
        for (uint32_t i : gpu_idx)
            if (!s.h_rbuf[i].fallback)
                keep.push_back(i);
        gpu_idx.swap(keep);
    }
    for (uint32_t i = 0, k = 0; i < n; ++i) {
        rec_first[i] = total;
        if (k < gpu_idx.size() && gpu_idx[k] == i) {
            total += s.h_rbuf[i].nmsgs + s.h_rbuf[i].nac; /* its Mode S messages, then its Mode A/C replies (0: off) */
            ++k;
        }
    }
    rec_first[n] = total;
    if (total) {
        rc = ensure_req(c, s, total);
        if (rc)
            return gfail(g, rc, "records: %s", c->err);
        /* (s.h_fields after ensure_req, which moves the arrays when it grows them) */
        rc = msd_launch_emit(&rp, n, reinterpret_cast<const unsigned long long *>(s.d_powr), s.h_side, s.h_wire,
                             want_fields ? s.h_fields : nullptr, (uint32_t)s.req_cap, c->stream);
        if (rc)
            return gfail(g, rc, "emit kernel launch failed");
    }
    if (to.want_wire) {
        /* the worst case, known before the launch: 44 bytes per Mode S message and 20 per Mode A/C reply (a Beast frame
         * of two bytes with every byte escaped; an AVR line of a reply is 19), every entry rounded up to 16 */
        size_t worst = 0;
        for (uint32_t i : gpu_idx)
            worst += ((size_t)MSD_BEAST_MAX * s.h_rbuf[i].nmsgs + 20u * (size_t)s.h_rbuf[i].nac + 15u) & ~(size_t)15u;
        rc = group_make_wire(g, worst);
        if (rc)
            return rc;
        memset(g->h_wire_entries, 0, sizeof(uint32_t) * 4 * n);
        if (total) {
            rc = msd_launch_group_wire(&rp, n, reinterpret_cast<const unsigned long long *>(s.d_powr), to.wire_format,
                                       (to.wire_flags & MSD_WIRE_VERBATIM) ? 1 : 0, g->d_wire_counts, g->h_wire_out,
                                       g->wire_cap, g->h_wire_entries, c->stream);
            if (rc)
                return gfail(g, rc, "wire kernel launch failed");
        }
    }
    /* the filter changes, in each receiver's order: adds, then the flip (readsb.c:331) -- on the host filters here, on
     * the device snapshots by the filter kernel below */
    const uint32_t m = (uint32_t)gpu_idx.size();
    uint32_t *a_slot = g->h_apply, *a_first = g->h_apply + g->max_receivers, *a_flip = a_first + g->max_receivers + 1;
    a_first[0] = 0;
    for (uint32_t k = 0; k < m; ++k) { /* the add lists, concatenated */
        const uint32_t i = gpu_idx[k];
        const msd_rbuf &rb = s.h_rbuf[i];
        const uint32_t *adds = rb.nshort <= MSD_RB_ADD_INLINE ? rb.adds : s.d_adds + (size_t)i * MSD_RB_MSG_CAP;
        const uint32_t na = rb.nshort <= MSD_RB_ADD_INLINE ? rb.nshort : rb.nadds;
        memcpy(g->h_adds + a_first[k], adds, sizeof(uint32_t) * na);
        a_first[k + 1] = a_first[k] + na;
        a_slot[k] = e[i].receiver;
    }
    parallel_for(m, g->threads, [&](uint32_t k) {
        const uint32_t i = gpu_idx[k];
        const msd_rbuf &rb = s.h_rbuf[i];
        GroupReceiver &r = g->rx[e[i].receiver];
        for (uint32_t j = a_first[k]; j < a_first[k + 1]; ++j)
            msd_filter_add(&r.resolver.filter, g->h_adds[j]);
        const int active = r.resolver.filter.active;
        const uint64_t next_flip = r.resolver.filter.next_flip;
        msd_filter_expire(&r.resolver.filter, rb.end_now);
        a_flip[k] = (r.resolver.filter.active != active || r.resolver.filter.next_flip != next_flip) ? 1u : 0u;
        r.resolver.sample_counter += MSD_CHUNK_SAMPLES;
        r.resolver.ifile_now = rb.end_now;
        msd_gpu_resolve_commit_stats(&r.resolver, 1, &ctl.h_valid[i], &rb);
    });
    rc = msd_launch_group_filter_apply(g->d_snaps, m, a_slot, a_first, g->h_adds, a_flip, c->stream);
    if (rc)
        return gfail(g, rc, "group filter kernel launch failed");
    GHIPCHK(g, hipStreamSynchronize(c->stream));
    /* signal level is in the records; the order-sensitive power statistics per receiver, in its own message order */
    parallel_for(m, g->threads, [&](uint32_t k) {
        const uint32_t i = gpu_idx[k];
        GroupReceiver &r = g->rx[e[i].receiver];
        const uint32_t nm = rec_first[i + 1] - rec_first[i];
        const std::vector<uint32_t> buf(nm ? nm : 1, 0u);
        msd_resolve_power_stats(&r.resolver, 1, &ctl.h_valid[i], g->out[i].means, buf.data(),
                                reinterpret_cast<const uint64_t *>(s.h_side) + rec_first[i], nm);
    });
    return 0;
}

/* one call: scan (group instantiation); then every entry resolved against its own receiver's state -- on the GPU, or
 * on host threads (MSD_CFG_HOST_RESOLVE, a rescanned overflow, the kernel's fallback); tails; delivery in entry order */
int group_run(msd_group *g, const uint8_t *d_iq, const msd_group_entry *e, uint32_t n, const GroupSink &to)
{
    msd_ctx *c = g->ctx;
    const int format = c->cfg.format;
    const uint64_t nsamples = (uint64_t)n * MSD_CHUNK_SAMPLES;
    /* look-behind: the receiver's tail slot unless it has none yet or lost samples in front of this buffer (fifo.c:178-181) */
    uint32_t *lb = g->h_ctl, *slot = g->h_ctl + g->max_receivers, *opt = g->h_ctl + 2 * g->max_receivers;
    uint32_t *ac = g->h_ctl + 3 * g->max_receivers, nac = 0;
    bool fix2 = false;
    for (uint32_t i = 0; i < n; ++i) {
        GroupReceiver &r = g->rx[e[i].receiver];
        lb[i] = r.have_tail && e[i].dropped == 0 ? e[i].receiver : MSD_GROUP_NO_TAIL;
        slot[i] = e[i].receiver;
        opt[i] = (uint32_t)r.opt.preamble_threshold | (uint32_t)r.opt.nfix_crc << 16;
        fix2 |= r.opt.nfix_crc == 2;
        r.history = true;
        if (r.mode_ac) /* readsb.c:829-833: the switch as it stands when the buffer is demodulated */
            ac[nac++] = i;
        r.resolver.mode_ac = r.mode_ac; /* (the host resolver, if the buffer goes there) */
    }
    GHIPCHK(g, hipMemcpyAsync(g->d_ctl, g->h_ctl, sizeof(uint32_t) * (3 * (size_t)g->max_receivers + nac), hipMemcpyHostToDevice,
                              c->stream));

    GroupCall call;
    call.tails = g->d_tails;
    call.lb = g->d_ctl;
    call.opt = g->d_ctl + 2 * g->max_receivers;
    call.ac = g->d_ctl + 3 * g->max_receivers;
    call.ac_host = ac;
    call.nac = nac;
    call.fix2 = fix2;
    Slot &s = c->slots[0];
    s.group = &call;
    s.busy = true;
    s.d_iq = d_iq;
    s.d_prev = nullptr;
    s.have_prev = 0;
    s.threshold = c->cfg.preamble_threshold;
    s.dropped_before = 0;
    s.gpu_resolve = false; /* no prediction table from the scan */
    s.resolve_inflight = false;
    s.reset_before = false;
    s.dc = false;
    s.batch_first = 0;
    s.nsamples = nsamples;
    s.nbuffers = n;
    s.last = 0;
    s.tail_dst = nullptr; /* the group keeps its own tails */
    struct Release { /* on every way out: the slot is free again, and no later batch in it sees the call */
        Slot &s;
        ~Release()
        {
            s.group = nullptr;
            s.busy = false;
            s.download_started = false;
        }
    } release{s};
    int rc = enqueue(c, s, format, nullptr);
    s.gpu_resolve = g->gpu; /* start_download: the lists stay on the device unless the arenas overflowed */
    if (!rc)
        rc = start_download(c, s, format); /* an arena overflow is scanned again in pieces here (rerun_in_pieces) */
    if (rc)
        return gfail(g, rc, "scan: %s", c->err);
    GHIPCHK(g, hipEventSynchronize(s.ev_copy1));
    const bool fm = format == MSD_FMT_SC16 || format == MSD_FMT_SC16Q11;

    if (g->out.size() < n)
        g->out.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        GroupEntryOut &o = g->out[i];
        GroupReceiver &r = g->rx[e[i].receiver];
        o.msgs.clear();
        o.req.clear();
        if (fm) { /* convert.c:245-251 */
            o.means[0] = (double)(s.h_fmeans[2 * i] / (float)MSD_CHUNK_SAMPLES);
            o.means[1] = (double)(s.h_fmeans[2 * i + 1] / (float)MSD_CHUNK_SAMPLES);
        } else { /* convert.c:104-110 */
            o.means[0] = (double)s.h_sums[2 * i] / 65536.0 / (double)MSD_CHUNK_SAMPLES;
            o.means[1] = (double)s.h_sums[2 * i + 1] / 65535.0 / 65535.0 / (double)MSD_CHUNK_SAMPLES;
        }
        /* samples lost in front of the buffer go onto its receiver's clock first (sdr_rtlsdr.c:284,299; readsb.c:836) */
        r.resolver.sample_counter += e[i].dropped;
        r.stats.samples_dropped += e[i].dropped;
    }
    std::vector<uint32_t> gpu_idx, host, rec_first;
    if (s.gpu_resolve) {
        rc = group_gpu_entries(g, s, e, gpu_idx, host, rec_first, to);
        if (rc)
            return rc;
        if (!host.empty()) { /* their candidate lists after all */
            std::sort(host.begin(), host.end());
            rc = ensure_host(c, s, s.h_totals[0], s.h_totals[1]);
            if (rc)
                return gfail(g, rc, "lists: %s", c->err);
            if (s.h_totals[0])
                GHIPCHK(g, hipMemcpyAsync(s.h_hits, s.d_hits, s.h_totals[0] * sizeof(msd_hit), hipMemcpyDeviceToHost, c->stream));
            if (s.h_totals[1])
                GHIPCHK(g, hipMemcpyAsync(s.h_tries, s.d_tries, s.h_totals[1] * sizeof(msd_try), hipMemcpyDeviceToHost, c->stream));
            if (nac) {
                rc = ensure_ac_host(c, s, s.h_ac_totals[0]);
                if (rc)
                    return gfail(g, rc, "lists: %s", c->err);
                if (s.h_ac_totals[0])
                    GHIPCHK(g, hipMemcpyAsync(s.h_ac, s.d_ac, s.h_ac_totals[0] * sizeof(msd_ac_hit), hipMemcpyDeviceToHost,
                                              c->stream));
            }
            GHIPCHK(g, hipStreamSynchronize(c->stream));
        }
    } else {
        for (uint32_t i = 0; i < n; ++i)
            host.push_back(i);
    }
    c->timing.hits = s.h_totals[0];
    c->timing.tries = s.h_totals[1];
    c->timing.resolve_passes = gpu_idx.empty() ? 0 : 1;
    if (!host.empty()) {
        rc = group_host_entries(g, s, e, host, to);
        if (rc)
            return rc;
    }
    c->timing.resolve_fallback = g->host_buffers;
    /* every buffer's end becomes its receiver's look-behind (behind the scan, its reruns and the power kernels) */
    rc = msd_launch_group_tails(d_iq, n, g->d_ctl + g->max_receivers, g->d_tails, (uint32_t)c->bps, c->stream);
    if (rc)
        return gfail(g, rc, "group tail kernel launch failed");
    GHIPCHK(g, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; ++i)
        g->rx[e[i].receiver].have_tail = true;
    if (to.want_wire) { /* each entry's bytes from wherever it was resolved: one call per entry */
        std::vector<bool> on_gpu(n, false);
        for (uint32_t i : gpu_idx)
            on_gpu[i] = true;
        for (uint32_t i : gpu_idx) {
            const uint32_t *we = g->h_wire_entries + 4 * (size_t)i;
            if (we[1] == 0xffffffffu || (size_t)we[0] + we[1] > g->wire_cap)
                return gfail(g, -EIO, "wire kernel: entry %u does not fit the output array", i);
        }
        for (uint32_t i = 0; i < n && to.wsink; ++i) {
            const GroupEntryOut &o = g->out[i];
            if (on_gpu[i]) {
                const uint32_t *we = g->h_wire_entries + 4 * (size_t)i;
                to.wsink(e[i].receiver, g->h_wire_out + we[0], we[1], we[2], to.user);
            } else {
                to.wsink(e[i].receiver, o.wire.data(), o.wire.size(), o.wire_msgs, to.user);
            }
        }
    } else if (to.sink || to.fsink) { /* each entry's records, and its fields, from wherever it was resolved */
        std::vector<bool> on_gpu(n, false);
        for (uint32_t i : gpu_idx)
            on_gpu[i] = true;
        for (uint32_t i = 0; i < n; ++i) {
            const GroupEntryOut &o = g->out[i];
            if (on_gpu[i]) {
                for (uint32_t k = rec_first[i]; k < rec_first[i + 1]; ++k) {
                    if (to.fsink)
                        to.fsink(e[i].receiver, &s.h_wire[k].mm, &s.h_fields[k], to.user);
                    else
                        to.sink(e[i].receiver, &s.h_wire[k].mm, to.user);
                }
            } else {
                for (size_t k = 0; k < o.msgs.size(); ++k) {
                    if (to.fsink)
                        to.fsink(e[i].receiver, &o.msgs[k], &o.fields[k], to.user);
                    else
                        to.sink(e[i].receiver, &o.msgs[k], to.user);
                }
            }
        }
    }
    return 0;
}

/* the six submit entries: the checks that leave the group untouched, the copy of a host call's IQ to the staging
 * buffer, then the call */
int group_submit(msd_group *g, const void *iq, const msd_group_entry *e, uint32_t n, bool from_host, const GroupSink &to)
{
    if (!g)
        return -EINVAL;
    msd_ctx *c = g->ctx;
    if (to.want_fields && !c->want_fields)
        return gfail(g, -EINVAL, "the group was created without MSD_CFG_DECODE_FIELDS");
    if (to.want_wire && ((to.wire_format != MSD_WIRE_BEAST && to.wire_format != MSD_WIRE_AVR &&
                          to.wire_format != MSD_WIRE_AVR_MLAT) || (to.wire_flags & ~MSD_WIRE_VERBATIM)))
        return gfail(g, -EINVAL, "wire output: unknown format %d or flags 0x%x", to.wire_format, to.wire_flags);
    if (group_check(g, e, n))
        return gfail(g, -EINVAL, "entries: a receiver out of range or given twice, nonzero flags, or more than max_receivers");
    if (n && !iq)
        return gfail(g, -EINVAL, from_host ? "IQ pointer must be non-null" : "IQ pointer must be non-null and 16-byte aligned");
    if (n && !from_host && (reinterpret_cast<uintptr_t>(iq) & 15u))
        return gfail(g, -EINVAL, "IQ pointer must be non-null and 16-byte aligned");
    if (c->failed)
        return gfail(g, -EIO, "an earlier call failed");
    if (n == 0)
        return 0;
    auto run = [&]() -> int {
        GHIPCHK(g, hipSetDevice(c->cfg.device));
        if (from_host) {
            if (!c->d_stage)
                GHIPCHK(g, hipMalloc(reinterpret_cast<void **>(&c->d_stage), c->cfg.max_batch_samples * 4 + 64));
            GHIPCHK(g, hipMemcpyAsync(c->d_stage, iq, (size_t)n * MSD_CHUNK_SAMPLES * c->bps, hipMemcpyHostToDevice, c->stream));
            iq = c->d_stage;
        }
        return group_run(g, static_cast<const uint8_t *>(iq), e, n, to);
    };
    const int rc = run();
    if (rc)
        c->failed = true;
    return rc;
}

/* the output of a fields or wire accept call (out = NULL: a plain call), checked as group_submit checks its own */
int group_check_out(msd_group *g, const msd_gb_out *out)
{
    if (!out)
        return 0;
    if (out->want_fields && !g->ctx->want_fields)
        return gfail(g, -EINVAL, "the group was created without MSD_CFG_DECODE_FIELDS");
    if (out->want_wire && ((out->format != MSD_WIRE_BEAST && out->format != MSD_WIRE_AVR && out->format != MSD_WIRE_AVR_MLAT) ||
                           (out->verbatim & ~(int)MSD_WIRE_VERBATIM)))
        return gfail(g, -EINVAL, "wire output: unknown format %d or flags 0x%x", out->format, (unsigned)out->verbatim);
    return 0;
}

msd_gb_out fields_out(msd_group_fields_fn sink)
{
    msd_gb_out o{};
    o.want_fields = 1;
    o.fsink = sink;
    return o;
}

/* (verbatim carries the call's flags until group_check_out has seen them: MSD_WIRE_VERBATIM is 1) */
msd_gb_out wire_out(int format, uint32_t flags, msd_group_wire_fn sink)
{
    msd_gb_out o{};
    o.want_wire = 1;
    o.wsink = sink;
    o.format = format;
    o.verbatim = (int)flags;
    return o;
}

/* what differs between the remote inputs in group_accept_remote, by the public entry type of each */
template <class Entry> struct RemoteInput;
template <> struct RemoteInput<msd_group_beast_entry> {
    static constexpr int FORMAT = MSD_GR_BEAST;
    static constexpr const char *NAME = "Beast", *BAD_ENTRY = "or nonzero flags or reserved"; /* in the error texts */
    static constexpr uint32_t FLAGS_OK = 0, ENTRY_MAX = MSD_GROUP_BEAST_ENTRY_MAX;
    static constexpr uint64_t OFFSET_MAX = MSD_GROUP_BEAST_OFFSET_MAX;
    static void **state(msd_group *g) { return &g->beast; }
};
template <> struct RemoteInput<msd_group_avr_entry> {
    static constexpr int FORMAT = MSD_GR_AVR;
    static constexpr const char *NAME = "AVR", *BAD_ENTRY = "an unknown flag or nonzero reserved";
    static constexpr uint32_t FLAGS_OK = MSD_AVR_KEEP_TIMESTAMP, ENTRY_MAX = MSD_GROUP_AVR_ENTRY_MAX;
    static constexpr uint64_t OFFSET_MAX = MSD_GROUP_AVR_OFFSET_MAX;
    static void **state(msd_group *g) { return &g->avr; }
};

/* Beast or AVR input per receiver (Entry: msd_group_beast_entry or msd_group_avr_entry, of one layout): the checks that
 * leave the group untouched, each entry's receiver options, then the call (msd_group_remote.cpp) */
template <class Entry>
int group_accept_remote(msd_group *g, const void *bytes, int on_device, const Entry *e, uint32_t n, msd_group_message_fn sink,
                        const msd_gb_out *out, void *user)
{
    using F = RemoteInput<Entry>;
    if (!g)
        return -EINVAL;
    msd_ctx *c = g->ctx;
    if (int rc = group_check_out(g, out))
        return rc;
    if (n > g->max_receivers)
        return gfail(g, -EINVAL, "%s entries: more than max_receivers", F::NAME);
    if (n && (!e || !bytes))
        return gfail(g, -EINVAL, "%s entries: NULL bytes or entries", F::NAME);
    std::vector<bool> seen(g->max_receivers, false);
    for (uint32_t i = 0; i < n; ++i) {
        if (e[i].receiver >= g->max_receivers || seen[e[i].receiver] || (e[i].flags & ~F::FLAGS_OK) || e[i].reserved)
            return gfail(g, -EINVAL, "%s entry %u: a receiver out of range or given twice, %s", F::NAME, i, F::BAD_ENTRY);
        if (e[i].nbytes > F::ENTRY_MAX || e[i].offset > F::OFFSET_MAX)
            return gfail(g, -EINVAL, "%s entry %u: more than %u bytes, or an offset above 2^47", F::NAME, i, F::ENTRY_MAX);
        seen[e[i].receiver] = true;
    }
    if (c->failed)
        return gfail(g, -EIO, "an earlier call failed");
    if (n == 0)
        return 0;
    msd_frames_view fv;
    int rc = msd_frames_get_view(c, &fv); /* the CRC and repair tables of the group's context */
    if (rc)
        return gfail(g, rc, "%s input: no tables", F::NAME);
    msd_gb_view v{};
    v.format = F::FORMAT;
    v.stream = fv.stream;
    v.device = fv.device;
    v.max_receivers = g->max_receivers;
    v.tables = fv.tables;
    v.d_snaps = g->gpu ? g->d_snaps : nullptr;
    v.remote = g->remote;
    v.state = F::state(g);
    v.err = g->err;
    v.errlen = sizeof g->err;
    std::vector<msd_gr_input> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        GroupReceiver &r = g->rx[e[i].receiver];
        in[i].receiver = e[i].receiver;
        in[i].nbytes = e[i].nbytes;
        in[i].flags = e[i].flags;
        in[i].offset = e[i].offset;
        in[i].now_ms = e[i].now_ms;
        in[i].filter = &r.resolver.filter;
        in[i].nfix = r.opt.nfix_crc;
        in[i].mode_ac = r.mode_ac ? 1 : 0;
        r.history = true; /* the repair level is fixed from here on, as by a buffer */
    }
    rc = msd_gr_accept(&v, bytes, on_device ? 1 : 0, in.data(), n, sink, out, user);
    if (rc)
        c->failed = true;
    return rc;
}

} /* namespace */

extern "C" {

int msd_group_create(const msd_config *cfg, uint32_t max_receivers, msd_group **out)
{
    if (!cfg || !out)
        return -EINVAL;
    *out = nullptr;
    if (max_receivers == 0 || (uint64_t)max_receivers * MSD_CHUNK_SAMPLES > MSD_MAX_BATCH_SAMPLES / 2 ||
        cfg->mode_ac || (cfg->flags & MSD_CFG_DC_FILTER) || cfg->format == MSD_FMT_MAG16 || cfg->sc16q11_table_bits)
        return -EINVAL;
    msd_group *g = new (std::nothrow) msd_group;
    if (!g)
        return -ENOMEM;
    g->gpu = !(cfg->flags & MSD_CFG_HOST_RESOLVE);
    msd_config cc = *cfg;
    cc.max_batch_samples = (uint64_t)max_receivers * MSD_CHUNK_SAMPLES;
    cc.flags |= MSD_CFG_NO_HELPER | MSD_CFG_NO_LEAN; /* synchronous calls over the dense candidate lists */
    if (cc.nfix_crc == 0) /* the single-bit tables always: a receiver may be set to level 1 (the scan gates by level) */
        cc.nfix_crc = 1;
    int rc = msd_create(&cc, &g->ctx);
    if (rc) {
        delete g;
        return rc;
    }
    g->max_receivers = max_receivers;
    const unsigned hw = std::thread::hardware_concurrency();
    g->threads = cfg->resolve_threads > 0 ? (uint32_t)cfg->resolve_threads : std::max(1u, std::min(16u, hw / 8u));
    g->rx = new (std::nothrow) GroupReceiver[max_receivers];
    g->remote = new (std::nothrow) msd_remote_stats[max_receivers]();
    const size_t tail_bytes = (size_t)max_receivers * MSD_HALO_FRONT * g->ctx->bps;
    if (!g->rx || !g->remote || hipMalloc(reinterpret_cast<void **>(&g->d_tails), tail_bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&g->d_ctl), sizeof(uint32_t) * 4 * max_receivers) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&g->h_ctl), sizeof(uint32_t) * 4 * max_receivers, hipHostMallocDefault) != hipSuccess ||
        (g->gpu && (hipMalloc(reinterpret_cast<void **>(&g->d_snaps), sizeof(uint32_t) * MSD_SNAP_WORDS * max_receivers) != hipSuccess ||
                    hipHostMalloc(reinterpret_cast<void **>(&g->h_apply), sizeof(uint32_t) * (3 * (size_t)max_receivers + 1),
                                  hipHostMallocDefault) != hipSuccess ||
                    hipHostMalloc(reinterpret_cast<void **>(&g->h_adds), sizeof(uint32_t) * MSD_RB_MSG_CAP * (size_t)max_receivers,
                                  hipHostMallocDefault) != hipSuccess ||
                    hipHostMalloc(reinterpret_cast<void **>(&g->h_snap), sizeof(uint32_t) * MSD_SNAP_WORDS, hipHostMallocDefault) != hipSuccess))) {
        (void)hipGetLastError();
        msd_group_destroy(g);
        return -ENOMEM;
    }
    for (uint32_t r = 0; r < max_receivers; ++r) {
        g->rx[r].resolver.stats = &g->rx[r].stats;
        g->rx[r].resolver.threads = 1;
        g->rx[r].opt.preamble_threshold = cfg->preamble_threshold;
        g->rx[r].opt.nfix_crc = cfg->nfix_crc;
        group_receiver_reset(g->rx[r]);
        rc = group_upload_snapshot(g, r);
        if (rc) {
            msd_group_destroy(g);
            return rc;
        }
    }
    *out = g;
    return 0;
}

void msd_group_destroy(msd_group *g)
{
    if (!g)
        return;
    if (g->ctx)
        (void)hipSetDevice(g->ctx->cfg.device);
    if (g->rx) {
        for (uint32_t r = 0; r < g->max_receivers; ++r)
            msd_resolver_free(&g->rx[r].resolver);
        delete[] g->rx;
    }
    (void)hipFree(g->d_tails);
    (void)hipFree(g->d_ctl);
    (void)hipHostFree(g->h_ctl);
    (void)hipFree(g->d_snaps);
    (void)hipHostFree(g->h_apply);
    (void)hipHostFree(g->h_adds);
    (void)hipHostFree(g->h_snap);
    (void)hipHostFree(g->h_wire_out);
    (void)hipHostFree(g->h_wire_entries);
    (void)hipFree(g->d_wire_counts);
    msd_gr_free(g->beast);
    msd_gr_free(g->avr);
    delete[] g->remote;
    msd_destroy(g->ctx);
    delete g;
}

const char *msd_group_last_error(const msd_group *g)
{
    return g ? g->err : "no group";
}

int msd_group_submit_device(msd_group *g, const void *d_iq, const msd_group_entry *e, uint32_t n,
                            msd_group_message_fn sink, void *user)
{
    GroupSink to;
    to.sink = sink;
    to.user = user;
    return group_submit(g, d_iq, e, n, false, to);
}

int msd_group_submit_host(msd_group *g, const void *h_iq, const msd_group_entry *e, uint32_t n,
                          msd_group_message_fn sink, void *user)
{
    GroupSink to;
    to.sink = sink;
    to.user = user;
    return group_submit(g, h_iq, e, n, true, to);
}

int msd_group_submit_device_fields(msd_group *g, const void *d_iq, const msd_group_entry *e, uint32_t n,
                                   msd_group_fields_fn sink, void *user)
{
    GroupSink to;
    to.fsink = sink;
    to.user = user;
    to.want_fields = true;
    return group_submit(g, d_iq, e, n, false, to);
}

int msd_group_submit_host_fields(msd_group *g, const void *h_iq, const msd_group_entry *e, uint32_t n,
                                 msd_group_fields_fn sink, void *user)
{
    GroupSink to;
    to.fsink = sink;
    to.user = user;
    to.want_fields = true;
    return group_submit(g, h_iq, e, n, true, to);
}

int msd_group_submit_device_wire(msd_group *g, const void *d_iq, const msd_group_entry *e, uint32_t n, int format,
                                 uint32_t flags, msd_group_wire_fn sink, void *user)
{
    GroupSink to;
    to.wsink = sink;
    to.user = user;
    to.want_wire = true;
    to.wire_format = format;
    to.wire_flags = flags;
    return group_submit(g, d_iq, e, n, false, to);
}

int msd_group_submit_host_wire(msd_group *g, const void *h_iq, const msd_group_entry *e, uint32_t n, int format,
                               uint32_t flags, msd_group_wire_fn sink, void *user)
{
    GroupSink to;
    to.wsink = sink;
    to.user = user;
    to.want_wire = true;
    to.wire_format = format;
    to.wire_flags = flags;
    return group_submit(g, h_iq, e, n, true, to);
}

int msd_group_reset_receiver(msd_group *g, uint32_t receiver)
{
    if (!g || receiver >= g->max_receivers)
        return -EINVAL;
    if (g->ctx->failed)
        return gfail(g, -EIO, "an earlier call failed");
    group_receiver_reset(g->rx[receiver]);
    memset(&g->remote[receiver], 0, sizeof g->remote[receiver]);
    msd_gr_reset_receiver(g->beast, receiver); /* its kept frame and pending gap */
    msd_gr_reset_receiver(g->avr, receiver);   /* its kept line, discard flag and msd_avr_stats */
    const int rc = group_upload_snapshot(g, receiver);
    if (rc)
        g->ctx->failed = true;
    return rc;
}

int msd_group_get_stats(const msd_group *g, uint32_t receiver, msd_stats *st)
{
    if (!g || !st || receiver >= g->max_receivers)
        return -EINVAL;
    *st = g->rx[receiver].stats;
    return 0;
}

int msd_group_set_preamble_threshold(msd_group *g, int threshold)
{
    if (!g)
        return -EINVAL;
    const int rc = msd_set_preamble_threshold(g->ctx, threshold);
    if (rc)
        return gfail(g, rc, "%s", g->ctx->err);
    for (uint32_t r = 0; r < g->max_receivers; ++r)
        g->rx[r].opt.preamble_threshold = threshold;
    return 0;
}

int msd_group_set_receiver_options(msd_group *g, uint32_t receiver, const msd_group_receiver_options *o)
{
    if (!g)
        return -EINVAL;
    if (!o || receiver >= g->max_receivers)
        return gfail(g, -EINVAL, "receiver options: a receiver out of range or no options");
    if (o->preamble_threshold < 1 || o->preamble_threshold > MSD_MAX_PREAMBLE_THRESHOLD || o->nfix_crc < 0 ||
        o->nfix_crc > 2 || o->reserved[0] || o->reserved[1])
        return gfail(g, -EINVAL, "receiver options: threshold %d outside 1..%d, repair level %d outside 0..2, or nonzero "
                     "reserved words", o->preamble_threshold, MSD_MAX_PREAMBLE_THRESHOLD, o->nfix_crc);
    GroupReceiver &r = g->rx[receiver];
    if (o->nfix_crc != r.opt.nfix_crc && r.history) /* readsb cannot change --fix in a running process either */
        return gfail(g, -EBUSY, "receiver %u: the repair level changes only before its first buffer (after a reset)",
                     receiver);
    if (o->nfix_crc == 2) {
        const int rc = group_make_fix2(g);
        if (rc)
            return rc;
    }
    r.opt.preamble_threshold = o->preamble_threshold;
    r.opt.nfix_crc = o->nfix_crc;
    return 0;
}

int msd_group_get_receiver_options(const msd_group *g, uint32_t receiver, msd_group_receiver_options *o)
{
    if (!g || !o || receiver >= g->max_receivers)
        return -EINVAL;
    *o = g->rx[receiver].opt;
    return 0;
}

int msd_group_set_receiver_mode_ac(msd_group *g, uint32_t receiver, int on)
{
    if (!g)
        return -EINVAL;
    if (receiver >= g->max_receivers || (on != 0 && on != 1))
        return gfail(g, -EINVAL, "Mode A/C: receiver %u out of range or switch %d not 0 or 1", receiver, on);
    if (on) {
        const int rc = group_make_ac(g);
        if (rc)
            return rc;
    }
    g->rx[receiver].mode_ac = on != 0;
    return 0;
}

int msd_group_get_receiver_mode_ac(const msd_group *g, uint32_t receiver, int *on)
{
    if (!g || !on || receiver >= g->max_receivers)
        return -EINVAL;
    *on = g->rx[receiver].mode_ac ? 1 : 0;
    return 0;
}

int msd_group_get_timing(const msd_group *g, msd_timing *t)
{
    if (!g)
        return -EINVAL;
    return msd_get_timing(g->ctx, t);
}

int msd_group_accept_beast(msd_group *g, const void *bytes, int on_device, const msd_group_beast_entry *e, uint32_t n,
                           msd_group_message_fn sink, void *user)
{
    return group_accept_remote(g, bytes, on_device, e, n, sink, nullptr, user);
}

int msd_group_accept_beast_fields(msd_group *g, const void *bytes, int on_device, const msd_group_beast_entry *e, uint32_t n,
                                  msd_group_fields_fn sink, void *user)
{
    const msd_gb_out o = fields_out(sink);
    return group_accept_remote(g, bytes, on_device, e, n, nullptr, &o, user);
}

int msd_group_accept_beast_wire(msd_group *g, const void *bytes, int on_device, const msd_group_beast_entry *e, uint32_t n,
                                int format, uint32_t flags, msd_group_wire_fn sink, void *user)
{
    const msd_gb_out o = wire_out(format, flags, sink);
    return group_accept_remote(g, bytes, on_device, e, n, nullptr, &o, user);
}

int msd_group_get_remote_stats(const msd_group *g, uint32_t receiver, msd_remote_stats *st)
{
    if (!g || !st || receiver >= g->max_receivers)
        return -EINVAL;
    *st = g->remote[receiver];
    return 0;
}

int msd_group_accept_avr(msd_group *g, const void *bytes, int on_device, const msd_group_avr_entry *e, uint32_t n,
                         msd_group_message_fn sink, void *user)
{
    return group_accept_remote(g, bytes, on_device, e, n, sink, nullptr, user);
}

int msd_group_accept_avr_fields(msd_group *g, const void *bytes, int on_device, const msd_group_avr_entry *e, uint32_t n,
                                msd_group_fields_fn sink, void *user)
{
    const msd_gb_out o = fields_out(sink);
    return group_accept_remote(g, bytes, on_device, e, n, nullptr, &o, user);
}

int msd_group_accept_avr_wire(msd_group *g, const void *bytes, int on_device, const msd_group_avr_entry *e, uint32_t n,
                              int format, uint32_t flags, msd_group_wire_fn sink, void *user)
{
    const msd_gb_out o = wire_out(format, flags, sink);
    return group_accept_remote(g, bytes, on_device, e, n, nullptr, &o, user);
}

int msd_group_get_avr_stats(const msd_group *g, uint32_t receiver, msd_avr_stats *st)
{
    if (!g || !st || receiver >= g->max_receivers)
        return -EINVAL;
    msd_gr_get_avr_stats(g->avr, receiver, st);
    return 0;
}

} /* extern "C" */
