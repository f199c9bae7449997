/*
 * msd_frames.cpp -- host side of the Beast / AVR input (msd_accept_beast, msd_accept_frames, msd_accept_avr,
 * msd_get_remote_stats, msd_get_avr_stats): pieces, device scratch, the three launches of msd_frames_kernels.hip per
 * piece (AVR text: the framing launches of msd_avr_kernels.hip in front of the records path's), and what stays on the
 * host -- the kept incomplete frame or line, the pending gap, the context's ICAO filter (the device inserts a piece's
 * new addresses into a copy; the same inserts are repeated here, in the same order) and the counters.  DESIGN.md 4.8.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "modes_hip.h"
#include "msd_avr.h"
#include "msd_frames.h"
#include "msd_internal.h"

namespace {

constexpr uint32_t RECORDS_PIECE = 1u << 20; /* msd_accept_frames: records per piece */

struct Buf {
    void *p = nullptr;
    size_t cap = 0;
};

struct State {
    uint8_t tail[MSD_FR_TAIL_MAX];
    uint32_t tl = 0;
    uint64_t pending_gap = 0;
    msd_remote_stats rs{};
    Buf stage, tailbuf, succ, info, mark, first, exitl, entry, good, cnt, nodes, cls, addr, flags, scan_tmp, newlist,
        newaddr, hash, out, snap, in, ctr;
    unsigned long long *h_ctr = nullptr;
    uint32_t *h_snap = nullptr;
    std::vector<msd_message> recs;
    std::vector<uint32_t> newaddr_h;
    /* msd_accept_avr: the incomplete line, or the flag that an overlong one is being discarded */
    uint8_t avr_tail[MSD_AVR_LINE_MAX];
    uint32_t avr_tl = 0;
    int avr_discard = 0;
    msd_avr_stats as{};
    Buf avr_tailbuf, avr_wg, avr_rec;
};

int fail(const msd_frames_view &v, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(v.err, v.errlen, fmt, ap);
    va_end(ap);
    return code;
}

#define HCK(v, call)                                                                                                   \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return fail((v), -EIO, "%s failed: %s", #call, hipGetErrorString(e_));                                     \
    } while (0)

int grow(const msd_frames_view &v, Buf &b, size_t bytes)
{
    if (b.cap >= bytes)
        return 0;
    (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    size_t cap = bytes + bytes / 4 + 256;
    HCK(v, hipMalloc(&b.p, cap));
    b.cap = cap;
    return 0;
}

template <class T> T *as(Buf &b)
{
    return static_cast<T *>(b.p);
}

int get_state(const msd_frames_view &v, State **out)
{
    State *s = static_cast<State *>(*v.state);
    if (!s) {
        s = new (std::nothrow) State();
        if (!s)
            return fail(v, -ENOMEM, "out of host memory");
        if (hipHostMalloc(reinterpret_cast<void **>(&s->h_ctr), sizeof(unsigned long long) * MSD_FR_CTR_WORDS) !=
                hipSuccess ||
            hipHostMalloc(reinterpret_cast<void **>(&s->h_snap), sizeof(uint32_t) * MSD_SNAP_WORDS) != hipSuccess) {
            msd_frames_free(s);
            return fail(v, -ENOMEM, "hipHostMalloc failed");
        }
        *v.state = s;
    }
    *out = s;
    return 0;
}

/* scratch for a piece of nbytes bytes (0: the records path) holding up to nitems nodes / records */
int ensure(const msd_frames_view &v, State &s, uint32_t nbytes, uint32_t nitems)
{
    int rc = 0;
    const uint32_t ntiles = (nbytes + MSD_FR_TILE - 1u) / MSD_FR_TILE;
    const size_t words = (size_t)(nbytes > nitems ? nbytes : nitems) + 2;
    if (nbytes) {
        if ((rc = grow(v, s.succ, sizeof(uint32_t) * nbytes)) || (rc = grow(v, s.info, sizeof(uint16_t) * nbytes)) ||
            (rc = grow(v, s.mark, nbytes)) || (rc = grow(v, s.first, sizeof(uint32_t) * (ntiles + 1))) ||
            (rc = grow(v, s.exitl, sizeof(uint32_t) * (ntiles + 1))) ||
            (rc = grow(v, s.entry, sizeof(uint32_t) * (ntiles + 1))) || (rc = grow(v, s.good, ntiles + 1)))
            return rc;
    }
    if ((rc = grow(v, s.cnt, sizeof(uint32_t) * words)) || (rc = grow(v, s.nodes, sizeof(uint32_t) * words)) ||
        (rc = grow(v, s.cls, words)) || (rc = grow(v, s.addr, sizeof(uint32_t) * words)) ||
        (rc = grow(v, s.flags, sizeof(uint32_t) * words)) ||
        (rc = grow(v, s.scan_tmp, sizeof(uint32_t) * msd_fr_scan_tmp_words((uint32_t)words))) ||
        (rc = grow(v, s.newlist, sizeof(uint32_t) * (nitems + 1))) ||
        (rc = grow(v, s.newaddr, sizeof(uint32_t) * (nitems + 1))) ||
        (rc = grow(v, s.out, sizeof(msd_message) * (nitems + 1))) || (rc = grow(v, s.snap, sizeof(uint32_t) * MSD_SNAP_WORDS)) ||
        (rc = grow(v, s.tailbuf, MSD_FR_TAIL_MAX)) ||
        (rc = grow(v, s.ctr, sizeof(unsigned long long) * MSD_FR_CTR_WORDS)))
        return rc;
    return 0;
}

msd_fr_scratch scratch(State &s)
{
    msd_fr_scratch x{};
    x.succ = as<uint32_t>(s.succ);
    x.info = as<uint16_t>(s.info);
    x.mark = as<uint8_t>(s.mark);
    x.first = as<uint32_t>(s.first);
    x.exitl = as<uint32_t>(s.exitl);
    x.entry = as<uint32_t>(s.entry);
    x.good = as<uint8_t>(s.good);
    x.cnt = as<uint32_t>(s.cnt);
    x.nodes = as<uint32_t>(s.nodes);
    x.cls = as<uint8_t>(s.cls);
    x.addr = as<uint32_t>(s.addr);
    x.flags = as<uint32_t>(s.flags);
    x.scan_tmp = as<uint32_t>(s.scan_tmp);
    x.newlist = as<uint32_t>(s.newlist);
    x.newaddr = as<uint32_t>(s.newaddr);
    x.hash = as<uint32_t>(s.hash);
    x.snap = as<uint32_t>(s.snap);
    x.out = as<msd_message>(s.out);
    x.ctr = as<unsigned long long>(s.ctr);
    return x;
}

/* the live filter as a snapshot (MSD_SNAP_WORDS, the two tables interleaved, as the resolve kernel reads them) */
int upload_filter(const msd_frames_view &v, State &s, hipStream_t st)
{
    const msd_filter *f = v.filter;
    for (uint32_t h = 0; h < 8192; ++h) {
        s.h_snap[2 * h] = f->slot[0][h];
        s.h_snap[2 * h + 1] = f->slot[1][h];
    }
    s.h_snap[16384] = (uint32_t)f->active;
    HCK(v, hipMemcpyAsync(s.snap.p, s.h_snap, sizeof(uint32_t) * MSD_SNAP_WORDS, hipMemcpyHostToDevice, st));
    return 0;
}

int read_ctr(const msd_frames_view &v, State &s, hipStream_t st)
{
    HCK(v, hipMemcpyAsync(s.h_ctr, s.ctr.p, sizeof(unsigned long long) * MSD_FR_CTR_WORDS, hipMemcpyDeviceToHost, st));
    HCK(v, hipStreamSynchronize(st));
    return 0;
}

/* the add table of a piece: a power of two >= 2 * adds slots, all vacant */
int prepare_hash(const msd_frames_view &v, State &s, uint32_t nadds, hipStream_t st, msd_fr_scratch &x)
{
    uint32_t hs = 64;
    while (hs < 2u * nadds)
        hs <<= 1;
    int rc = grow(v, s.hash, (size_t)16 * hs);
    if (rc)
        return rc;
    HCK(v, hipMemsetAsync(s.hash.p, 0xff, (size_t)16 * hs, st));
    x.hash = as<uint32_t>(s.hash);
    x.hslots = hs;
    return 0;
}

/* decode, filter and finish n records in device memory: what both msd_accept_frames and msd_accept_avr do to a piece */
int finish_piece(const msd_frames_view &v, State &s, hipStream_t st, msd_message_fn sink, void *user);
int decide_records(const msd_frames_view &v, State &s, const msd_message *d_in, uint32_t n, uint64_t now_ms,
                   hipStream_t st, msd_message_fn sink, void *user)
{
    int rc;
    if ((rc = upload_filter(v, s, st)))
        return rc;
    msd_fr_scratch x = scratch(s);
    if ((rc = msd_fr_launch_records_decode(d_in, n, &v.tables, &x, st)))
        return fail(v, rc, "decode kernel failed to launch");
    if ((rc = read_ctr(v, s, st)))
        return rc;
    const uint32_t nadds = (uint32_t)s.h_ctr[MSD_FR_CTR_ADDS];
    if (nadds && (rc = prepare_hash(v, s, nadds, st, x)))
        return rc;
    if ((rc = msd_fr_launch_records_filter(d_in, n, nadds, now_ms, &v.tables, &x, st)))
        return fail(v, rc, "filter kernels failed to launch");
    return finish_piece(v, s, st, sink, user);
}

/* after stage 3: records and new addresses to the host; the filter, the counters, the sink */
int finish_piece(const msd_frames_view &v, State &s, hipStream_t st, msd_message_fn sink, void *user)
{
    int rc = read_ctr(v, s, st);
    if (rc)
        return rc;
    const unsigned long long *c = s.h_ctr;
    const uint32_t nrec = (uint32_t)c[MSD_FR_CTR_RECORDS], nnew = (uint32_t)c[MSD_FR_CTR_NEW];
    s.recs.resize(nrec);
    s.newaddr_h.resize(nnew);
    if (nrec)
        HCK(v, hipMemcpyAsync(s.recs.data(), s.out.p, sizeof(msd_message) * nrec, hipMemcpyDeviceToHost, st));
    if (nnew)
        HCK(v, hipMemcpyAsync(s.newaddr_h.data(), s.newaddr.p, sizeof(uint32_t) * nnew, hipMemcpyDeviceToHost, st));
    HCK(v, hipStreamSynchronize(st));
    /* icaoFilterAdd of the piece's new addresses in order of first add: the device's copy had the same inserts */
    for (uint32_t a : s.newaddr_h)
        msd_filter_add(v.filter, a);
    msd_remote_stats &r = s.rs;
    r.remote_received_modes += c[MSD_FR_CTR_MODES];
    r.remote_received_modeac += c[MSD_FR_CTR_MODEAC];
    r.remote_rejected_bad += c[MSD_FR_CTR_BAD];
    r.remote_rejected_unknown_icao += c[MSD_FR_CTR_UNKNOWN];
    for (int i = 0; i < 3; ++i)
        r.remote_accepted[i] += c[MSD_FR_CTR_ACC0 + i];
    r.frames += c[MSD_FR_CTR_FRAMES];
    r.other_frames += c[MSD_FR_CTR_OTHER];
    r.garbage_bytes += c[MSD_FR_CTR_GARBAGE];
    r.tile_rewalks += c[MSD_FR_CTR_REWALKS];
    if (sink)
        for (const msd_message &m : s.recs)
            sink(&m, user);
    return 0;
}

int enter(msd_ctx *ctx, msd_frames_view &v, State **s)
{
    int rc = msd_frames_get_view(ctx, &v);
    if (rc)
        return rc;
    if (v.failed)
        return fail(v, -EIO, "a batch could not be finished: msd_reset first");
    if (v.busy)
        return fail(v, -EBUSY, "batches outstanding");
    HCK(v, hipSetDevice(v.device));
    return get_state(v, s);
}

} // namespace

extern "C" {

void msd_frames_free(void *state)
{
    State *s = static_cast<State *>(state);
    if (!s)
        return;
    Buf *all[] = {&s->stage, &s->tailbuf, &s->succ, &s->info, &s->mark, &s->first, &s->exitl, &s->entry, &s->good,
                  &s->cnt, &s->nodes, &s->cls, &s->addr, &s->flags, &s->scan_tmp, &s->newlist, &s->newaddr, &s->hash,
                  &s->out, &s->snap, &s->in, &s->ctr, &s->avr_tailbuf, &s->avr_wg, &s->avr_rec};
    for (Buf *b : all)
        (void)hipFree(b->p);
    if (s->h_ctr)
        (void)hipHostFree(s->h_ctr);
    if (s->h_snap)
        (void)hipHostFree(s->h_snap);
    delete s;
}

void msd_frames_reset(void *state)
{
    State *s = static_cast<State *>(state);
    if (!s)
        return;
    s->tl = 0;
    s->pending_gap = 0;
    memset(&s->rs, 0, sizeof s->rs);
    s->avr_tl = 0;
    s->avr_discard = 0;
    memset(&s->as, 0, sizeof s->as);
}

int msd_get_remote_stats(const msd_ctx *ctx, msd_remote_stats *st)
{
    if (!ctx || !st)
        return -EINVAL;
    msd_frames_view v;
    int rc = msd_frames_get_view(const_cast<msd_ctx *>(ctx), &v);
    if (rc)
        return rc;
    const State *s = static_cast<const State *>(*v.state);
    if (s)
        *st = s->rs;
    else
        memset(st, 0, sizeof *st);
    return 0;
}

int msd_accept_beast(msd_ctx *ctx, const void *bytes, size_t n, int on_device, uint64_t now_ms, msd_message_fn sink,
                     void *user)
{
    if (!ctx || (n && !bytes))
        return -EINVAL;
    msd_frames_view v;
    State *s = nullptr;
    int rc = enter(ctx, v, &s);
    if (rc)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(v.stream);
    const uint8_t *src = static_cast<const uint8_t *>(bytes);
    for (size_t pos = 0; pos < n;) {
        const uint32_t take = (uint32_t)(n - pos < MSD_FR_PIECE ? n - pos : MSD_FR_PIECE);
        const uint32_t tl = s->tl, total = tl + take;
        if ((rc = ensure(v, *s, total, total / 11u + 2u))) /* a message frame takes at least 11 bytes */
            return rc;
        const uint8_t *d_data = src + pos;
        if (!on_device) {
            if ((rc = grow(v, s->stage, take)))
                return rc;
            HCK(v, hipMemcpyAsync(s->stage.p, src + pos, take, hipMemcpyHostToDevice, st));
            d_data = as<uint8_t>(s->stage);
        }
        if (tl)
            HCK(v, hipMemcpyAsync(s->tailbuf.p, s->tail, tl, hipMemcpyHostToDevice, st));
        if ((rc = upload_filter(v, *s, st)))
            return rc;
        msd_fr_scratch x = scratch(*s);
        const uint8_t *d_tail = as<uint8_t>(s->tailbuf);
        if ((rc = msd_fr_launch_chain(d_tail, tl, d_data, total, &x, st)))
            return fail(v, rc, "chain kernels failed to launch");
        if ((rc = read_ctr(v, *s, st)))
            return rc;
        const uint32_t nnodes = (uint32_t)s->h_ctr[MSD_FR_CTR_NODES];
        if ((rc = msd_fr_launch_decode(d_tail, tl, d_data, total, nnodes, s->pending_gap, &v.tables, &x, st)))
            return fail(v, rc, "decode kernel failed to launch");
        if ((rc = read_ctr(v, *s, st)))
            return rc;
        const uint32_t nadds = (uint32_t)s->h_ctr[MSD_FR_CTR_ADDS];
        const uint64_t exit_v = s->h_ctr[MSD_FR_CTR_EXIT], last_end = s->h_ctr[MSD_FR_CTR_LAST_END];
        if (nadds && (rc = prepare_hash(v, *s, nadds, st, x)))
            return rc;
        if ((rc = msd_fr_launch_filter(d_tail, tl, d_data, total, nnodes, nadds, now_ms, &v.tables, &x, st)))
            return fail(v, rc, "filter kernels failed to launch");
        /* what the next piece starts with: the incomplete frame, or the bytes since the last frame counted as a gap */
        uint8_t newtail[MSD_FR_TAIL_MAX];
        uint32_t ntl = 0;
        if (exit_v & MSD_FR_INC) {
            const uint32_t q = (uint32_t)(exit_v & ~(uint64_t)MSD_FR_INC);
            if (total - q > MSD_FR_TAIL_MAX)
                return fail(v, -EIO, "incomplete frame of %u bytes", total - q);
            for (uint32_t i = q; i < tl; ++i)
                newtail[ntl++] = s->tail[i];
            const uint32_t from = q > tl ? q - tl : 0;
            if (take > from) {
                HCK(v, hipMemcpyAsync(newtail + ntl, d_data + from, take - from, hipMemcpyDeviceToHost, st));
                ntl += take - from;
            }
        }
        if ((rc = finish_piece(v, *s, st, sink, user)))
            return rc;
        memcpy(s->tail, newtail, ntl);
        s->tl = ntl;
        if (!(exit_v & MSD_FR_INC))
            s->pending_gap = (nnodes ? 0 : s->pending_gap) + (total - last_end);
        else
            s->pending_gap = 0;
        pos += take;
    }
    msd_filter_expire(v.filter, now_ms); /* readsb.c:331 */
    return 0;
}

int msd_accept_frames(msd_ctx *ctx, const msd_message *frames, size_t n, int on_device, uint64_t now_ms,
                      msd_message_fn sink, void *user)
{
    if (!ctx || (n && !frames))
        return -EINVAL;
    msd_frames_view v;
    State *s = nullptr;
    int rc = enter(ctx, v, &s);
    if (rc)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(v.stream);
    for (size_t pos = 0; pos < n;) {
        const uint32_t take = (uint32_t)(n - pos < RECORDS_PIECE ? n - pos : RECORDS_PIECE);
        if ((rc = ensure(v, *s, 0, take)))
            return rc;
        const msd_message *d_in = frames + pos;
        if (!on_device) {
            if ((rc = grow(v, s->in, sizeof(msd_message) * take)))
                return rc;
            HCK(v, hipMemcpyAsync(s->in.p, frames + pos, sizeof(msd_message) * take, hipMemcpyHostToDevice, st));
            d_in = as<msd_message>(s->in);
        }
        if ((rc = decide_records(v, *s, d_in, take, now_ms, st, sink, user)))
            return rc;
        pos += take;
    }
    msd_filter_expire(v.filter, now_ms); /* readsb.c:331 */
    return 0;
}

int msd_get_avr_stats(const msd_ctx *ctx, msd_avr_stats *st)
{
    if (!ctx || !st)
        return -EINVAL;
    msd_frames_view v;
    int rc = msd_frames_get_view(const_cast<msd_ctx *>(ctx), &v);
    if (rc)
        return rc;
    const State *s = static_cast<const State *>(*v.state);
    if (s)
        *st = s->as;
    else
        memset(st, 0, sizeof *st);
    return 0;
}

int msd_accept_avr(msd_ctx *ctx, const void *bytes, size_t n, int on_device, uint32_t flags, uint64_t now_ms,
                   msd_message_fn sink, void *user)
{
    if (!ctx || (n && !bytes) || (flags & ~MSD_AVR_KEEP_TIMESTAMP))
        return -EINVAL;
    msd_frames_view v;
    State *s = nullptr;
    int rc = enter(ctx, v, &s);
    if (rc)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(v.stream);
    const uint8_t *src = static_cast<const uint8_t *>(bytes);
    const int keep = (flags & MSD_AVR_KEEP_TIMESTAMP) != 0;
    for (size_t pos = 0; pos < n;) {
        const uint32_t take = (uint32_t)(n - pos < MSD_FR_PIECE ? n - pos : MSD_FR_PIECE);
        const uint32_t tl = s->avr_tl, total = tl + take;
        const uint32_t spans = (total + MSD_AVR_SPAN - 1u) / MSD_AVR_SPAN;
        if ((rc = ensure(v, *s, 0, 0)) || (rc = grow(v, s->avr_tailbuf, MSD_AVR_LINE_MAX)) ||
            (rc = grow(v, s->avr_wg, sizeof(uint32_t) * (spans + 1))))
            return rc;
        const uint8_t *d_data = src + pos;
        if (!on_device) {
            if ((rc = grow(v, s->stage, take)))
                return rc;
            HCK(v, hipMemcpyAsync(s->stage.p, src + pos, take, hipMemcpyHostToDevice, st));
            d_data = as<uint8_t>(s->stage);
        }
        if (tl)
            HCK(v, hipMemcpyAsync(s->avr_tailbuf.p, s->avr_tail, tl, hipMemcpyHostToDevice, st));
        const uint8_t *d_tail = as<uint8_t>(s->avr_tailbuf);
        const int discard = s->avr_discard;
        if ((rc = msd_avr_launch_count(d_tail, tl, d_data, total, discard, v.tables.mode_ac, as<uint32_t>(s->avr_wg),
                                       as<unsigned long long>(s->ctr), st)))
            return fail(v, rc, "line kernels failed to launch");
        if ((rc = read_ctr(v, *s, st)))
            return rc;
        const uint32_t nrec = (uint32_t)s->h_ctr[MSD_AVR_CTR_RECORDS];
        const uint64_t lines = s->h_ctr[MSD_AVR_CTR_LINES], dropped = s->h_ctr[MSD_AVR_CTR_DROPPED],
                       longl = s->h_ctr[MSD_AVR_CTR_LONG];
        const uint32_t from = (uint32_t)s->h_ctr[MSD_AVR_CTR_LAST_NL]; /* where the incomplete line starts */
        /* what the next piece starts with: the bytes behind the last '\n', unless they are too many already */
        uint8_t newtail[MSD_AVR_LINE_MAX];
        uint32_t ntl = 0;
        int ndiscard = from ? 0 : discard;
        if (!ndiscard && total - from > MSD_AVR_LINE_MAX)
            ndiscard = 1;
        if (!ndiscard) {
            for (uint32_t i = from; i < tl; ++i)
                newtail[ntl++] = s->avr_tail[i];
            const uint32_t dfrom = from > tl ? from - tl : 0;
            if (take > dfrom) {
                if (on_device) {
                    HCK(v, hipMemcpyAsync(newtail + ntl, d_data + dfrom, take - dfrom, hipMemcpyDeviceToHost, st));
                    HCK(v, hipStreamSynchronize(st));
                } else {
                    memcpy(newtail + ntl, src + pos + dfrom, take - dfrom);
                }
                ntl += take - dfrom;
            }
        }
        if (nrec) {
            if ((rc = ensure(v, *s, 0, nrec)) || (rc = grow(v, s->avr_rec, sizeof(msd_message) * nrec)))
                return rc;
            if ((rc = msd_avr_launch_store(d_tail, tl, d_data, total, discard, v.tables.mode_ac, keep,
                                           as<uint32_t>(s->avr_wg), as<msd_message>(s->avr_rec), st)))
                return fail(v, rc, "line store kernel failed to launch");
            if ((rc = decide_records(v, *s, as<msd_message>(s->avr_rec), nrec, now_ms, st, sink, user)))
                return rc;
        }
        memcpy(s->avr_tail, newtail, ntl);
        s->avr_tl = ntl;
        s->avr_discard = ndiscard;
        s->as.lines += lines;
        s->as.frames += nrec;
        s->as.dropped_lines += dropped;
        s->as.long_lines += longl;
        pos += take;
    }
    msd_filter_expire(v.filter, now_ms); /* readsb.c:331 */
    return 0;
}

} // extern "C"
