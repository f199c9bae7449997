/*
 * msd_group_remote.cpp -- host side of msd_group_accept_beast and msd_group_accept_avr ("Beast input per
 * receiver", "AVR text input per receiver"): one driver for both formats.  It cuts a call into pieces of whole entries,
 * keeps the device scratch (made by the first call of a format), launches the format's first stage
 * (msd_group_beast_kernels.hip or msd_group_avr_kernels.hip) and the filter stage they share, and keeps what stays on the
 * host per receiver: the format's carry (struct Beast, struct Avr below) and the host copy of the ICAO filter, on which
 * every entry's new addresses are inserted again in the device's order before the flip.  The remote counters are the
 * group's (msd_gb_view.remote): both formats add to the same ones.  A piece costs two host synchronisations and a fixed
 * number of launches and copies, whatever its number of entries.
 *
 * A format is a traits type: NAME, KEEP (the bytes a receiver can carry into its next entry), OUT_BY_CAND, Rx (the
 * carry), and entry / scratch / launch_decode / check_totals / launch_filter / check_carry / commit.
 */
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "msd_group_avr.h"
#include "msd_kernels.h"

namespace {

struct Buf { /* device or page-locked host memory, grown to the largest piece seen and released with its owner */
    void *p = nullptr;
    size_t cap = 0;
    const bool pinned;
    explicit Buf(bool pinned_ = false) : pinned(pinned_) {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    void release()
    {
        if (pinned)
            (void)hipHostFree(p);
        else
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

int fail(const msd_gb_view *v, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(v->err, v->errlen, fmt, ap);
    va_end(ap);
    return code;
}

#define HCK(v, call)                                                                                                   \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return fail((v), -EIO, "%s failed: %s", #call, hipGetErrorString(e_));                                     \
    } while (0)

int grow(const msd_gb_view *v, Buf &b, size_t bytes)
{
    if (b.cap >= bytes)
        return 0;
    b.release();
    const size_t cap = bytes + bytes / 4 + 256;
    const hipError_t e = b.pinned ? hipHostMalloc(&b.p, cap, hipHostMallocDefault) : hipMalloc(&b.p, cap);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(v, -ENOMEM, "remote input scratch: %zu bytes of %s memory: %s", cap, b.pinned ? "page-locked" : "device",
                    hipGetErrorString(e));
    }
    b.cap = cap;
    return 0;
}

template <class T> T *as(Buf &b)
{
    return static_cast<T *>(b.p);
}

size_t up8(size_t x)
{
    return (x + 7u) & ~(size_t)7u;
}

/* the filter as a snapshot: MSD_SNAP_WORDS words, the two tables interleaved, then the active one */
void snapshot_of(const msd_filter *f, uint32_t *h)
{
    for (uint32_t k = 0; k < 8192; ++k) {
        h[2 * k] = f->slot[0][k];
        h[2 * k + 1] = f->slot[1][k];
    }
    h[16384] = (uint32_t)f->active;
}

/* a piece's counter row into its receiver's remote counters */
void add_remote(msd_remote_stats &rs, const unsigned long long *c)
{
    rs.remote_received_modes += c[MSD_FR_CTR_MODES];
    rs.remote_received_modeac += c[MSD_FR_CTR_MODEAC];
    rs.remote_rejected_bad += c[MSD_FR_CTR_BAD];
    rs.remote_rejected_unknown_icao += c[MSD_FR_CTR_UNKNOWN];
    for (int k = 0; k < 3; ++k)
        rs.remote_accepted[k] += c[MSD_FR_CTR_ACC0 + k];
    rs.frames += c[MSD_FR_CTR_FRAMES];
    rs.other_frames += c[MSD_FR_CTR_OTHER];
    rs.garbage_bytes += c[MSD_FR_CTR_GARBAGE];
    rs.tile_rewalks += c[MSD_FR_CTR_REWALKS];
}

/* ---- the output stage of a fields or wire call (msd_group_remote_out_kernels.hip) ---- */
struct OutBufs {
    Buf fields, lens, sums, starts, errbits;
    Buf h_fields{true}, h_wire{true}, h_ranges{true};
};

/* Before the filter stage of a verbatim wire call: where its records kernel leaves the repaired bit positions of the
 * piece's at most ncand records; NULL (and 0) for every other call */
int out_errbits(const msd_gb_view *v, OutBufs &ob, const msd_gb_out *o, uint32_t ncand, uint8_t **errbits)
{
    *errbits = nullptr;
    if (!o || !o->want_wire || !o->verbatim)
        return 0;
    if (int rc = grow(v, ob.errbits, 2 * ((size_t)ncand + 1)))
        return rc;
    *errbits = as<uint8_t>(ob.errbits);
    return 0;
}

/* Queued between the filter stage and the piece's second synchronisation: d_out[0 .. *d_count) are the piece's records,
 * ncand (> 0) the host's bound of their number, d_ctr the n entries' counter rows, errbits what out_errbits gave the
 * filter stage.  The fields cross in a copy of that synchronisation; the wire bytes and the entries' ranges are written
 * to page-locked memory by the kernels. */
int out_queue(const msd_gb_view *v, OutBufs &ob, const msd_gb_out &o, const msd_message *d_out, const uint32_t *d_count,
              uint32_t ncand, const unsigned long long *d_ctr, uint32_t n, const uint8_t *errbits, hipStream_t st)
{
    int rc = 0;
    if (o.want_fields) {
        if ((rc = grow(v, ob.fields, sizeof(msd_fields) * (size_t)ncand)) ||
            (rc = grow(v, ob.h_fields, sizeof(msd_fields) * (size_t)ncand)))
            return rc;
        if ((rc = msd_gro_launch_fields(d_out, d_count, ncand, as<msd_fields>(ob.fields), st)))
            return fail(v, rc, "remote input: fields kernel failed to launch");
        HCK(v, hipMemcpyAsync(ob.h_fields.p, ob.fields.p, sizeof(msd_fields) * (size_t)ncand, hipMemcpyDeviceToHost, st));
    }
    if (o.want_wire) {
        if ((rc = grow(v, ob.lens, ncand)) || (rc = grow(v, ob.sums, 4 * ((size_t)ncand / 256u + 2))) ||
            (rc = grow(v, ob.starts, 4 * (size_t)ncand)) || (rc = grow(v, ob.h_wire, (size_t)MSD_GRO_WIRE_MAX * ncand)) ||
            (rc = grow(v, ob.h_ranges, 8 * (size_t)n)))
            return rc;
        if ((rc = msd_gro_launch_wire(d_out, d_count, ncand, d_ctr, n, o.format, errbits, as<uint8_t>(ob.lens),
                                      as<uint32_t>(ob.sums), as<uint32_t>(ob.starts), as<uint8_t>(ob.h_wire),
                                      as<uint32_t>(ob.h_ranges), st)))
            return fail(v, rc, "remote input: wire kernels failed to launch");
    }
    return 0;
}

/* after the second synchronisation, before anything is committed: entry e's range lies in what a piece of ncand
 * records can have written (queued: out_queue ran for this piece) */
bool out_range_ok(OutBufs &ob, const msd_gb_out &o, bool queued, uint32_t e, uint32_t ncand)
{
    if (!o.want_wire || !queued)
        return true;
    const uint32_t *r = as<uint32_t>(ob.h_ranges) + 2 * (size_t)e;
    return r[1] != 0xffffffffu && (size_t)r[0] + r[1] <= (size_t)MSD_GRO_WIRE_MAX * ncand;
}

/* entry e's delivery: its records [first, first + nrec) of the piece with their fields, or its bytes in one call */
void out_deliver(OutBufs &ob, const msd_gb_out &o, bool queued, uint32_t receiver, uint32_t e, const msd_message *recs,
                 uint32_t first, uint32_t nrec, void *user)
{
    if (o.want_fields && o.fsink)
        for (uint32_t k = 0; k < nrec; ++k)
            o.fsink(receiver, recs + first + k, as<msd_fields>(ob.h_fields) + first + k, user);
    if (o.want_wire && o.wsink) {
        static const uint8_t nothing[1] = {0};
        if (queued) {
            const uint32_t *r = as<uint32_t>(ob.h_ranges) + 2 * (size_t)e;
            o.wsink(receiver, as<uint8_t>(ob.h_wire) + r[0], r[1], nrec, user);
        } else { /* a piece without records ran no kernel */
            o.wsink(receiver, nothing, 0, 0, user);
        }
    }
}

/* ---- the driver's state: one per format and group; *msd_gb_view.state points to its Bufs ---- */
struct Bufs {
    const int format; /* MSD_GR_*: which State it is part of */
    explicit Bufs(int format_) : format(format_) {}
    Buf up, buf, cnt, nodes, cls, addr, flags, off, scan_tmp, newlist, newaddr, hash, snaps, add_first, out, ctr, tot,
        keep_out, stage;
    Buf first, nxt, succ, info, mark, exitl, entry, good; /* the chain walk: Beast only */
    Buf rec;                                              /* the parsed lines: AVR only */
    Buf h_up{true}, h_ctr{true}, h_tot{true}, h_keep{true}, h_out{true}, h_new{true}, h_stage{true}, h_snaps{true};
    OutBufs ob; /* of the fields and wire calls, made by the first of them */
};

template <class F> struct State : Bufs {
    State() : Bufs(F::FORMAT) {}
    std::vector<typename F::Rx> rx;
};

template <class F> State<F> *state_of(const void *state)
{
    return static_cast<State<F> *>(static_cast<Bufs *>(const_cast<void *>(state)));
}

struct Beast {
    static constexpr int FORMAT = MSD_GR_BEAST;
    static constexpr const char *NAME = "Beast";
    static constexpr uint32_t KEEP = MSD_FR_TAIL_MAX;
    static constexpr bool OUT_BY_CAND = false; /* `out` is sized with the scratch, before the first synchronisation */
    struct Rx {
        uint8_t keep[KEEP]; /* the incomplete frame */
        uint32_t tl = 0;
        uint64_t pending_gap = 0;
    };

    static void entry(const Rx &r, const msd_gr_input &, msd_gb_entry &E)
    {
        E.pending_gap = r.pending_gap;
    }

    /* by the bytes of the piece (every byte can be a node), the records by its shortest frame (11 bytes).  Beside these,
     * run_piece grows for both formats: up, stage, snaps, keep_out, add_first, ctr, tot, hash and the page-locked h_* */
    static int scratch(const msd_gb_view *v, Bufs &s, const uint8_t *keep_in, msd_ga_scratch &x, size_t *nrec_max)
    {
        const uint32_t ntiles = x.f.ntiles;
        const size_t words = (size_t)x.f.len + 2, nrec = (size_t)x.f.len / 11u + 2;
        int rc = 0;
        if ((rc = grow(v, s.buf, x.f.len + 16)) || (rc = grow(v, s.first, 4 * (size_t)(ntiles + 1))) ||
            (rc = grow(v, s.nxt, 4 * (size_t)(ntiles + 1))) || (rc = grow(v, s.succ, 4 * words)) ||
            (rc = grow(v, s.info, 2 * words)) || (rc = grow(v, s.mark, words)) ||
            (rc = grow(v, s.exitl, 4 * (size_t)(ntiles + 1))) || (rc = grow(v, s.entry, 4 * (size_t)(ntiles + 1))) ||
            (rc = grow(v, s.good, ntiles + 1)) || (rc = grow(v, s.cnt, 4 * (size_t)(ntiles + 2))) ||
            (rc = grow(v, s.nodes, 4 * words)) || (rc = grow(v, s.cls, words)) || (rc = grow(v, s.addr, 4 * words)) ||
            (rc = grow(v, s.flags, 4 * words)) || (rc = grow(v, s.off, 4 * words)) ||
            (rc = grow(v, s.scan_tmp, 4 * msd_fr_scan_tmp_words((uint32_t)words))) ||
            (rc = grow(v, s.newlist, 4 * nrec)) || (rc = grow(v, s.newaddr, 4 * nrec)) ||
            (rc = grow(v, s.out, sizeof(msd_message) * nrec)))
            return rc;
        x.f.tails_in = keep_in;
        x.f.tails_out = as<uint8_t>(s.keep_out);
        x.f.first = as<uint32_t>(s.first);
        x.f.nxt = as<uint32_t>(s.nxt);
        x.f.succ = as<uint32_t>(s.succ);
        x.f.info = as<uint16_t>(s.info);
        x.f.mark = as<uint8_t>(s.mark);
        x.f.exitl = as<uint32_t>(s.exitl);
        x.f.entry = as<uint32_t>(s.entry);
        x.f.good = as<uint8_t>(s.good);
        *nrec_max = nrec;
        return 0;
    }

    static int launch_decode(const msd_gb_view *v, const uint8_t *src, const msd_ga_scratch &x, hipStream_t st)
    {
        if (int rc = msd_gb_launch_chain_decode(src, &v->tables, &x.f, st))
            return fail(v, rc, "Beast input: chain and decode kernels failed to launch");
        return 0;
    }

    static int check_totals(const msd_gb_view *v, const unsigned long long *tot, uint32_t len, size_t nrec_max)
    {
        const uint32_t nnodes = (uint32_t)tot[MSD_GB_TOT_NODES], nadds = (uint32_t)tot[MSD_GB_TOT_ADDS],
                       ncand = (uint32_t)tot[MSD_GB_TOT_CAND];
        if (nnodes > len || ncand > nrec_max || nadds > nrec_max)
            return fail(v, -EIO, "Beast input: %u nodes, %u messages in a piece of %u bytes", nnodes, ncand, len);
        return 0;
    }

    static int launch_filter(const msd_gb_view *v, const msd_ga_scratch &x, uint32_t nnodes, uint32_t nadds, hipStream_t st)
    {
        return msd_gb_launch_filter(nnodes, nadds, &v->tables, &x.f, st);
    }

    static int check_carry(const msd_gb_view *v, uint32_t receiver, const unsigned long long *c)
    {
        if (c[MSD_GB_CTR_NTL] > KEEP)
            return fail(v, -EIO, "Beast input: receiver %u: incomplete frame of %llu bytes", receiver, c[MSD_GB_CTR_NTL]);
        return 0;
    }

    /* what the receiver's next entry starts with: the incomplete frame, or the bytes since the last frame as a gap */
    static void commit(Rx &r, const msd_gr_input &I, const msd_gb_entry &E, const unsigned long long *c, const uint8_t *kept)
    {
        if (!I.nbytes)
            return;
        if ((uint32_t)c[MSD_FR_CTR_EXIT] & MSD_FR_INC) {
            r.tl = (uint32_t)c[MSD_GB_CTR_NTL];
            memcpy(r.keep, kept, r.tl);
            r.pending_gap = 0;
        } else {
            r.tl = 0;
            r.pending_gap = (c[MSD_FR_CTR_NODES] ? 0 : r.pending_gap) + ((E.s1 - E.s0) - c[MSD_FR_CTR_LAST_END]);
        }
    }
};

struct Avr {
    static constexpr int FORMAT = MSD_GR_AVR;
    static constexpr const char *NAME = "AVR";
    static constexpr uint32_t KEEP = MSD_AVR_LINE_MAX;
    static constexpr bool OUT_BY_CAND = true; /* `out` is sized by the candidates the first synchronisation reports */
    struct Rx {
        uint8_t keep[KEEP]; /* the incomplete line */
        uint32_t tl = 0;
        uint32_t discard = 0; /* inside an overlong line (and tl is 0) */
        msd_avr_stats as{};
    };

    static void entry(const Rx &r, const msd_gr_input &I, msd_gb_entry &E)
    {
        E.opt |= ((I.flags & MSD_AVR_KEEP_TIMESTAMP) ? MSD_GA_OPT_KEEP_TS : 0u) | (r.discard ? MSD_GA_OPT_DISCARD : 0u);
    }

    /* the piece's bytes, and the records by its shortest line that yields one (7 bytes).  Beside these, run_piece grows
     * for both formats: up, stage, snaps, keep_out, add_first, ctr, tot, hash and the page-locked h_*, and here `out` */
    static int scratch(const msd_gb_view *v, Bufs &s, const uint8_t *keep_in, msd_ga_scratch &x, size_t *nrec_max)
    {
        const uint32_t nspans = x.f.ntiles;
        const size_t nrec = (size_t)x.f.len / 7u + 2;
        int rc = 0;
        if ((rc = grow(v, s.buf, (size_t)x.f.len + 16)) || (rc = grow(v, s.cnt, 4 * (size_t)(nspans + 2))) ||
            (rc = grow(v, s.nodes, 4 * nrec)) || (rc = grow(v, s.cls, nrec)) || (rc = grow(v, s.addr, 4 * nrec)) ||
            (rc = grow(v, s.flags, 4 * nrec)) || (rc = grow(v, s.off, 4 * (nrec + 1))) ||
            (rc = grow(v, s.scan_tmp, 4 * msd_fr_scan_tmp_words((uint32_t)(nrec > nspans ? nrec : nspans)))) ||
            (rc = grow(v, s.newlist, 4 * nrec)) || (rc = grow(v, s.newaddr, 4 * nrec)) ||
            (rc = grow(v, s.rec, sizeof(msd_message) * nrec)))
            return rc;
        x.lines_in = keep_in;
        x.lines_out = as<uint8_t>(s.keep_out);
        x.rec = as<msd_message>(s.rec);
        *nrec_max = nrec;
        return 0;
    }

    static int launch_decode(const msd_gb_view *v, const uint8_t *src, const msd_ga_scratch &x, hipStream_t st)
    {
        if (int rc = msd_ga_launch_frame_decode(src, &v->tables, &x, st))
            return fail(v, rc, "AVR input: line and decode kernels failed to launch");
        return 0;
    }

    static int check_totals(const msd_gb_view *v, const unsigned long long *tot, uint32_t len, size_t nrec_max)
    {
        const uint32_t nrec = (uint32_t)tot[MSD_GB_TOT_NODES], nadds = (uint32_t)tot[MSD_GB_TOT_ADDS],
                       ncand = (uint32_t)tot[MSD_GB_TOT_CAND];
        if (tot[MSD_GB_TOT_NODES] + 2 > nrec_max || ncand > nrec || nadds > nrec)
            return fail(v, -EIO, "AVR input: %llu records, %u messages in a piece of %u bytes", tot[MSD_GB_TOT_NODES], ncand, len);
        return 0;
    }

    static int launch_filter(const msd_gb_view *v, const msd_ga_scratch &x, uint32_t nrec, uint32_t nadds, hipStream_t st)
    {
        return msd_gb_launch_filter_records(x.rec, nrec, nadds, &v->tables, &x.f, st);
    }

    static int check_carry(const msd_gb_view *v, uint32_t receiver, const unsigned long long *c)
    {
        if (c[MSD_GB_CTR_NTL] > KEEP || c[MSD_GA_CTR_DISCARD] > 1 || (c[MSD_GA_CTR_DISCARD] && c[MSD_GB_CTR_NTL]))
            return fail(v, -EIO, "AVR input: receiver %u: incomplete line of %llu bytes", receiver, c[MSD_GB_CTR_NTL]);
        return 0;
    }

    /* the statistics of every entry, one that completes no line included; then what its next entry starts with */
    static void commit(Rx &r, const msd_gr_input &I, const msd_gb_entry &, const unsigned long long *c, const uint8_t *kept)
    {
        r.as.lines += c[MSD_GA_CTR_LINES];
        r.as.frames += c[MSD_FR_CTR_NODES];
        r.as.dropped_lines += c[MSD_GA_CTR_DROPPED];
        r.as.long_lines += c[MSD_GA_CTR_LONG];
        if (I.nbytes) {
            r.tl = (uint32_t)c[MSD_GB_CTR_NTL];
            r.discard = (uint32_t)c[MSD_GA_CTR_DISCARD];
            memcpy(r.keep, kept, r.tl);
        }
    }
};

/* host memory per receiver, as modes_hip.h states it for each format */
static_assert(sizeof(Beast::Rx) == 80 && sizeof(Avr::Rx) == 296, "the receivers' carries");

/* entries [a, b) of the call as one piece */
template <class F>
int run_piece(const msd_gb_view *v, State<F> &s, const uint8_t *bytes, int on_device, const msd_gr_input *in, uint32_t a,
              uint32_t b, msd_group_message_fn sink, const msd_gb_out *out, void *user)
{
    hipStream_t st = static_cast<hipStream_t>(v->stream);
    const uint32_t n = b - a;
    int rc = 0;

    /* the upload block: entries | tile -> entry | kept bytes | snapshot slots | flips */
    uint32_t ntiles = 0;
    size_t newbytes = 0;
    for (uint32_t i = a; i < b; ++i) {
        const uint32_t seg = in[i].nbytes ? s.rx[in[i].receiver].tl + in[i].nbytes : 0u;
        ntiles += (seg + MSD_FR_TILE - 1u) / MSD_FR_TILE;
        newbytes += in[i].nbytes;
    }
    const uint32_t len = ntiles * MSD_FR_TILE;
    const size_t o_ent = 0, o_tile = up8(sizeof(msd_gb_entry) * n), o_keep = o_tile + up8(sizeof(uint32_t) * ntiles),
                 o_slot = o_keep + (size_t)F::KEEP * n, o_flip = o_slot + up8(sizeof(uint32_t) * n),
                 up_bytes = o_flip + up8(sizeof(uint32_t) * n);
    if ((rc = grow(v, s.h_up, up_bytes)) || (rc = grow(v, s.up, up_bytes)))
        return rc;
    if (!on_device && ((rc = grow(v, s.h_stage, newbytes + 1)) || (rc = grow(v, s.stage, newbytes + 1))))
        return rc;
    uint8_t *hu = as<uint8_t>(s.h_up);
    msd_gb_entry *ent = reinterpret_cast<msd_gb_entry *>(hu + o_ent);
    uint32_t *tile_ent = reinterpret_cast<uint32_t *>(hu + o_tile);
    uint8_t *keeps = hu + o_keep;
    uint32_t *slot = reinterpret_cast<uint32_t *>(hu + o_slot), *flip = reinterpret_cast<uint32_t *>(hu + o_flip);
    uint32_t t = 0;
    size_t staged = 0;
    for (uint32_t i = a; i < b; ++i) {
        const msd_gr_input &I = in[i];
        const typename F::Rx &r = s.rx[I.receiver];
        msd_gb_entry &E = ent[i - a];
        memset(&E, 0, sizeof E);
        E.tl = I.nbytes ? r.tl : 0u; /* an empty entry leaves its receiver's carry alone */
        E.now_ms = I.now_ms;
        E.s0 = t * MSD_FR_TILE;
        E.s1 = E.s0 + (I.nbytes ? E.tl + I.nbytes : 0u);
        E.tile0 = t;
        E.ntiles = (E.s1 - E.s0 + MSD_FR_TILE - 1u) / MSD_FR_TILE;
        E.snap = v->d_snaps ? I.receiver : i - a;
        E.opt = (uint32_t)I.nfix | (I.mode_ac ? MSD_GB_OPT_MODEAC : 0u);
        F::entry(r, I, E);
        if (on_device) {
            E.src = I.offset;
        } else { /* the call's bytes packed densely into one page-locked array: one copy to the device */
            E.src = staged;
            memcpy(as<uint8_t>(s.h_stage) + staged, bytes + I.offset, I.nbytes);
            staged += I.nbytes;
        }
        for (uint32_t k = 0; k < E.ntiles; ++k)
            tile_ent[t++] = i - a;
        memcpy(keeps + (size_t)F::KEEP * (i - a), r.keep, F::KEEP);
        slot[i - a] = I.receiver;
        flip[i - a] = I.now_ms >= I.filter->next_flip ? 1u : 0u; /* icaoFilterExpire's own test (icao_filter.c:150-164) */
    }

    /* scratch: the format's own by the size of the piece, the rest by its entries */
    msd_ga_scratch x{};
    msd_gb_scratch &f = x.f;
    uint8_t *du = as<uint8_t>(s.up);
    size_t nrec_max = 0;
    f.n = n;
    f.ntiles = ntiles;
    f.len = len;
    if ((rc = grow(v, s.keep_out, (size_t)F::KEEP * n)) || (rc = F::scratch(v, s, du + o_keep, x, &nrec_max)) ||
        (rc = grow(v, s.add_first, 4 * (size_t)(n + 1))) || (rc = grow(v, s.ctr, 8 * (size_t)MSD_FR_CTR_WORDS * n)) ||
        (rc = grow(v, s.tot, 8 * MSD_GB_TOT_WORDS)) || (rc = grow(v, s.h_ctr, 8 * (size_t)MSD_FR_CTR_WORDS * n)) ||
        (rc = grow(v, s.h_tot, 8 * MSD_GB_TOT_WORDS)) || (rc = grow(v, s.h_keep, (size_t)F::KEEP * n)))
        return rc;
    uint32_t *snaps = v->d_snaps;
    if (!snaps) { /* a group that resolves on the host keeps no snapshots on the device: those of this piece */
        const size_t sb = sizeof(uint32_t) * MSD_SNAP_WORDS * (size_t)n;
        if ((rc = grow(v, s.h_snaps, sb)) || (rc = grow(v, s.snaps, sb)))
            return rc;
        uint32_t *h = as<uint32_t>(s.h_snaps);
        for (uint32_t i = a; i < b; ++i, h += MSD_SNAP_WORDS)
            snapshot_of(in[i].filter, h);
        HCK(v, hipMemcpyAsync(s.snaps.p, s.h_snaps.p, sb, hipMemcpyHostToDevice, st));
        snaps = as<uint32_t>(s.snaps);
    }
    HCK(v, hipMemcpyAsync(s.up.p, s.h_up.p, up_bytes, hipMemcpyHostToDevice, st));
    if (!on_device && staged)
        HCK(v, hipMemcpyAsync(s.stage.p, s.h_stage.p, staged, hipMemcpyHostToDevice, st));

    f.ent = reinterpret_cast<const msd_gb_entry *>(du + o_ent);
    f.tile_ent = reinterpret_cast<const uint32_t *>(du + o_tile);
    f.buf = as<uint8_t>(s.buf);
    f.cnt = as<uint32_t>(s.cnt);
    f.nodes = as<uint32_t>(s.nodes);
    f.cls = as<uint8_t>(s.cls);
    f.addr = as<uint32_t>(s.addr);
    f.flags = as<uint32_t>(s.flags);
    f.off = as<uint32_t>(s.off);
    f.scan_tmp = as<uint32_t>(s.scan_tmp);
    f.newlist = as<uint32_t>(s.newlist);
    f.newaddr = as<uint32_t>(s.newaddr);
    f.snaps = snaps;
    f.add_first = as<uint32_t>(s.add_first);
    f.ctr = as<unsigned long long>(s.ctr);
    f.tot = as<unsigned long long>(s.tot);

    if ((rc = F::launch_decode(v, on_device ? bytes : as<uint8_t>(s.stage), x, st)))
        return rc;
    /* first synchronisation: the piece's nodes (Beast) or records (AVR), its adds and an upper bound of the records it
     * delivers */
    HCK(v, hipMemcpyAsync(s.h_tot.p, s.tot.p, 8 * MSD_GB_TOT_WORDS, hipMemcpyDeviceToHost, st));
    HCK(v, hipStreamSynchronize(st));
    const unsigned long long *tot = as<unsigned long long>(s.h_tot);
    if ((rc = F::check_totals(v, tot, len, nrec_max)))
        return rc;
    const uint32_t nnodes = (uint32_t)tot[MSD_GB_TOT_NODES], nadds = (uint32_t)tot[MSD_GB_TOT_ADDS],
                   ncand = (uint32_t)tot[MSD_GB_TOT_CAND];
    if (nadds) {
        uint32_t hs = 64;
        while (hs < 2u * nadds)
            hs <<= 1;
        if ((rc = grow(v, s.hash, (size_t)16 * hs)))
            return rc;
        HCK(v, hipMemsetAsync(s.hash.p, 0xff, (size_t)16 * hs, st));
        f.hash = as<unsigned long long>(s.hash);
        f.hslots = hs;
    }
    if ((F::OUT_BY_CAND && (rc = grow(v, s.out, sizeof(msd_message) * ((size_t)ncand + 1)))) ||
        (rc = grow(v, s.h_out, sizeof(msd_message) * ((size_t)ncand + 1))) ||
        (rc = grow(v, s.h_new, sizeof(uint32_t) * ((size_t)nadds + 1))))
        return rc;
    f.out = as<msd_message>(s.out);
    if ((rc = out_errbits(v, s.ob, out, ncand, &f.errbits)))
        return rc;
    if ((rc = F::launch_filter(v, x, nnodes, nadds, st)))
        return fail(v, rc, "%s input: filter kernels failed to launch", F::NAME);
    if (v->d_snaps && /* the resident snapshots: every entry's inserts, then its flip */
        (rc = msd_launch_group_filter_apply(v->d_snaps, n, reinterpret_cast<const uint32_t *>(du + o_slot), f.add_first,
                                            f.newaddr, reinterpret_cast<const uint32_t *>(du + o_flip), st)))
        return fail(v, rc, "%s input: group filter kernel launch failed", F::NAME);
    /* a fields or wire call: the output stage over the piece's records, whose number only the device knows */
    const bool queued = out && nnodes && ncand;
    if (queued && (rc = out_queue(v, s.ob, *out, f.out, f.off + nnodes, ncand, f.ctr, n, f.errbits, st)))
        return rc;
    /* second synchronisation: counters, the carries, records and the new-address lists */
    HCK(v, hipMemcpyAsync(s.h_ctr.p, s.ctr.p, 8 * (size_t)MSD_FR_CTR_WORDS * n, hipMemcpyDeviceToHost, st));
    HCK(v, hipMemcpyAsync(s.h_keep.p, s.keep_out.p, (size_t)F::KEEP * n, hipMemcpyDeviceToHost, st));
    if (nnodes && ncand)
        HCK(v, hipMemcpyAsync(s.h_out.p, s.out.p, sizeof(msd_message) * ncand, hipMemcpyDeviceToHost, st));
    if (nnodes && nadds)
        HCK(v, hipMemcpyAsync(s.h_new.p, s.newaddr.p, sizeof(uint32_t) * nadds, hipMemcpyDeviceToHost, st));
    HCK(v, hipStreamSynchronize(st));

    const unsigned long long *ctr = as<unsigned long long>(s.h_ctr);
    for (uint32_t i = a; i < b; ++i) { /* nothing is committed before every entry has been looked at */
        const unsigned long long *c = ctr + (size_t)MSD_FR_CTR_WORDS * (i - a);
        if ((rc = F::check_carry(v, in[i].receiver, c)))
            return rc;
        if (c[MSD_GB_CTR_REC_FIRST] + c[MSD_FR_CTR_RECORDS] > ncand || c[MSD_GB_CTR_NEW_FIRST] + c[MSD_FR_CTR_NEW] > nadds)
            return fail(v, -EIO, "%s input: receiver %u: record or address range outside the piece's", F::NAME, in[i].receiver);
        if (out && !out_range_ok(s.ob, *out, queued, i - a, ncand))
            return fail(v, -EIO, "%s input: receiver %u: wire bytes outside the piece's", F::NAME, in[i].receiver);
    }
    const msd_message *recs = as<msd_message>(s.h_out);
    const uint32_t *newaddr = as<uint32_t>(s.h_new);
    for (uint32_t i = a; i < b; ++i) {
        const msd_gr_input &I = in[i];
        const unsigned long long *c = ctr + (size_t)MSD_FR_CTR_WORDS * (i - a);
        /* icaoFilterAdd of the entry's new addresses in order of first add, as the device inserted them; then the flip */
        for (uint32_t k = 0; k < (uint32_t)c[MSD_FR_CTR_NEW]; ++k)
            msd_filter_add(I.filter, newaddr[c[MSD_GB_CTR_NEW_FIRST] + k]);
        msd_filter_expire(I.filter, I.now_ms); /* readsb.c:331 */
        add_remote(v->remote[I.receiver], c);
        F::commit(s.rx[I.receiver], I, ent[i - a], c, as<uint8_t>(s.h_keep) + (size_t)F::KEEP * (i - a));
        if (out)
            out_deliver(s.ob, *out, queued, I.receiver, i - a, recs, (uint32_t)c[MSD_GB_CTR_REC_FIRST],
                        (uint32_t)c[MSD_FR_CTR_RECORDS], user);
        else if (sink)
            for (uint32_t k = 0; k < (uint32_t)c[MSD_FR_CTR_RECORDS]; ++k)
                sink(I.receiver, recs + c[MSD_GB_CTR_REC_FIRST] + k, user);
    }
    return 0;
}

template <class F>
int accept(const msd_gb_view *v, const uint8_t *bytes, int on_device, const msd_gr_input *in, uint32_t n,
           msd_group_message_fn sink, const msd_gb_out *out, void *user)
{
    State<F> *s = state_of<F>(*v->state);
    if (!s) {
        s = new (std::nothrow) State<F>();
        if (!s)
            return fail(v, -ENOMEM, "out of host memory");
        try {
            s->rx.resize(v->max_receivers);
        } catch (...) {
            delete s;
            return fail(v, -ENOMEM, "out of host memory");
        }
        *v->state = static_cast<Bufs *>(s);
    }
    HCK(v, hipSetDevice(v->device));
    /* pieces of whole entries: a piece is closed when the next entry would take its new bytes past MSD_FR_PIECE */
    for (uint32_t a = 0; a < n;) {
        uint32_t b = a;
        size_t sum = 0;
        while (b < n && (b == a || sum + in[b].nbytes <= MSD_FR_PIECE))
            sum += in[b++].nbytes;
        const int rc = run_piece(v, *s, bytes, on_device, in, a, b, sink, out, user);
        if (rc)
            return rc;
        a = b;
    }
    return 0;
}

template <class F> void reset_receiver(State<F> *s, uint32_t receiver)
{
    if (receiver < s->rx.size())
        s->rx[receiver] = typename F::Rx();
}

} // namespace

extern "C" {

int msd_gr_accept(const msd_gb_view *v, const void *bytes, int on_device, const msd_gr_input *in, uint32_t n,
                  msd_group_message_fn sink, const msd_gb_out *out, void *user)
{
    const uint8_t *p = static_cast<const uint8_t *>(bytes);
    return v->format == MSD_GR_AVR ? accept<Avr>(v, p, on_device, in, n, sink, out, user)
                                   : accept<Beast>(v, p, on_device, in, n, sink, out, user);
}

void msd_gr_reset_receiver(void *state, uint32_t receiver)
{
    if (!state)
        return;
    if (static_cast<Bufs *>(state)->format == MSD_GR_AVR)
        reset_receiver(state_of<Avr>(state), receiver);
    else
        reset_receiver(state_of<Beast>(state), receiver);
}

void msd_gr_get_avr_stats(const void *avr_state, uint32_t receiver, msd_avr_stats *st)
{
    const State<Avr> *s = state_of<Avr>(avr_state);
    if (s && receiver < s->rx.size())
        *st = s->rx[receiver].as;
    else
        memset(st, 0, sizeof *st);
}

/* the buffers go with the state (~Buf), on the device the caller has made current */
void msd_gr_free(void *state)
{
    if (!state)
        return;
    if (static_cast<Bufs *>(state)->format == MSD_GR_AVR)
        delete state_of<Avr>(state);
    else
        delete state_of<Beast>(state);
}

} // extern "C"
