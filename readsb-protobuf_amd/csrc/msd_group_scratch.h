/*
 * msd_group_scratch.h -- what the two drivers of the remote input per receiver of a group share on the host
 * (msd_group_beast.cpp, msd_group_avr.cpp): the buffers that grow to the largest piece seen, the error
 * text of the view, and a receiver's host filter as the snapshot the kernels read.  Host C++ only.
 */
#ifndef MSD_GROUP_SCRATCH_H
#define MSD_GROUP_SCRATCH_H

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdarg>
#include <cstdio>

#include "msd_group_beast.h"

namespace msd_group_scratch {

struct Buf { /* device (pinned = false) or page-locked host memory */
    void *p = nullptr;
    size_t cap = 0;
    bool pinned = false;
};

inline int fail(const msd_gb_view *v, int code, const char *fmt, ...)
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
            return msd_group_scratch::fail((v), -EIO, "%s failed: %s", #call, hipGetErrorString(e_));                  \
    } while (0)

inline int grow(const msd_gb_view *v, Buf &b, size_t bytes)
{
    if (b.cap >= bytes)
        return 0;
    if (b.pinned)
        (void)hipHostFree(b.p);
    else
        (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
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

inline void release(Buf &b)
{
    if (b.pinned)
        (void)hipHostFree(b.p);
    else
        (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

template <class T> T *as(Buf &b)
{
    return static_cast<T *>(b.p);
}

inline size_t up8(size_t x)
{
    return (x + 7u) & ~(size_t)7u;
}

/* the filter as a snapshot: MSD_SNAP_WORDS words, the two tables interleaved, then the active one */
inline void snapshot_of(const msd_filter *f, uint32_t *h)
{
    for (uint32_t k = 0; k < 8192; ++k) {
        h[2 * k] = f->slot[0][k];
        h[2 * k + 1] = f->slot[1][k];
    }
    h[16384] = (uint32_t)f->active;
}

/* a piece's counter row into its receiver's remote counters */
inline void add_remote(msd_remote_stats &rs, const unsigned long long *c)
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

/* ---- the output stage of a fields or wire call (msd_group_remote_out_kernels.hip), the same for both drivers ---- */
struct OutBufs {
    Buf fields, lens, sums, starts, errbits;
    Buf h_fields{nullptr, 0, true}, h_wire{nullptr, 0, true}, h_ranges{nullptr, 0, true};
    Buf *all[8] = {&fields, &lens, &sums, &starts, &errbits, &h_fields, &h_wire, &h_ranges};
};

/* Before the filter stage of a verbatim wire call: where its records kernel leaves the repaired bit positions of the
 * piece's at most ncand records; NULL (and 0) for every other call */
inline int out_errbits(const msd_gb_view *v, OutBufs &ob, const msd_gb_out *o, uint32_t ncand, uint8_t **errbits)
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
inline int out_queue(const msd_gb_view *v, OutBufs &ob, const msd_gb_out &o, const msd_message *d_out, const uint32_t *d_count,
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
inline bool out_range_ok(OutBufs &ob, const msd_gb_out &o, bool queued, uint32_t e, uint32_t ncand)
{
    if (!o.want_wire || !queued)
        return true;
    const uint32_t *r = as<uint32_t>(ob.h_ranges) + 2 * (size_t)e;
    return r[1] != 0xffffffffu && (size_t)r[0] + r[1] <= (size_t)MSD_GRO_WIRE_MAX * ncand;
}

/* entry e's delivery: its records [first, first + nrec) of the piece with their fields, or its bytes in one call */
inline void out_deliver(OutBufs &ob, const msd_gb_out &o, bool queued, uint32_t receiver, uint32_t e, const msd_message *recs,
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

} // namespace msd_group_scratch

#endif
