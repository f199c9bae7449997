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

} // namespace msd_group_scratch

#endif
