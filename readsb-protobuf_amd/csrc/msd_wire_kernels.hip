/*
 * msd_wire_kernels.hip -- Beast frames and AVR lines written on the GPU (msd_wire_impl.h encodes one message).
 *
 *   msd_wire_encode (msd_capi.cpp): n records -> one dense stream in record order.  msd_wire_len_kernel leaves a
 *   length per record and a sum per workgroup of 256, scan_kernel (msd_wire_store_impl.h) turns the sums into offsets (one
 *   workgroup), msd_wire_store_kernel encodes and stores.
 *
 *   receiver groups (msd_group.cpp): one workgroup per buffer of a call builds the buffer's messages the way
 *   msd_emit_kernel does and leaves every entry's bytes contiguous in one array of page-locked host memory.
 *   msd_group_wire_count_kernel leaves the bytes per buffer, msd_group_wire_kernel sums them over the buffers in
 *   front and stores.
 *
 * Both store through wire_store_run (msd_wire_store_impl.h): the bytes of up to 256 messages are put together in LDS
 * and leave as whole-wavefront runs of consecutive aligned dwords, for the reason msd_emit_kernel gives for its rows --
 * the destination may be host memory, where a store per message byte would cost a PCIe write each.
 */
#include <hip/hip_runtime.h>

#include "msd_emit_impl.h"
#include "msd_wire_impl.h"
#include "msd_wire_store_impl.h"

namespace {

using namespace msd_wire_store; /* WT, IMAGE_WORDS, block_scan, scan_kernel, image_at, wire_store_run */

/* ------------------------------------------------------------------------------------------------------------------ */
/* msd_wire_encode */

__global__ void __launch_bounds__(WT) msd_wire_len_kernel(const msd_message *msgs, uint32_t n, int format, int verbatim,
                                                          uint8_t *lens, uint32_t *block_sums)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        const msd_message mm = msgs[i];
        len = msd_wire_length(msd_wire_source(mm, verbatim != 0, false, 0xffu, 0xffu), format);
        lens[i] = (uint8_t)len;
    }
    uint32_t total;
    (void)block_scan<WT>(len, part, total);
    if (threadIdx.x == 0)
        block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(WT) msd_wire_store_kernel(const msd_message *msgs, uint32_t n, int format, int verbatim,
                                                            const uint8_t *lens, const uint32_t *block_off, uint8_t *out,
                                                            uint32_t *ends)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t image[IMAGE_WORDS];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    const uint32_t len = i < n ? lens[i] : 0u;
    uint32_t total;
    const uint32_t off = block_scan<WT>(len, part, total);
    uint8_t *dst = out + block_off[blockIdx.x];
    if (i < n) {
        if (ends)
            ends[i] = block_off[blockIdx.x] + off + len;
        if (len) {
            const msd_message mm = msgs[i];
            msd_wire_put(msd_wire_source(mm, verbatim != 0, false, 0xffu, 0xffu), format, image_at(image, dst, off));
        }
    }
    __syncthreads();
    wire_store_run(dst, image, total);
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* receiver groups */

/* message m of buffer b as msd_emit_kernel builds it -- m < nm: Mode S message m, else Mode A/C reply m - nm -- ready
 * for the encoder; verbatim takes the received bytes from the try's repaired positions */
__device__ __forceinline__ msd_wire_src group_message(const MsdResolveParams &P, const unsigned long long *power, uint32_t b,
                                                      uint32_t m, uint32_t nm, bool verbatim)
{
    const uint64_t sample_ts = P.ts[2 * b], sys_ts = P.ts[2 * b + 1];
    if (m < nm) {
        const msd_acc rec = P.acc[(size_t)b * MSD_RB_MSG_CAP + m];
        unsigned long long side;
        const msd_message mm = msd_emit_mode_s(rec, P.tries, power[(size_t)b * MSD_RB_MSG_CAP + m], sample_ts, sys_ts,
                                               b * MSD_CHUNK_SAMPLES, side);
        const unsigned char *t = reinterpret_cast<const unsigned char *>(P.tries + rec.try_index);
        return msd_wire_source(mm, verbatim, true, t[15], t[28]); /* errbit, errbit2: as msd_emit_mode_s reads them */
    }
    const msd_ac_hit c = P.ac[P.acc_ac[(size_t)b * MSD_RB_AC_CAP + (m - nm)]];
    return msd_wire_source(msd_emit_mode_ac(c, sample_ts, sys_ts), verbatim, true, 0xffu, 0xffu);
}

/* counts[2 b] = bytes of buffer b's entry, counts[2 b + 1] = messages they carry */
__global__ void __launch_bounds__(WT) msd_group_wire_count_kernel(const MsdResolveParams P, const unsigned long long *power,
                                                                  int format, int verbatim, uint32_t *counts)
{
    __shared__ uint32_t part[4];
    const uint32_t b = blockIdx.x;
    const bool off = P.totals[2] || (P.ac && P.ac_totals[2]); /* as msd_emit_kernel: an overflowed call has no records */
    const uint32_t nm = off ? 0u : P.nmsgs[b], na = off || !P.ac ? 0u : P.nac[b];
    uint32_t bytes = 0, fwd = 0;
    for (uint32_t m = threadIdx.x; m < nm + na; m += WT) {
        const uint32_t len = msd_wire_length(group_message(P, power, b, m, nm, verbatim != 0), format);
        bytes += len;
        fwd += len ? 1u : 0u;
    }
    uint32_t total_bytes, total_fwd;
    (void)block_scan<WT>(bytes, part, total_bytes);
    (void)block_scan<WT>(fwd, part, total_fwd);
    if (threadIdx.x == 0) {
        counts[2 * b] = total_bytes;
        counts[2 * b + 1] = total_fwd;
    }
}

/* Buffer b's bytes to out + the 16-byte-aligned offset that follows from the counts of the buffers in front of it;
 * entries[b] = {offset, bytes, messages, 0}.  What would pass cap is not written: bytes = 0xffffffff tells the host. */
__global__ void __launch_bounds__(WT) msd_group_wire_kernel(const MsdResolveParams P, const unsigned long long *power,
                                                            int format, int verbatim, const uint32_t *counts, uint8_t *out,
                                                            uint64_t cap, uint32_t *entries)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t image[IMAGE_WORDS];
    const uint32_t b = blockIdx.x;
    /* o = bytes in front of this buffer's, every entry rounded up to 16 (msd_emit_kernel's idiom for its records) */
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < b; i += WT)
        mine += (counts[2 * i] + 15u) & ~15u;
    uint32_t o;
    (void)block_scan<WT>(mine, part, o);
    const uint32_t mybytes = counts[2 * b];
    const bool fits = (uint64_t)o + mybytes <= cap;
    if (threadIdx.x == 0) {
        entries[4 * b] = o;
        entries[4 * b + 1] = fits ? mybytes : 0xffffffffu;
        entries[4 * b + 2] = counts[2 * b + 1];
        entries[4 * b + 3] = 0;
    }
    if (!fits || !mybytes)
        return;
    const uint32_t nm = P.nmsgs[b], na = P.ac ? P.nac[b] : 0u;
    uint32_t run = 0; /* bytes of the chunks before */
    for (uint32_t m0 = 0; m0 < nm + na; m0 += WT) { /* Mode S first, then the buffer's Mode A/C replies */
        const uint32_t m = m0 + threadIdx.x;
        msd_wire_src src;
        uint32_t len = 0;
        if (m < nm + na) {
            src = group_message(P, power, b, m, nm, verbatim != 0);
            len = msd_wire_length(src, format);
        }
        uint32_t total;
        const uint32_t off = block_scan<WT>(len, part, total);
        uint8_t *dst = out + o + run;
        if (run + total > mybytes) /* (cannot happen: the counts come from the same arithmetic) */
            return;
        if (len)
            msd_wire_put(src, format, image_at(image, dst, off));
        __syncthreads();
        wire_store_run(dst, image, total);
        run += total;
        /* (block_scan's first barrier stands between this store's reads of the image and its next writes) */
    }
}

} /* namespace */

extern "C" int msd_launch_wire_lengths(const msd_message *d_msgs, uint32_t n, int format, int verbatim, uint8_t *d_lens,
                                       uint32_t *d_block_sums, hipStream_t stream)
{
    if (n == 0)
        return 0;
    const uint32_t nblocks = (n + WT - 1) / WT;
    hipLaunchKernelGGL(msd_wire_len_kernel, dim3(nblocks), dim3(WT), 0, stream, d_msgs, n, format, verbatim, d_lens,
                       d_block_sums);
    hipLaunchKernelGGL(scan_kernel<>, dim3(1), dim3(WT), 0, stream, d_block_sums, nblocks);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int msd_launch_wire_store(const msd_message *d_msgs, uint32_t n, int format, int verbatim, const uint8_t *d_lens,
                                     const uint32_t *d_block_off, uint8_t *out, uint32_t *ends, hipStream_t stream)
{
    if (n == 0)
        return 0;
    hipLaunchKernelGGL(msd_wire_store_kernel, dim3((n + WT - 1) / WT), dim3(WT), 0, stream, d_msgs, n, format, verbatim,
                       d_lens, d_block_off, out, ends);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int msd_launch_group_wire(const MsdResolveParams *p, uint32_t nbuffers, const unsigned long long *power, int format,
                                     int verbatim, uint32_t *d_counts, uint8_t *out, uint64_t cap, uint32_t *entries,
                                     hipStream_t stream)
{
    if (nbuffers == 0)
        return 0;
    hipLaunchKernelGGL(msd_group_wire_count_kernel, dim3(nbuffers), dim3(WT), 0, stream, *p, power, format, verbatim, d_counts);
    hipLaunchKernelGGL(msd_group_wire_kernel, dim3(nbuffers), dim3(WT), 0, stream, *p, power, format, verbatim, d_counts, out,
                       cap, entries);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
