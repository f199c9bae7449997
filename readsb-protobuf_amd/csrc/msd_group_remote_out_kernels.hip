/*
 * msd_group_remote_out_kernels.hip -- the output stage of the remote inputs of a receiver group
 * (msd_group_accept_beast_fields / _wire, msd_group_accept_avr_fields / _wire): decoded fields and Beast
 * frames or AVR lines of the records a piece accepted, made on the GPU between the filter stage and the piece's second
 * synchronisation.
 *
 * Both inputs leave their records in the same place -- `out`, entry after entry, stream order within one, every entry's
 * range in its counter row (MSD_GB_CTR_REC_FIRST, MSD_FR_CTR_RECORDS) --, so one stage serves both.  The number of
 * records is on the device only (the last word of the filter stage's scan, `count`); the host knows a bound of it from
 * the first synchronisation.  Every kernel is launched on the bound and guards with the count.
 *
 *   fields: msd_gro_fields_kernel, one thread per record, msd_fields_impl.h; fields[k] belongs to out[k].
 *   wire:   msd_gro_len_kernel leaves a length per record and a sum per workgroup of 256, scan_kernel turns the
 *           sums into offsets (one workgroup), msd_gro_store_kernel encodes and stores one dense stream in record
 *           order, coalesced through LDS (msd_wire_store_impl.h) because the stream is page-locked host memory, and
 *           leaves every record's start; msd_gro_ranges_kernel gives every entry its bytes of the stream -- an entry
 *           without records an empty range where its records would be.
 *
 * Verbatim output takes the received bytes from the repaired bit positions the records kernels leave beside the records
 * for such a call (`errbits`, two bytes per record, 0xff for none): msd_wire_source(..., have_errbits = true, ...), no
 * search.  Every correctable syndrome belongs to one pattern of one or two bits only, so these are the positions the
 * host writers' search finds (tests/test_remote_verbatim_positions.py enumerates them).  Without verbatim errbits is
 * NULL and nothing is flipped.  The wire kernels keep msd_wire_impl.h's rule: no private array indexed at run time, no
 * scratch.
 */
#include <hip/hip_runtime.h>

#include "msd_fields_impl.h"
#include "msd_group_beast.h"
#include "msd_wire_impl.h"
#include "msd_wire_store_impl.h"

namespace {

using namespace msd_wire_store; /* WT, IMAGE_WORDS, block_scan, scan_kernel, image_at, wire_store_run */

constexpr uint32_t CW = MSD_FR_CTR_WORDS;
static_assert(MSD_GRO_WIRE_MAX == MSD_WIRE_MAX, "the host sizes the stream by MSD_GRO_WIRE_MAX");

__global__ void __launch_bounds__(WT) msd_gro_fields_kernel(const msd_message *out, const uint32_t *count, uint32_t bound,
                                                            msd_fields *fields)
{
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    if (i >= min(*count, bound))
        return;
    const msd_message mm = out[i];
    msd_fields f;
    if (mm.msgtype == 32) /* no carry: every remote frame is decoded into a zeroed message (net_io.c:1538) */
        msd_fields_mode_ac(((uint32_t)mm.msg[0] << 8) | mm.msg[1], nullptr, &f);
    else
        msd_fields_mode_s(mm.msg, mm.msgtype, mm.addr, &f);
    fields[i] = f;
}

/* record i ready for the encoder */
__device__ __forceinline__ msd_wire_src record_source(const msd_message *out, const uint8_t *errbits, uint32_t i)
{
    const msd_message mm = out[i];
    const uint32_t e0 = errbits ? errbits[2 * (size_t)i] : 0xffu, e1 = errbits ? errbits[2 * (size_t)i + 1] : 0xffu;
    return msd_wire_source(mm, errbits != nullptr, true, e0, e1);
}

__global__ void __launch_bounds__(WT) msd_gro_len_kernel(const msd_message *out, const uint32_t *count, uint32_t bound,
                                                         int format, const uint8_t *errbits, uint8_t *lens,
                                                         uint32_t *block_sums)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0;
    if (i < min(*count, bound)) {
        len = msd_wire_length(record_source(out, errbits, i), format);
        lens[i] = (uint8_t)len;
    }
    uint32_t total;
    (void)block_scan<WT>(len, part, total);
    if (threadIdx.x == 0)
        block_sums[blockIdx.x] = total;
}

/* record i's bytes to stream + starts[i]; the stream holds at least MSD_WIRE_MAX * bound bytes */
__global__ void __launch_bounds__(WT) msd_gro_store_kernel(const msd_message *out, const uint32_t *count, uint32_t bound,
                                                           int format, const uint8_t *errbits, const uint8_t *lens,
                                                           const uint32_t *block_off, uint8_t *stream, uint32_t *starts)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t image[IMAGE_WORDS];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    const bool mine = i < min(*count, bound);
    const uint32_t len = mine ? lens[i] : 0u;
    uint32_t total;
    const uint32_t off = block_scan<WT>(len, part, total);
    uint8_t *dst = stream + block_off[blockIdx.x];
    if (mine) {
        starts[i] = block_off[blockIdx.x] + off;
        if (len)
            msd_wire_put(record_source(out, errbits, i), format, image_at(image, dst, off));
    }
    __syncthreads();
    wire_store_run(dst, image, total);
}

/* ranges[2 e] = where entry e's bytes start in the stream, ranges[2 e + 1] = how many they are (0xffffffff: its records
 * are not among the piece's, which the host reports) */
__global__ void __launch_bounds__(WT) msd_gro_ranges_kernel(const unsigned long long *ctr, uint32_t n, const uint32_t *count,
                                                            uint32_t bound, const uint32_t *starts,
                                                            const uint32_t *stream_len, uint32_t *ranges)
{
    const uint32_t e = blockIdx.x * WT + threadIdx.x;
    if (e >= n)
        return;
    const uint32_t cnt = min(*count, bound);
    const unsigned long long r0 = ctr[(size_t)e * CW + MSD_GB_CTR_REC_FIRST], r1 = r0 + ctr[(size_t)e * CW + MSD_FR_CTR_RECORDS];
    if (r1 > cnt) {
        ranges[2 * e] = 0;
        ranges[2 * e + 1] = 0xffffffffu;
        return;
    }
    const uint32_t b0 = r0 < cnt ? starts[r0] : *stream_len, b1 = r1 < cnt ? starts[r1] : *stream_len;
    ranges[2 * e] = b0;
    ranges[2 * e + 1] = b1 - b0;
}

} // namespace

extern "C" int msd_gro_launch_fields(const msd_message *out, const uint32_t *count, uint32_t bound, msd_fields *fields,
                                     void *stream)
{
    if (bound == 0)
        return 0;
    hipLaunchKernelGGL(msd_gro_fields_kernel, dim3((bound + WT - 1) / WT), dim3(WT), 0, (hipStream_t)stream, out, count,
                       bound, fields);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int msd_gro_launch_wire(const msd_message *out, const uint32_t *count, uint32_t bound,
                                   const unsigned long long *ctr, uint32_t n, int format, const uint8_t *errbits, uint8_t *lens,
                                   uint32_t *block_sums, uint32_t *starts, uint8_t *bytes, uint32_t *ranges, void *stream)
{
    if (bound == 0 || n == 0)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nblocks = (bound + WT - 1) / WT;
    hipLaunchKernelGGL(msd_gro_len_kernel, dim3(nblocks), dim3(WT), 0, st, out, count, bound, format, errbits, lens,
                       block_sums);
    hipLaunchKernelGGL(scan_kernel<>, dim3(1), dim3(WT), 0, st, block_sums, nblocks);
    hipLaunchKernelGGL(msd_gro_store_kernel, dim3(nblocks), dim3(WT), 0, st, out, count, bound, format, errbits, lens,
                       block_sums, bytes, starts);
    hipLaunchKernelGGL(msd_gro_ranges_kernel, dim3((n + WT - 1) / WT), dim3(WT), 0, st, ctr, n, count, bound, starts,
                       block_sums + nblocks, ranges);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
