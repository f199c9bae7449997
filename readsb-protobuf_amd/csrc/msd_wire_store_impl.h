/* msd_wire_store_impl.h -- how the wire kernels lay a stream out and store it: the workgroup scan over the messages'
 * lengths and the scan over the workgroups' sums (msd_block_scan_impl.h), and the LDS image of up to 256 messages that
 * leaves as whole-wavefront runs of consecutive aligned dwords (the destination may be host memory, where a store per
 * message byte would cost a PCIe write each).  Shared by msd_wire_kernels.hip, msd_group_remote_out_kernels.hip and the
 * position tracker's four writers (msd_reduce_kernels.hip, msd_sbs_kernels.hip, msd_pb_kernels.hip,
 * msd_vrs_kernels.hip).  Device code only. */
#ifndef MSD_WIRE_STORE_IMPL_H
#define MSD_WIRE_STORE_IMPL_H

#include <hip/hip_runtime.h>

#include "msd_block_scan_impl.h"
#include "msd_wire_impl.h"

namespace msd_wire_store {

/* threads, and messages per LDS image; tests/test_gpu_receiver_group_remote_wire.py sizes its entries around this value
 * (its B) to meet the workgroup seams: change both together */
constexpr uint32_t WT = 256;
constexpr uint32_t IMAGE_WORDS = WT * MSD_WIRE_MAX / 4 + 2; /* the image starts at the destination's offset in its dword */

/* the workgroup scan over the messages' lengths and the scan over the workgroups' sums; the writers call both at WT */
using msd_block_scan::block_scan;
using msd_block_scan::block_sums_scan;

/* The scan step of every writer, one workgroup: each of ARRAYS consecutive arrays of nblocks + 1 words, as block_sums_scan
 * leaves it. */
template <uint32_t ARRAYS = 1> __global__ void __launch_bounds__(WT) scan_kernel(uint32_t *block_sums, uint32_t nblocks)
{
    __shared__ uint32_t part[4];
    for (uint32_t q = 0; q < ARRAYS; ++q)
        block_sums_scan<WT>(block_sums + q * (nblocks + 1u), nblocks, part);
}

/* Where thread t's bytes go in the image of a run that will be stored at dst: the image mirrors the destination's
 * alignment, byte j of it is byte j - (dst & 3) of the run. */
__device__ __forceinline__ uint8_t *image_at(uint32_t *image, const uint8_t *dst, uint32_t off)
{
    return reinterpret_cast<uint8_t *>(image) + (reinterpret_cast<uintptr_t>(dst) & 3u) + off;
}

/* The len bytes of the image to dst .. dst + len: the aligned dwords inside the run by the whole workgroup, lane after
 * lane; the bytes in front of the first and behind the last of them one by one (at most three each).  Needs a barrier
 * between the image's writes and the call, and one before the image is written again. */
__device__ inline void wire_store_run(uint8_t *dst, const uint32_t *image, uint32_t len)
{
    const uint32_t start = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u), end = start + len;
    const uint32_t w0 = (start + 3u) / 4u, w1 = end / 4u;
    const uint32_t head_end = min(4u * w0, end), tail_begin = max(4u * w1, head_end);
    uint8_t *base = dst - start; /* dword-aligned */
    uint32_t *d32 = reinterpret_cast<uint32_t *>(base);
    for (uint32_t w = w0 + threadIdx.x; w < w1; w += WT)
        d32[w] = image[w];
    const uint8_t *ib = reinterpret_cast<const uint8_t *>(image);
    const uint32_t j = threadIdx.x;
    if (start + j < head_end)
        base[start + j] = ib[start + j];
    if (j >= 4 && tail_begin + (j - 4) < end) /* (other lanes than the head's) */
        base[tail_begin + (j - 4)] = ib[tail_begin + (j - 4)];
}

} // namespace msd_wire_store

#endif
