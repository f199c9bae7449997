/*
 * msd_reduce_kernels.hip -- the compacting Beast writer of the reduced output (modes_hip.h "Reduced Beast output").
 *
 * msd_pos_reduce_wire (msd_pos.cpp): n records and their verdict bytes -> one dense stream of the records that pass the
 * delivery conditions, in record order.  The three steps of msd_wire_encode (msd_wire_kernels.hip) with the verdict in
 * front: msd_reduce_len_kernel leaves a length per record -- 0 for one that stays behind -- and a sum per workgroup of
 * 256, scan_kernel (msd_wire_store_impl.h) turns the sums into offsets (one workgroup), msd_reduce_store_kernel encodes into LDS and
 * stores through wire_store_run as whole-wavefront runs of aligned dwords.  No place is handed out by an atomic: a
 * record's offset is a prefix sum, so the stream is the same on every run.
 */
#include "msd_pos.h"
#include "msd_wire_store_impl.h"

namespace {

using namespace msd_wire_store; /* WT, IMAGE_WORDS, block_scan, scan_kernel, image_at, wire_store_run */

/* mode_s.c:2164-2172 and net_io.c:1282: the verdict says forward, and the aircraft has been seen twice unless
 * --net-verbatim or --net-only; msd_wire_source adds net_io.c:1278's correctedbits < 2 unless --net-verbatim */
__device__ __forceinline__ bool delivered(uint32_t verdict, uint32_t flags)
{
    return (verdict & MSD_REDUCE_FORWARD) &&
           ((flags & (MSD_WIRE_VERBATIM | MSD_REDUCE_NET_ONLY)) || (verdict & MSD_REDUCE_SEEN_TWICE));
}

__global__ void __launch_bounds__(WT) msd_reduce_len_kernel(const msd_message *msgs, const uint8_t *forward, uint32_t n,
                                                            uint32_t flags, uint8_t *lens, uint32_t *block_sums)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        if (delivered(forward[i], flags)) {
            const msd_message mm = msgs[i];
            len = msd_wire_length(msd_wire_source(mm, (flags & MSD_WIRE_VERBATIM) != 0, false, 0xffu, 0xffu), MSD_WIRE_BEAST);
        }
        lens[i] = (uint8_t)len;
    }
    uint32_t total;
    (void)block_scan<WT>(len, part, total);
    if (threadIdx.x == 0)
        block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(WT) msd_reduce_store_kernel(const msd_message *msgs, uint32_t n, uint32_t flags,
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
        ends[i] = block_off[blockIdx.x] + off + len;
        if (len) { /* a length above 0 says the record is delivered */
            const msd_message mm = msgs[i];
            msd_wire_put(msd_wire_source(mm, (flags & MSD_WIRE_VERBATIM) != 0, false, 0xffu, 0xffu), MSD_WIRE_BEAST,
                         image_at(image, dst, off));
        }
    }
    __syncthreads();
    wire_store_run(dst, image, total);
}

} // namespace

void msd_reduce_launch_lengths(hipStream_t stream, const msd_message *msgs, const uint8_t *forward, uint32_t n, uint32_t flags,
                               uint8_t *lens, uint32_t *block_sums)
{
    const uint32_t nblocks = (n + WT - 1u) / WT;
    msd_reduce_len_kernel<<<nblocks, WT, 0, stream>>>(msgs, forward, n, flags, lens, block_sums);
    scan_kernel<><<<1, WT, 0, stream>>>(block_sums, nblocks);
}

void msd_reduce_launch_store(hipStream_t stream, const msd_message *msgs, uint32_t n, uint32_t flags, const uint8_t *lens,
                             const uint32_t *block_off, uint8_t *out, uint32_t *ends)
{
    msd_reduce_store_kernel<<<(n + WT - 1u) / WT, WT, 0, stream>>>(msgs, n, flags, lens, block_off, out, ends);
}
