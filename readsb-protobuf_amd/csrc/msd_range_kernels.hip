/*
 * msd_range_kernels.hip -- the writer of Statistics.polar_range (modes_hip.h "Receiver range", msd_pos_range_pb).
 *
 * The entries of a call are the 72 buckets of every receiver, in order: entry i is bucket i % 72 of receiver i / 72.  The
 * three steps of the reduced Beast writer (msd_reduce_kernels.hip) over them: msd_range_pb_len_kernel leaves a length per
 * entry -- 2 to 10 bytes, never 0 -- and a sum per workgroup of 256, scan_kernel (msd_wire_store_impl.h) turns the sums into
 * offsets (one workgroup), msd_range_pb_store_kernel encodes into LDS and stores through wire_store_run as whole-wavefront
 * runs of aligned dwords; the lane of a receiver's last bucket leaves the receiver's end offset.  No place is handed out
 * by an atomic.  Both kernels run msd_range_pb_entry (msd_pb_impl.h), the length kernel with no destination.
 */
#include "msd_pos.h"
#include "msd_pb_impl.h"
#include "msd_wire_store_impl.h"

namespace {

using namespace msd_wire_store; /* WT, IMAGE_WORDS, block_scan, scan_kernel, image_at, wire_store_run */

static_assert(MSD_RANGE_PB_ENTRY_MAX <= MSD_WIRE_MAX, "an entry fits the image's share of a lane");

__global__ void __launch_bounds__(WT)
msd_range_pb_len_kernel(const msd_range_state *rng, uint32_t n, uint8_t *lens, uint32_t *block_sums)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        len = msd_range_pb_entry(i % MSD_RANGE_BUCKETS, rng[i / MSD_RANGE_BUCKETS].polar[i % MSD_RANGE_BUCKETS], nullptr);
        lens[i] = (uint8_t)len;
    }
    uint32_t total;
    (void)block_scan<WT>(len, part, total);
    if (threadIdx.x == 0)
        block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(WT)
msd_range_pb_store_kernel(const msd_range_state *rng, uint32_t n, const uint8_t *lens, const uint32_t *block_off, uint8_t *out,
                          unsigned long long *end)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t image[IMAGE_WORDS];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    const uint32_t len = i < n ? lens[i] : 0u;
    uint32_t total;
    const uint32_t off = block_scan<WT>(len, part, total);
    uint8_t *dst = out + block_off[blockIdx.x];
    if (i < n) {
        const uint32_t r = i / MSD_RANGE_BUCKETS, b = i % MSD_RANGE_BUCKETS;
        (void)msd_range_pb_entry(b, rng[r].polar[b], image_at(image, dst, off));
        if (b == MSD_RANGE_BUCKETS - 1u)
            end[r] = (unsigned long long)block_off[blockIdx.x] + off + len;
    }
    __syncthreads();
    wire_store_run(dst, image, total);
}

} // namespace

void msd_range_pb_launch_lengths(hipStream_t stream, const msd_range_state *rng, uint32_t nrx, uint8_t *lens, uint32_t *block_sums)
{
    const uint32_t n = nrx * MSD_RANGE_BUCKETS, nblocks = (n + WT - 1u) / WT;
    msd_range_pb_len_kernel<<<nblocks, WT, 0, stream>>>(rng, n, lens, block_sums);
    scan_kernel<><<<1, WT, 0, stream>>>(block_sums, nblocks);
}

void msd_range_pb_launch_store(hipStream_t stream, const msd_range_state *rng, uint32_t nrx, const uint8_t *lens,
                               const uint32_t *block_off, uint8_t *out, unsigned long long *end)
{
    const uint32_t n = nrx * MSD_RANGE_BUCKETS;
    msd_range_pb_store_kernel<<<(n + WT - 1u) / WT, WT, 0, stream>>>(rng, n, lens, block_off, out, end);
}
