/*
 * msd_sbs_kernels.hip -- the compacting text writer of the SBS output (modes_hip.h "SBS output").
 *
 * msd_pos_sbs_wire (msd_pos.cpp): n records, their fields and their rows -> one dense stream of the lines of the records
 * that pass the delivery conditions, in record order.  The three steps of msd_reduce_kernels.hip with text in place of
 * frames: msd_sbs_len_kernel leaves a length per record -- 0 for one that writes nothing -- and a sum per workgroup of
 * 256, scan_kernel (msd_wire_store_impl.h) turns the sums into offsets (one workgroup), msd_sbs_store_kernel has every lane format its
 * record into the LDS image and stores the image through wire_store_run as whole-wavefront runs of aligned dwords.  No
 * place is handed out by an atomic: a record's offset is a prefix sum, so the stream is the same on every run.
 * Both kernels run msd_sbs_line (msd_sbs_impl.h): the length kernel with no destination, so that a length is by
 * construction what the store kernel writes.  Lines are 80 to MSD_SBS_MAX bytes, which a uint8_t length holds.
 * The image is 256 x MSD_SBS_MAX bytes, 37 KB of LDS: four workgroups, sixteen wavefronts, per CU of 160 KB.  The kernels
 * are bound by the formatting's integer divisions and byte stores into LDS, not by occupancy: one tile per workgroup,
 * WT as it is.
 */
#include "msd_pos.h"
#include "msd_sbs_impl.h"
#include "msd_wire_store_impl.h"

namespace {

using namespace msd_wire_store; /* WT, block_scan, scan_kernel, image_at, wire_store_run */

static_assert(MSD_SBS_MAX <= 255, "a line's length is kept in a byte");
/* the image starts at the destination's offset in its dword; behind the tile's 256 longest lines there is room for one
 * more, so that a record whose arrays changed between the two kernels cannot be formatted past the image */
constexpr uint32_t SBS_IMAGE_WORDS = (WT * MSD_SBS_MAX + MSD_SBS_MAX + 3u) / 4u + 2u;

__global__ void __launch_bounds__(WT)
msd_sbs_len_kernel(const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk, uint32_t n, msd_sbs_options opt,
                   const uint16_t *track_table, uint8_t *lens, uint32_t *block_sums)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        const msd_sbs_track row = trk[i];
        if (row.flags & MSD_SBS_TRACKED) { /* (a skipped record: its message and fields are not read) */
            const msd_message mm = msgs[i];
            const msd_fields f = fields[i];
            len = msd_sbs_line(&mm, &f, &row, opt.flags, opt.now_ms, opt.utc_offset_ms, track_table, nullptr);
        }
        lens[i] = (uint8_t)len;
    }
    uint32_t total;
    (void)block_scan<WT>(len, part, total);
    if (threadIdx.x == 0)
        block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(WT)
msd_sbs_store_kernel(const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk, uint32_t n, msd_sbs_options opt,
                     const uint16_t *track_table, const uint8_t *lens, const uint32_t *block_off, uint8_t *out, uint32_t *ends)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t image[SBS_IMAGE_WORDS];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    const uint32_t len = i < n ? lens[i] : 0u;
    uint32_t total;
    const uint32_t off = block_scan<WT>(len, part, total);
    uint8_t *dst = out + block_off[blockIdx.x];
    if (i < n) {
        ends[i] = block_off[blockIdx.x] + off + len;
        if (len) { /* a length above 0 says the record writes a line */
            const msd_message mm = msgs[i];
            const msd_fields f = fields[i];
            const msd_sbs_track row = trk[i];
            (void)msd_sbs_line(&mm, &f, &row, opt.flags, opt.now_ms, opt.utc_offset_ms, track_table, image_at(image, dst, off));
        }
    }
    __syncthreads();
    wire_store_run(dst, image, total);
}

} // namespace

void msd_sbs_launch_lengths(hipStream_t stream, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk,
                            uint32_t n, msd_sbs_options opt, const uint16_t *track_table, uint8_t *lens, uint32_t *block_sums)
{
    const uint32_t nblocks = (n + WT - 1u) / WT;
    msd_sbs_len_kernel<<<nblocks, WT, 0, stream>>>(msgs, fields, trk, n, opt, track_table, lens, block_sums);
    scan_kernel<><<<1, WT, 0, stream>>>(block_sums, nblocks);
}

void msd_sbs_launch_store(hipStream_t stream, const msd_message *msgs, const msd_fields *fields, const msd_sbs_track *trk,
                          uint32_t n, msd_sbs_options opt, const uint16_t *track_table, const uint8_t *lens,
                          const uint32_t *block_off, uint8_t *out, uint32_t *ends)
{
    msd_sbs_store_kernel<<<(n + WT - 1u) / WT, WT, 0, stream>>>(msgs, fields, trk, n, opt, track_table, lens, block_off, out, ends);
}
