/*
 * msd_history_kernels.hip -- the compacting writer of history_N.pb (modes_hip.h "history_N.pb"): every receiver's history
 * file from the aircraft table, one dense stream.
 *
 * msd_pos_history_pb (msd_pos.cpp) orders the live slots by (receiver, address) with the snapshot's passes and then follows
 * the aircraft.pb writer (msd_pb_kernels.hip) over ITEMS: every receiver's file head and every live aircraft, in stream
 * order -- receiver r's head is item first[r] + r, the aircraft at place j of the ordered list, of receiver r, is item
 * j + r + 1 (items_kernel<1>, msd_items_impl.h).  So an empty receiver still has its head, and every place in the stream is
 * a prefix sum over items -- none is handed out by an atomic, the stream is the same on every run.
 *   msd_history_len_kernel    one lane per item.  An aircraft's lane picks the members it needs where they lie -- key, seen,
 *                             messages, the position and its validity of the position state; of the 592-byte table entry
 *                             airground's, altitude_baro's and altitude_geom's validity, altitude_baro_reliable and the
 *                             three values (msd_history_altitude), nothing else and no copy --, decides selection and
 *                             leaves an 8-bit length (0: not written); per item the exclusive prefix inside its workgroup
 *                             of the bytes and of the written aircraft (16 bits each: at most 9 216 and 256), per
 *                             workgroup their sums.
 *   scan_kernel<2>            the two sums into offsets (one workgroup; msd_wire_store_impl.h).
 *   msd_history_rx_kernel     one lane per receiver: its row from the prefixes at its head's item and at the next head's.
 *   msd_history_store_kernel  lanes encode into an LDS image, wire_store_run stores it as whole-wavefront runs of aligned
 *                             dwords.
 * Both encoding kernels run msd_history_entry / msd_history_header (msd_history_impl.h), the length kernel with no
 * destination: a length is by construction what the store kernel writes.  No kernel changes the table or aircraft.pb's
 * written state: the call is stateless.
 * The image.  An entry is at most MSD_HISTORY_ENTRY_MAX = 36 bytes, so the image of a whole workgroup's 256 items is
 * 9 216 bytes: HISTORY_TILE = 256, the workgroup fills and stores its image once.  tiled_store (msd_items_impl.h) is the
 * store of a workgroup whose image holds half its items -- two fills, five barriers -- and is not used: the one round here
 * is block_scan, a barrier and wire_store_run, as in msd_range_kernels.hip.  With 9 224 bytes of image and 16 of `part` a
 * workgroup takes 9 248 bytes (the compiler's figure) of a CU's 160 KiB of LDS, which would allow seventeen; the CU's 32
 * wavefronts allow eight workgroups of 256 threads (73 984 bytes), and that cap, not the LDS, bounds the occupancy: eight
 * wavefronts per SIMD at 58 vector registers -- against three workgroups, twelve wavefronts, of aircraft.pb's store kernel.  A smaller tile would buy nothing: the wavefront cap is already reached.
 */
#include "msd_pos.h"
#include "msd_history_impl.h"
#include "msd_items_impl.h"

namespace {

using namespace msd_items; /* HEAD, items_kernel; of msd_wire_store: WT, block_scan, scan_kernel, image_at, wire_store_run */

constexpr uint32_t HISTORY_TILE = WT; /* items per LDS image: the whole workgroup's */
static_assert(MSD_HISTORY_HEADER_MAX <= MSD_HISTORY_ENTRY_MAX, "an item is at most an entry");
static_assert(MSD_HISTORY_ENTRY_MAX <= 255u && HISTORY_TILE * MSD_HISTORY_ENTRY_MAX <= 65535u, "8-bit lengths, 16-bit prefixes");
/* the image starts at the destination's offset in its dword */
constexpr uint32_t HISTORY_IMAGE_WORDS = HISTORY_TILE * MSD_HISTORY_ENTRY_MAX / 4u + 2u;

/* the length of item i, and with out its bytes; an aircraft that is not selected has none */
__device__ __forceinline__ uint32_t history_item(const msd_history_call &c, uint32_t i, uint8_t *out)
{
    const uint32_t item = c.items[i];
    if (item & HEAD)
        return msd_history_header(c.now_ms, out);
    const uint32_t s = c.idx[item];
    msd_pb_head h;
    msd_pb_head_of_state(c.t.keys[s], &c.t.st[s], &h);
    if (!msd_history_selected(&h, c.now_ms))
        return 0;
    return msd_history_entry(&h, msd_history_altitude(&c.t.trk[s], c.now_ms), out);
}

__global__ void __launch_bounds__(WT)
msd_history_len_kernel(msd_history_call c, uint8_t *lens, uint16_t *within, uint16_t *cwithin, uint32_t *block_sums, uint32_t nblocks)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0, written = 0;
    if (i < c.nitems) {
        len = history_item(c, i, nullptr);
        written = len != 0 && !(c.items[i] & HEAD);
        lens[i] = (uint8_t)len;
    }
    uint32_t total, ctotal;
    const uint32_t off = block_scan<WT>(len, part, total);
    const uint32_t coff = block_scan<WT>(written, part, ctotal);
    if (i < c.nitems) {
        within[i] = (uint16_t)off;
        cwithin[i] = (uint16_t)coff;
    }
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = total;
        block_sums[nblocks + 1u + blockIdx.x] = ctotal;
    }
}

/* the sum in front of item i (i == nitems: over all of them) of array q: 0 the bytes, 1 the written aircraft */
__device__ __forceinline__ uint32_t history_prefix(uint32_t q, uint32_t i, uint32_t nitems, const uint16_t *within,
                                                    const uint16_t *cwithin, const uint32_t *block_sums, uint32_t nblocks)
{
    const uint32_t *sums = block_sums + q * (nblocks + 1u);
    if (i >= nitems)
        return sums[nblocks];
    return sums[i / WT] + (q == 0 ? within[i] : cwithin[i]);
}

__global__ void __launch_bounds__(WT)
msd_history_rx_kernel(const uint32_t *first, uint32_t nrx, uint32_t nitems, const uint16_t *within, const uint16_t *cwithin,
                      const uint32_t *block_sums, uint32_t nblocks, msd_history_receiver *rx)
{
    const uint32_t r = blockIdx.x * WT + threadIdx.x;
    if (r >= nrx)
        return;
    const uint32_t i0 = first[r] + r, i1 = first[r + 1u] + r + 1u; /* this head's item, the next one's (or nitems) */
    msd_history_receiver row;
    row.end = history_prefix(0, i1, nitems, within, cwithin, block_sums, nblocks);
    row.aircraft = history_prefix(1, i1, nitems, within, cwithin, block_sums, nblocks) -
                   history_prefix(1, i0, nitems, within, cwithin, block_sums, nblocks);
    row.reserved = 0;
    rx[r] = row;
}

__global__ void __launch_bounds__(WT)
msd_history_store_kernel(msd_history_call c, const uint8_t *lens, const uint32_t *block_off, uint8_t *out)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t image[HISTORY_IMAGE_WORDS];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    const uint32_t len = i < c.nitems ? lens[i] : 0u;
    uint32_t total;
    const uint32_t off = block_scan<WT>(len, part, total);
    uint8_t *dst = out + block_off[blockIdx.x];
    if (len) /* (a head with something to say, a selected aircraft) */
        (void)history_item(c, i, image_at(image, dst, off));
    __syncthreads();
    wire_store_run(dst, image, total);
}

} // namespace

void msd_history_launch_lengths(hipStream_t stream, msd_history_call c, uint32_t live, uint32_t *first, uint32_t *items,
                                uint8_t *lens, uint16_t *within, uint16_t *cwithin, uint32_t *block_sums, msd_history_receiver *rx)
{
    const uint32_t nblocks = (c.nitems + WT - 1u) / WT;
    const uint32_t most = live > c.nrx + 1u ? live : c.nrx + 1u;
    items_kernel<1><<<(most + WT - 1u) / WT, WT, 0, stream>>>(c.t.keys, c.idx, live, c.nrx, first, items);
    msd_history_len_kernel<<<nblocks, WT, 0, stream>>>(c, lens, within, cwithin, block_sums, nblocks);
    scan_kernel<2><<<1, WT, 0, stream>>>(block_sums, nblocks);
    msd_history_rx_kernel<<<(c.nrx + WT - 1u) / WT, WT, 0, stream>>>(first, c.nrx, c.nitems, within, cwithin, block_sums, nblocks, rx);
}

void msd_history_launch_store(hipStream_t stream, msd_history_call c, const uint8_t *lens, const uint32_t *block_off, uint8_t *out)
{
    msd_history_store_kernel<<<(c.nitems + WT - 1u) / WT, WT, 0, stream>>>(c, lens, block_off, out);
}
