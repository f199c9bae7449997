/*
 * msd_vrs_kernels.hip -- the compacting writer of the VRS feed (modes_hip.h "VRS output"): one part of every receiver's
 * JSON aircraft list from the aircraft table, one dense stream.
 *
 * msd_pos_vrs (msd_pos.cpp) orders the live slots by (receiver, address) with the snapshot's passes and then follows the
 * aircraft.pb writer (msd_pb_kernels.hip) over ITEMS.  The items of a call are, per receiver, a head (`{"acList":[`), its
 * live aircraft and a tail (`]}\n`), in stream order: with first[r] the place of receiver r's first aircraft in the ordered
 * list, r's head is item first[r] + 2r, the aircraft at place j, of receiver r, is item j + 2r + 1, r's tail is item
 * first[r + 1] + 2r + 1.  So an empty receiver still has its 14 bytes, and every place in the stream is a prefix sum over
 * items -- none is handed out by an atomic, the stream is the same on every run.
 * What pb does not have is the comma: an object carries one in front unless it is the first SELECTED aircraft of its
 * document, so an aircraft's length depends on whether any aircraft between its receiver's head and itself was selected.
 * That is a difference of two prefix counts, and a count across workgroups exists only after a scan; so there are two
 * length passes:
 *   items_kernel<2>        first[] by a binary search per receiver, the items by a scatter per aircraft (msd_items_impl.h)
 *   msd_vrs_select_kernel  one lane per item.  An aircraft's lane reads its entry once, where it lies, decides selection
 *                          and leaves the object's length without a comma (0: not written); per item the selected
 *                          aircraft before it inside its workgroup, per workgroup their sum
 *   scan_kernel            the sums into offsets (one workgroup; msd_wire_store_impl.h)
 *   msd_vrs_len_kernel     one lane per item: selected before me minus selected before my receiver's head says whether the
 *                          comma is there (bit 15 of the length); the bytes before the item inside its workgroup, per
 *                          workgroup their sum.  Of the table it reads a selected aircraft's key alone
 *   scan_kernel            again, over the bytes
 *   msd_vrs_rx_kernel      one lane per receiver: its row from the prefixes at its head's item and at the next head's
 *   msd_vrs_store_kernel   lanes write into an LDS image, tiled_store (msd_items_impl.h) stores it as whole-wavefront runs of
 *                          aligned dwords
 * Both object passes run msd_vrs_aircraft (msd_vrs_impl.h), the select kernel with no destination: a length is by
 * construction what the store kernel writes.  No kernel changes the table: the call is stateless.
 * The image.  An object is at most MSD_VRS_AIRCRAFT_MAX = 418 bytes, three more than an aircraft.pb entry, and the
 * image still holds what pb's does: VRS_TILE = 128 items, 53.9 KB, three workgroups, twelve wavefronts, per CU of 160 KB
 * (3 x 53 952 = 161 856 of 163 840 bytes) -- the pb store kernel's occupancy.  A workgroup keeps the writers' 256
 * threads (block_scan and wire_store_run are built on them) and fills and stores the image twice (tiled_store).
 */
#include "msd_pos.h"
#include "msd_vrs_impl.h"
#include "msd_items_impl.h"

namespace {

using namespace msd_items; /* HEAD, TAIL, items_kernel, tiled_store; of msd_wire_store: WT, block_scan, scan_kernel */

constexpr uint32_t VRS_TILE = MSD_VRS_TILE;
constexpr uint32_t VRS_COMMA = 0x8000u;    /* in a length: the object has its comma; the low bits include it */
static_assert(MSD_VRS_HEAD_LEN <= MSD_VRS_AIRCRAFT_MAX && MSD_VRS_AIRCRAFT_MAX < VRS_COMMA, "an item is at most an object");
/* the image starts at the destination's offset in its dword; behind the tile's longest items there is room for one more */
constexpr uint32_t VRS_IMAGE_WORDS = (VRS_TILE * MSD_VRS_AIRCRAFT_MAX + MSD_VRS_AIRCRAFT_MAX + 3u) / 4u + 2u;

__global__ void __launch_bounds__(WT)
msd_vrs_select_kernel(msd_vrs_call c, uint16_t *lens, uint16_t *swithin, uint32_t *sel_sums)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0, selected = 0;
    if (i < c.nitems) {
        const uint32_t item = c.items[i];
        if (item & HEAD) {
            len = MSD_VRS_HEAD_LEN;
        } else if (item & TAIL) {
            len = MSD_VRS_TAIL_LEN;
        } else {
            const uint32_t s = c.idx[item];
            msd_vrs_head h;
            msd_vrs_head_of_state(c.t.keys[s], &c.t.st[s], &h);
            if (msd_vrs_selected(&h, c.now_ms, c.part, c.part_shift)) {
                len = msd_vrs_aircraft(&h, &c.t.trk[s], c.now_ms, 0, c.track_table, nullptr);
                selected = 1u;
            }
        }
        lens[i] = (uint16_t)len;
    }
    uint32_t total;
    const uint32_t before = block_scan<WT>(selected, part, total);
    if (i < c.nitems)
        swithin[i] = (uint16_t)before;
    if (threadIdx.x == 0)
        sel_sums[blockIdx.x] = total;
}

/* the selected aircraft in front of item i (i == nitems: all of them) */
__device__ __forceinline__ uint32_t vrs_selected_before(uint32_t i, uint32_t nitems, const uint16_t *swithin, const uint32_t *sel_sums,
                                                         uint32_t nblocks)
{
    return i >= nitems ? sel_sums[nblocks] : sel_sums[i / WT] + swithin[i];
}

__global__ void __launch_bounds__(WT)
msd_vrs_len_kernel(msd_vrs_call c, uint16_t *lens, const uint16_t *swithin, const uint32_t *sel_sums, uint32_t *within,
                   uint32_t *byte_sums, uint32_t nblocks)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0;
    if (i < c.nitems) {
        len = lens[i];
        const uint32_t item = c.items[i];
        if (len && !(item & (HEAD | TAIL))) {
            const uint32_t r = (uint32_t)(c.t.keys[c.idx[item]] >> 25);
            const uint32_t head = c.first[r] + 2u * r;
            if (vrs_selected_before(i, c.nitems, swithin, sel_sums, nblocks) !=
                vrs_selected_before(head, c.nitems, swithin, sel_sums, nblocks)) {
                len += 1u;
                lens[i] = (uint16_t)(len | VRS_COMMA);
            }
        }
    }
    uint32_t total;
    const uint32_t off = block_scan<WT>(len, part, total);
    if (i < c.nitems)
        within[i] = off;
    if (threadIdx.x == 0)
        byte_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(WT)
msd_vrs_rx_kernel(const uint32_t *first, uint32_t nrx, uint32_t nitems, const uint16_t *swithin, const uint32_t *sel_sums,
                  const uint32_t *within, const uint32_t *byte_sums, uint32_t nblocks, msd_vrs_receiver *rx)
{
    const uint32_t r = blockIdx.x * WT + threadIdx.x;
    if (r >= nrx)
        return;
    const uint32_t i0 = first[r] + 2u * r, i1 = first[r + 1u] + 2u * r + 2u; /* this head's item, the next one's (or nitems) */
    msd_vrs_receiver row;
    row.end = i1 >= nitems ? byte_sums[nblocks] : byte_sums[i1 / WT] + within[i1];
    row.aircraft = vrs_selected_before(i1, nitems, swithin, sel_sums, nblocks) -
                   vrs_selected_before(i0, nitems, swithin, sel_sums, nblocks);
    row.reserved = 0;
    rx[r] = row;
}

__global__ void __launch_bounds__(WT)
msd_vrs_store_kernel(msd_vrs_call c, const uint16_t *lens, const uint32_t *block_off, uint8_t *out)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t half;
    __shared__ uint32_t image[VRS_IMAGE_WORDS];
    const uint32_t me = blockIdx.x * WT + threadIdx.x;
    const uint32_t coded = me < c.nitems ? lens[me] : 0u;
    /* (a length above 0: a head, a tail, a selected aircraft) */
    tiled_store<VRS_TILE>(coded & (VRS_COMMA - 1u), out, block_off, part, half, image, [&](uint32_t i, uint8_t *at) {
        const uint32_t item = c.items[i];
        if (item & HEAD) {
            (void)msd_vrs_head_text(at);
        } else if (item & TAIL) {
            (void)msd_vrs_tail_text(at);
        } else {
            const uint32_t s = c.idx[item];
            msd_vrs_head h;
            msd_vrs_head_of_state(c.t.keys[s], &c.t.st[s], &h);
            (void)msd_vrs_aircraft(&h, &c.t.trk[s], c.now_ms, (coded & VRS_COMMA) != 0, c.track_table, at);
        }
    });
}

} // namespace

void msd_vrs_launch_lengths(hipStream_t stream, msd_vrs_call c, uint32_t live, uint32_t *first, uint32_t *items, uint16_t *lens,
                            uint16_t *swithin, uint32_t *within, uint32_t *sel_sums, uint32_t *byte_sums, msd_vrs_receiver *rx)
{
    const uint32_t nblocks = (c.nitems + WT - 1u) / WT;
    const uint32_t most = live > c.nrx + 1u ? live : c.nrx + 1u;
    items_kernel<2><<<(most + WT - 1u) / WT, WT, 0, stream>>>(c.t.keys, c.idx, live, c.nrx, first, items);
    msd_vrs_select_kernel<<<nblocks, WT, 0, stream>>>(c, lens, swithin, sel_sums);
    scan_kernel<><<<1, WT, 0, stream>>>(sel_sums, nblocks);
    msd_vrs_len_kernel<<<nblocks, WT, 0, stream>>>(c, lens, swithin, sel_sums, within, byte_sums, nblocks);
    scan_kernel<><<<1, WT, 0, stream>>>(byte_sums, nblocks);
    msd_vrs_rx_kernel<<<(c.nrx + WT - 1u) / WT, WT, 0, stream>>>(first, c.nrx, c.nitems, swithin, sel_sums, within, byte_sums, nblocks, rx);
}

void msd_vrs_launch_store(hipStream_t stream, msd_vrs_call c, const uint16_t *lens, const uint32_t *block_off, uint8_t *out)
{
    msd_vrs_store_kernel<<<(c.nitems + WT - 1u) / WT, WT, 0, stream>>>(c, lens, block_off, out);
}
