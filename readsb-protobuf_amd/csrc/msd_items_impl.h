/* msd_items_impl.h -- what the writers over ITEMS share (msd_pb_kernels.hip, msd_vrs_kernels.hip): the items of a call
 * -- every receiver's marks and every live aircraft, in stream order -- and the store of a workgroup's 256 items through
 * an LDS image of half as many.  Device code only. */
#ifndef MSD_ITEMS_IMPL_H
#define MSD_ITEMS_IMPL_H

#include "msd_wire_store_impl.h"

namespace msd_items {

using namespace msd_wire_store;

constexpr uint32_t HEAD = 0x80000000u; /* an item that is a receiver's head; the low bits are the receiver */
constexpr uint32_t TAIL = 0x40000000u; /* its tail */

/* idx: the live slots ordered by (receiver, address).  first[r] is the place of receiver r's first aircraft (a binary
 * search per receiver; first[nrx] = live).  A receiver has MARKS items of its own: with 1 a head, item first[r] + r; with
 * 2 a head, item first[r] + 2r, and a tail, the item in front of the next head.  The aircraft at place j, of receiver r,
 * is item j + MARKS * r + 1 (a scatter per aircraft). */
template <uint32_t MARKS>
__global__ void __launch_bounds__(WT)
items_kernel(const uint64_t *keys, const uint32_t *idx, uint32_t live, uint32_t nrx, uint32_t *first, uint32_t *items)
{
    static_assert(MARKS == 1u || MARKS == 2u, "a head, or a head and a tail");
    const uint32_t g = blockIdx.x * WT + threadIdx.x;
    if (g <= nrx) { /* the first place whose receiver is g or above; first[nrx] = live */
        uint32_t lo = 0, hi = live;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if ((keys[idx[mid]] >> 25) < g)
                lo = mid + 1u;
            else
                hi = mid;
        }
        first[g] = lo;
        if (g < nrx)
            items[lo + MARKS * g] = HEAD | g;
        if (MARKS == 2u && g > 0)
            items[lo + 2u * g - 1u] = TAIL | (g - 1u);
    }
    if (g < live) {
        const uint64_t r = keys[idx[g]] >> 25;
        if (r < nrx) /* (every key's receiver is: msd_pos_update refuses any other) */
            items[g + MARKS * (uint32_t)r + 1u] = g;
    }
}

/* The store of a workgroup whose items are too long for an image of all 256: the image holds TILE = 128 of them, and the
 * workgroup fills and stores it twice, lanes 0-127 then lanes 128-255; all 256 threads store both times.  len: this
 * lane's item's bytes (0: it writes nothing); encode(i, at) writes item i at `at`, and is called for the items with a
 * length alone.  part (4 words), half (one) and image are the kernel's LDS: an image of TILE longest items and one more,
 * from the destination's offset in its dword.  The order of the barriers is the point: half is read behind one; an image
 * is stored behind one and written again behind the next. */
template <uint32_t TILE, typename Encode>
__device__ __forceinline__ void tiled_store(uint32_t len, uint8_t *out, const uint32_t *block_off, uint32_t *part, uint32_t &half,
                                            uint32_t *image, Encode encode)
{
    static_assert(WT == 2u * TILE, "a workgroup fills the image twice");
    uint32_t total;
    const uint32_t off = block_scan<WT>(len, part, total);
    if (threadIdx.x == TILE)
        half = off; /* the bytes of the workgroup's first TILE items */
    __syncthreads();
    const uint32_t first_bytes = half;
    uint8_t *const dst0 = out + block_off[blockIdx.x];
    for (uint32_t round = 0; round < 2u; ++round) {
        uint8_t *const dst = round ? dst0 + first_bytes : dst0;
        const uint32_t run = round ? total - first_bytes : first_bytes;
        if (threadIdx.x / TILE == round && len)
            encode(blockIdx.x * WT + threadIdx.x, image_at(image, dst, round ? off - first_bytes : off));
        __syncthreads();
        wire_store_run(dst, image, run);
        __syncthreads();
    }
}

} // namespace msd_items

#endif
