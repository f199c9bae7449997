/*
 * msd_pb_kernels.hip -- the compacting writer of aircraft.pb (modes_hip.h "aircraft.pb"): every receiver's file from the
 * aircraft table, one dense stream.
 *
 * msd_pos_aircraft_pb (msd_pos.cpp) orders the live slots by (receiver, address) with the snapshot's passes and then runs
 * the SBS writer's three steps over ITEMS instead of records.  The items of a call are every receiver's file head and
 * every live aircraft, in stream order: receiver r's head is item first[r] + r, the aircraft at place j of the ordered
 * list, of receiver r, is item j + r + 1, where first[r] is the place of r's first aircraft (items_kernel<1>,
 * msd_items_impl.h: a binary search per receiver, a scatter per aircraft).  So an empty receiver still has its head, and every place in the stream
 * is a prefix sum over items -- none is handed out by an atomic, the stream is the same on every run.
 *   msd_pb_len_kernel    one lane per item.  An aircraft's lane reads its entry once, where it lies -- the position state
 *                        and the 592-byte table entry are picked over member by member, not copied --, decides selection,
 *                        leaves the next written state in the call's shadow copy and a 16-bit length (0: not written);
 *                        per item the exclusive prefix inside its workgroup of the bytes and of the three counts (written,
 *                        with position, TIS-B; packed, at most 256 each), per workgroup their sums.
 *   scan_kernel<4>       the four sums into offsets (one workgroup; msd_wire_store_impl.h).
 *   msd_pb_rx_kernel     one lane per receiver: its row from the prefixes at its head's item and at the next head's.
 *   msd_pb_store_kernel  lanes encode into an LDS image, tiled_store (msd_items_impl.h) stores it as whole-wavefront runs
 *                        of aligned dwords; an aircraft's lane then commits its shadow state to the slot.  Only a call that fits
 *                        its buffer launches it, so a refused call moves no state.
 * Both encoding kernels run msd_pb_aircraft / msd_pb_header (msd_pb_impl.h), the length kernel with no destination: a
 * length is by construction what the store kernel writes.
 * A tracker that keeps the receiver range hands over its distances (c.dist): the entry then has distance (13) and can be
 * MSD_PB_AIRCRAFT_MAX_RANGE = 421 bytes long, and the store kernel's instantiation with the larger image runs; a tracker
 * without runs the one it always ran.
 * The image.  An entry is at most MSD_PB_AIRCRAFT_MAX = 415 bytes; 256 of them are 106 KB, one workgroup per CU of 160 KB.
 * The image therefore holds PB_TILE = 128 items, 53.6 KB: three workgroups, twelve wavefronts, per CU.  A workgroup keeps
 * the writers' 256 threads (block_scan and wire_store_run are built on them) and fills and stores the image twice
 * (tiled_store).  64 items would allow six workgroups, but the encoder's
 * dependent byte stores into LDS, not the wavefront count, bound the kernel, and four rounds cost two more barriers each.
 * The written state lies beside the table, not in msd_pos_table: the position kernels are what they were.
 * msd_pb_fresh_kernel starts the state of a call's new aircraft at 0, msd_pb_move_kernel carries it into the rebuilt table.
 */
#include "msd_pos.h"
#include "msd_pb_impl.h"
#include "msd_items_impl.h"

namespace {

using namespace msd_items; /* HEAD, items_kernel, tiled_store; of msd_wire_store: WT, block_scan, scan_kernel */

constexpr uint32_t PB_TILE = MSD_PB_TILE;
static_assert(MSD_PB_HEADER_MAX <= MSD_PB_AIRCRAFT_MAX, "an item is at most an aircraft entry");
/* the image starts at the destination's offset in its dword; behind the tile's longest items there is room for one more */
constexpr uint32_t image_words(uint32_t entry_max)
{
    return (PB_TILE * entry_max + entry_max + 3u) / 4u + 2u;
}

__global__ void __launch_bounds__(WT)
msd_pb_len_kernel(msd_pb_call c, uint64_t *shadow, uint16_t *lens, uint32_t *within, uint32_t *cwithin, uint32_t *block_sums,
                  uint32_t nblocks)
{
    __shared__ uint32_t part[4];
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    uint32_t len = 0, counts = 0;
    if (i < c.nitems) {
        const uint32_t item = c.items[i];
        if (item & HEAD) {
            const uint32_t r = item & ~HEAD;
            len = msd_pb_header(c.now_ms, c.messages_total ? c.messages_total[r] : 0u, nullptr);
        } else {
            const uint32_t s = c.idx[item];
            msd_pb_head h;
            msd_pb_head_of_state(c.t.keys[s], &c.t.st[s], &h);
            if (c.dist)
                h.distance = c.dist[s];
            uint64_t st = c.state[s];
            if (msd_pb_selected(&h, c.now_ms)) {
                const msd_trk_aircraft *a = &c.t.trk[s];
                st = msd_pb_next_state(st, &h, a, c.now_ms);
                len = msd_pb_aircraft(&h, a, st, c.track_table, nullptr);
                counts = 1u;
                if (msd_pb_position_valid(&h, c.now_ms))
                    counts |= 1u << 10 | (h.position_source == 5u /* SOURCE_TISB */ ? 1u << 20 : 0u);
            }
            shadow[i] = st;
        }
        lens[i] = (uint16_t)len;
    }
    uint32_t total, ctotal;
    const uint32_t off = block_scan<WT>(len, part, total);
    const uint32_t coff = block_scan<WT>(counts, part, ctotal);
    if (i < c.nitems) {
        within[i] = off;
        cwithin[i] = coff;
    }
    if (threadIdx.x == 0) {
        const uint32_t stride = nblocks + 1u;
        block_sums[blockIdx.x] = total;
        block_sums[stride + blockIdx.x] = ctotal & 1023u;
        block_sums[2u * stride + blockIdx.x] = (ctotal >> 10) & 1023u;
        block_sums[3u * stride + blockIdx.x] = ctotal >> 20;
    }
}

__device__ __forceinline__ uint32_t pb_prefix(uint32_t q, uint32_t i, uint32_t nitems, const uint32_t *within,
                                               const uint32_t *cwithin, const uint32_t *block_sums, uint32_t nblocks)
{
    const uint32_t *sums = block_sums + q * (nblocks + 1u);
    if (i >= nitems)
        return sums[nblocks];
    const uint32_t w = q == 0 ? within[i] : (cwithin[i] >> (10u * (q - 1u))) & 1023u;
    return sums[i / WT] + w;
}

__global__ void __launch_bounds__(WT)
msd_pb_rx_kernel(const uint32_t *first, uint32_t nrx, uint32_t nitems, const uint32_t *within, const uint32_t *cwithin,
                 const uint32_t *block_sums, uint32_t nblocks, msd_pb_receiver *rx)
{
    const uint32_t r = blockIdx.x * WT + threadIdx.x;
    if (r >= nrx)
        return;
    const uint32_t i0 = first[r] + r, i1 = first[r + 1u] + r + 1u; /* this head's item, the next one's (or nitems) */
    msd_pb_receiver row;
    row.end = pb_prefix(0, i1, nitems, within, cwithin, block_sums, nblocks);
    row.aircraft = pb_prefix(1, i1, nitems, within, cwithin, block_sums, nblocks) -
                   pb_prefix(1, i0, nitems, within, cwithin, block_sums, nblocks);
    row.with_positions = pb_prefix(2, i1, nitems, within, cwithin, block_sums, nblocks) -
                         pb_prefix(2, i0, nitems, within, cwithin, block_sums, nblocks);
    row.tisb_positions = pb_prefix(3, i1, nitems, within, cwithin, block_sums, nblocks) -
                         pb_prefix(3, i0, nitems, within, cwithin, block_sums, nblocks);
    row.reserved = 0;
    rx[r] = row;
}

template <uint32_t ENTRY_MAX>
__global__ void __launch_bounds__(WT)
msd_pb_store_kernel(msd_pb_call c, const uint64_t *shadow, const uint16_t *lens, const uint32_t *block_off, uint8_t *out)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t half;
    __shared__ uint32_t image[image_words(ENTRY_MAX)];
    const uint32_t me = blockIdx.x * WT + threadIdx.x;
    /* (a length above 0: a head with something to say, a selected aircraft) */
    tiled_store<PB_TILE>(me < c.nitems ? lens[me] : 0u, out, block_off, part, half, image, [&](uint32_t i, uint8_t *at) {
        const uint32_t item = c.items[i];
        if (item & HEAD) {
            const uint32_t r = item & ~HEAD;
            (void)msd_pb_header(c.now_ms, c.messages_total ? c.messages_total[r] : 0u, at);
        } else {
            const uint32_t s = c.idx[item];
            const uint64_t st = shadow[i];
            msd_pb_head h;
            msd_pb_head_of_state(c.t.keys[s], &c.t.st[s], &h);
            if (ENTRY_MAX > MSD_PB_AIRCRAFT_MAX)
                h.distance = c.dist[s];
            (void)msd_pb_aircraft(&h, &c.t.trk[s], st, c.track_table, at);
            c.state[s] = st;
        }
    });
}

__global__ void __launch_bounds__(WT)
msd_pb_fresh_kernel(const uint32_t *slot, const uint8_t *fresh, uint32_t n, uint32_t cap, uint64_t *state)
{
    const uint32_t i = blockIdx.x * WT + threadIdx.x;
    if (i < n && fresh[i] && slot[i] < cap)
        state[slot[i]] = 0;
}

/* every surviving aircraft of `from` is in `to` (msd_pos_launch_rebuild ran before): its state follows it */
__global__ void __launch_bounds__(WT)
msd_pb_move_kernel(const uint64_t *from_keys, const uint64_t *from_state, const uint64_t *to_keys, uint64_t *to_state, uint32_t cap)
{
    const uint32_t s = blockIdx.x * WT + threadIdx.x;
    if (s >= cap)
        return;
    const uint64_t key = from_keys[s];
    if (key >= MSD_POS_EMPTY - 1u) /* free, or expired */
        return;
    uint32_t d = msd_pos_hash(key) & (cap - 1u);
    for (uint32_t probes = 0; probes < cap; ++probes, d = (d + 1u) & (cap - 1u)) {
        const uint64_t k = to_keys[d];
        if (k == key) {
            to_state[d] = from_state[s];
            return;
        }
        if (k == MSD_POS_EMPTY)
            return;
    }
}

} // namespace

void msd_pb_launch_fresh(hipStream_t stream, const uint32_t *slot, const uint8_t *fresh, uint32_t n, uint32_t cap, uint64_t *state)
{
    msd_pb_fresh_kernel<<<(n + WT - 1u) / WT, WT, 0, stream>>>(slot, fresh, n, cap, state);
}

void msd_pb_launch_move(hipStream_t stream, msd_pos_table from, const uint64_t *from_state, msd_pos_table to, uint64_t *to_state)
{
    msd_pb_move_kernel<<<(from.cap + WT - 1u) / WT, WT, 0, stream>>>(from.keys, from_state, to.keys, to_state, from.cap);
}

void msd_pb_launch_lengths(hipStream_t stream, msd_pb_call c, uint32_t live, uint32_t *first, uint32_t *items, uint64_t *shadow,
                           uint16_t *lens, uint32_t *within, uint32_t *cwithin, uint32_t *block_sums, msd_pb_receiver *rx)
{
    const uint32_t nblocks = (c.nitems + WT - 1u) / WT;
    const uint32_t most = live > c.nrx + 1u ? live : c.nrx + 1u;
    items_kernel<1><<<(most + WT - 1u) / WT, WT, 0, stream>>>(c.t.keys, c.idx, live, c.nrx, first, items);
    msd_pb_len_kernel<<<nblocks, WT, 0, stream>>>(c, shadow, lens, within, cwithin, block_sums, nblocks);
    scan_kernel<4><<<1, WT, 0, stream>>>(block_sums, nblocks);
    msd_pb_rx_kernel<<<(c.nrx + WT - 1u) / WT, WT, 0, stream>>>(first, c.nrx, c.nitems, within, cwithin, block_sums, nblocks, rx);
}

void msd_pb_launch_store(hipStream_t stream, msd_pb_call c, const uint64_t *shadow, const uint16_t *lens, const uint32_t *block_off,
                         uint8_t *out)
{
    if (c.dist)
        msd_pb_store_kernel<MSD_PB_AIRCRAFT_MAX_RANGE><<<(c.nitems + WT - 1u) / WT, WT, 0, stream>>>(c, shadow, lens, block_off, out);
    else
        msd_pb_store_kernel<MSD_PB_AIRCRAFT_MAX><<<(c.nitems + WT - 1u) / WT, WT, 0, stream>>>(c, shadow, lens, block_off, out);
}
