/*
 * msd_group_beast_kernels.hip -- Beast input for every receiver of a group call at once (msd_group_accept_beast;
 * DESIGN.md 4.9, "Beast input per receiver").  The steps are those of msd_frames_kernels.hip, made
 * parallel across receivers the way that file makes them parallel within a stream:
 *  - a piece holds one segment per entry, each starting on a tile boundary, so a tile, its chain and its first-0x1A
 *    search belong to one receiver; the in-order reconciliation runs one wavefront per entry;
 *  - the decode runs one workgroup per tile with the entry's repair level and Mode A/C switch loaded once, and sums
 *    its counters in LDS before it adds them to the entry's own;
 *  - the first add is found per (entry, address); the ordered inserts run one workgroup per entry on an LDS copy of
 *    that receiver's active table; verdicts are per node against the entry's snapshot and stamps; the records are
 *    compacted over the whole piece, which is entry after entry in stream order.
 * The number of launches does not depend on the number of entries.
 */
#include <hip/hip_runtime.h>

#include "msd_frames_impl.h"
#include "msd_group_beast.h"

namespace {

constexpr uint32_t CW = MSD_FR_CTR_WORDS;
constexpr uint32_t TM = MSD_FR_TAIL_MAX;
constexpr unsigned long long VACANT64 = ~0ull;

__device__ __forceinline__ uint32_t seg_tile_end(uint32_t t, uint32_t s1)
{
    const uint32_t e = (t + 1u) * FT;
    return e < s1 ? e : s1;
}

/* the piece: every segment's kept frame, then its new bytes; one workgroup per tile */
__global__ void __launch_bounds__(NT) msd_gb_layout_kernel(const uint8_t *src, const msd_gb_entry *ent,
                                                          const uint32_t *tile_ent, const uint8_t *tails_in, uint8_t *buf)
{
    const uint32_t t = blockIdx.x, ei = tile_ent[t];
    const msd_gb_entry E = ent[ei];
    const uint32_t e = seg_tile_end(t, E.s1);
    const uint8_t *data = src + E.src;
    for (uint32_t i = t * FT + threadIdx.x; i < e; i += NT) {
        const uint32_t rel = i - E.s0;
        buf[i] = rel < E.tl ? tails_in[ei * TM + rel] : data[rel - E.tl];
    }
}

/* first 0x1A in each tile (0xFFFFFFFF: none) */
__global__ void __launch_bounds__(NT) msd_gb_tile_first_kernel(const uint8_t *buf, const msd_gb_entry *ent,
                                                              const uint32_t *tile_ent, uint32_t *first)
{
    __shared__ uint32_t best;
    const uint32_t t = blockIdx.x;
    if (threadIdx.x == 0)
        best = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t e = seg_tile_end(t, ent[tile_ent[t]].s1);
    for (uint32_t i = t * FT + threadIdx.x; i < e; i += NT)
        if (buf[i] == 0x1a) {
            atomicMin(&best, i);
            break;
        }
    __syncthreads();
    if (threadIdx.x == 0)
        first[t] = best;
}

/* per entry, over its own tiles only: first[t] = the first 0x1A at or after the start of tile t, nxt[t] = at or after
 * its end; s1 when the segment holds none.  At most 257 tiles (MSD_GROUP_BEAST_ENTRY_MAX + a kept frame). */
__global__ void __launch_bounds__(NT) msd_gb_suffix_kernel(const msd_gb_entry *ent, uint32_t n, uint32_t *first,
                                                          uint32_t *nxt)
{
    const uint32_t ei = blockIdx.x * NT + threadIdx.x;
    if (ei >= n)
        return;
    const uint32_t t0 = ent[ei].tile0, nt = ent[ei].ntiles;
    uint32_t m = ent[ei].s1;
    for (uint32_t t = t0 + nt; t-- > t0;) {
        nxt[t] = m;
        m = first[t] < m ? first[t] : m;
        first[t] = m;
    }
}

/* first 0x1A at or after q in the segment that ends at s1 (s1: none) */
__device__ __forceinline__ uint32_t next_1a(const uint8_t *buf, const uint32_t *nxt, uint32_t q, uint32_t s1)
{
    if (q >= s1)
        return s1;
    const uint32_t t = q / FT, e = seg_tile_end(t, s1);
    for (uint32_t i = q; i < e; ++i)
        if (buf[i] == 0x1a)
            return i;
    return nxt[t];
}

/* msd_fr_succ_kernel with every bound the segment's own: what the scanner does from som = p (net_io.c:2510-2568) */
__global__ void __launch_bounds__(NT) msd_gb_succ_kernel(const uint8_t *buf, uint32_t len, const msd_gb_entry *ent,
                                                        const uint32_t *tile_ent, const uint32_t *nxt, uint32_t *succ,
                                                        uint16_t *info, uint8_t *mark)
{
    for (uint32_t p = blockIdx.x * NT + threadIdx.x; p < len; p += gridDim.x * NT) {
        const uint32_t n = ent[tile_ent[p / FT]].s1;
        if (p >= n || buf[p] != 0x1a)
            continue;
        mark[p] = 0;
        if (p + 1 >= n) { /* the type byte has not arrived */
            info[p] = MSD_FR_K_INC;
            succ[p] = MSD_FR_INC | p;
            continue;
        }
        const uint8_t type = buf[p + 1];
        uint32_t eom;
        if (type == '1')
            eom = p + 11;
        else if (type == '2')
            eom = p + 16;
        else if (type == '3' || type == '4' || type == '5')
            eom = p + 23;
        else if (type == 'H') {
            if (p + 3 >= n) {
                info[p] = MSD_FR_K_INC;
                succ[p] = MSD_FR_INC | p;
                continue;
            }
            const uint32_t hl = buf[p + 3];
            if (hl > 24) { /* skip this 0x1A */
                info[p] = (uint16_t)(MSD_FR_K_SKIP | (1u << 8));
                succ[p] = next_1a(buf, nxt, p + 1, n);
                continue;
            }
            eom = p + hl + 4;
        } else {
            info[p] = (uint16_t)(MSD_FR_K_SKIP | (1u << 8));
            succ[p] = next_1a(buf, nxt, p + 1, n);
            continue;
        }
        uint32_t q = p + 1; /* doubled 0x1A bytes lengthen the frame (net_io.c:2547-2552) */
        for (; q < n && q < eom; ++q)
            if (buf[q] == 0x1a) {
                ++q;
                ++eom;
            }
        if (eom > n) {
            info[p] = MSD_FR_K_INC;
            succ[p] = MSD_FR_INC | p;
            continue;
        }
        info[p] = (uint16_t)(type | ((eom - p) << 8));
        succ[p] = next_1a(buf, nxt, eom, n);
    }
}

/* each tile's own chain, from its first 0x1A to the first node past its end */
__global__ void __launch_bounds__(NT) msd_gb_walk_kernel(uint32_t ntiles, const msd_gb_entry *ent, const uint32_t *tile_ent,
                                                        const uint32_t *first, const uint32_t *succ, const uint16_t *info,
                                                        uint8_t *mark, uint32_t *exitl)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= ntiles)
        return;
    const uint32_t e = seg_tile_end(t, ent[tile_ent[t]].s1);
    uint32_t v = first[t];
    while (v < e) {
        if ((info[v] & 0xffu) == MSD_FR_K_INC) {
            v |= MSD_FR_INC;
            break;
        }
        mark[v] = 1;
        v = succ[v];
    }
    exitl[t] = v;
}

/* the true chain of tile t, entered at v: does it leave the tile where the tile's own chain does? */
__device__ __forceinline__ bool follows_own(uint32_t v, uint32_t t, uint32_t s1, const uint8_t *mark, const uint32_t *exitl)
{
    return v >= seg_tile_end(t, s1) ? v == exitl[t] : mark[v] != 0;
}

__global__ void __launch_bounds__(NT) msd_gb_good_kernel(uint32_t ntiles, const msd_gb_entry *ent, const uint32_t *tile_ent,
                                                        const uint8_t *mark, const uint32_t *exitl, uint8_t *good)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= ntiles)
        return;
    const msd_gb_entry &E = ent[tile_ent[t]];
    good[t] = t > E.tile0 && follows_own(exitl[t - 1], t, E.s1, mark, exitl);
}

/* msd_fr_reconcile_kernel, one wavefront per entry over the entry's own tiles: the entries are reconciled in parallel,
 * and each leaves its final chain value and its re-walks in its own counters */
__global__ void __launch_bounds__(64) msd_gb_reconcile_kernel(const msd_gb_entry *ent, const uint32_t *first,
                                                             const uint32_t *succ, const uint16_t *info,
                                                             const uint8_t *mark, const uint32_t *exitl,
                                                             const uint8_t *good, uint32_t *entry, unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x;
    const msd_gb_entry E = ent[blockIdx.x];
    unsigned long long *c = ctr + (size_t)blockIdx.x * CW;
    const uint32_t tb = E.tile0, te = E.tile0 + E.ntiles, n = E.s1;
    if (tb == te) { /* an empty segment: no node, the chain ends where it starts */
        if (lane == 0)
            c[MSD_FR_CTR_EXIT] = E.s0;
        return;
    }
    uint32_t carry = first[tb]; /* true chain value entering tile t0 */
    uint32_t t0 = tb, rewalks = 0;
    while (t0 < te) {
        const uint32_t t = t0 + lane;
        bool ok = false;
        if (t < te)
            ok = lane == 0 ? follows_own(carry, t, n, mark, exitl) : good[t] != 0;
        const uint64_t bad = __ballot(!ok);
        const uint32_t k = bad ? (uint32_t)__builtin_ctzll(bad) : 64u; /* tiles t0 .. t0 + k - 1 follow their own chains */
        if (lane < k && t < te)
            entry[t] = lane == 0 ? carry : exitl[t - 1];
        const uint32_t tk = t0 + k;
        if (tk >= te) { /* k >= 1 here: the last tile followed its own chain */
            carry = exitl[te - 1];
            break;
        }
        uint32_t v = k == 0 ? carry : exitl[tk - 1];
        if (lane == 0) {
            entry[tk] = v;
            const uint32_t e = seg_tile_end(tk, n);
            if (v < e && !mark[v]) {
                ++rewalks;
                while (v < e && !mark[v]) {
                    if ((info[v] & 0xffu) == MSD_FR_K_INC) {
                        v |= MSD_FR_INC;
                        break;
                    }
                    v = succ[v];
                }
            }
            if (v < e) /* met the tile's own chain */
                v = exitl[tk];
        }
        carry = __shfl(v, 0);
        t0 = tk + 1;
    }
    if (lane == 0) {
        c[MSD_FR_CTR_EXIT] = carry;
        c[MSD_FR_CTR_REWALKS] = rewalks;
    }
}

/* nodes of the true chain per tile (an incomplete frame at a segment's end is not one) */
__global__ void __launch_bounds__(NT) msd_gb_count_kernel(uint32_t ntiles, const msd_gb_entry *ent, const uint32_t *tile_ent,
                                                         const uint32_t *entry, const uint32_t *succ, const uint16_t *info,
                                                         uint32_t *cnt, uint32_t *out, const uint32_t *off)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= ntiles)
        return;
    const uint32_t e = seg_tile_end(t, ent[tile_ent[t]].s1);
    uint32_t v = entry[t], c = 0, o = off ? off[t] : 0;
    while (v < e && (info[v] & 0xffu) != MSD_FR_K_INC) {
        if (out)
            out[o + c] = v;
        ++c;
        v = succ[v];
    }
    if (cnt)
        cnt[t] = c;
}

/* The end of every segment, one wavefront per entry: what lies behind its last node is charged or left pending as
 * msd_fr_decode_kernel does for a stream's end, and the incomplete frame to keep is copied out. */
__global__ void __launch_bounds__(64) msd_gb_end_kernel(const uint8_t *buf, const msd_gb_entry *ent, const uint32_t *cnt,
                                                       const uint32_t *nodes, const uint16_t *info, uint8_t *tails_out,
                                                       unsigned long long *ctr, unsigned long long *tot, uint32_t ntiles)
{
    const uint32_t ei = blockIdx.x, lane = threadIdx.x;
    const msd_gb_entry E = ent[ei];
    unsigned long long *c = ctr + (size_t)ei * CW;
    const uint32_t nf = cnt[E.tile0], ne = cnt[E.tile0 + E.ntiles], nn = ne - nf;
    const uint32_t ex = (uint32_t)c[MSD_FR_CTR_EXIT];
    const uint32_t end = nn ? nodes[ne - 1] + (info[nodes[ne - 1]] >> 8) : E.s0;
    if (ex & MSD_FR_INC) {
        const uint32_t q = ex & ~MSD_FR_INC, ntl = E.s1 - q;
        if (lane < ntl && lane < TM)
            tails_out[ei * TM + lane] = buf[q + lane];
        if (lane == 0) { /* the incomplete frame's 0x1A was found: its gap is charged now */
            const uint64_t gap = (uint64_t)(q - end) + (nn ? 0 : E.pending_gap);
            c[MSD_FR_CTR_BAD] += gap / 15u;
            c[MSD_FR_CTR_GARBAGE] += q - end;
            c[MSD_FR_CTR_LAST_END] = MSD_FR_NEVER;
            c[MSD_GB_CTR_NTL] = ntl;
        }
    } else if (lane == 0) { /* trailing bytes without a 0x1A: garbage now, charged when the next 0x1A arrives */
        c[MSD_FR_CTR_GARBAGE] += E.s1 - end;
        c[MSD_FR_CTR_LAST_END] = end - E.s0;
    }
    if (lane == 0) {
        c[MSD_FR_CTR_NODES] = nn;
        if (ei == 0)
            tot[MSD_GB_TOT_NODES] = cnt[ntiles];
    }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* decode: one workgroup per tile, the entry's options loaded once                                                 */
/* ---------------------------------------------------------------------------------------------------------------- */
enum { L_BAD = 0, L_GARBAGE, L_OTHER, L_MODEAC, L_FRAMES, L_MODES, L_ADDS, L_CAND, L_WORDS };

__global__ void __launch_bounds__(NT) msd_gb_decode_kernel(const uint8_t *buf, const msd_gb_entry *ent,
                                                          const uint32_t *tile_ent, msd_fr_tables T, const uint32_t *cnt,
                                                          const uint32_t *nodes, const uint16_t *info, uint8_t *cls,
                                                          uint32_t *addr, unsigned long long *ctr, unsigned long long *tot)
{
    __shared__ unsigned long long lc[L_WORDS];
    const uint32_t t = blockIdx.x;
    const uint32_t k0 = cnt[t], k1 = cnt[t + 1];
    if (k0 == k1)
        return;
    const uint32_t ei = tile_ent[t]; /* the same for the whole workgroup: scalar loads */
    const uint32_t opt = ent[ei].opt, s0 = ent[ei].s0, nf = cnt[ent[ei].tile0];
    const uint64_t pending = ent[ei].pending_gap;
    T.nfix = (int)MSD_GB_OPT_NFIX(opt);
    T.mode_ac = (opt & MSD_GB_OPT_MODEAC) ? 1 : 0;
    if (threadIdx.x < L_WORDS)
        lc[threadIdx.x] = 0;
    __syncthreads();
    const Bytes B{buf, 0, buf, ent[ei].s1};
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += NT) {
        const uint32_t p = nodes[k];
        const bool head = k == nf; /* the entry's first node: the pending gap ends here */
        const uint32_t prev_end = head ? s0 : nodes[k - 1] + (info[nodes[k - 1]] >> 8);
        const uint64_t gap = (uint64_t)(p - prev_end) + (head ? pending : 0);
        if (gap / 15u) /* net_io.c:2510, per gap */
            atomicAdd(lc + L_BAD, (unsigned long long)(gap / 15u));
        const uint32_t type = info[p] & 0xffu;
        uint8_t c = MSD_FR_C_NONE;
        uint32_t a = 0;
        if (type == MSD_FR_K_SKIP) {
            atomicAdd(lc + L_GARBAGE, (unsigned long long)(p - prev_end + 1));
        } else {
            if (p != prev_end)
                atomicAdd(lc + L_GARBAGE, (unsigned long long)(p - prev_end));
            if (type == '4' || type == '5' || type == 'H') {
                atomicAdd(lc + L_OTHER, 1ull);
            } else if (type == '1') {
                atomicAdd(lc + L_MODEAC, 1ull);
                if (T.mode_ac) {
                    atomicAdd(lc + L_FRAMES, 1ull);
                    atomicAdd(lc + L_CAND, 1ull);
                    c = MSD_FR_C_MODEAC;
                }
            } else { /* '2', '3' */
                Frame f;
                read_frame(B, p, (uint8_t)type, f);
                atomicAdd(lc + L_FRAMES, 1ull);
                atomicAdd(lc + L_MODES, 1ull);
                decide(T, f.nbytes, f.d);
                c = f.d.cls;
                a = f.d.addr;
                if (c == MSD_FR_C_BAD)
                    atomicAdd(lc + L_BAD, 1ull);
                else
                    atomicAdd(lc + L_CAND, 1ull);
                if (c == MSD_FR_C_ADD)
                    atomicAdd(lc + L_ADDS, 1ull);
            }
        }
        cls[k] = c;
        addr[k] = a;
    }
    __syncthreads();
    if (threadIdx.x < L_WORDS && lc[threadIdx.x]) {
        const uint32_t w = threadIdx.x;
        const int d = w == L_BAD ? MSD_FR_CTR_BAD : w == L_GARBAGE ? MSD_FR_CTR_GARBAGE : w == L_OTHER ? MSD_FR_CTR_OTHER
                      : w == L_MODEAC ? MSD_FR_CTR_MODEAC : w == L_FRAMES ? MSD_FR_CTR_FRAMES
                      : w == L_MODES ? MSD_FR_CTR_MODES : w == L_ADDS ? MSD_FR_CTR_ADDS : -1;
        if (d >= 0)
            atomicAdd(ctr + (size_t)ei * CW + d, lc[threadIdx.x]);
        if (threadIdx.x == L_ADDS)
            atomicAdd(tot + MSD_GB_TOT_ADDS, lc[L_ADDS]);
        if (threadIdx.x == L_CAND)
            atomicAdd(tot + MSD_GB_TOT_CAND, lc[L_CAND]);
    }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* the filter stage                                                                                                 */
/* ---------------------------------------------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t pair_hash(unsigned long long key, uint32_t hslots)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & (hslots - 1u);
}

/* the (entry, address) pair's two words behind its key: first add, member-from stamp; NULL if it never adds */
__device__ uint32_t *pair_find(unsigned long long *hash, uint32_t hslots, uint32_t ei, uint32_t a)
{
    const unsigned long long key = (unsigned long long)ei << 32 | a;
    for (uint32_t h = pair_hash(key, hslots);; h = (h + 1) & (hslots - 1u)) {
        const unsigned long long k = hash[2 * h];
        if (k == key)
            return reinterpret_cast<uint32_t *>(hash + 2 * h + 1);
        if (k == VACANT64)
            return nullptr;
    }
}

/* first add of every (entry, address): atomicMin on the node index */
__global__ void __launch_bounds__(NT) msd_gb_first_add_kernel(uint32_t nnodes, const uint32_t *tile_ent,
                                                             const uint32_t *nodes, const uint8_t *cls,
                                                             const uint32_t *addr, unsigned long long *hash,
                                                             uint32_t hslots)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes || cls[k] != MSD_FR_C_ADD)
        return;
    const unsigned long long key = (unsigned long long)tile_ent[nodes[k] / FT] << 32 | addr[k];
    for (uint32_t h = pair_hash(key, hslots);; h = (h + 1) & (hslots - 1u)) {
        const unsigned long long old = atomicCAS(hash + 2 * h, VACANT64, key);
        if (old == VACANT64 || old == key) {
            atomicMin(reinterpret_cast<uint32_t *>(hash + 2 * h + 1), k);
            return;
        }
    }
}

/* 1 for the first add of an address its receiver's active table does not hold yet */
__global__ void __launch_bounds__(NT) msd_gb_new_flags_kernel(uint32_t nnodes, const msd_gb_entry *ent,
                                                             const uint32_t *tile_ent, const uint32_t *nodes,
                                                             const uint8_t *cls, const uint32_t *addr,
                                                             unsigned long long *hash, uint32_t hslots,
                                                             const uint32_t *snaps, uint32_t *flags)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes)
        return;
    uint32_t f = 0;
    if (cls[k] == MSD_FR_C_ADD) {
        const uint32_t ei = tile_ent[nodes[k] / FT];
        const uint32_t *snap = snaps + (size_t)ent[ei].snap * MSD_SNAP_WORDS;
        const uint32_t *e = pair_find(hash, hslots, ei, addr[k]);
        f = e && e[0] == k && !snap_table_has(snap, snap[2 * SLOTS], addr[k]);
    }
    flags[k] = f;
}

__global__ void __launch_bounds__(NT) msd_gb_compact_kernel(uint32_t nnodes, const uint32_t *flags_in, const uint32_t *off,
                                                           uint32_t *out)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k < nnodes && flags_in[k])
        out[off[k]] = k;
}

/* icaoFilterAdd (icao_filter.c:76-97) of every entry's new addresses in order of first add, one workgroup per entry,
 * into an LDS copy of that receiver's active table, on one lane: each address is stamped with the node from which on
 * it is a member (never if the table was full).  Leaves the entry's range of `newaddr`; the host repeats the inserts
 * on its filter and msd_group_filter_apply_kernel on the resident snapshot. */
__global__ void __launch_bounds__(NT) msd_gb_insert_kernel(const msd_gb_entry *ent, uint32_t n, const uint32_t *cnt,
                                                          const uint32_t *off, const uint32_t *snaps,
                                                          const uint32_t *newlist, const uint32_t *addr,
                                                          unsigned long long *hash, uint32_t hslots, uint32_t *newaddr,
                                                          uint32_t *add_first, unsigned long long *ctr)
{
    __shared__ uint32_t t[SLOTS];
    const uint32_t ei = blockIdx.x;
    const msd_gb_entry E = ent[ei];
    const uint32_t i0 = off[cnt[E.tile0]], i1 = off[cnt[E.tile0 + E.ntiles]];
    if (threadIdx.x == 0) {
        ctr[(size_t)ei * CW + MSD_GB_CTR_NEW_FIRST] = i0;
        ctr[(size_t)ei * CW + MSD_FR_CTR_NEW] = i1 - i0;
        add_first[ei] = i0;
        if (ei + 1 == n)
            add_first[n] = i1;
    }
    if (i0 == i1)
        return;
    const uint32_t *snap = snaps + (size_t)E.snap * MSD_SNAP_WORDS;
    const uint32_t w = snap[2 * SLOTS];
    for (uint32_t i = threadIdx.x; i < SLOTS; i += NT)
        t[i] = snap[2 * i + w];
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t k = newlist[i], a = addr[k];
        newaddr[i] = a;
        uint32_t *e = pair_find(hash, hslots, ei, a);
        uint32_t h0 = hash24(a), h = h0;
        bool full = false;
        while (t[h] != VACANT && t[h] != a) {
            h = (h + 1) & (SLOTS - 1);
            if (h == h0) {
                full = true;
                break;
            }
        }
        if (full)
            continue; /* gives up before the second insert; stays a non-member */
        if (t[h] == VACANT)
            t[h] = a;
        e[1] = k;
        const uint32_t low = a & 0xffffu;
        h0 = h = hash24(low);
        bool full2 = false;
        while (t[h] != VACANT && (t[h] & 0xffffu) != low) {
            h = (h + 1) & (SLOTS - 1);
            if (h == h0) {
                full2 = true;
                break;
            }
        }
        if (!full2 && t[h] == VACANT)
            t[h] = a;
    }
}

/* the verdict of every tested message against its entry's snapshot and stamps; flags of the records */
__global__ void __launch_bounds__(NT) msd_gb_verdict_kernel(uint32_t nnodes, const msd_gb_entry *ent,
                                                           const uint32_t *tile_ent, const uint32_t *nodes, uint8_t *cls,
                                                           const uint32_t *addr, unsigned long long *hash,
                                                           uint32_t hslots, const uint32_t *snaps, uint32_t *flags,
                                                           unsigned long long *ctr)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes)
        return;
    uint8_t c = cls[k];
    if (c == MSD_FR_C_TEST) {
        const uint32_t a = addr[k], ei = tile_ent[nodes[k] / FT];
        bool known = snap_test(snaps + (size_t)ent[ei].snap * MSD_SNAP_WORDS, a);
        if (!known && hslots) {
            const uint32_t *e = pair_find(hash, hslots, ei, a);
            known = e && e[1] < k;
        }
        if (!known) {
            c = MSD_FR_C_UNKNOWN;
            cls[k] = c;
            atomicAdd(ctr + (size_t)ei * CW + MSD_FR_CTR_UNKNOWN, 1ull);
        }
    }
    flags[k] = c == MSD_FR_C_ACC || c == MSD_FR_C_ADD || c == MSD_FR_C_TEST || c == MSD_FR_C_MODEAC;
}

/* for a verbatim wire call (errbits not NULL; msd_group_remote_out_kernels.hip): the one or two bit positions decide
 * repaired in record r, 0xff for none; every other call passes NULL and stores what it always stored */
__device__ __forceinline__ void leave_errbits(uint8_t *errbits, uint32_t r, uint32_t e0, uint32_t e1)
{
    if (errbits) {
        errbits[2 * (size_t)r] = (uint8_t)e0;
        errbits[2 * (size_t)r + 1] = (uint8_t)e1;
    }
}

__global__ void __launch_bounds__(NT) msd_gb_records_kernel(const uint8_t *buf, uint32_t nnodes, const msd_gb_entry *ent,
                                                           const uint32_t *tile_ent, msd_fr_tables T,
                                                           const uint32_t *nodes, const uint16_t *info, const uint8_t *cls,
                                                           const uint32_t *off, msd_message *out, unsigned long long *ctr,
                                                           uint8_t *errbits)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes || off[k + 1] == off[k])
        return;
    const uint32_t p = nodes[k], ei = tile_ent[p / FT];
    const msd_gb_entry &E = ent[ei];
    const Bytes B{buf, 0, buf, E.s1};
    Frame f;
    read_frame(B, p, (uint8_t)(info[p] & 0xffu), f);
    msd_message &o = out[off[k]];
    if (cls[k] == MSD_FR_C_MODEAC) {
        modeac_record(o, f.d.msg, f.ts, f.level, E.now_ms);
        leave_errbits(errbits, off[k], 0xffu, 0xffu);
        return;
    }
    T.nfix = (int)MSD_GB_OPT_NFIX(E.opt);
    decide(T, f.nbytes, f.d);
    finish_record(o, f.d, f.ts, f.level, E.now_ms, ctr + (size_t)ei * CW);
    leave_errbits(errbits, off[k], f.d.errbit[0], f.d.errbit[1]);
}

/* the records of an input that is framed already (AVR text): record k from in[k] instead of a frame of `buf`, with its
 * entry's repair level, clock and counters */
__global__ void __launch_bounds__(NT) msd_gb_records_in_kernel(const msd_message *in, uint32_t nnodes,
                                                              const msd_gb_entry *ent, const uint32_t *tile_ent,
                                                              msd_fr_tables T, const uint32_t *nodes, const uint8_t *cls,
                                                              const uint32_t *off, msd_message *out,
                                                              unsigned long long *ctr, uint8_t *errbits)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes || off[k + 1] == off[k])
        return;
    const uint32_t ei = tile_ent[nodes[k] / FT];
    const msd_gb_entry &E = ent[ei];
    const msd_message &m = in[k];
    msd_message &o = out[off[k]];
    if (cls[k] == MSD_FR_C_MODEAC) {
        modeac_record(o, m.msg, m.timestampMsg, m.signalLevel, E.now_ms);
        leave_errbits(errbits, off[k], 0xffu, 0xffu);
        return;
    }
    Decoded d;
    const int nb = m.msgbits == 112 ? 14 : 7;
    for (int j = 0; j < 14; ++j)
        d.msg[j] = j < nb ? m.msg[j] : 0;
    T.nfix = (int)MSD_GB_OPT_NFIX(E.opt);
    decide(T, nb, d);
    finish_record(o, d, m.timestampMsg, m.signalLevel, E.now_ms, ctr + (size_t)ei * CW);
    leave_errbits(errbits, off[k], d.errbit[0], d.errbit[1]);
}

/* every entry's range of `out` */
__global__ void __launch_bounds__(NT) msd_gb_ranges_kernel(const msd_gb_entry *ent, uint32_t n, const uint32_t *cnt,
                                                          const uint32_t *off, unsigned long long *ctr)
{
    const uint32_t ei = blockIdx.x * NT + threadIdx.x;
    if (ei >= n)
        return;
    const uint32_t r0 = off[cnt[ent[ei].tile0]], r1 = off[cnt[ent[ei].tile0 + ent[ei].ntiles]];
    ctr[(size_t)ei * CW + MSD_GB_CTR_REC_FIRST] = r0;
    ctr[(size_t)ei * CW + MSD_FR_CTR_RECORDS] = r1 - r0;
}

} // namespace

extern "C" int msd_gb_launch_chain_decode(const uint8_t *src, const msd_fr_tables *t, const msd_gb_scratch *s, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = s->n, ntiles = s->ntiles;
    if (hipMemsetAsync(s->ctr, 0, sizeof(unsigned long long) * CW * n, st) != hipSuccess ||
        hipMemsetAsync(s->tot, 0, sizeof(unsigned long long) * MSD_GB_TOT_WORDS, st) != hipSuccess ||
        hipMemsetAsync(s->add_first, 0, sizeof(uint32_t) * (n + 1), st) != hipSuccess)
        return -5;
    if (ntiles) {
        hipLaunchKernelGGL(msd_gb_layout_kernel, dim3(ntiles), dim3(NT), 0, st, src, s->ent, s->tile_ent, s->tails_in,
                           s->buf);
        hipLaunchKernelGGL(msd_gb_tile_first_kernel, dim3(ntiles), dim3(NT), 0, st, s->buf, s->ent, s->tile_ent, s->first);
        hipLaunchKernelGGL(msd_gb_suffix_kernel, dim3(blocks(n)), dim3(NT), 0, st, s->ent, n, s->first, s->nxt);
        const uint32_t gb = blocks(s->len) < 8192u ? blocks(s->len) : 8192u;
        hipLaunchKernelGGL(msd_gb_succ_kernel, dim3(gb), dim3(NT), 0, st, s->buf, s->len, s->ent, s->tile_ent, s->nxt,
                           s->succ, s->info, s->mark);
        hipLaunchKernelGGL(msd_gb_walk_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, ntiles, s->ent, s->tile_ent,
                           s->first, s->succ, s->info, s->mark, s->exitl);
        hipLaunchKernelGGL(msd_gb_good_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, ntiles, s->ent, s->tile_ent,
                           s->mark, s->exitl, s->good);
    }
    hipLaunchKernelGGL(msd_gb_reconcile_kernel, dim3(n), dim3(64), 0, st, s->ent, s->first, s->succ, s->info, s->mark,
                       s->exitl, s->good, s->entry, s->ctr);
    if (ntiles)
        hipLaunchKernelGGL(msd_gb_count_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, ntiles, s->ent, s->tile_ent,
                           s->entry, s->succ, s->info, s->cnt, (uint32_t *)nullptr, (const uint32_t *)nullptr);
    scan_excl(s->cnt, s->cnt, ntiles, s->scan_tmp, st);
    if (ntiles)
        hipLaunchKernelGGL(msd_gb_count_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, ntiles, s->ent, s->tile_ent,
                           s->entry, s->succ, s->info, (uint32_t *)nullptr, s->nodes, s->cnt);
    hipLaunchKernelGGL(msd_gb_end_kernel, dim3(n), dim3(64), 0, st, s->buf, s->ent, s->cnt, s->nodes, s->info,
                       s->tails_out, s->ctr, s->tot, ntiles);
    if (ntiles)
        hipLaunchKernelGGL(msd_gb_decode_kernel, dim3(ntiles), dim3(NT), 0, st, s->buf, s->ent, s->tile_ent, *t, s->cnt,
                           s->nodes, s->info, s->cls, s->addr, s->ctr, s->tot);
    return check(hipGetLastError());
}

/* stage 3 up to the flags of the records and their offsets: the same for frames of `buf` and for parsed records */
static void filter_stage(uint32_t nnodes, uint32_t nadds, const msd_gb_scratch *s, hipStream_t st)
{
    const uint32_t n = s->n;
    if (nadds) {
        hipLaunchKernelGGL(msd_gb_first_add_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->tile_ent, s->nodes,
                           s->cls, s->addr, s->hash, s->hslots);
        hipLaunchKernelGGL(msd_gb_new_flags_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->ent, s->tile_ent,
                           s->nodes, s->cls, s->addr, s->hash, s->hslots, s->snaps, s->flags);
        scan_excl(s->flags, s->off, nnodes, s->scan_tmp, st);
        hipLaunchKernelGGL(msd_gb_compact_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->flags, s->off,
                           s->newlist);
        hipLaunchKernelGGL(msd_gb_insert_kernel, dim3(n), dim3(NT), 0, st, s->ent, n, s->cnt, s->off, s->snaps,
                           s->newlist, s->addr, s->hash, s->hslots, s->newaddr, s->add_first, s->ctr);
    }
    hipLaunchKernelGGL(msd_gb_verdict_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->ent, s->tile_ent,
                       s->nodes, s->cls, s->addr, s->hash, nadds ? s->hslots : 0u, s->snaps, s->flags, s->ctr);
    scan_excl(s->flags, s->off, nnodes, s->scan_tmp, st);
}

extern "C" int msd_gb_launch_filter(uint32_t nnodes, uint32_t nadds, const msd_fr_tables *t, const msd_gb_scratch *s,
                                    void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (nnodes == 0) /* no message: the counters stay as the decode left them */
        return 0;
    filter_stage(nnodes, nadds, s, st);
    hipLaunchKernelGGL(msd_gb_records_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, s->buf, nnodes, s->ent, s->tile_ent,
                       *t, s->nodes, s->info, s->cls, s->off, s->out, s->ctr, s->errbits);
    hipLaunchKernelGGL(msd_gb_ranges_kernel, dim3(blocks(s->n)), dim3(NT), 0, st, s->ent, s->n, s->cnt, s->off, s->ctr);
    return check(hipGetLastError());
}

extern "C" int msd_gb_launch_filter_records(const msd_message *in, uint32_t nnodes, uint32_t nadds, const msd_fr_tables *t,
                                            const msd_gb_scratch *s, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (nnodes == 0)
        return 0;
    filter_stage(nnodes, nadds, s, st);
    hipLaunchKernelGGL(msd_gb_records_in_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, in, nnodes, s->ent, s->tile_ent,
                       *t, s->nodes, s->cls, s->off, s->out, s->ctr, s->errbits);
    hipLaunchKernelGGL(msd_gb_ranges_kernel, dim3(blocks(s->n)), dim3(NT), 0, st, s->ent, s->n, s->cnt, s->off, s->ctr);
    return check(hipGetLastError());
}
