/*
 * msd_frames_kernels.hip -- Beast / AVR input on the GPU: the READ_MODE_BEAST scanner (net_io.c:2504-2569),
 * decodeBinMessage (net_io.c:1486-1627) and decodeModesMessage's acceptance (mode_s.c:424-555,717-726) against the
 * context's ICAO filter, for a whole byte stream at once.  DESIGN.md section 4.8.
 *
 * Two steps of that look sequential and are made parallel exactly:
 *  - the scanner moves from one 0x1A to the next by a pure function of the bytes behind it.  Every 0x1A gets its
 *    successor (msd_fr_succ_kernel); every tile follows the chain from its own first 0x1A (msd_fr_walk_kernel); one
 *    wavefront then checks, in order, whether the true chain enters each tile at a node of the tile's own chain --
 *    from there on both are the same chain -- and walks the tile again from the true entry when it does not
 *    (msd_fr_reconcile_kernel);
 *  - within one call only clean DF17 and zero-syndrome DF11 frames add addresses, and they are accepted without a
 *    filter test, so the adds are known before any test is made.  A test of frame k is "in the filter as the piece
 *    began, or inserted by an add of a frame before k"; whether an add is inserted at all (the active table can be
 *    full) is decided by inserting the piece's new addresses in order of first add, on one lane, into a copy of the
 *    active table (msd_fr_insert_kernel).
 */
#include <hip/hip_runtime.h>

#include "msd_frames.h"
#include "msd_frames_impl.h"

namespace {

__device__ __forceinline__ uint32_t tile_end(uint32_t t, uint32_t n)
{
    const uint64_t e = (uint64_t)(t + 1) * FT;
    return e < n ? (uint32_t)e : n;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* the successor graph                                                                                               */
/* ---------------------------------------------------------------------------------------------------------------- */

/* first 0x1A in each tile (n: none) */
__global__ void __launch_bounds__(NT) msd_fr_tile_first_kernel(Bytes B, uint32_t *first, uint32_t ntiles)
{
    __shared__ uint32_t best;
    const uint32_t t = blockIdx.x;
    if (threadIdx.x == 0)
        best = B.n;
    __syncthreads();
    const uint32_t s = t * FT, e = tile_end(t, B.n);
    for (uint32_t i = s + threadIdx.x; i < e; i += NT)
        if (B[i] == 0x1a) {
            atomicMin(&best, i);
            break;
        }
    __syncthreads();
    if (threadIdx.x == 0)
        first[t] = best;
    if (t == 0 && threadIdx.x == 0)
        first[ntiles] = B.n;
}

/* first[t] = the first 0x1A at or after the start of tile t: a suffix minimum, one workgroup */
__global__ void __launch_bounds__(1024) msd_fr_suffix_kernel(uint32_t *first, uint32_t ntiles)
{
    __shared__ uint32_t seg[1024];
    const uint32_t per = (ntiles + 1023u) / 1024u, lo = threadIdx.x * per;
    const uint32_t hi = lo + per < ntiles ? lo + per : ntiles;
    uint32_t m = first[ntiles];
    for (uint32_t i = hi; i-- > lo;)
        m = first[i] < m ? first[i] : m;
    seg[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) /* 1024 steps */
        for (int i = 1022; i >= 0; --i)
            seg[i] = seg[i + 1] < seg[i] ? seg[i + 1] : seg[i];
    __syncthreads();
    m = threadIdx.x + 1 < 1024 ? seg[threadIdx.x + 1] : first[ntiles];
    if (m > first[ntiles])
        m = first[ntiles];
    for (uint32_t i = hi; i-- > lo;) {
        m = first[i] < m ? first[i] : m;
        first[i] = m;
    }
}

/* first 0x1A at or after q (n: none) */
__device__ __forceinline__ uint32_t next_1a(const Bytes &B, const uint32_t *first, uint32_t q)
{
    if (q >= B.n)
        return B.n;
    const uint32_t t = q / FT, e = tile_end(t, B.n);
    for (uint32_t i = q; i < e; ++i)
        if (B[i] == 0x1a)
            return i;
    return first[t + 1];
}

/* What the scanner does from som = p for every 0x1A at p (net_io.c:2510-2568). */
__global__ void __launch_bounds__(NT) msd_fr_succ_kernel(Bytes B, const uint32_t *first, uint32_t *succ, uint16_t *info,
                                                        uint8_t *mark)
{
    const uint32_t n = B.n;
    for (uint32_t p = blockIdx.x * NT + threadIdx.x; p < n; p += gridDim.x * NT) {
        if (B[p] != 0x1a)
            continue;
        mark[p] = 0;
        if (p + 1 >= n) { /* the type byte has not arrived */
            info[p] = MSD_FR_K_INC;
            succ[p] = MSD_FR_INC | p;
            continue;
        }
        const uint8_t type = B[p + 1];
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
            const uint32_t len = B[p + 3];
            if (len > 24) { /* skip this 0x1A */
                info[p] = (uint16_t)(MSD_FR_K_SKIP | (1u << 8));
                succ[p] = next_1a(B, first, p + 1);
                continue;
            }
            eom = p + len + 4;
        } else {
            info[p] = (uint16_t)(MSD_FR_K_SKIP | (1u << 8));
            succ[p] = next_1a(B, first, p + 1);
            continue;
        }
        /* doubled 0x1A bytes lengthen the frame (net_io.c:2547-2552) */
        uint32_t q = p + 1;
        for (; q < n && q < eom; ++q)
            if (B[q] == 0x1a) {
                ++q;
                ++eom;
            }
        if (eom > n) {
            info[p] = MSD_FR_K_INC;
            succ[p] = MSD_FR_INC | p;
            continue;
        }
        info[p] = (uint16_t)(type | ((eom - p) << 8));
        succ[p] = next_1a(B, first, eom);
    }
}

/* Each tile's own chain, from its first 0x1A to the first node past its end. */
__global__ void __launch_bounds__(NT) msd_fr_walk_kernel(uint32_t n, uint32_t ntiles, const uint32_t *first,
                                                        const uint32_t *succ, const uint16_t *info, uint8_t *mark,
                                                        uint32_t *exitl)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= ntiles)
        return;
    const uint32_t e = tile_end(t, n);
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
__device__ __forceinline__ bool follows_own(uint32_t v, uint32_t t, uint32_t n, const uint8_t *mark, const uint32_t *exitl)
{
    return v >= tile_end(t, n) ? v == exitl[t] : mark[v] != 0;
}

__global__ void __launch_bounds__(NT) msd_fr_good_kernel(uint32_t n, uint32_t ntiles, const uint8_t *mark,
                                                        const uint32_t *exitl, uint8_t *good)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= ntiles)
        return;
    good[t] = t > 0 && follows_own(exitl[t - 1], t, n, mark, exitl);
}

/* In order over the tiles, 64 at a time: while every tile is entered where its predecessor's own chain leaves and
 * that node is on its own chain (good), the true chain is the tiles' own chains.  The first tile where that fails is
 * walked again from its true entry on one lane until it meets its own chain or leaves the tile. */
__global__ void __launch_bounds__(64) msd_fr_reconcile_kernel(uint32_t n, uint32_t ntiles, const uint32_t *first,
                                                             const uint32_t *succ, const uint16_t *info,
                                                             const uint8_t *mark, const uint32_t *exitl,
                                                             const uint8_t *good, uint32_t *entry,
                                                             unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x;
    uint32_t carry = first[0]; /* true chain value entering tile t0 */
    uint32_t t0 = 0, rewalks = 0;
    while (t0 < ntiles) {
        const uint32_t t = t0 + lane;
        bool ok = false;
        if (t < ntiles)
            ok = lane == 0 ? follows_own(carry, t, n, mark, exitl) : good[t] != 0;
        const uint64_t bad = __ballot(!ok);
        const uint32_t k = bad ? (uint32_t)__builtin_ctzll(bad) : 64u; /* tiles t0 .. t0 + k - 1 follow their own chains */
        if (lane < k && t < ntiles)
            entry[t] = lane == 0 ? carry : exitl[t - 1];
        const uint32_t tk = t0 + k;
        if (tk >= ntiles) { /* k >= 1 here: the last tile followed its own chain */
            carry = exitl[ntiles - 1];
            break;
        }
        uint32_t v = k == 0 ? carry : exitl[tk - 1];
        if (lane == 0) {
            entry[tk] = v;
            const uint32_t e = tile_end(tk, n);
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
        ctr[MSD_FR_CTR_EXIT] = carry;
        ctr[MSD_FR_CTR_REWALKS] = rewalks;
    }
}

/* nodes of the true chain per tile (the incomplete frame at the end is not one) */
__global__ void __launch_bounds__(NT) msd_fr_count_kernel(uint32_t n, uint32_t ntiles, const uint32_t *entry,
                                                         const uint32_t *succ, const uint16_t *info, uint32_t *cnt,
                                                         uint32_t *out, const uint32_t *off)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= ntiles)
        return;
    const uint32_t e = tile_end(t, n);
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

/* the piece's add table: open addressing on the address */
__device__ __forceinline__ uint32_t add_hash(uint32_t a, uint32_t hslots)
{
    return (a * 2654435761u) & (hslots - 1u);
}

__device__ uint32_t *add_find(uint32_t *hash, uint32_t hslots, uint32_t addr)
{
    for (uint32_t h = add_hash(addr, hslots);; h = (h + 1) & (hslots - 1u)) {
        const uint32_t k = hash[4 * h];
        if (k == addr)
            return hash + 4 * h;
        if (k == VACANT)
            return nullptr;
    }
}

__device__ void count_gap(unsigned long long *ctr, uint64_t gap)
{
    if (gap / 15u) /* net_io.c:2510, per gap */
        atomicAdd(ctr + MSD_FR_CTR_BAD, (unsigned long long)(gap / 15u));
}

/* per node: the gap in front of it, its kind, and for a message its class */
__global__ void __launch_bounds__(NT) msd_fr_decode_kernel(Bytes B, uint32_t nnodes, uint64_t pending_gap,
                                                          const msd_fr_tables T, const uint32_t *nodes,
                                                          const uint16_t *info, uint8_t *cls, uint32_t *addr,
                                                          unsigned long long *ctr)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k > nnodes)
        return;
    if (k == nnodes) { /* behind the last node */
        const uint32_t ex = (uint32_t)ctr[MSD_FR_CTR_EXIT];
        const uint64_t end = nnodes ? nodes[nnodes - 1] + (info[nodes[nnodes - 1]] >> 8) : 0;
        if (ex & MSD_FR_INC) { /* the incomplete frame's 0x1A was found: its gap is charged now */
            const uint64_t gap = (ex & ~MSD_FR_INC) - end + (nnodes ? 0 : pending_gap);
            count_gap(ctr, gap);
            atomicAdd(ctr + MSD_FR_CTR_GARBAGE, (unsigned long long)((ex & ~MSD_FR_INC) - end));
            ctr[MSD_FR_CTR_LAST_END] = MSD_FR_NEVER;
        } else { /* trailing bytes without a 0x1A: counted as garbage now, charged when the next 0x1A arrives */
            atomicAdd(ctr + MSD_FR_CTR_GARBAGE, (unsigned long long)(B.n - end));
            ctr[MSD_FR_CTR_LAST_END] = end;
        }
        return;
    }
    const uint32_t p = nodes[k];
    const uint64_t prev_end = k ? nodes[k - 1] + (info[nodes[k - 1]] >> 8) : 0;
    const uint64_t gap = p - prev_end + (k ? 0 : pending_gap);
    count_gap(ctr, gap);
    const uint32_t type = info[p] & 0xffu;
    uint8_t c = MSD_FR_C_NONE;
    uint32_t a = 0;
    if (type == MSD_FR_K_SKIP) {
        atomicAdd(ctr + MSD_FR_CTR_GARBAGE, (unsigned long long)(p - prev_end + 1));
    } else {
        if (p != prev_end)
            atomicAdd(ctr + MSD_FR_CTR_GARBAGE, (unsigned long long)(p - prev_end));
        if (type == '4' || type == '5' || type == 'H') {
            atomicAdd(ctr + MSD_FR_CTR_OTHER, 1ull);
        } else if (type == '1') {
            atomicAdd(ctr + MSD_FR_CTR_MODEAC, 1ull);
            if (T.mode_ac) {
                atomicAdd(ctr + MSD_FR_CTR_FRAMES, 1ull);
                c = MSD_FR_C_MODEAC;
            }
        } else { /* '2', '3' */
            Frame f;
            read_frame(B, p, (uint8_t)type, f);
            atomicAdd(ctr + MSD_FR_CTR_FRAMES, 1ull);
            atomicAdd(ctr + MSD_FR_CTR_MODES, 1ull);
            decide(T, f.nbytes, f.d);
            c = f.d.cls;
            a = f.d.addr;
            if (c == MSD_FR_C_BAD)
                atomicAdd(ctr + MSD_FR_CTR_BAD, 1ull);
            else if (c == MSD_FR_C_ADD)
                atomicAdd(ctr + MSD_FR_CTR_ADDS, 1ull);
        }
    }
    cls[k] = c;
    addr[k] = a;
}

/* the same classes for records framed on the host (msd_accept_frames) */
__global__ void __launch_bounds__(NT) msd_fr_records_decode_kernel(const msd_message *in, uint32_t n,
                                                                  const msd_fr_tables T, uint8_t *cls, uint32_t *addr,
                                                                  unsigned long long *ctr)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= n)
        return;
    const msd_message &m = in[k];
    uint8_t c;
    uint32_t a = 0;
    if (m.msgbits == 16) {
        atomicAdd(ctr + MSD_FR_CTR_MODEAC, 1ull);
        c = T.mode_ac ? MSD_FR_C_MODEAC : MSD_FR_C_NONE;
        if (T.mode_ac)
            atomicAdd(ctr + MSD_FR_CTR_FRAMES, 1ull);
    } else {
        Decoded d;
        const int nb = m.msgbits == 112 ? 14 : 7;
        for (int j = 0; j < 14; ++j)
            d.msg[j] = j < nb ? m.msg[j] : 0;
        atomicAdd(ctr + MSD_FR_CTR_FRAMES, 1ull);
        atomicAdd(ctr + MSD_FR_CTR_MODES, 1ull);
        decide(T, nb, d);
        c = d.cls;
        a = d.addr;
        if (c == MSD_FR_C_BAD)
            atomicAdd(ctr + MSD_FR_CTR_BAD, 1ull);
        else if (c == MSD_FR_C_ADD)
            atomicAdd(ctr + MSD_FR_CTR_ADDS, 1ull);
    }
    cls[k] = c;
    addr[k] = a;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* the filter stage                                                                                                 */
/* ---------------------------------------------------------------------------------------------------------------- */

/* first add of every address: a hash with atomicMin on the node index */
__global__ void __launch_bounds__(NT) msd_fr_first_add_kernel(uint32_t nnodes, const uint8_t *cls, const uint32_t *addr,
                                                             uint32_t *hash, uint32_t hslots)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes || cls[k] != MSD_FR_C_ADD)
        return;
    const uint32_t a = addr[k];
    for (uint32_t h = add_hash(a, hslots);; h = (h + 1) & (hslots - 1u)) {
        const uint32_t old = atomicCAS(hash + 4 * h, VACANT, a);
        if (old == VACANT || old == a) {
            atomicMin(hash + 4 * h + 1, k);
            return;
        }
    }
}

/* 1 for the first add of an address the active table does not hold yet */
__global__ void __launch_bounds__(NT) msd_fr_new_flags_kernel(uint32_t nnodes, const uint8_t *cls, const uint32_t *addr,
                                                             uint32_t *hash, uint32_t hslots, const uint32_t *snap,
                                                             uint32_t *flags)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes)
        return;
    uint32_t f = 0;
    if (cls[k] == MSD_FR_C_ADD) {
        const uint32_t *e = add_find(hash, hslots, addr[k]);
        f = e && e[1] == k && !snap_table_has(snap, snap[2 * SLOTS], addr[k]);
    }
    flags[k] = f;
}

__global__ void __launch_bounds__(NT) msd_fr_compact_kernel(uint32_t nnodes, const uint32_t *flags_in,
                                                           const uint32_t *off, uint32_t *out)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k < nnodes && flags_in[k])
        out[off[k]] = k;
}

/* icaoFilterAdd (icao_filter.c:76-97) of the new addresses in order of first add, into an LDS copy of the active
 * table, on one lane: each address is stamped with the node from which on it is a member (never if the table was
 * full).  The host repeats the same inserts on its own filter. */
__global__ void __launch_bounds__(64) msd_fr_insert_kernel(const uint32_t *snap, const uint32_t *newlist,
                                                          const unsigned long long *ctr, const uint32_t *addr,
                                                          uint32_t *hash, uint32_t hslots, uint32_t *newaddr)
{
    __shared__ uint32_t t[SLOTS];
    const uint32_t w = snap[2 * SLOTS];
    for (uint32_t i = threadIdx.x; i < SLOTS; i += 64)
        t[i] = snap[2 * i + w];
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    const uint32_t nnew = (uint32_t)ctr[MSD_FR_CTR_NEW];
    for (uint32_t i = 0; i < nnew; ++i) {
        const uint32_t k = newlist[i], a = addr[k];
        newaddr[i] = a;
        uint32_t *e = add_find(hash, hslots, a);
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
        e[2] = k;
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

/* the verdict of every tested message; flags of the records */
__global__ void __launch_bounds__(NT) msd_fr_verdict_kernel(uint32_t nnodes, uint8_t *cls, const uint32_t *addr,
                                                           const uint32_t *hash, uint32_t hslots, const uint32_t *snap,
                                                           uint32_t *flags, unsigned long long *ctr)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes)
        return;
    uint8_t c = cls[k];
    if (c == MSD_FR_C_TEST) {
        const uint32_t a = addr[k];
        bool known = snap_test(snap, a);
        if (!known && hslots) {
            const uint32_t *e = add_find(const_cast<uint32_t *>(hash), hslots, a);
            known = e && e[2] < k;
        }
        if (!known) {
            c = MSD_FR_C_UNKNOWN;
            cls[k] = c;
            atomicAdd(ctr + MSD_FR_CTR_UNKNOWN, 1ull);
        }
    }
    flags[k] = c == MSD_FR_C_ACC || c == MSD_FR_C_ADD || c == MSD_FR_C_TEST || c == MSD_FR_C_MODEAC;
}

__global__ void __launch_bounds__(NT) msd_fr_records_kernel(Bytes B, uint32_t nnodes, uint64_t now_ms,
                                                           const msd_fr_tables T, const uint32_t *nodes,
                                                           const uint16_t *info, const uint8_t *cls,
                                                           const uint32_t *off, msd_message *out,
                                                           unsigned long long *ctr)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= nnodes || off[k + 1] == off[k])
        return;
    const uint32_t p = nodes[k];
    Frame f;
    read_frame(B, p, (uint8_t)(info[p] & 0xffu), f);
    msd_message &o = out[off[k]];
    if (cls[k] == MSD_FR_C_MODEAC) {
        modeac_record(o, f.d.msg, f.ts, f.level, now_ms);
        return;
    }
    decide(T, f.nbytes, f.d);
    finish_record(o, f.d, f.ts, f.level, now_ms, ctr);
}

__global__ void __launch_bounds__(NT) msd_fr_records_out_kernel(const msd_message *in, uint32_t n, uint64_t now_ms,
                                                               const msd_fr_tables T, const uint8_t *cls,
                                                               const uint32_t *off, msd_message *out,
                                                               unsigned long long *ctr)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= n || off[k + 1] == off[k])
        return;
    const msd_message &m = in[k];
    msd_message &o = out[off[k]];
    if (cls[k] == MSD_FR_C_MODEAC) {
        modeac_record(o, m.msg, m.timestampMsg, m.signalLevel, now_ms);
        return;
    }
    Decoded d;
    const int nb = m.msgbits == 112 ? 14 : 7;
    for (int j = 0; j < 14; ++j)
        d.msg[j] = j < nb ? m.msg[j] : 0;
    decide(T, nb, d);
    finish_record(o, d, m.timestampMsg, m.signalLevel, now_ms, ctr);
}

__global__ void msd_fr_copy_ctr_kernel(unsigned long long *ctr, const uint32_t *src, int dst)
{
    ctr[dst] = *src;
}

/* stage 3, shared by both inputs */
void filter_stage(uint32_t nnodes, uint32_t nadds, const msd_fr_scratch *s, hipStream_t st)
{
    if (nadds) {
        hipLaunchKernelGGL(msd_fr_first_add_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->cls, s->addr,
                           s->hash, s->hslots);
        hipLaunchKernelGGL(msd_fr_new_flags_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->cls, s->addr,
                           s->hash, s->hslots, s->snap, s->flags);
        scan_excl(s->flags, s->cnt, nnodes, s->scan_tmp, st);
        hipLaunchKernelGGL(msd_fr_compact_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->flags, s->cnt,
                           s->newlist);
        hipLaunchKernelGGL(msd_fr_copy_ctr_kernel, dim3(1), dim3(1), 0, st, s->ctr, s->cnt + nnodes, (int)MSD_FR_CTR_NEW);
        hipLaunchKernelGGL(msd_fr_insert_kernel, dim3(1), dim3(64), 0, st, s->snap, s->newlist, s->ctr, s->addr,
                           s->hash, s->hslots, s->newaddr);
    }
    hipLaunchKernelGGL(msd_fr_verdict_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, nnodes, s->cls, s->addr, s->hash,
                       nadds ? s->hslots : 0u, s->snap, s->flags, s->ctr);
    scan_excl(s->flags, s->cnt, nnodes, s->scan_tmp, st);
    hipLaunchKernelGGL(msd_fr_copy_ctr_kernel, dim3(1), dim3(1), 0, st, s->ctr, s->cnt + nnodes,
                       (int)MSD_FR_CTR_RECORDS);
}

} // namespace

extern "C" size_t msd_fr_scan_tmp_words(uint32_t n)
{
    return (n + SCAN_PER - 1u) / SCAN_PER + 16u;
}

extern "C" int msd_fr_launch_chain(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n,
                                   const msd_fr_scratch *s, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const Bytes B{tail, tl, data, n};
    const uint32_t ntiles = (n + FT - 1u) / FT;
    if (hipMemsetAsync(s->ctr, 0, sizeof(unsigned long long) * MSD_FR_CTR_WORDS, st) != hipSuccess)
        return -5;
    if (ntiles == 0) /* an empty piece: no node; the chain ends at 0 = n */
        return 0;
    hipLaunchKernelGGL(msd_fr_tile_first_kernel, dim3(ntiles), dim3(NT), 0, st, B, s->first, ntiles);
    hipLaunchKernelGGL(msd_fr_suffix_kernel, dim3(1), dim3(1024), 0, st, s->first, ntiles);
    const uint32_t gb = blocks(n) < 8192u ? blocks(n) : 8192u;
    hipLaunchKernelGGL(msd_fr_succ_kernel, dim3(gb), dim3(NT), 0, st, B, s->first, s->succ, s->info, s->mark);
    hipLaunchKernelGGL(msd_fr_walk_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, n, ntiles, s->first, s->succ,
                       s->info, s->mark, s->exitl);
    hipLaunchKernelGGL(msd_fr_good_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, n, ntiles, s->mark, s->exitl,
                       s->good);
    hipLaunchKernelGGL(msd_fr_reconcile_kernel, dim3(1), dim3(64), 0, st, n, ntiles, s->first, s->succ, s->info,
                       s->mark, s->exitl, s->good, s->entry, s->ctr);
    hipLaunchKernelGGL(msd_fr_count_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, n, ntiles, s->entry, s->succ,
                       s->info, s->cnt, (uint32_t *)nullptr, (const uint32_t *)nullptr);
    scan_excl(s->cnt, s->cnt, ntiles, s->scan_tmp, st);
    hipLaunchKernelGGL(msd_fr_count_kernel, dim3(blocks(ntiles)), dim3(NT), 0, st, n, ntiles, s->entry, s->succ,
                       s->info, (uint32_t *)nullptr, s->nodes, s->cnt);
    hipLaunchKernelGGL(msd_fr_copy_ctr_kernel, dim3(1), dim3(1), 0, st, s->ctr, s->cnt + ntiles, (int)MSD_FR_CTR_NODES);
    return check(hipGetLastError());
}

extern "C" int msd_fr_launch_decode(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, uint32_t nnodes,
                                    uint64_t pending_gap, const msd_fr_tables *t, const msd_fr_scratch *s, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const Bytes B{tail, tl, data, n};
    hipLaunchKernelGGL(msd_fr_decode_kernel, dim3(blocks((uint64_t)nnodes + 1)), dim3(NT), 0, st, B, nnodes,
                       pending_gap, *t, s->nodes, s->info, s->cls, s->addr, s->ctr);
    return check(hipGetLastError());
}

extern "C" int msd_fr_launch_filter(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, uint32_t nnodes,
                                    uint32_t nadds, uint64_t now_ms, const msd_fr_tables *t, const msd_fr_scratch *s,
                                    void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const Bytes B{tail, tl, data, n};
    if (nnodes == 0) /* no message: the counters stay as stage 2 left them */
        return 0;
    filter_stage(nnodes, nadds, s, st);
    hipLaunchKernelGGL(msd_fr_records_kernel, dim3(blocks(nnodes)), dim3(NT), 0, st, B, nnodes, now_ms, *t, s->nodes,
                       s->info, s->cls, s->cnt, s->out, s->ctr);
    return check(hipGetLastError());
}

extern "C" int msd_fr_launch_records_decode(const msd_message *in, uint32_t n, const msd_fr_tables *t,
                                            const msd_fr_scratch *s, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(s->ctr, 0, sizeof(unsigned long long) * MSD_FR_CTR_WORDS, st) != hipSuccess)
        return -5;
    hipLaunchKernelGGL(msd_fr_records_decode_kernel, dim3(blocks(n)), dim3(NT), 0, st, in, n, *t, s->cls, s->addr,
                       s->ctr);
    return check(hipGetLastError());
}

extern "C" int msd_fr_launch_records_filter(const msd_message *in, uint32_t n, uint32_t nadds, uint64_t now_ms,
                                            const msd_fr_tables *t, const msd_fr_scratch *s, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (n == 0)
        return 0;
    filter_stage(n, nadds, s, st);
    hipLaunchKernelGGL(msd_fr_records_out_kernel, dim3(blocks(n)), dim3(NT), 0, st, in, n, now_ms, *t, s->cls, s->cnt,
                       s->out, s->ctr);
    return check(hipGetLastError());
}
