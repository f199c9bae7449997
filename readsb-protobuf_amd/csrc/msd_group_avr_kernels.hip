/*
 * msd_group_avr_kernels.hip -- AVR raw text input for every receiver of a group call at once (msd_group_accept_avr;
 * DESIGN.md 4.9, "AVR text input per receiver").  The framing rule is the stream input's, from the one
 * place that holds it for both, msd_avr_impl.h: a line's start is a pure function of the MSD_AVR_LINE_MAX + 1 bytes in
 * front of its '\n'.  Here a piece holds one segment per entry, each starting on a span boundary, so a span and its '\n'
 * belong to one receiver:
 *   msd_ga_layout_kernel  the piece: every segment's kept line, then its new bytes.
 *   msd_ga_count_kernel   one workgroup per span.  The window of msd_avr_count_kernel, with the look-back clipped at the
 *                         entry's s0 and nothing at or behind its s1; the discard flag is the entry's own.  Leaves the
 *                         records per span and adds the entry's line counters, summed in LDS first.
 *   (prefix sum)          the spans' record counts to offsets over the whole piece, entry after entry.
 *   msd_ga_store_kernel   the parsed records at their ranks, and the position of each record's '\n' (which names its
 *                         entry for the filter stage); mode_ac and keep_timestamp are the entry's.
 *   msd_ga_end_kernel     one wavefront per entry: the bytes behind its last '\n' to keep, or the discard flag.
 *   msd_ga_decode_kernel  the class of every record as msd_fr_records_decode_kernel classes it, one workgroup per span
 *                         with the entry's repair level and Mode A/C switch, counters in the entry's row.
 * The filter stage behind them is the Beast input's (msd_gb_launch_filter_records).  The number of launches
 * does not depend on the number of entries.
 */
#include <hip/hip_runtime.h>

#include "msd_avr_impl.h"
#include "msd_frames_impl.h"
#include "msd_group_avr.h"

namespace {

constexpr uint32_t CW = MSD_FR_CTR_WORDS;
constexpr uint32_t LM = MSD_AVR_LINE_MAX;
static_assert(AT == (uint32_t)NT && SPAN == FT, "one workgroup per span, a span a tile of the filter stage");

/* the piece: every segment's kept line, then its new bytes; one workgroup per span */
__global__ void __launch_bounds__(AT) msd_ga_layout_kernel(const uint8_t *src, const msd_gb_entry *ent,
                                                          const uint32_t *tile_ent, const uint8_t *lines_in, uint8_t *buf)
{
    const uint32_t t = blockIdx.x, ei = tile_ent[t];
    const msd_gb_entry E = ent[ei];
    const uint32_t e = (t + 1u) * SPAN < E.s1 ? (t + 1u) * SPAN : E.s1;
    const uint8_t *data = src + E.src;
    for (uint32_t i = t * SPAN + threadIdx.x; i < e; i += AT) {
        const uint32_t rel = i - E.s0;
        buf[i] = rel < E.tl ? lines_in[ei * LM + rel] : data[rel - E.tl];
    }
}

/* an entry's bytes for classify.  Only bytes of the segment [s0, s1) get a class: the look-back of a segment's first
 * span is empty, and neither a '\n' nor text exists at or behind s1. */
struct Segment {
    const uint8_t *buf;
    uint32_t s0, s1;
    __device__ __forceinline__ uint32_t operator()(int32_t p) const
    {
        uint32_t ch = 0xffu;
        if (p >= (int32_t)s0 && (uint32_t)p < s1)
            ch = buf[p];
        return ch;
    }
};

/* the window of span t of entry E: its base, and the window position of the segment's first byte */
__device__ __forceinline__ void span_window(uint32_t t, const msd_gb_entry &E, int32_t &base, int &rmin)
{
    base = (int32_t)(t * SPAN) - (int32_t)LB;
    rmin = (int32_t)E.s0 > base ? (int32_t)E.s0 - base : 0;
}

__global__ void __launch_bounds__(AT) msd_ga_count_kernel(const uint8_t *buf, const msd_gb_entry *ent,
                                                         const uint32_t *tile_ent, uint32_t *cnt,
                                                         unsigned long long *ctr)
{
    __shared__ Window W;
    __shared__ uint32_t tot[4];
    const uint32_t ei = tile_ent[blockIdx.x];
    const msd_gb_entry E = ent[ei];
    int32_t base;
    int rmin;
    span_window(blockIdx.x, E, base, rmin);
    if (threadIdx.x < 4)
        tot[threadIdx.x] = 0;
    classify(W, Segment{buf, E.s0, E.s1}, base);
    const bool discard = (E.opt & MSD_GA_OPT_DISCARD) != 0;
    const int mode_ac = (E.opt & MSD_GB_OPT_MODEAC) ? 1 : 0;
    const Lines c = count_lines(W, base, rmin, discard, mode_ac); /* (c.end has no use here) */
    if (c.n) {
        atomicAdd(&tot[3], c.n);
        for (int k = 0; k < 3; ++k)
            if (c.kind[k])
                atomicAdd(&tot[k], c.kind[k]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = tot[L_REC];
        if (tot[3]) { /* the entry's own row: no counter is shared between entries */
            unsigned long long *row = ctr + (size_t)ei * CW;
            atomicAdd(row + MSD_GA_CTR_LINES, (unsigned long long)tot[3]);
            if (tot[L_DROP])
                atomicAdd(row + MSD_GA_CTR_DROPPED, (unsigned long long)tot[L_DROP]);
            if (tot[L_LONG])
                atomicAdd(row + MSD_GA_CTR_LONG, (unsigned long long)tot[L_LONG]);
        }
    }
}

__global__ void __launch_bounds__(AT) msd_ga_store_kernel(const uint8_t *buf, const msd_gb_entry *ent,
                                                         const uint32_t *tile_ent, const uint32_t *cnt,
                                                         msd_message *rec, uint32_t *nodes)
{
    __shared__ Window W;
    __shared__ uint32_t part[AT / 64];
    if (cnt[blockIdx.x + 1] == cnt[blockIdx.x]) /* no record ends here */
        return;
    const msd_gb_entry E = ent[tile_ent[blockIdx.x]];
    int32_t base;
    int rmin;
    span_window(blockIdx.x, E, base, rmin);
    classify(W, Segment{buf, E.s0, E.s1}, base);
    const bool discard = (E.opt & MSD_GA_OPT_DISCARD) != 0;
    const int mode_ac = (E.opt & MSD_GB_OPT_MODEAC) ? 1 : 0;
    const int keep = (E.opt & MSD_GA_OPT_KEEP_TS) ? 1 : 0;
    const Records r = my_records(W, rmin, discard, mode_ac);
    uint32_t total;
    const uint32_t rank = cnt[blockIdx.x] + block_scan<AT>(r.n, part, total);
#pragma unroll /* (three at most, as in msd_avr_store_kernel) */
    for (uint32_t k = 0; k < r.n && k < MAX_RECS; ++k) {
        const uint32_t d = r[k];
        put_record(W, rec_a(d), rec_skip(d), rec_plen(d), keep, rec[rank + k]);
        nodes[rank + k] = (uint32_t)(base + r.first + rec_bit(d));
    }
}

/* The end of every segment, one wavefront per entry.  The bytes behind its last '\n' are the line to keep when they
 * are at most MSD_AVR_LINE_MAX -- so the last MSD_AVR_LINE_MAX + 1 bytes decide: a '\n' among them, or the segment is
 * no longer than MSD_AVR_LINE_MAX and began outside an overlong line.  Otherwise the entry ends inside an overlong line
 * (one it began in, or one that has passed MSD_AVR_LINE_MAX bytes here). */
__global__ void __launch_bounds__(64) msd_ga_end_kernel(const uint8_t *buf, const msd_gb_entry *ent, const uint32_t *cnt,
                                                       uint8_t *lines_out, unsigned long long *ctr,
                                                       unsigned long long *tot, uint32_t nspans)
{
    const uint32_t ei = blockIdx.x, lane = threadIdx.x;
    const msd_gb_entry E = ent[ei];
    unsigned long long *c = ctr + (size_t)ei * CW;
    if (lane == 0) {
        c[MSD_FR_CTR_NODES] = cnt[E.tile0 + E.ntiles] - cnt[E.tile0];
        if (ei == 0)
            tot[MSD_GB_TOT_NODES] = cnt[nspans];
    }
    if (E.s1 == E.s0) /* an empty entry leaves its receiver's kept line alone */
        return;
    const uint32_t len = E.s1 - E.s0;
    const uint32_t lo = len > LM + 1u ? E.s1 - (LM + 1u) : E.s0;
    uint32_t from = 0xFFFFFFFFu; /* the byte behind the last '\n' of [lo, s1) */
    for (uint32_t b = lo; b < E.s1; b += 64) {
        const uint32_t p = b + lane;
        const uint64_t m = __ballot(p < E.s1 && buf[p] == '\n');
        if (m)
            from = b + 64u - (uint32_t)__clzll((long long)m);
    }
    uint32_t ntl = 0, discard = 0;
    if (from != 0xFFFFFFFFu) {
        ntl = E.s1 - from; /* at most MSD_AVR_LINE_MAX: from > lo >= s1 - (MSD_AVR_LINE_MAX + 1) */
    } else if (len > LM || (E.opt & MSD_GA_OPT_DISCARD)) {
        discard = 1;
    } else {
        from = E.s0;
        ntl = len;
    }
    for (uint32_t i = lane; i < ntl && i < LM; i += 64)
        lines_out[ei * LM + i] = buf[from + i];
    if (lane == 0) {
        c[MSD_GB_CTR_NTL] = ntl;
        c[MSD_GA_CTR_DISCARD] = discard;
    }
}

/* the class of every record, one workgroup per span with the entry's options loaded once (msd_fr_records_decode_kernel
 * per record, msd_gb_decode_kernel's counters) */
enum { C_BAD = 0, C_MODEAC, C_FRAMES, C_MODES, C_ADDS, C_CAND, C_WORDS };

__global__ void __launch_bounds__(NT) msd_ga_decode_kernel(const msd_message *rec, const msd_gb_entry *ent,
                                                          const uint32_t *tile_ent, msd_fr_tables T, const uint32_t *cnt,
                                                          uint8_t *cls, uint32_t *addr, unsigned long long *ctr,
                                                          unsigned long long *tot)
{
    __shared__ unsigned long long lc[C_WORDS];
    const uint32_t t = blockIdx.x;
    const uint32_t k0 = cnt[t], k1 = cnt[t + 1];
    if (k0 == k1)
        return;
    const uint32_t ei = tile_ent[t];
    const uint32_t opt = ent[ei].opt;
    T.nfix = (int)MSD_GB_OPT_NFIX(opt);
    T.mode_ac = (opt & MSD_GB_OPT_MODEAC) ? 1 : 0;
    if (threadIdx.x < C_WORDS)
        lc[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += NT) {
        const msd_message &m = rec[k];
        uint8_t c;
        uint32_t a = 0;
        if (m.msgbits == 16) {
            atomicAdd(lc + C_MODEAC, 1ull);
            c = T.mode_ac ? MSD_FR_C_MODEAC : MSD_FR_C_NONE;
            if (T.mode_ac) {
                atomicAdd(lc + C_FRAMES, 1ull);
                atomicAdd(lc + C_CAND, 1ull);
            }
        } else {
            Decoded d;
            const int nb = m.msgbits == 112 ? 14 : 7;
            for (int j = 0; j < 14; ++j)
                d.msg[j] = j < nb ? m.msg[j] : 0;
            atomicAdd(lc + C_FRAMES, 1ull);
            atomicAdd(lc + C_MODES, 1ull);
            decide(T, nb, d);
            c = d.cls;
            a = d.addr;
            if (c == MSD_FR_C_BAD)
                atomicAdd(lc + C_BAD, 1ull);
            else
                atomicAdd(lc + C_CAND, 1ull);
            if (c == MSD_FR_C_ADD)
                atomicAdd(lc + C_ADDS, 1ull);
        }
        cls[k] = c;
        addr[k] = a;
    }
    __syncthreads();
    if (threadIdx.x < C_WORDS && lc[threadIdx.x]) {
        const uint32_t w = threadIdx.x;
        const int d = w == C_BAD ? MSD_FR_CTR_BAD : w == C_MODEAC ? MSD_FR_CTR_MODEAC : w == C_FRAMES ? MSD_FR_CTR_FRAMES
                      : w == C_MODES ? MSD_FR_CTR_MODES : w == C_ADDS ? MSD_FR_CTR_ADDS : -1;
        if (d >= 0)
            atomicAdd(ctr + (size_t)ei * CW + d, lc[w]);
        if (w == C_ADDS)
            atomicAdd(tot + MSD_GB_TOT_ADDS, lc[C_ADDS]);
        if (w == C_CAND)
            atomicAdd(tot + MSD_GB_TOT_CAND, lc[C_CAND]);
    }
}

} // namespace

extern "C" int msd_ga_launch_frame_decode(const uint8_t *src, const msd_fr_tables *t, const msd_ga_scratch *s,
                                          void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const msd_gb_scratch &f = s->f;
    const uint32_t n = f.n, nspans = f.ntiles;
    if (hipMemsetAsync(f.ctr, 0, sizeof(unsigned long long) * CW * n, st) != hipSuccess ||
        hipMemsetAsync(f.tot, 0, sizeof(unsigned long long) * MSD_GB_TOT_WORDS, st) != hipSuccess ||
        hipMemsetAsync(f.add_first, 0, sizeof(uint32_t) * (n + 1), st) != hipSuccess)
        return -5;
    if (nspans) {
        hipLaunchKernelGGL(msd_ga_layout_kernel, dim3(nspans), dim3(AT), 0, st, src, f.ent, f.tile_ent, s->lines_in,
                           f.buf);
        hipLaunchKernelGGL(msd_ga_count_kernel, dim3(nspans), dim3(AT), 0, st, f.buf, f.ent, f.tile_ent, f.cnt, f.ctr);
    }
    scan_excl(f.cnt, f.cnt, nspans, f.scan_tmp, st);
    if (nspans)
        hipLaunchKernelGGL(msd_ga_store_kernel, dim3(nspans), dim3(AT), 0, st, f.buf, f.ent, f.tile_ent, f.cnt, s->rec,
                           f.nodes);
    hipLaunchKernelGGL(msd_ga_end_kernel, dim3(n), dim3(64), 0, st, f.buf, f.ent, f.cnt, s->lines_out, f.ctr, f.tot,
                       nspans);
    if (nspans)
        hipLaunchKernelGGL(msd_ga_decode_kernel, dim3(nspans), dim3(NT), 0, st, s->rec, f.ent, f.tile_ent, *t, f.cnt,
                           f.cls, f.addr, f.ctr, f.tot);
    return check(hipGetLastError());
}
