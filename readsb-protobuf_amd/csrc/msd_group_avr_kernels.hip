/*
 * msd_group_avr_kernels.hip -- AVR raw text input for every receiver of a group call at once (msd_group_accept_avr;
 * DESIGN.md 4.9, "AVR text input per receiver").  The framing rule is the one of msd_avr_kernels.hip: a
 * line's start is a pure function of the MSD_AVR_LINE_MAX + 1 bytes in front of its '\n'.  Here a piece holds one
 * segment per entry, each starting on a span boundary, so a span and its '\n' belong to one receiver:
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
 * The filter stage behind them is the Beast input's (msd_gb_launch_filter_records).  Window, the mask searches, line_at,
 * block_scan, hexval and put_record are msd_avr_kernels.hip's, line for line: that file's are in its unnamed namespace,
 * and it stays as it is.  The number of launches does not depend on the number of entries.
 */
#include <hip/hip_runtime.h>

#include "msd_frames_impl.h"
#include "msd_group_avr.h"

namespace {

constexpr uint32_t CW = MSD_FR_CTR_WORDS;
constexpr uint32_t LM = MSD_AVR_LINE_MAX;
constexpr uint32_t AT = 256;                /* threads */
constexpr uint32_t SPAN = MSD_AVR_SPAN;     /* bytes whose '\n' a workgroup owns */
constexpr uint32_t LB = MSD_AVR_LOOKBACK;   /* bytes in front of them it classifies as well */
constexpr uint32_t WIN = LB + SPAN;         /* the window, in LDS */
constexpr uint32_t NW = WIN / 64;           /* mask words */
constexpr uint32_t PER = SPAN / AT;         /* bytes whose '\n' a thread owns */
constexpr int REACH = (int)MSD_AVR_LINE_MAX + 1; /* bytes in front of a '\n' that decide where its line starts */
constexpr uint32_t MIN_LINE = 7;            /* "*XXXX;" and its '\n': the shortest line that yields a record */
constexpr uint32_t MAX_RECS = 3;            /* ... so a thread's bytes end at most this many of them */
static_assert(LB % 64 == 0 && LB >= (uint32_t)REACH, "the window must hold every byte a line start depends on");
static_assert(SPAN % 64 == 0 && 64 % PER == 0 && PER <= 32, "a thread's bytes lie in one mask word");
static_assert((PER - 1) / MIN_LINE + 1 <= MAX_RECS, "records per thread");
static_assert(AT == (uint32_t)NT && SPAN == FT, "one workgroup per span, a span a tile of the filter stage");

enum { L_LONG = 0, L_DROP = 1, L_REC = 2 };

struct Window {
    uint64_t nl[NW + 1], ws[NW + 1], nul[NW + 1], hex[NW + 1]; /* one word more, zero: two-word reads need no bound */
    uint8_t ch[WIN];
};

/* bits [0, top] of a word */
__device__ __forceinline__ uint64_t upto(int top)
{
    return (2ull << top) - 1ull;
}

/* the highest position in [lo, hi) whose bit is set (INV: clear), -1 if none */
template <bool INV> __device__ int last_in(const uint64_t *m, int lo, int hi)
{
    if (hi <= lo)
        return -1;
    int k = (hi - 1) >> 6;
    const int k0 = lo >> 6;
    uint64_t w = (INV ? ~m[k] : m[k]) & upto((hi - 1) & 63);
    for (;;) {
        if (k == k0)
            w &= ~0ull << (lo & 63);
        if (w)
            return k * 64 + 63 - __clzll((long long)w);
        if (k == k0)
            return -1;
        --k;
        w = INV ? ~m[k] : m[k];
    }
}

/* the lowest such position */
template <bool INV> __device__ int first_in(const uint64_t *m, int lo, int hi)
{
    if (hi <= lo)
        return -1;
    int k = lo >> 6;
    const int k1 = (hi - 1) >> 6;
    uint64_t w = (INV ? ~m[k] : m[k]) & (~0ull << (lo & 63));
    for (;;) {
        if (k == k1)
            w &= upto((hi - 1) & 63);
        if (w)
            return k * 64 + __ffsll((unsigned long long)w) - 1;
        if (k == k1)
            return -1;
        ++k;
        w = INV ? ~m[k] : m[k];
    }
}

/* cnt <= 32 mask bits from position start on */
__device__ __forceinline__ uint32_t bits_at(const uint64_t *m, int start, int cnt)
{
    const int k = start >> 6, o = start & 63;
    uint64_t v = m[k] >> o;
    if (o)
        v |= m[k + 1] << (64 - o);
    return (uint32_t)v & (uint32_t)((1ull << cnt) - 1ull);
}

/* The line that the '\n' at window position r ends.  rmin: the window position of the piece's first byte.  For a line
 * that yields a record: a = where its text starts, skip = prefix and timestamp / signal digits, plen = payload digits. */
__device__ int line_at(const Window &W, int r, int rmin, bool discard, int mode_ac, int &a, int &skip, int &plen)
{
    const bool reach = r - REACH >= rmin; /* REACH bytes of the piece lie in front of the '\n' */
    const int j = last_in<false>(W.nl, reach ? r - REACH : rmin, r);
    int s;
    if (j >= 0)
        s = j + 1;
    else if (reach || discard) /* more than MSD_AVR_LINE_MAX bytes, in this piece or counting the ones before it */
        return L_LONG;
    else
        s = rmin;
    const int z = first_in<false>(W.nul, s, r);
    const int e = z < 0 ? r : z; /* strlen */
    const int bl = last_in<true>(W.ws, s, e);
    if (bl < 0)
        return L_DROP; /* empty, or white space only */
    const int b = bl + 1;
    a = first_in<true>(W.ws, s, b);
    const int l = b - a;
    if (W.ch[b - 1] != ';')
        return L_DROP;
    switch (W.ch[a]) {
    case '<': skip = 15; break;
    case '@':
    case '%': skip = 13; break;
    case '*':
    case ':': skip = 1; break;
    default: return L_DROP;
    }
    if (l < skip + 1)
        return L_DROP;
    plen = l - skip - 1;
    if (plen != 4 && plen != 14 && plen != 28)
        return L_DROP;
    if (plen == 4 && !mode_ac)
        return L_DROP;
    if (bits_at(W.hex, a + skip, plen) != (uint32_t)((1ull << plen) - 1ull))
        return L_DROP;
    return L_REC;
}

/* the '\n' among the calling thread's bytes, bit i for window position first + i */
__device__ __forceinline__ uint32_t my_newlines(const Window &W, int &first)
{
    const uint32_t off = threadIdx.x * PER;
    first = (int)(LB + off);
    return (uint32_t)(W.nl[(LB + off) >> 6] >> (off & 63u)) & ((1u << PER) - 1u);
}

/* exclusive prefix of v over the workgroup's 256 threads, and the total; `part`: 4 words of LDS */
__device__ inline uint32_t block_scan(uint32_t v, uint32_t *part, uint32_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d)
            incl += up;
    }
    __syncthreads(); /* part may still be read from the call before */
    if (lane == 63)
        part[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w)
        before += w < wave ? part[w] : 0u;
    total = part[0] + part[1] + part[2] + part[3];
    return before + incl - v;
}

/* hexval of msd_wire.c: -1 for anything else */
__device__ __forceinline__ int hexval(uint32_t c)
{
    if (c - '0' < 10u)
        return (int)(c - '0');
    if ((c | 0x20u) - 'a' < 6u)
        return (int)((c | 0x20u) - 'a') + 10;
    return -1;
}

/* the record of the line whose text starts at window position a (msd_avr_parse_line behind its checks) */
__device__ void put_record(const Window &W, int a, int skip, int plen, int keep_timestamp, msd_message &o)
{
    uint64_t ts = 0;
    double level = 0.0;
    if (skip > 1) {
        if (bits_at(W.hex, a + 1, 12) == 0xfffu) /* a digit that is none: 0 */
            for (int i = 1; i < 13; ++i)
                ts = (ts << 4) | (uint64_t)hexval(W.ch[a + i]);
        if (skip == 15) {
            const int hi = hexval(W.ch[a + 13]), lo = hexval(W.ch[a + 14]);
            level = (double)((hi * 16) | lo) / 255.0; /* net_io.c:1690-1691, whatever the digits are */
            level *= level;
        }
    }
    msd_message m;
    m.timestampMsg = keep_timestamp ? ts : 0;
    m.sysTimestampMsg = 0;
    m.signalLevel = level;
    m.addr = 0;
    m.crc = 0;
    m.score = 0;
    m.msgtype = 0;
    m.msgbits = (uint8_t)(4 * plen);
    m.correctedbits = 0;
    m.bestphase = 0;
    const int p = a + skip;
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        uint8_t v = 0;
        if (2 * j < plen)
            v = (uint8_t)((hexval(W.ch[p + 2 * j]) << 4) | hexval(W.ch[p + 2 * j + 1]));
        m.msg[j] = v;
    }
    m.iid = 0;
    m.pad = 0;
    o = m;
}

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

/* Window position r is piece position base + r.  Only bytes of the segment [s0, s1) get a class: the look-back of a
 * segment's first span is empty, and neither a '\n' nor text exists at or behind s1. */
__device__ void classify(Window &W, const uint8_t *buf, uint32_t s0, uint32_t s1, int32_t base)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t c = wave; c < NW; c += AT / 64) {
        const int32_t p = base + (int32_t)(c * 64 + lane);
        uint32_t ch = 0xffu;
        if (p >= (int32_t)s0 && (uint32_t)p < s1)
            ch = buf[p];
        W.ch[c * 64 + lane] = (uint8_t)ch;
        const uint64_t m_nl = __ballot(ch == '\n');
        const uint64_t m_ws = __ballot(ch == ' ' || ch - 9u <= 4u); /* space, 0x09..0x0D */
        const uint64_t m_nul = __ballot(ch == 0u);
        const uint64_t m_hex = __ballot(ch - '0' < 10u || (ch | 0x20u) - 'a' < 6u);
        if (lane == 0) {
            W.nl[c] = m_nl;
            W.ws[c] = m_ws;
            W.nul[c] = m_nul;
            W.hex[c] = m_hex;
        }
    }
    if (threadIdx.x == 0)
        W.nl[NW] = W.ws[NW] = W.nul[NW] = W.hex[NW] = 0;
    __syncthreads();
}

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
    classify(W, buf, E.s0, E.s1, base);
    const bool discard = (E.opt & MSD_GA_OPT_DISCARD) != 0;
    const int mode_ac = (E.opt & MSD_GB_OPT_MODEAC) ? 1 : 0;
    int first;
    uint32_t mine = my_newlines(W, first);
    uint32_t c[3] = {0, 0, 0}, nlines = 0;
    while (mine) {
        const int bit = __ffs(mine) - 1;
        mine &= mine - 1u;
        int a, skip, plen;
        const int kind = line_at(W, first + bit, rmin, discard, mode_ac, a, skip, plen);
        c[0] += kind == L_LONG;
        c[1] += kind == L_DROP;
        c[2] += kind == L_REC;
        ++nlines;
    }
    if (nlines) {
        atomicAdd(&tot[3], nlines);
        for (int k = 0; k < 3; ++k)
            if (c[k])
                atomicAdd(&tot[k], c[k]);
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
    __shared__ uint32_t part[4];
    if (cnt[blockIdx.x + 1] == cnt[blockIdx.x]) /* no record ends here */
        return;
    const msd_gb_entry E = ent[tile_ent[blockIdx.x]];
    int32_t base;
    int rmin;
    span_window(blockIdx.x, E, base, rmin);
    classify(W, buf, E.s0, E.s1, base);
    const bool discard = (E.opt & MSD_GA_OPT_DISCARD) != 0;
    const int mode_ac = (E.opt & MSD_GB_OPT_MODEAC) ? 1 : 0;
    const int keep = (E.opt & MSD_GA_OPT_KEEP_TS) ? 1 : 0;
    int first;
    uint32_t mine = my_newlines(W, first);
    uint32_t d0 = 0, d1 = 0, d2 = 0, c = 0; /* a | skip << 16 | the '\n' among the thread's bytes << 20 | plen << 24 */
    while (mine) {
        const int bit = __ffs(mine) - 1;
        mine &= mine - 1u;
        int a, skip, plen;
        if (line_at(W, first + bit, rmin, discard, mode_ac, a, skip, plen) != L_REC)
            continue;
        const uint32_t d = (uint32_t)a | ((uint32_t)skip << 16) | ((uint32_t)bit << 20) | ((uint32_t)plen << 24);
        if (c == 0)
            d0 = d;
        else if (c == 1)
            d1 = d;
        else
            d2 = d;
        ++c;
    }
    uint32_t total;
    const uint32_t rank = cnt[blockIdx.x] + block_scan(c, part, total);
    for (uint32_t k = 0; k < c && k < MAX_RECS; ++k) {
        const uint32_t d = k == 0 ? d0 : k == 1 ? d1 : d2;
        put_record(W, (int)(d & 0xffffu), (int)((d >> 16) & 0xfu), (int)(d >> 24), keep, rec[rank + k]);
        nodes[rank + k] = (uint32_t)(base + first + (int)((d >> 20) & 0xfu));
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
