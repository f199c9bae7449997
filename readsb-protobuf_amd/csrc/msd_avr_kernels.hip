/*
 * msd_avr_kernels.hip -- AVR raw text input on the GPU: the READ_MODE_ASCII line cutting of the --net-ri-port service
 * (net_io.c:501, 2448-2500) and decodeHexMessage's framing (net_io.c:1656-1764) as msd_avr_parse_line restates it, for a
 * whole byte stream at once.  DESIGN.md section 4.8.
 *
 * With lines bounded by MSD_AVR_LINE_MAX, where a line starts is a pure function of the MSD_AVR_LINE_MAX + 1 bytes in
 * front of its '\n': the byte behind the nearest '\n' among them, the start of the piece when the piece is shorter, or
 * nowhere -- the line is overlong and dropped.  So every '\n' is decided on its own:
 *   msd_avr_count_kernel    a workgroup owns the '\n' of MSD_AVR_SPAN bytes.  It classifies those bytes and the
 *                           MSD_AVR_LOOKBACK in front of them once -- newline, white space, NUL, hex digit -- into
 *                           64-bit masks in LDS, one ballot per class and 64 bytes.  A thread then takes the '\n' of its
 *                           16 bytes and finds the line's start, the end of its text (the first NUL), the text without
 *                           its white space and whether all its payload digits are hex with a few word operations on
 *                           the masks; only the prefix character and the ';' are looked at as bytes.  Leaves the records
 *                           per workgroup and adds the piece's counters.
 *   msd_avr_offsets_kernel  the counts to offsets, one workgroup (as the wire writers' scan_kernel).
 *   msd_avr_store_kernel    the same classification again; every line that yields a record is parsed from LDS and
 *                           written at its rank.
 */
#include <hip/hip_runtime.h>

#include "msd_avr.h"
#include "msd_frames.h"

namespace {

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

enum { L_LONG = 0, L_DROP = 1, L_REC = 2 };

struct Window {
    uint64_t nl[NW + 1], ws[NW + 1], nul[NW + 1], hex[NW + 1]; /* one word more, zero: two-word reads need no bound */
    uint8_t ch[WIN];
};

/* Window position r is piece position base + r.  Bytes outside the piece get no class at all. */
__device__ void classify(Window &W, const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, int32_t base)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t c = wave; c < NW; c += AT / 64) {
        const int32_t p = base + (int32_t)(c * 64 + lane);
        uint32_t ch = 0xffu;
        if (p >= 0 && (uint32_t)p < n)
            ch = (uint32_t)p < tl ? tail[p] : data[(uint32_t)p - tl];
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

__global__ void __launch_bounds__(AT) msd_avr_count_kernel(const uint8_t *tail, uint32_t tl, const uint8_t *data,
                                                          uint32_t n, int discard, int mode_ac, uint32_t *wg,
                                                          unsigned long long *ctr)
{
    __shared__ Window W;
    __shared__ uint32_t tot[4], last;
    const int32_t base = (int32_t)(blockIdx.x * SPAN) - (int32_t)LB;
    const int rmin = base < 0 ? -base : 0;
    if (threadIdx.x < 4)
        tot[threadIdx.x] = 0;
    if (threadIdx.x == 0)
        last = 0;
    classify(W, tail, tl, data, n, base);
    int first;
    uint32_t mine = my_newlines(W, first);
    uint32_t c[3] = {0, 0, 0}, nlines = 0, hi = 0;
    while (mine) {
        const int bit = __ffs(mine) - 1;
        mine &= mine - 1u;
        int a, skip, plen;
        const int kind = line_at(W, first + bit, rmin, discard != 0, mode_ac, a, skip, plen);
        c[0] += kind == L_LONG;
        c[1] += kind == L_DROP;
        c[2] += kind == L_REC;
        ++nlines;
        hi = (uint32_t)(base + first + bit) + 1u;
    }
    if (nlines) {
        atomicAdd(&tot[3], nlines);
        atomicMax(&last, hi);
        for (int k = 0; k < 3; ++k)
            if (c[k])
                atomicAdd(&tot[k], c[k]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        wg[blockIdx.x] = tot[L_REC];
        if (tot[3]) {
            atomicAdd(ctr + MSD_AVR_CTR_LINES, (unsigned long long)tot[3]);
            atomicAdd(ctr + MSD_AVR_CTR_DROPPED, (unsigned long long)tot[L_DROP]);
            atomicAdd(ctr + MSD_AVR_CTR_LONG, (unsigned long long)tot[L_LONG]);
            atomicMax(ctr + MSD_AVR_CTR_LAST_NL, (unsigned long long)last);
        }
    }
}

/* wg[0 .. spans) -> their exclusive prefix in place, wg[spans] and the record counter = the total.  One workgroup. */
__global__ void __launch_bounds__(AT) msd_avr_offsets_kernel(uint32_t *wg, uint32_t spans, unsigned long long *ctr)
{
    __shared__ uint32_t part[4];
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < spans; b0 += AT) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < spans ? wg[b] : 0u;
        uint32_t total;
        const uint32_t before = block_scan(v, part, total);
        if (b < spans)
            wg[b] = run + before;
        run += total;
    }
    if (threadIdx.x == 0) {
        wg[spans] = run;
        ctr[MSD_AVR_CTR_RECORDS] = run;
    }
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

__global__ void __launch_bounds__(AT) msd_avr_store_kernel(const uint8_t *tail, uint32_t tl, const uint8_t *data,
                                                          uint32_t n, int discard, int mode_ac, int keep_timestamp,
                                                          const uint32_t *wg, msd_message *out)
{
    __shared__ Window W;
    __shared__ uint32_t part[4];
    if (wg[blockIdx.x + 1] == wg[blockIdx.x]) /* no record ends here */
        return;
    const int32_t base = (int32_t)(blockIdx.x * SPAN) - (int32_t)LB;
    const int rmin = base < 0 ? -base : 0;
    classify(W, tail, tl, data, n, base);
    int first;
    uint32_t mine = my_newlines(W, first);
    uint32_t d0 = 0, d1 = 0, d2 = 0, c = 0; /* a | skip << 16 | plen << 24 of this thread's records */
    while (mine) {
        const int bit = __ffs(mine) - 1;
        mine &= mine - 1u;
        int a, skip, plen;
        if (line_at(W, first + bit, rmin, discard != 0, mode_ac, a, skip, plen) != L_REC)
            continue;
        const uint32_t d = (uint32_t)a | ((uint32_t)skip << 16) | ((uint32_t)plen << 24);
        if (c == 0)
            d0 = d;
        else if (c == 1)
            d1 = d;
        else
            d2 = d;
        ++c;
    }
    uint32_t total;
    const uint32_t rank = wg[blockIdx.x] + block_scan(c, part, total);
    for (uint32_t k = 0; k < c && k < MAX_RECS; ++k) {
        const uint32_t d = k == 0 ? d0 : k == 1 ? d1 : d2;
        put_record(W, (int)(d & 0xffffu), (int)((d >> 16) & 0xffu), (int)(d >> 24), keep_timestamp, out[rank + k]);
    }
}

int check(hipError_t e)
{
    return e == hipSuccess ? 0 : -5 /* -EIO */;
}

} // namespace

extern "C" uint32_t msd_avr_span_bytes(void)
{
    return SPAN;
}

extern "C" uint32_t msd_avr_lookback_bytes(void)
{
    return LB;
}

extern "C" uint32_t msd_avr_piece_bytes(void)
{
    return MSD_FR_PIECE;
}

extern "C" int msd_avr_launch_count(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, int discard,
                                    int mode_ac, uint32_t *wg, unsigned long long *ctr, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t spans = (n + SPAN - 1u) / SPAN;
    if (hipMemsetAsync(ctr, 0, sizeof(unsigned long long) * MSD_FR_CTR_WORDS, st) != hipSuccess)
        return -5;
    if (spans == 0)
        return 0;
    hipLaunchKernelGGL(msd_avr_count_kernel, dim3(spans), dim3(AT), 0, st, tail, tl, data, n, discard, mode_ac, wg, ctr);
    hipLaunchKernelGGL(msd_avr_offsets_kernel, dim3(1), dim3(AT), 0, st, wg, spans, ctr);
    return check(hipGetLastError());
}

extern "C" int msd_avr_launch_store(const uint8_t *tail, uint32_t tl, const uint8_t *data, uint32_t n, int discard,
                                    int mode_ac, int keep_timestamp, const uint32_t *wg, msd_message *out, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const uint32_t spans = (n + SPAN - 1u) / SPAN;
    if (spans == 0)
        return 0;
    hipLaunchKernelGGL(msd_avr_store_kernel, dim3(spans), dim3(AT), 0, st, tail, tl, data, n, discard, mode_ac,
                       keep_timestamp, wg, out);
    return check(hipGetLastError());
}
