/*
 * msd_avr_impl.h -- the line rule of the AVR text input, once, for msd_avr_kernels.hip (one stream per call, DESIGN.md
 * 4.8) and msd_group_avr_kernels.hip (one stream per receiver of a group).  With lines bounded by
 * MSD_AVR_LINE_MAX, where a line starts is a pure function of the MSD_AVR_LINE_MAX + 1 bytes in front of its '\n': the
 * byte behind the nearest '\n' among them, the start of the piece when the piece is shorter, or nowhere -- the line is
 * overlong and dropped.  So every '\n' is decided on its own.  A workgroup owns the '\n' of MSD_AVR_SPAN bytes; it
 * classifies those bytes and the MSD_AVR_LOOKBACK in front of them once -- newline, white space, NUL, hex digit -- into
 * 64-bit masks in LDS (Window), one ballot per class and 64 bytes.  A thread then takes the '\n' of its 16 bytes and
 * finds the line's start, the end of its text (the first NUL), the text without its white space and whether all its
 * payload digits are hex with a few word operations on the masks (line_at); only the prefix character and the ';' are
 * looked at as bytes.  A line that yields a record is parsed from the window (put_record).
 *
 * The two files differ in where a piece's bytes come from, which they hand to classify, and in where counts and records
 * go.  Each includes this header for its own unnamed namespace, as with msd_frames_impl.h.  What works on a filled
 * Window compiles on the host as well, where tests/c/avr_rule_units.cpp holds it to msd_avr_reader_feed; what needs a
 * workgroup (classify, my_newlines and the two loops over a thread's '\n') is device code only.
 */
#ifndef MSD_AVR_IMPL_H
#define MSD_AVR_IMPL_H

#include <stdint.h>

#include "msd_avr.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "msd_block_scan_impl.h"
#define MSD_AVR_FN __device__
#define MSD_AVR_INLINE __device__ __forceinline__
#else
#define MSD_AVR_FN
#define MSD_AVR_INLINE inline
#endif

namespace {

/* the leading zeros of a non-zero word, and 1 + the position of its lowest set bit */
#ifdef __HIPCC__
MSD_AVR_INLINE int clz64(uint64_t w) { return __clzll((long long)w); }
MSD_AVR_INLINE int ffs64(uint64_t w) { return __ffsll((unsigned long long)w); }
#else
MSD_AVR_INLINE int clz64(uint64_t w) { return __builtin_clzll(w); }
MSD_AVR_INLINE int ffs64(uint64_t w) { return __builtin_ffsll((long long)w); }
#endif

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

/* the four classes of a byte; 0xff, which stands for a byte outside the piece, has none */
MSD_AVR_INLINE bool is_nl(uint32_t ch) { return ch == '\n'; }
MSD_AVR_INLINE bool is_ws(uint32_t ch) { return ch == ' ' || ch - 9u <= 4u; /* space, 0x09..0x0D */ }
MSD_AVR_INLINE bool is_nul(uint32_t ch) { return ch == 0u; }
MSD_AVR_INLINE bool is_hex(uint32_t ch) { return ch - '0' < 10u || (ch | 0x20u) - 'a' < 6u; }

/* bits [0, top] of a word */
MSD_AVR_INLINE uint64_t upto(int top)
{
    return (2ull << top) - 1ull;
}

/* the highest position in [lo, hi) whose bit is set (INV: clear), -1 if none */
template <bool INV> MSD_AVR_FN int last_in(const uint64_t *m, int lo, int hi)
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
            return k * 64 + 63 - clz64(w);
        if (k == k0)
            return -1;
        --k;
        w = INV ? ~m[k] : m[k];
    }
}

/* the lowest such position */
template <bool INV> MSD_AVR_FN int first_in(const uint64_t *m, int lo, int hi)
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
            return k * 64 + ffs64(w) - 1;
        if (k == k1)
            return -1;
        ++k;
        w = INV ? ~m[k] : m[k];
    }
}

/* cnt <= 32 mask bits from position start on */
MSD_AVR_INLINE uint32_t bits_at(const uint64_t *m, int start, int cnt)
{
    const int k = start >> 6, o = start & 63;
    uint64_t v = m[k] >> o;
    if (o)
        v |= m[k + 1] << (64 - o);
    return (uint32_t)v & (uint32_t)((1ull << cnt) - 1ull);
}

/* The line that the '\n' at window position r ends.  rmin: the window position of the piece's first byte.  For a line
 * that yields a record: a = where its text starts, skip = prefix and timestamp / signal digits, plen = payload digits. */
MSD_AVR_FN int line_at(const Window &W, int r, int rmin, bool discard, int mode_ac, int &a, int &skip, int &plen)
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

/* hexval of msd_wire.c: -1 for anything else */
MSD_AVR_INLINE int hexval(uint32_t c)
{
    if (c - '0' < 10u)
        return (int)(c - '0');
    if ((c | 0x20u) - 'a' < 6u)
        return (int)((c | 0x20u) - 'a') + 10;
    return -1;
}

/* the record of the line whose text starts at window position a (msd_avr_parse_line behind its checks) */
MSD_AVR_FN void put_record(const Window &W, int a, int skip, int plen, int keep_timestamp, msd_message &o)
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

#ifdef __HIPCC__
using msd_block_scan::block_scan;
using msd_block_scan::block_sums_scan;

/* Window position r is piece position base + r.  src(p): the byte at piece position p, 0xff where the caller's piece
 * has none, so that bytes outside the piece get no class at all. */
template <class SRC> __device__ void classify(Window &W, const SRC &src, int32_t base)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t c = wave; c < NW; c += AT / 64) {
        const uint32_t ch = src(base + (int32_t)(c * 64 + lane));
        W.ch[c * 64 + lane] = (uint8_t)ch;
        const uint64_t m_nl = __ballot(is_nl(ch));
        const uint64_t m_ws = __ballot(is_ws(ch));
        const uint64_t m_nul = __ballot(is_nul(ch));
        const uint64_t m_hex = __ballot(is_hex(ch));
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

/* the '\n' among the calling thread's bytes, bit i for window position first + i */
__device__ __forceinline__ uint32_t my_newlines(const Window &W, int &first)
{
    const uint32_t off = threadIdx.x * PER;
    first = (int)(LB + off);
    return (uint32_t)(W.nl[(LB + off) >> 6] >> (off & 63u)) & ((1u << PER) - 1u);
}

/* The lines that the calling thread's '\n' end: how many of each kind, how many in all, and 1 + the piece position of
 * the last of them (0: none). */
struct Lines {
    uint32_t kind[3], n, end;
};

__device__ Lines count_lines(const Window &W, int32_t base, int rmin, bool discard, int mode_ac)
{
    int first;
    uint32_t mine = my_newlines(W, first);
    uint32_t c[3] = {0, 0, 0}, nlines = 0, hi = 0;
    while (mine) {
        const int bit = __ffs(mine) - 1;
        mine &= mine - 1u;
        int a, skip, plen;
        const int kind = line_at(W, first + bit, rmin, discard, mode_ac, a, skip, plen);
        c[0] += kind == L_LONG;
        c[1] += kind == L_DROP;
        c[2] += kind == L_REC;
        ++nlines;
        hi = (uint32_t)(base + first + bit) + 1u;
    }
    return Lines{{c[0], c[1], c[2]}, nlines, hi};
}

/* The records among them, in order: n of them, each a | skip << 16 | bit << 20 | plen << 24 with a, skip and plen as
 * line_at leaves them and the '\n' at window position `first` + bit. */
struct Records {
    uint32_t d0, d1, d2, n;
    int first;
    __device__ __forceinline__ uint32_t operator[](uint32_t k) const { return k == 0 ? d0 : k == 1 ? d1 : d2; }
};
__device__ __forceinline__ int rec_a(uint32_t d) { return (int)(d & 0xffffu); }
__device__ __forceinline__ int rec_skip(uint32_t d) { return (int)((d >> 16) & 0xfu); }
__device__ __forceinline__ int rec_bit(uint32_t d) { return (int)((d >> 20) & 0xfu); }
__device__ __forceinline__ int rec_plen(uint32_t d) { return (int)(d >> 24); }
static_assert(WIN <= 0x10000u && PER <= 16, "a record's fields in 32 bits");

__device__ Records my_records(const Window &W, int rmin, bool discard, int mode_ac)
{
    Records r = {0, 0, 0, 0, 0};
    uint32_t mine = my_newlines(W, r.first);
    while (mine) {
        const int bit = __ffs(mine) - 1;
        mine &= mine - 1u;
        int a, skip, plen;
        if (line_at(W, r.first + bit, rmin, discard, mode_ac, a, skip, plen) != L_REC)
            continue;
        const uint32_t d = (uint32_t)a | ((uint32_t)skip << 16) | ((uint32_t)bit << 20) | ((uint32_t)plen << 24);
        if (r.n == 0)
            r.d0 = d;
        else if (r.n == 1)
            r.d1 = d;
        else
            r.d2 = d;
        ++r.n;
    }
    return r;
}
#endif /* __HIPCC__ */

} // namespace

#endif
