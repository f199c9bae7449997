/*
 * msd_frames_impl.h -- device code shared by the kernels of the Beast / AVR input: msd_frames_kernels.hip (one stream
 * per call) and msd_group_beast_kernels.hip (one stream per receiver of a group).  The
 * byte source, the exclusive prefix sums, decodeModesMessage's acceptance for one frame, the filter snapshot test and
 * the record writers.  Included inside each file's own unnamed namespace, so every object has its own copy.
 */
#ifndef MSD_FRAMES_IMPL_H
#define MSD_FRAMES_IMPL_H

#include <hip/hip_runtime.h>

#include "msd_frames.h"

namespace {

constexpr uint32_t FT = MSD_FR_TILE;
constexpr uint32_t SLOTS = 8192u;
constexpr uint32_t VACANT = 0xFFFFFFFFu;
constexpr int NT = 256;

struct Bytes {
    const uint8_t *tail;
    uint32_t tl;
    const uint8_t *data;
    uint32_t n;
    __device__ __forceinline__ uint8_t operator[](uint32_t i) const { return i < tl ? tail[i] : data[i - tl]; }
};

/* ---------------------------------------------------------------------------------------------------------------- */
/* exclusive prefix sums of uint32 (three kernels)                                                                  */
/* ---------------------------------------------------------------------------------------------------------------- */
constexpr uint32_t SCAN_PER = 4096u; /* elements per workgroup */

__device__ uint32_t block_excl(uint32_t x, uint32_t *sh, uint32_t *total)
{
    const uint32_t tid = threadIdx.x;
    sh[tid] = x;
    __syncthreads();
    for (uint32_t d = 1; d < NT; d <<= 1) {
        const uint32_t y = tid >= d ? sh[tid - d] : 0u;
        __syncthreads();
        sh[tid] += y;
        __syncthreads();
    }
    const uint32_t incl = sh[tid];
    *total = sh[NT - 1];
    __syncthreads();
    return incl - x;
}

__global__ void __launch_bounds__(NT) msd_fr_scan_sums_kernel(const uint32_t *in, uint32_t n, uint32_t *sums)
{
    __shared__ uint32_t sh[NT];
    const uint32_t base = blockIdx.x * SCAN_PER;
    uint32_t s = 0;
    for (uint32_t i = base + threadIdx.x; i < base + SCAN_PER && i < n; i += NT)
        s += in[i];
    uint32_t tot;
    block_excl(s, sh, &tot);
    if (threadIdx.x == 0)
        sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(NT) msd_fr_scan_top_kernel(uint32_t *sums, uint32_t nb, uint32_t *total_out)
{
    __shared__ uint32_t sh[NT];
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += NT) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t x = i < nb ? sums[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl(x, sh, &tot);
        if (i < nb)
            sums[i] = run + ex;
        run += tot;
    }
    if (threadIdx.x == 0 && total_out)
        *total_out = run;
}

__global__ void __launch_bounds__(NT) msd_fr_scan_apply_kernel(const uint32_t *in, uint32_t n, const uint32_t *sums,
                                                              uint32_t *out)
{
    __shared__ uint32_t sh[NT];
    const uint32_t base = blockIdx.x * SCAN_PER;
    constexpr uint32_t PER = SCAN_PER / NT; /* 16 consecutive elements per lane */
    const uint32_t my = base + threadIdx.x * PER;
    uint32_t v[PER], s = 0;
    for (uint32_t j = 0; j < PER; ++j) {
        v[j] = my + j < n ? in[my + j] : 0u;
        s += v[j];
    }
    uint32_t tot;
    uint32_t run = sums[blockIdx.x] + block_excl(s, sh, &tot);
    for (uint32_t j = 0; j < PER; ++j)
        if (my + j < n) {
            out[my + j] = run;
            run += v[j];
        }
}

/* out[i] = in[0] + .. + in[i - 1] for i < n, and out[n] = the total (in and out may be the same array) */
void scan_excl(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *tmp, hipStream_t st)
{
    const uint32_t nb = (n + SCAN_PER - 1u) / SCAN_PER;
    if (nb == 0) {
        (void)hipMemsetAsync(out, 0, sizeof(uint32_t), st);
        return;
    }
    hipLaunchKernelGGL(msd_fr_scan_sums_kernel, dim3(nb), dim3(NT), 0, st, in, n, tmp);
    hipLaunchKernelGGL(msd_fr_scan_top_kernel, dim3(1), dim3(NT), 0, st, tmp, nb, out + n);
    hipLaunchKernelGGL(msd_fr_scan_apply_kernel, dim3(nb), dim3(NT), 0, st, in, n, tmp, out);
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* decodeModesMessage's acceptance, one lane per frame                                                             */
/* ---------------------------------------------------------------------------------------------------------------- */

__device__ uint32_t crc24(const msd_fr_tables &T, const uint8_t *msg, int nbits)
{
    const int n = nbits / 8; /* crc.c:67-82 */
    uint32_t rem = 0;
    for (int i = 0; i < n - 3; ++i)
        rem = ((rem << 8) ^ T.crc_byte[msg[i] ^ (rem >> 16)]) & 0xffffffu;
    return rem ^ ((uint32_t)msg[n - 3] << 16) ^ ((uint32_t)msg[n - 2] << 8) ^ msg[n - 1];
}

/* modesChecksumDiagnose (crc.c:389-412) for a non-zero syndrome: number of bits (1, 2), -1 if none */
__device__ int diagnose(const msd_fr_tables &T, uint32_t syndrome, int nbits, int bit[2])
{
    bit[0] = bit[1] = -1;
    const int k = nbits == 112;
    if (T.nfix >= 2) {
        const uint64_t *tab = T.fix2[k];
        const uint32_t lg = T.fix2_lg[k];
        for (uint32_t slot = MSD_FIX2_HASH(syndrome, lg);; slot = (slot + 1) & ((1u << lg) - 1u)) {
            const uint64_t e = tab[slot];
            if (e == ~0ull)
                return -1;
            if (((uint32_t)e & 0xffffffu) == syndrome) {
                bit[0] = (int)((e >> 32) & 0xffu);
                const uint32_t b1 = (uint32_t)(e >> 40) & 0xffu;
                bit[1] = b1 == 0xffu ? -1 : (int)b1;
                return bit[1] < 0 ? 1 : 2;
            }
        }
    }
    if (T.nfix < 1 || !T.synhash)
        return -1;
    const uint32_t bkt = k ? (4u << MSD_SYNH_LG56) / 4u + ((syndrome * T.synh_mul112) >> (32u - MSD_SYNH_LG112))
                           : (syndrome * T.synh_mul56) >> (32u - MSD_SYNH_LG56);
    for (int j = 0; j < 4; ++j) {
        const uint32_t e = T.synhash[4u * bkt + j];
        if ((e & 0xffffffu) == syndrome) {
            bit[0] = (int)(e >> 24);
            return 1;
        }
    }
    return -1;
}

struct Decoded {
    uint8_t msg[14];
    uint32_t crc, addr;
    uint8_t df, msgbits, corrected, cls;
    uint8_t errbit[2]; /* the repaired bit positions, as diagnose names them (0xff: none) */
};

/* msg: nbytes (7 or 14) received bytes; the rest zero */
__device__ void decide(const msd_fr_tables &T, int nbytes, Decoded &d)
{
    d.corrected = 0;
    d.errbit[0] = d.errbit[1] = 0xff;
    d.crc = 0;
    d.addr = 0;
    d.df = d.msg[0] >> 3;
    d.msgbits = (d.df & 0x10u) ? 112 : 56; /* modesMessageLenByType */
    bool zero = true;
    for (int i = 0; i < 7; ++i)
        zero = zero && d.msg[i] == 0;
    if (zero) { /* mode_s.c:434-436 */
        d.cls = MSD_FR_C_BAD;
        return;
    }
    if (d.msgbits > 8 * nbytes) { /* a 56-bit frame with a long DF: DESIGN.md 4.8, the documented divergence */
        d.cls = MSD_FR_C_BAD;
        return;
    }
    d.crc = crc24(T, d.msg, d.msgbits);
    const uint32_t aa = ((uint32_t)d.msg[1] << 16) | ((uint32_t)d.msg[2] << 8) | d.msg[3];
    int bit[2];
    switch (d.df) {
    case 0: case 4: case 5: case 16: case 24: case 25: case 26: case 27: case 28: case 29: case 30: case 31:
    case 20: case 21: /* address/parity: accepted iff the syndrome is a known address */
        d.addr = d.crc;
        d.cls = MSD_FR_C_TEST;
        return;
    case 11:
        if (d.crc & 0xffff80u) {
            const int ne = diagnose(T, d.crc & 0xffff80u, d.msgbits, bit);
            if (ne != 1) { /* uncorrectable, or two bits: ambiguous in DF11 (mode_s.c:479-490) */
                d.cls = MSD_FR_C_BAD;
                return;
            }
            d.msg[bit[0] >> 3] ^= (uint8_t)(0x80u >> (bit[0] & 7));
            d.corrected = 1;
            d.errbit[0] = (uint8_t)bit[0];
            d.addr = ((uint32_t)d.msg[1] << 16) | ((uint32_t)d.msg[2] << 8) | d.msg[3];
            d.cls = MSD_FR_C_TEST;
            return;
        }
        d.addr = aa;
        d.cls = (d.crc & 0x7fu) == 0 ? MSD_FR_C_ADD : MSD_FR_C_ACC;
        return;
    case 17: case 18:
        if (d.crc != 0) {
            const int ne = diagnose(T, d.crc, d.msgbits, bit);
            if (ne < 0) {
                d.cls = MSD_FR_C_BAD;
                return;
            }
            for (int j = 0; j < ne; ++j) {
                d.msg[bit[j] >> 3] ^= (uint8_t)(0x80u >> (bit[j] & 7));
                d.errbit[j] = (uint8_t)bit[j];
            }
            d.corrected = (uint8_t)ne;
            d.addr = ((uint32_t)d.msg[1] << 16) | ((uint32_t)d.msg[2] << 8) | d.msg[3];
            d.cls = d.addr != aa ? MSD_FR_C_TEST : MSD_FR_C_ACC; /* mode_s.c:522-526 */
            return;
        }
        d.addr = aa;
        d.cls = d.df == 17 ? MSD_FR_C_ADD : MSD_FR_C_ACC;
        return;
    default:
        d.cls = MSD_FR_C_BAD;
        return;
    }
}

/* unescaped bytes of the frame at p: out[0..cnt) after the type byte */
__device__ __forceinline__ void unescape(const Bytes &B, uint32_t p, uint8_t *out, int cnt)
{
    uint32_t q = p + 2;
    for (int j = 0; j < cnt; ++j) {
        const uint8_t ch = B[q++];
        out[j] = ch;
        if (ch == 0x1a)
            ++q;
    }
}

struct Frame {
    uint64_t ts;
    double level;
    Decoded d;
    int nbytes;
};

__device__ void read_frame(const Bytes &B, uint32_t p, uint8_t type, Frame &f)
{
    uint8_t raw[21];
    f.nbytes = type == '1' ? 2 : type == '2' ? 7 : 14;
    unescape(B, p, raw, 7 + f.nbytes);
    f.ts = 0;
    for (int j = 0; j < 6; ++j)
        f.ts = (f.ts << 8) | raw[j];
    const double lvl = raw[6] / 255.0; /* net_io.c:1563-1565 */
    f.level = lvl * lvl;
    for (int j = 0; j < 14; ++j)
        f.d.msg[j] = j < f.nbytes ? raw[7 + j] : 0;
}

/* A filter snapshot (MSD_SNAP_WORDS, the two tables interleaved): icaoFilterTest (icao_filter.c:99-119) */
__device__ uint32_t hash24(uint32_t a)
{
    uint32_t h = 0;
    h += a & 0xff;         h += h << 10; h ^= h >> 6;
    h += (a >> 8) & 0xff;  h += h << 10; h ^= h >> 6;
    h += (a >> 16) & 0xff; h += h << 10; h ^= h >> 6;
    h += h << 3;
    h ^= h >> 11;
    h += h << 15;
    return h & (SLOTS - 1);
}

__device__ bool snap_table_has(const uint32_t *snap, uint32_t w, uint32_t addr)
{
    const uint32_t h0 = hash24(addr);
    uint32_t h = h0;
    while (snap[2 * h + w] != VACANT && snap[2 * h + w] != addr) {
        h = (h + 1) & (SLOTS - 1);
        if (h == h0)
            break;
    }
    return snap[2 * h + w] == addr;
}

__device__ bool snap_test(const uint32_t *snap, uint32_t addr)
{
    return snap_table_has(snap, 0, addr) || snap_table_has(snap, 1, addr);
}

__device__ void finish_record(msd_message &o, const Decoded &d, uint64_t ts, double level, uint64_t now_ms,
                              unsigned long long *ctr)
{
    o.timestampMsg = ts;
    o.sysTimestampMsg = now_ms;
    o.signalLevel = level;
    o.addr = d.addr;
    o.crc = d.crc;
    o.score = 0;
    o.msgtype = d.df;
    o.msgbits = d.msgbits;
    o.correctedbits = d.corrected;
    o.bestphase = 0;
    for (int j = 0; j < 14; ++j)
        o.msg[j] = d.msg[j];
    o.iid = d.df == 11 ? (uint8_t)(d.crc & 0x7fu) : 0;
    o.pad = 0;
    atomicAdd(ctr + MSD_FR_CTR_ACC0 + d.corrected, 1ull);
}

__device__ void modeac_record(msd_message &o, const uint8_t *b, uint64_t ts, double level, uint64_t now_ms)
{
    /* decodeModeAMessage (mode_ac.c:168-202), as msd_beast_reader delivers it */
    const uint32_t modeac = ((uint32_t)b[0] << 8) | b[1];
    o.timestampMsg = ts;
    o.sysTimestampMsg = now_ms;
    o.signalLevel = level;
    o.addr = (modeac & 0x0000FF7Fu) | (1u << 24);
    o.crc = 0;
    o.score = 0;
    o.msgtype = 32;
    o.msgbits = 16;
    o.correctedbits = 0;
    o.bestphase = 0;
    for (int j = 0; j < 14; ++j)
        o.msg[j] = j < 2 ? b[j] : 0;
    o.iid = 0;
    o.pad = 0;
}

inline uint32_t blocks(uint64_t n)
{
    return (uint32_t)((n + NT - 1) / NT);
}

int check(hipError_t e)
{
    return e == hipSuccess ? 0 : -5 /* -EIO */;
}

} // namespace

#endif
