/*
 * msd_avr_kernels.hip -- AVR raw text input on the GPU: the READ_MODE_ASCII line cutting of the --net-ri-port service
 * (net_io.c:501, 2448-2500) and decodeHexMessage's framing (net_io.c:1656-1764) as msd_avr_parse_line restates it, for a
 * whole byte stream at once.  DESIGN.md section 4.8.
 *
 * The rule that decides every '\n' on its own -- the window of masks, where a line starts, what it yields and its
 * record -- is msd_avr_impl.h's, shared with the group call's kernels.  Here the piece is the kept line followed by the
 * new bytes, and the counters are the stream's:
 *   msd_avr_count_kernel    a workgroup owns the '\n' of MSD_AVR_SPAN bytes: it classifies them and the
 *                           MSD_AVR_LOOKBACK in front of them, and every thread decides the lines that end among its 16
 *                           bytes.  Leaves the records per workgroup and adds the piece's counters.
 *   msd_avr_offsets_kernel  the counts to offsets, one workgroup (as the wire writers' scan_kernel).
 *   msd_avr_store_kernel    the same classification again; every line that yields a record is parsed from LDS and
 *                           written at its rank.
 */
#include <hip/hip_runtime.h>

#include "msd_avr_impl.h"
#include "msd_frames.h"

namespace {

/* the piece's bytes for classify: `tail`, then `data`, n in all */
struct Piece {
    const uint8_t *tail;
    uint32_t tl;
    const uint8_t *data;
    uint32_t n;
    __device__ __forceinline__ uint32_t operator()(int32_t p) const
    {
        uint32_t ch = 0xffu;
        if (p >= 0 && (uint32_t)p < n)
            ch = (uint32_t)p < tl ? tail[p] : data[(uint32_t)p - tl];
        return ch;
    }
};

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
    classify(W, Piece{tail, tl, data, n}, base);
    const Lines c = count_lines(W, base, rmin, discard != 0, mode_ac);
    if (c.n) {
        atomicAdd(&tot[3], c.n);
        atomicMax(&last, c.end);
        for (int k = 0; k < 3; ++k)
            if (c.kind[k])
                atomicAdd(&tot[k], c.kind[k]);
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
    __shared__ uint32_t part[AT / 64];
    const uint32_t total = block_sums_scan<AT>(wg, spans, part);
    if (threadIdx.x == 0)
        ctr[MSD_AVR_CTR_RECORDS] = total;
}

__global__ void __launch_bounds__(AT) msd_avr_store_kernel(const uint8_t *tail, uint32_t tl, const uint8_t *data,
                                                          uint32_t n, int discard, int mode_ac, int keep_timestamp,
                                                          const uint32_t *wg, msd_message *out)
{
    __shared__ Window W;
    __shared__ uint32_t part[AT / 64];
    if (wg[blockIdx.x + 1] == wg[blockIdx.x]) /* no record ends here */
        return;
    const int32_t base = (int32_t)(blockIdx.x * SPAN) - (int32_t)LB;
    const int rmin = base < 0 ? -base : 0;
    classify(W, Piece{tail, tl, data, n}, base);
    const Records r = my_records(W, rmin, discard != 0, mode_ac);
    uint32_t total;
    const uint32_t rank = wg[blockIdx.x] + block_scan<AT>(r.n, part, total);
#pragma unroll /* (three at most, each with its own copy of put_record) */
    for (uint32_t k = 0; k < r.n && k < MAX_RECS; ++k) {
        const uint32_t d = r[k];
        put_record(W, rec_a(d), rec_skip(d), rec_plen(d), keep_timestamp, out[rank + k]);
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
