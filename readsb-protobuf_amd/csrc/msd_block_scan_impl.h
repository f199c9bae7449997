/* msd_block_scan_impl.h -- the exclusive prefix sum of one value per thread over a workgroup, by wavefront shuffles and
 * one LDS word per wavefront, and the scan of an array of workgroup sums built on it.  Used by the wire writers
 * (msd_wire_store_impl.h) and the AVR text input (msd_avr_impl.h).  Device code only.
 *
 * block_sums_scan walks the sums THREADS at a time and carries `run` from round to round: up to THREADS workgroups --
 * 65 536 items at the writers' 256 -- the carry is never used, past that every offset rests on it.  The tests that hold
 * the second and later rounds: tests/test_gpu_scan_check.py (scripts/micro/scan_check.hip: scan_kernel<1> and <4> alone,
 * up to 65 537 sums, against a 64-bit host prefix, and block_scan twice on one `part`),
 * test_bytes_and_ends_past_one_round_of_the_scan in tests/test_gpu_wire_encode.py, tests/test_gpu_writer_scale.py (the
 * tracker's five writers), test_the_scan_past_one_round in tests/test_gpu_receiver_group_remote_wire.py, and
 * test_a_call_longer_than_one_piece of the AVR input.  They are sized around THREADS = 256: change both together. */
#ifndef MSD_BLOCK_SCAN_IMPL_H
#define MSD_BLOCK_SCAN_IMPL_H

#include <hip/hip_runtime.h>

#include <utility>

namespace msd_block_scan {

/* part[0] + part[1] + ..., as one written-out expression.  A loop over the words, unrolled, gives the same sum but the
 * compiler then orders its additions, and the instructions around them in every writer, in another way than it does for
 * the expression; the fold keeps each writer's kernels as they were measured. */
template <uint32_t... W>
__device__ __forceinline__ uint32_t sum_of(const uint32_t *part, std::integer_sequence<uint32_t, W...>)
{
    return (... + part[W]);
}

/* exclusive prefix of v over the workgroup's THREADS threads, and the total; `part`: THREADS / 64 words of LDS */
template <uint32_t THREADS> __device__ inline uint32_t block_scan(uint32_t v, uint32_t *part, uint32_t &total)
{
    static_assert(THREADS % 64 == 0, "whole wavefronts");
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
    for (uint32_t w = 0; w < THREADS / 64; ++w)
        before += w < wave ? part[w] : 0u;
    total = sum_of(part, std::make_integer_sequence<uint32_t, THREADS / 64>());
    return before + incl - v;
}

/* block_sums[0 .. nblocks) -> their exclusive prefix in place, block_sums[nblocks] = their total, which is also
 * returned.  One workgroup of THREADS. */
template <uint32_t THREADS>
__device__ inline uint32_t block_sums_scan(uint32_t *block_sums, uint32_t nblocks, uint32_t *part)
{
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < nblocks; b0 += THREADS) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nblocks ? block_sums[b] : 0u;
        uint32_t total;
        const uint32_t before = block_scan<THREADS>(v, part, total);
        if (b < nblocks)
            block_sums[b] = run + before;
        run += total;
    }
    if (threadIdx.x == 0)
        block_sums[nblocks] = run;
    return run;
}

} // namespace msd_block_scan

#endif
