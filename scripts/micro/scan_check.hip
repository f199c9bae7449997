// The scan primitive of every stream writer alone (msd_block_scan_impl.h through msd_wire_store_impl.h), against a 64-bit
// prefix sum on the host: hipcc --offload-arch=gfx950 -O3 -I../../readsb-protobuf_amd/csrc -I../../include scan_check.hip -o scan_check
//
//   (a) msd_wire_store::scan_kernel<1> and <4> on arrays of nblocks workgroup sums, below, at and past the 256 sums that
//       one round of block_sums_scan covers -- from 257 on every offset rests on the carry between the rounds.  Every
//       word, the total at [nblocks], for <4> each of the four arrays (array q starts at q * (nblocks + 1)), and one
//       guard word behind the arrays and one in front, which must be untouched.  Values: random in [0, 256 * 44] (the most
//       a workgroup of the wire writers can sum to), all zero, and one whose grand total is exactly 2^32 - 1.
//   (b) block_scan<256> called twice in a row on the same `part`, one value per thread with runs of zeros.
//
// The comparison is host code (first_diff); the program first shows on host arrays that are wrong on purpose that it
// names the first differing index.  Prints "N cases, 0 differ" and exits 0, or says what differed and exits 1.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "msd_wire_store_impl.h"

#define HIP_OK(call)                                                                                                        \
    do {                                                                                                                    \
        const hipError_t e_ = (call);                                                                                       \
        if (e_ != hipSuccess) {                                                                                             \
            printf("%s: %s\n", #call, hipGetErrorString(e_));                                                               \
            exit(2);                                                                                                        \
        }                                                                                                                   \
    } while (0)

constexpr uint32_t GUARD = 0xA5C3F00Du;
constexpr uint32_t T = msd_wire_store::WT;

/* the first i with got[i] != want[i], or -1: want is 64 bits wide, so a sum that wrapped in 32 differs */
static long first_diff(const uint32_t *got, const uint64_t *want, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if ((uint64_t)got[i] != want[i])
            return (long)i;
    return -1;
}

/* want[0 .. n) = exclusive prefix of v, want[n] = the total */
static void host_prefix(const uint32_t *v, size_t n, uint64_t *want)
{
    uint64_t run = 0;
    for (size_t i = 0; i < n; ++i) {
        want[i] = run;
        run += v[i];
    }
    want[n] = run;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t bound) /* [0, bound] */
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(((rng_state >> 32) * ((uint64_t)bound + 1)) >> 32);
}

enum Values { RANDOM, ZERO, FULL };
static const char *const VALUES_NAME[] = {"random", "zero", "total 2^32-1"};

static void fill(uint32_t *v, uint32_t n, Values how)
{
    if (how == FULL) { /* n - 1 values of at most (2^32 - 1) / n, and what is missing to 2^32 - 1 at a random place */
        const uint32_t each = (uint32_t)(0xffffffffull / n);
        uint64_t sum = 0;
        for (uint32_t i = 0; i < n; ++i)
            sum += v[i] = rnd(each);
        const uint32_t k = rnd(n - 1);
        sum -= v[k];
        v[k] = (uint32_t)(0xffffffffull - sum);
        return;
    }
    for (uint32_t i = 0; i < n; ++i)
        v[i] = how == ZERO ? 0u : rnd(256u * 44u);
}

/* The comparison must be able to fail: right answers pass, and an array wrong at k (and again behind k) is reported at
 * k -- at the first word, at the first word of the second round, at the total, and for a sum that only wrapped. */
static int comparison_can_fail()
{
    const uint32_t n = 600;
    std::vector<uint32_t> v(n), got(n + 1);
    std::vector<uint64_t> want(n + 1);
    fill(v.data(), n, RANDOM);
    host_prefix(v.data(), n, want.data());
    int bad = 0;
    for (const long k : {0l, 1l, 255l, 256l, 257l, 599l, 600l}) {
        for (uint32_t i = 0; i <= n; ++i)
            got[i] = (uint32_t)want[i];
        if (first_diff(got.data(), want.data(), n + 1) != -1)
            ++bad;
        got[k] += 1;
        got[n] ^= 4u;
        if (first_diff(got.data(), want.data(), n + 1) != k)
            ++bad;
    }
    /* a carry forgotten between the rounds: every word of the second round short by the first round's total */
    for (uint32_t i = 0; i <= n; ++i)
        got[i] = (uint32_t)(i < 256 ? want[i] : want[i] - want[256]);
    if (first_diff(got.data(), want.data(), n + 1) != 256)
        ++bad;
    /* 2^32 against 0 */
    const uint32_t zero = 0;
    const uint64_t wrapped = 1ull << 32;
    if (first_diff(&zero, &wrapped, 1) != 0)
        ++bad;
    return bad;
}

template <uint32_t ARRAYS> static int scan_case(uint32_t nblocks, Values how)
{
    const size_t stride = (size_t)nblocks + 1, words = ARRAYS * stride;
    std::vector<uint32_t> h(words + 2), got(words + 2);
    std::vector<uint64_t> want(words);
    h[0] = h[words + 1] = GUARD;
    for (uint32_t q = 0; q < ARRAYS; ++q) {
        uint32_t *a = h.data() + 1 + q * stride;
        fill(a, nblocks, how);
        a[nblocks] = GUARD ^ q; /* the total's word holds anything before the launch */
        host_prefix(a, nblocks, want.data() + q * stride);
    }
    uint32_t *d = nullptr;
    HIP_OK(hipMalloc(&d, (words + 2) * sizeof(uint32_t)));
    HIP_OK(hipMemcpy(d, h.data(), (words + 2) * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(msd_wire_store::scan_kernel<ARRAYS>, dim3(1), dim3(T), 0, 0, d + 1, nblocks);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(got.data(), d, (words + 2) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d));
    int bad = 0;
    for (uint32_t q = 0; q < ARRAYS; ++q) {
        const long at = first_diff(got.data() + 1 + q * stride, want.data() + q * stride, stride);
        if (at >= 0) {
            printf("scan_kernel<%u> nblocks %u %s: array %u word %ld is %u, want %llu\n", ARRAYS, nblocks, VALUES_NAME[how], q,
                   at, got[1 + q * stride + at], (unsigned long long)want[q * stride + at]);
            bad = 1;
        }
    }
    if (got[0] != GUARD || got[words + 1] != GUARD) {
        printf("scan_kernel<%u> nblocks %u %s: guard words %08x %08x\n", ARRAYS, nblocks, VALUES_NAME[how], got[0],
               got[words + 1]);
        bad = 1;
    }
    return bad;
}

/* every workgroup scans its own T values of a, then its own T values of b, on the same part */
__global__ void __launch_bounds__(T) twice_kernel(const uint32_t *a, const uint32_t *b, uint32_t *before_a, uint32_t *before_b,
                                                  uint32_t *totals)
{
    __shared__ uint32_t part[T / 64];
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    uint32_t ta, tb;
    before_a[i] = msd_block_scan::block_scan<T>(a[i], part, ta);
    before_b[i] = msd_block_scan::block_scan<T>(b[i], part, tb);
    if (threadIdx.x == T - 1) { /* the last wavefront: the one that would read part before the others wrote it */
        totals[2 * blockIdx.x] = ta;
        totals[2 * blockIdx.x + 1] = tb;
    }
}

/* workgroup g's values: runs of zeros of every kind around a few values */
static void twice_values(uint32_t g, uint32_t *a, uint32_t *b)
{
    for (uint32_t t = 0; t < T; ++t) {
        a[t] = b[t] = 0;
        switch (g) {
        case 0: break;                                                  /* nothing at all, twice */
        case 1: a[t] = t == 0 ? 44u : 0u; b[t] = t == T - 1 ? 44u : 0u; break;
        case 2: a[t] = t == 63 ? 7u : 0u; b[t] = t == 64 ? 9u : 0u; break; /* either side of a wavefront's seam */
        case 3: a[t] = 44u; break;                                      /* a full part, then an empty one */
        case 4: b[t] = 44u; break;                                      /* and the other way round */
        case 5: a[t] = t / 64 == 1 ? rnd(44) : 0u; b[t] = t / 64 == 2 ? rnd(44) : 0u; break; /* one wavefront each */
        case 6: a[t] = (t / 16) % 3 == 0 ? rnd(44) : 0u; b[t] = (t / 5) % 4 == 3 ? rnd(1u << 20) : 0u; break;
        case 7: a[t] = t % 64 == 63 ? 0xffffffu : 0u; b[t] = t % 64 == 0 ? 0xffffffu : 0u; break;
        default: a[t] = rnd(3) ? 0u : rnd(256u * 44u); b[t] = rnd(7) ? 0u : rnd(0xffffffu); break; /* random runs */
        }
    }
}

static int twice_cases(uint32_t groups, int *cases)
{
    const size_t n = (size_t)groups * T;
    std::vector<uint32_t> a(n), b(n), ga(n), gb(n), gt(2 * groups);
    for (uint32_t g = 0; g < groups; ++g)
        twice_values(g, a.data() + (size_t)g * T, b.data() + (size_t)g * T);
    uint32_t *d = nullptr; /* a, b, before_a, before_b, totals */
    HIP_OK(hipMalloc(&d, (4 * n + 2 * groups) * sizeof(uint32_t)));
    HIP_OK(hipMemcpy(d, a.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d + n, b.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d + 2 * n, 0xEE, (2 * n + 2 * groups) * sizeof(uint32_t)));
    hipLaunchKernelGGL(twice_kernel, dim3(groups), dim3(T), 0, 0, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(ga.data(), d + 2 * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gb.data(), d + 3 * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gt.data(), d + 4 * n, 2 * groups * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d));
    int bad = 0;
    std::vector<uint64_t> want(T + 1);
    std::vector<uint32_t> got(T + 1);
    for (uint32_t g = 0; g < groups; ++g) {
        for (int second = 0; second < 2; ++second, ++*cases) {
            const uint32_t *v = (second ? b : a).data() + (size_t)g * T, *bef = (second ? gb : ga).data() + (size_t)g * T;
            host_prefix(v, T, want.data());
            for (uint32_t t = 0; t < T; ++t)
                got[t] = bef[t];
            got[T] = gt[2 * g + second];
            const long at = first_diff(got.data(), want.data(), T + 1);
            if (at >= 0) {
                printf("block_scan<%u> workgroup %u call %d: word %ld is %u, want %llu\n", T, g, second + 1, at, got[at],
                       (unsigned long long)want[at]);
                ++bad;
            }
        }
    }
    return bad;
}

int main()
{
    int cases = 0, bad = 0;
    const int blind = comparison_can_fail();
    if (blind) {
        printf("the comparison missed %d differences made on purpose\n", blind);
        return 1;
    }
    printf("the comparison names the first differing word of host arrays made wrong on purpose\n");
    const uint32_t sizes[] = {1, 2, 255, 256, 257, 511, 512, 513, 1000, 65537};
    for (const uint32_t nblocks : sizes)
        for (const Values how : {RANDOM, ZERO, FULL}) {
            bad += scan_case<1>(nblocks, how);
            bad += scan_case<4>(nblocks, how);
            cases += 2;
        }
    bad += twice_cases(24, &cases);
    printf("%d cases, %d differ\n", cases, bad);
    return bad != 0;
}
