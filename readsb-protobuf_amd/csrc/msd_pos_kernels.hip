/*
 * msd_pos_kernels.hip -- the position tracker's kernels for gfx950 (modes_hip.h "positions").
 *
 * A call over n records runs four steps:
 *   1. find: one lane per record finds or inserts its aircraft's slot in the open-addressing table (compare-and-swap on
 *      the key word, linear probing).  Which slot a new aircraft lands in depends on the order the swaps arrive; nothing
 *      that is delivered depends on the slot, only on the aircraft's own state.
 *   2. group: the record indices are sorted by slot with least-significant-digit counting passes of 8 bits.  Every pass
 *      is stable: a record's place is (digit's total in the tiles before) + (its rank among the same digit in its tile),
 *      the rank from wave ballots and per-wave counts, the totals from integer sums -- no place is handed out by an
 *      atomic's return value.  After the passes each aircraft's records are contiguous and in stream order.
 *   3. walk: one lane per aircraft -- the lane at the first record of its run -- loads the state into registers, feeds
 *      msd_pos_feed one record after the other, stores the state.  A batch of one aircraft is a serial walk by one lane.
 *   4. each result is written at the record's own index; the counters are summed with integer atomics, the gate margin
 *      with an integer minimum over the double's bits, both independent of arrival order.
 * A table tracker (msd_pos_create_table) adds, per piece, 5. a second walk by the same heads over the same runs that feeds
 * the aircraft table entry (msd_trk_impl.h) from each record and from what step 3 wrote for it; and msd_pos_snapshot
 * reuses step 2's passes with the digit taken from the slots' keys to deliver the table in key order.
 * A tracker that matches Mode A/C replies (msd_modeac_impl.h) adds 1b. a kernel that counts the call's msgtype 32 records
 * per (receiver, code) with integer atomics, and trackMatchAC as three kernels: match cleared, one lane per slot, one
 * lane per (receiver, code).
 * A tracker that reduces (modes_hip.h "Reduced Beast output") runs the reduce instantiations of the two walks: step 3
 * leaves one byte per record for step 5, which keeps the aircraft's timers and leaves the record's verdict in its place.
 * The compacting Beast writer is msd_reduce_kernels.hip.
 * msd_pos_update_sbs (modes_hip.h "SBS output") runs the SBS instantiations of the two walks, which leave one row per
 * record: step 3 everything it knows, step 5 the aircraft's geometric delta.  No other call runs them.  The text writer
 * is msd_sbs_kernels.hip.
 * A tracker that keeps the receiver range (modes_hip.h "Receiver range") runs the range instantiation of step 3, which
 * leaves one code byte per record, and behind each piece 6. msd_pos_range_kernel, one lane per record: greatcircle and
 * getBearing for the records the walk marked, integer atomic maxima into the receivers' rows, and the aircraft's distance
 * from its last decoded record.  The writer of Statistics.polar_range is msd_range_kernels.hip.
 * Wave64 throughout: ballots are 64 bits wide and a workgroup of 256 threads is four waves.  The walk is double
 * precision arithmetic with long dependent chains and divergent branches per aircraft; its rate comes from the number of
 * aircraft in flight, not from the vector width.
 */
#include "msd_pos.h"

namespace {

constexpr uint32_t NT = MSD_POS_TILE;
constexpr uint64_t TOMB = MSD_POS_EMPTY - 1u; /* a slot whose aircraft expired, until the table is rebuilt */
#ifndef MSD_MODEAC_COMBINE_ROUNDS
#define MSD_MODEAC_COMBINE_ROUNDS 4 /* 0: every reply adds one by itself (scripts/modeac_rate.py measures both) */
#endif

__global__ void __launch_bounds__(NT) msd_pos_fill_kernel(uint64_t *keys, uint32_t cap)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i < cap)
        keys[i] = MSD_POS_EMPTY;
}

/* the slot of key, inserted when absent (*fresh = 1); cap: the table is full */
__device__ uint32_t find_or_insert(const msd_pos_table &t, uint64_t key, int *fresh)
{
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(t.keys);
    uint32_t s = msd_pos_hash(key) & (t.cap - 1u);
    for (uint32_t probes = 0; probes < t.cap; ++probes, s = (s + 1u) & (t.cap - 1u)) {
        unsigned long long k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == MSD_POS_EMPTY) {
            k = atomicCAS(&keys[s], (unsigned long long)MSD_POS_EMPTY, (unsigned long long)key);
            if (k == MSD_POS_EMPTY) {
                *fresh = 1;
                return s;
            }
        }
        if (k == key)
            return s;
    }
    return t.cap;
}

__global__ void __launch_bounds__(NT)
msd_pos_find_kernel(msd_pos_table t, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver,
                    uint32_t nrx, uint32_t n, uint32_t *slot, uint8_t *fresh, msd_position *out, uint32_t *ctl)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t r = receiver ? receiver[i] : 0u;
    const uint32_t addr = fields[i].addr;
    uint32_t s = t.cap;
    int f = 0;
    if (r >= nrx) {
        atomicOr(&ctl[MSD_POS_CTL_BAD_RECEIVER], 1u);
    } else if (msgs[i].msgtype != 32 && addr != 0) { /* track.c:999-1008 */
        s = find_or_insert(t, msd_pos_key(r, addr), &f);
        if (s == t.cap)
            atomicOr(&ctl[MSD_POS_CTL_FULL], 1u);
        if (f) {
            msd_pos_aircraft_init(&t.st[s]);
            if (t.trk)
                msd_trk_init(&t.trk[s]);
            if (t.hits)
                t.hits[2u * s] = t.hits[2u * s + 1u] = 0;
            if (t.next_reduce)
                for (uint32_t k = 0; k < MSD_REDUCE_TIMERS; ++k)
                    t.next_reduce[(size_t)s * MSD_REDUCE_TIMERS + k] = 0;
            if (t.dist)
                t.dist[s] = 0;
            atomicAdd(&ctl[MSD_POS_CTL_INSERTED], 1u);
        }
    }
    if (s == t.cap) { /* a skipped record; the walk never sees it */
        msd_position o = {};
        o.result = MSD_POS_NOT_TRIED;
        out[i] = o;
    }
    slot[i] = s;
    fresh[i] = (uint8_t)f;
}

__global__ void __launch_bounds__(NT) msd_pos_rollback_kernel(msd_pos_table t, const uint32_t *slot, const uint8_t *fresh, uint32_t n)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i < n && fresh[i]) {
        t.keys[slot[i]] = MSD_POS_EMPTY;
        if (t.dist)
            t.dist[slot[i]] = 0;
    }
}

/* ---- one counting pass over the piece's n indices: digit = (slot >> shift) & 255 ---- */
/* the record (relative to the piece) at place e < n.  Every pass writes a permutation of 0 .. n-1: a tile's 256 counts
 * cover each of its records once, so the scanned counts plus a record's rank among its tile's records of the same digit
 * are n distinct places below n. */
__device__ __forceinline__ uint32_t element(const uint32_t *idx_in, uint32_t e)
{
    return idx_in ? idx_in[e] : e;
}

/* where a pass takes its digit from: a record's slot (the grouping of a call), or a slot's 64-bit key (the snapshot) */
struct SlotDigit {
    const uint32_t *slot;
    uint32_t shift;
    __device__ __forceinline__ uint32_t operator()(uint32_t rec) const { return (slot[rec] >> shift) & 255u; }
};
struct KeyDigit {
    const uint64_t *keys;
    uint32_t shift;
    __device__ __forceinline__ uint32_t operator()(uint32_t s) const { return (uint32_t)(keys[s] >> shift) & 255u; }
};
struct FreeDigit { /* 0 for a slot in use, 1 for a free one: the stable pass that compacts the live slots to the front */
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint32_t s) const { return keys[s] >= MSD_POS_EMPTY - 1u ? 1u : 0u; }
};

/* hist[d * ntiles + tile] = records of digit d in the tile */
template <typename Digit>
__global__ void __launch_bounds__(NT) msd_pos_hist_kernel(const uint32_t *idx_in, Digit digit, uint32_t n, uint32_t *hist)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t e = blockIdx.x * NT + threadIdx.x;
    if (e < n)
        atomicAdd(&cnt[digit(element(idx_in, e))], 1u); /* a sum: the order does not matter */
    __syncthreads();
    hist[threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

/* exclusive prefix sum of a[0 .. total) in place, one workgroup */
__global__ void __launch_bounds__(1024) msd_pos_scan_kernel(uint32_t *a, uint32_t total)
{
    __shared__ uint32_t sh[1024];
    __shared__ uint32_t carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0)
        carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < total; base += 1024u) {
        const uint32_t i = base + tid;
        const uint32_t x = i < total ? a[i] : 0u;
        sh[tid] = x;
        __syncthreads();
        for (uint32_t d = 1; d < 1024u; d <<= 1) {
            const uint32_t y = tid >= d ? sh[tid - d] : 0u;
            __syncthreads();
            sh[tid] += y;
            __syncthreads();
        }
        const uint32_t incl = sh[tid], c = carry;
        if (i < total)
            a[i] = c + incl - x;
        __syncthreads();
        if (tid == 1023u)
            carry = c + incl;
        __syncthreads();
    }
}

/* idx_out[hist[d][tile] + rank of the record among the tile's records of digit d] = the record: stable */
template <typename Digit>
__global__ void __launch_bounds__(NT)
msd_pos_scatter_kernel(const uint32_t *idx_in, Digit digit, uint32_t n, const uint32_t *hist, uint32_t *idx_out)
{
    __shared__ uint32_t wcnt[NT / 64][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t w = 0; w < NT / 64; ++w)
        wcnt[w][tid] = 0;
    __syncthreads();
    const uint32_t e = blockIdx.x * NT + tid;
    const bool valid = e < n;
    const uint32_t rec = valid ? element(idx_in, e) : 0u;
    const uint32_t d = valid ? digit(rec) : 0u;
    /* the lanes of this wave with the same digit */
    unsigned long long peers = __ballot(valid);
    for (uint32_t b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long m = __ballot(valid && bit);
        peers &= bit ? m : ~m;
    }
    const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0)
        wcnt[wave][d] = __popcll(peers);
    __syncthreads();
    if (valid) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; ++w)
            before += wcnt[w][d];
        idx_out[hist[d * gridDim.x + blockIdx.x] + before + rank] = rec;
    }
}

/* step 3 and 4: the lane at the head of an aircraft's run walks it.  REDUCE: the tracker reduces, and the walk leaves in
 * forward[i] what the table walk's rule needs of this one: the members msd_pos_feed accepted and whether the aircraft has
 * been seen twice; a tracker that does not runs the instantiation without it.  SBS: the call is msd_pos_update_sbs, and
 * the walk leaves the record's row in sbs[i] -- all of it but the geometric delta, which the table walk adds; every other
 * call runs the instantiation without it.  RANGE: the tracker keeps the receiver range, and the walk leaves the record's
 * msd_pos_range_code in rcode[i] -- two comparisons, no arithmetic: the trigonometry is msd_pos_range_kernel's -- and marks
 * the aircraft's last decoded record; a tracker that does not runs the instantiation without it. */
template <bool REDUCE, bool SBS, bool RANGE>
__global__ void __launch_bounds__(NT)
msd_pos_walk_kernel(msd_pos_table t, const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver,
                    const msd_pos_receiver *rx, int filter_persistence, uint32_t base, uint32_t n, const uint32_t *slot,
                    const uint32_t *idx, msd_position *out, unsigned long long *dstats, uint8_t *forward, msd_sbs_track *sbs,
                    uint8_t *rcode)
{
    const uint32_t j = blockIdx.x * NT + threadIdx.x;
    if (j >= n)
        return;
    const uint32_t s = slot[base + element(idx, j)];
    if (s >= t.cap || (j > 0 && slot[base + element(idx, j - 1u)] == s))
        return;
    msd_pos_aircraft a = t.st[s];
    msd_pos_acc acc = {};
    acc.margin = INFINITY;
    uint32_t last = UINT32_MAX, last_code = 0;
    for (uint32_t k = j; k < n; ++k) {
        const uint32_t i = base + element(idx, k);
        if (slot[i] != s)
            break;
        const msd_fields f = fields[i];
        const msd_pos_receiver r = rx[receiver ? receiver[i] : 0u];
        msd_position o = {};
        if (REDUCE)
            acc.accepted = 0;
        msd_pos_feed(&a, &r, filter_persistence, msgs[i].sysTimestampMsg, &f, &o, &acc);
        out[i] = o;
        if (REDUCE)
            forward[i] = (uint8_t)(acc.accepted | (a.messages > 1 ? MSD_REDUCE_WALK_SEEN_TWICE : 0u));
        if (SBS) {
            msd_sbs_track row;
            msd_pos_sbs(&o, &acc, a.messages, &row);
            sbs[i] = row;
        }
        if (RANGE) {
            const uint32_t code = msd_pos_range_code(&a, &f, &o);
            rcode[i] = (uint8_t)code;
            if (code) {
                last = i;
                last_code = code;
            }
        }
    }
    if (RANGE && last != UINT32_MAX)
        rcode[last] = (uint8_t)(last_code | MSD_RANGE_CODE_LAST);
    t.st[s] = a;
    for (int c = 0; c < MSD_PC_N; ++c)
        if (acc.c[c])
            atomicAdd(&dstats[c], (unsigned long long)acc.c[c]);
    if (acc.margin < INFINITY)
        atomicMin(&dstats[MSD_PC_N], (unsigned long long)__double_as_longlong(acc.margin));
}

/* step 5, table trackers: the same heads walk the same runs again and feed the table entry, in place in device memory --
 * a record touches a few members of the 592 bytes, and only those are loaded and stored.  Reads what step 3 wrote for
 * each record (out[i].result) and writes its NIC / Rc.  HITS: the tracker matches Mode A/C replies and the walk resets
 * the aircraft's hit bytes; a tracker that does not runs the instantiation without them.  REDUCE: the tracker reduces;
 * the walk applies accept_data's reduce_forward half to the aircraft's timers and turns forward[i] from what the position
 * walk left there into the record's verdict (MSD_REDUCE_FORWARD, MSD_REDUCE_SEEN_TWICE). */
template <bool HITS, bool REDUCE, bool SBS>
__global__ void __launch_bounds__(NT)
msd_trk_walk_kernel(msd_pos_table t, const msd_message *msgs, const msd_fields *fields, uint32_t base, uint32_t n,
                    const uint32_t *slot, const uint32_t *idx, const msd_position *out, msd_pos_nicrc *nicrc,
                    uint32_t reduce_interval, uint8_t *forward, msd_sbs_track *sbs)
{
    const uint32_t j = blockIdx.x * NT + threadIdx.x;
    if (j >= n)
        return;
    const uint32_t s = slot[base + element(idx, j)];
    if (s >= t.cap || (j > 0 && slot[base + element(idx, j - 1u)] == s))
        return;
    msd_trk_aircraft *a = &t.trk[s];
    uint8_t *const hits = HITS ? &t.hits[2u * s] : nullptr;
    uint64_t *const next_reduce = REDUCE ? &t.next_reduce[(size_t)s * MSD_REDUCE_TIMERS] : nullptr;
    for (uint32_t k = j; k < n; ++k) {
        const uint32_t i = base + element(idx, k);
        if (slot[i] != s)
            break;
        const msd_message m = msgs[i];
        const msd_fields f = fields[i];
        const msd_position o = out[i];
        msd_pos_nicrc q;
        if (REDUCE) {
            const uint32_t w = forward[i];
            const int fwd = msd_trk_feed(a, m.sysTimestampMsg, &m, &f, &o, &q, hits, next_reduce, reduce_interval, w & 63u);
            forward[i] = (uint8_t)((fwd ? MSD_REDUCE_FORWARD : 0u) | (w & MSD_REDUCE_WALK_SEEN_TWICE ? MSD_REDUCE_SEEN_TWICE : 0u));
        } else {
            (void)msd_trk_feed(a, m.sysTimestampMsg, &m, &f, &o, &q, hits, nullptr, 0u, 0u);
        }
        nicrc[i] = q;
        if (SBS) { /* the row the position walk left: the aircraft's geometric delta after this record */
            msd_sbs_track row = sbs[i];
            msd_trk_sbs(a, m.sysTimestampMsg, &row);
            sbs[i] = row;
        }
    }
}

__global__ void __launch_bounds__(NT) msd_pos_expire_kernel(msd_pos_table t, uint64_t now, uint32_t *ctl)
{
    const uint32_t s = blockIdx.x * NT + threadIdx.x;
    if (s >= t.cap || t.keys[s] == MSD_POS_EMPTY)
        return;
    msd_pos_aircraft a = t.st[s];
    if (msd_pos_expire_one(&a, now)) {
        t.keys[s] = TOMB;
        atomicAdd(&ctl[MSD_POS_CTL_REMOVED], 1u);
    } else {
        t.st[s] = a;
        if (t.trk)
            msd_trk_expire_one(&t.trk[s], now);
    }
}

__global__ void __launch_bounds__(NT) msd_pos_rebuild_kernel(msd_pos_table from, msd_pos_table to)
{
    const uint32_t s = blockIdx.x * NT + threadIdx.x;
    if (s >= from.cap || from.keys[s] >= TOMB)
        return;
    int fresh = 0;
    const uint32_t d = find_or_insert(to, from.keys[s], &fresh); /* found: `to` is as large as `from` and was empty */
    to.st[d] = from.st[s];
    if (from.trk)
        to.trk[d] = from.trk[s];
    if (from.hits) {
        to.hits[2u * d] = from.hits[2u * s];
        to.hits[2u * d + 1u] = from.hits[2u * s + 1u];
    }
    if (from.next_reduce)
        for (uint32_t k = 0; k < MSD_REDUCE_TIMERS; ++k)
            to.next_reduce[(size_t)d * MSD_REDUCE_TIMERS + k] = from.next_reduce[(size_t)s * MSD_REDUCE_TIMERS + k];
    if (from.dist)
        to.dist[d] = from.dist[s];
}

/* snapshot: entry j of the output is the aircraft in slot idx[j] */
__global__ void __launch_bounds__(NT) msd_trk_gather_kernel(msd_pos_table t, const uint32_t *idx, uint32_t live, msd_aircraft *out)
{
    const uint32_t j = blockIdx.x * NT + threadIdx.x;
    if (j >= live)
        return;
    const uint32_t s = idx[j];
    if (s < t.cap)
        msd_trk_export(t.keys[s], &t.st[s], &t.trk[s], &out[j]);
}

/* ---- Mode A/C matching ---- */
/* 1b: count[receiver][code] += 1 for every msgtype 32 record.  Replies of one aircraft hammer one word, so lanes of a wave
 * with the same (receiver, code) are combined first: the first pending lane's word is broadcast, the lanes with the same
 * word are counted by a ballot and leave, and the first adds their number.  That is repeated, up to COMBINE_ROUNDS times,
 * only while it pays: a group of fewer than COMBINE_MIN lanes says the wave holds many different codes, where nothing
 * contends, and the lanes still pending add one each.  Integer sums: the order does not matter.  The whole wave runs the
 * loop -- no lane returns early -- and leaves it together: every condition of the loop is a ballot's. */
constexpr int COMBINE_ROUNDS = MSD_MODEAC_COMBINE_ROUNDS;
constexpr int COMBINE_MIN = 4;
__global__ void __launch_bounds__(NT)
msd_modeac_count_kernel(const msd_message *msgs, const msd_fields *fields, const uint32_t *receiver, uint32_t nrx, uint32_t n,
                        uint32_t *ac)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool pending = false;
    uint32_t word = 0;
    if (i < n && msgs[i].msgtype == 32) {
        const uint32_t r = receiver ? receiver[i] : 0u;
        if (r < nrx) { /* the find step has refused a call with any other */
            pending = true;
            word = r * (uint32_t)MSD_MODEAC_WORDS + MSD_MODEAC_COUNT + msd_mode_a_to_index(fields[i].squawk);
        }
    }
    for (int round = 0; round < COMBINE_ROUNDS; ++round) {
        const unsigned long long left = __ballot(pending);
        if (!left)
            break;
        const int first = __ffsll((long long)left) - 1;
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)word, first);
        const bool same = pending && word == w;
        const int peers = __popcll(__ballot(same));
        if ((int)lane == first)
            atomicAdd(&ac[w], (uint32_t)peers);
        pending = pending && !same;
        if (peers < COMBINE_MIN)
            break;
    }
    if (pending)
        atomicAdd(&ac[word], 1u);
}

__global__ void __launch_bounds__(NT) msd_modeac_clear_match_kernel(uint32_t *ac, uint32_t codes)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i < codes)
        ac[(size_t)(i >> 12) * MSD_MODEAC_WORDS + MSD_MODEAC_MATCH + (i & 4095u)] = 0;
}

/* one lane per slot; the key is tested first, the 592-byte entry is read for live slots only and only in the members
 * the rule looks at */
__global__ void __launch_bounds__(NT)
msd_modeac_match_kernel(msd_pos_table t, uint32_t nrx, uint64_t now, uint64_t message_now, const uint16_t *c_to_a, uint32_t *ac)
{
    const uint32_t s = blockIdx.x * NT + threadIdx.x;
    if (s >= t.cap)
        return;
    const uint64_t key = t.keys[s];
    if (key >= TOMB)
        return;
    const uint32_t r = (uint32_t)(key >> 25);
    if (r >= nrx)
        return;
    msd_modeac_match_one(&t.trk[s], t.st[s].seen, (uint32_t)(key & 0x1FFFFFFu), now, message_now, c_to_a,
                         ac + (size_t)r * MSD_MODEAC_WORDS, &t.hits[2u * s]);
}

__global__ void __launch_bounds__(NT) msd_modeac_age_kernel(uint32_t *ac, uint32_t codes)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i < codes)
        msd_modeac_age_one(ac + (size_t)(i >> 12) * MSD_MODEAC_WORDS, i & 4095u);
}

__global__ void __launch_bounds__(NT) msd_modeac_codes_kernel(const uint32_t *rx_ac, msd_modeac_code *out)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i < MSD_MODEAC_CODES) {
        msd_modeac_code c;
        msd_modeac_export_code(rx_ac, i, &c);
        out[i] = c;
    }
}

/* entry j of the output is the hits of the aircraft in slot idx[j]: msd_trk_gather_kernel's row j */
__global__ void __launch_bounds__(NT) msd_modeac_gather_kernel(msd_pos_table t, const uint32_t *idx, uint32_t live, msd_modeac_hit *out)
{
    const uint32_t j = blockIdx.x * NT + threadIdx.x;
    if (j >= live)
        return;
    const uint32_t s = idx[j];
    if (s < t.cap) {
        msd_modeac_hit h;
        msd_modeac_export_hit(t.keys[s], &t.hits[2u * s], &h);
        out[j] = h;
    }
}

/* ---- the receiver range (msd_pos_impl.h, "the receiver range") ---- */
/* One lane per record of the piece, behind the piece's walk: the records the walk marked MSD_RANGE_CODE_EVAL compute
 * greatcircle and getBearing -- some 300 double operations that no lane waits on another for -- and add to their
 * receiver's maxima; the record marked MSD_RANGE_CODE_LAST stores its aircraft's distance.  The maxima are integer atomics
 * (a non-negative double orders as its bits), so arrival order does not matter.  A call's records often share a receiver
 * and, with one aircraft or a stream of them along one airway, a bucket: COMBINE reduces the lanes of a wave that have
 * the same word first, as msd_modeac_count_kernel does -- the first pending lane's word is broadcast, the lanes with the
 * same word take the maximum among themselves with six butterfly steps and leave, and the first issues one atomic --,
 * while a group has at least COMBINE_MIN lanes and for at most RANGE_ROUNDS rounds; the lanes still pending issue their
 * own.  The margins are two minima over the whole wave and one atomic each.  Without COMBINE every lane issues its own
 * five atomics: scripts/range_rate.py measures both.  The whole wave runs every loop: their conditions are ballots'. */
constexpr int RANGE_ROUNDS = 4;

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

template <bool COMBINE>
__global__ void __launch_bounds__(NT)
msd_pos_range_kernel(msd_pos_table t, const msd_position *out, const uint32_t *receiver, const msd_pos_receiver *rx,
                     const uint32_t *slot, const uint8_t *rcode, uint32_t base, uint32_t n, int polar, msd_range_state *rng,
                     unsigned long long *margins)
{
    const uint32_t j = blockIdx.x * NT + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = base + j;
    const uint32_t code = j < n ? rcode[i] : 0u; /* 0 for a record the walk never saw: the caller zeroed the array */
    const unsigned long long inf = (unsigned long long)__double_as_longlong(INFINITY);
    bool eval = false;
    uint32_t r = 0;
    msd_range_one e = {};
    if (code & MSD_RANGE_CODE_EVAL) {
        r = receiver ? receiver[i] : 0u; /* below nrx: the find step has refused a call with any other */
        const msd_pos_receiver x = rx[r];
        if (x.latlon_valid) { /* track.c:285 */
            const msd_position o = out[i];
            msd_pos_range_one(&x, o.lat, o.lon, polar, &e);
            eval = true;
        }
    }
    if (code & MSD_RANGE_CODE_LAST) /* a walked record: its slot is below cap */
        t.dist[slot[i]] = eval ? e.metres : 0u;
    const unsigned long long lbits = eval && e.longest ? (unsigned long long)__double_as_longlong(e.range) : 0ull;
    const unsigned long long rm = eval ? (unsigned long long)__double_as_longlong(e.range_margin) : inf;
    const unsigned long long bm = eval && polar ? (unsigned long long)__double_as_longlong(e.bearing_margin) : inf;
    const bool pol = eval && polar && e.counts;
    const uint32_t word = r * MSD_RANGE_BUCKETS + e.bucket; /* receivers <= 65536: below 2^23 */
    if (!COMBINE) {
        if (eval) {
            atomicAdd(&rng[r].evaluated, 1ull);
            if (lbits)
                atomicMax(&rng[r].longest_bits, lbits);
            atomicMin(&margins[0], rm);
            if (polar)
                atomicMin(&margins[1], bm);
        }
        if (pol)
            atomicMax(&rng[r].polar[e.bucket], e.metres);
        return;
    }
    if (!__ballot(eval)) /* the whole wave */
        return;
    const unsigned long long wrm = wave_min(rm), wbm = wave_min(bm);
    if (lane == 0) {
        if (wrm < inf)
            atomicMin(&margins[0], wrm);
        if (wbm < inf)
            atomicMin(&margins[1], wbm);
    }
    bool pending = eval; /* longest and evaluated: the word is the receiver */
    for (int round = 0; round < RANGE_ROUNDS; ++round) {
        const unsigned long long left = __ballot(pending);
        if (!left)
            break;
        const int first = __ffsll((long long)left) - 1;
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, first);
        const bool same = pending && r == r0;
        const int peers = __popcll(__ballot(same));
        const unsigned long long best = wave_max(same ? lbits : 0ull);
        if ((int)lane == first) {
            atomicAdd(&rng[r0].evaluated, (unsigned long long)peers);
            if (best)
                atomicMax(&rng[r0].longest_bits, best);
        }
        pending = pending && !same;
        if (peers < COMBINE_MIN)
            break;
    }
    if (pending) {
        atomicAdd(&rng[r].evaluated, 1ull);
        if (lbits)
            atomicMax(&rng[r].longest_bits, lbits);
    }
    pending = pol; /* the polar range: the word is (receiver, bucket) */
    for (int round = 0; round < RANGE_ROUNDS; ++round) {
        const unsigned long long left = __ballot(pending);
        if (!left)
            break;
        const int first = __ffsll((long long)left) - 1;
        const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)word, first);
        const bool same = pending && word == w0;
        const int peers = __popcll(__ballot(same));
        const uint32_t best = (uint32_t)wave_max(same ? (unsigned long long)e.metres : 0ull);
        if ((int)lane == first && best)
            atomicMax(&rng[w0 / MSD_RANGE_BUCKETS].polar[w0 % MSD_RANGE_BUCKETS], best);
        pending = pending && !same;
        if (peers < COMBINE_MIN)
            break;
    }
    if (pending && e.metres)
        atomicMax(&rng[r].polar[e.bucket], e.metres);
}

/* one lane per receiver: its row as msd_range_receiver; longest_m / longest_nm from the device's own double */
__global__ void __launch_bounds__(NT)
msd_pos_range_read_kernel(msd_range_state *rng, uint32_t first, uint32_t count, int take, msd_range_receiver *out)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= count)
        return;
    msd_range_state *const s = &rng[first + k];
    msd_range_receiver *const row = &out[k];
    for (uint32_t b = 0; b < MSD_RANGE_BUCKETS; ++b)
        row->polar_range[b] = s->polar[b];
    const double longest = __longlong_as_double((long long)s->longest_bits);
    row->longest_m = (uint32_t)longest;               /* net_io.c:2249 */
    row->longest_nm = (uint32_t)(longest / 1852.0);   /* net_io.c:2250 */
    row->evaluated = s->evaluated;
    if (take)
        s->longest_bits = 0;
}

/* entry j of the output is the distance of the aircraft in slot idx[j]: msd_trk_gather_kernel's row j */
__global__ void __launch_bounds__(NT) msd_pos_range_gather_kernel(msd_pos_table t, const uint32_t *idx, uint32_t live, uint32_t *out)
{
    const uint32_t j = blockIdx.x * NT + threadIdx.x;
    if (j >= live)
        return;
    const uint32_t s = idx[j];
    out[j] = s < t.cap ? t.dist[s] : 0u;
}

/* one stable counting pass over n elements */
template <typename Digit>
void counting_pass(hipStream_t stream, const uint32_t *in, Digit digit, uint32_t n, uint32_t *hist, uint32_t *out)
{
    const uint32_t tiles = (n + NT - 1u) / NT;
    msd_pos_hist_kernel<<<tiles, NT, 0, stream>>>(in, digit, n, hist);
    msd_pos_scan_kernel<<<1, 1024, 0, stream>>>(hist, 256u * tiles);
    msd_pos_scatter_kernel<<<tiles, NT, 0, stream>>>(in, digit, n, hist, out);
}

uint32_t blocks(uint32_t n)
{
    return (n + NT - 1u) / NT;
}

} // namespace

void msd_pos_launch_fill(hipStream_t stream, uint64_t *keys, uint32_t cap)
{
    msd_pos_fill_kernel<<<blocks(cap), NT, 0, stream>>>(keys, cap);
}

void msd_pos_launch_find(hipStream_t stream, msd_pos_table t, const msd_message *msgs, const msd_fields *fields,
                         const uint32_t *receiver, uint32_t nrx, uint32_t n, uint32_t *slot, uint8_t *fresh, msd_position *out,
                         uint32_t *ctl)
{
    msd_pos_find_kernel<<<blocks(n), NT, 0, stream>>>(t, msgs, fields, receiver, nrx, n, slot, fresh, out, ctl);
}

void msd_pos_launch_rollback(hipStream_t stream, msd_pos_table t, const uint32_t *slot, const uint8_t *fresh, uint32_t n)
{
    msd_pos_rollback_kernel<<<blocks(n), NT, 0, stream>>>(t, slot, fresh, n);
}

/* step 3 with or without the range codes */
template <bool REDUCE, bool SBS>
static void pos_walk(hipStream_t stream, uint32_t tiles, msd_pos_table t, const msd_message *msgs, const msd_fields *fields,
                     const uint32_t *receiver, const msd_pos_receiver *rx, int filter_persistence, uint32_t base, uint32_t n,
                     const uint32_t *slot, const uint32_t *in, msd_position *out, unsigned long long *dstats, uint8_t *forward,
                     msd_sbs_track *sbs, uint8_t *rcode)
{
    if (rcode)
        msd_pos_walk_kernel<REDUCE, SBS, true><<<tiles, NT, 0, stream>>>(t, msgs, fields, receiver, rx, filter_persistence, base, n,
                                                                         slot, in, out, dstats, forward, sbs, rcode);
    else
        msd_pos_walk_kernel<REDUCE, SBS, false><<<tiles, NT, 0, stream>>>(t, msgs, fields, receiver, rx, filter_persistence, base,
                                                                          n, slot, in, out, dstats, forward, sbs, nullptr);
}

/* steps 3 to 5 over the grouped order `in` */
template <bool SBS>
static void walks(hipStream_t stream, uint32_t tiles, msd_pos_table t, const msd_message *msgs, const msd_fields *fields,
                  const uint32_t *receiver, const msd_pos_receiver *rx, int filter_persistence, uint32_t base, uint32_t n,
                  const uint32_t *slot, const uint32_t *in, msd_position *out, unsigned long long *dstats, msd_pos_nicrc *nicrc,
                  uint32_t reduce_interval, uint8_t *forward, msd_sbs_track *sbs, uint8_t *rcode)
{
    if (t.next_reduce) { /* (a table tracker: msd_pos_reduce_enable refuses any other) */
        pos_walk<true, SBS>(stream, tiles, t, msgs, fields, receiver, rx, filter_persistence, base, n, slot, in, out, dstats,
                            forward, sbs, rcode);
        if (t.hits)
            msd_trk_walk_kernel<true, true, SBS><<<tiles, NT, 0, stream>>>(t, msgs, fields, base, n, slot, in, out, nicrc,
                                                                           reduce_interval, forward, sbs);
        else
            msd_trk_walk_kernel<false, true, SBS><<<tiles, NT, 0, stream>>>(t, msgs, fields, base, n, slot, in, out, nicrc,
                                                                            reduce_interval, forward, sbs);
        return;
    }
    pos_walk<false, SBS>(stream, tiles, t, msgs, fields, receiver, rx, filter_persistence, base, n, slot, in, out, dstats, nullptr,
                         sbs, rcode);
    if (t.trk && t.hits)
        msd_trk_walk_kernel<true, false, SBS><<<tiles, NT, 0, stream>>>(t, msgs, fields, base, n, slot, in, out, nicrc, 0u, nullptr,
                                                                        sbs);
    else if (t.trk)
        msd_trk_walk_kernel<false, false, SBS><<<tiles, NT, 0, stream>>>(t, msgs, fields, base, n, slot, in, out, nicrc, 0u,
                                                                         nullptr, sbs);
}

void msd_pos_launch_piece(hipStream_t stream, msd_pos_table t, const msd_message *msgs, const msd_fields *fields,
                          const uint32_t *receiver, const msd_pos_receiver *rx, int filter_persistence, uint32_t base,
                          uint32_t n, const uint32_t *slot, uint32_t *idx_a, uint32_t *idx_b, uint32_t *hist,
                          msd_position *out, unsigned long long *dstats, msd_pos_nicrc *nicrc, uint32_t reduce_interval,
                          uint8_t *forward, msd_sbs_track *sbs, uint8_t *rcode)
{
    const uint32_t tiles = blocks(n);
    /* slots run from 0 to cap inclusive (cap = skipped) */
    uint32_t bits = 1;
    while ((1u << bits) <= t.cap)
        ++bits;
    const uint32_t *in = nullptr; /* the first pass reads the identity */
    uint32_t *bufs[2] = {idx_a, idx_b};
    int w = 0;
    for (uint32_t shift = 0; shift < bits; shift += 8) {
        counting_pass(stream, in, SlotDigit{slot + base, shift}, n, hist, bufs[w]);
        in = bufs[w];
        w ^= 1;
    }
    if (sbs) /* msd_pos_update_sbs: the instantiations that leave the rows (a table tracker: msd_pos_sbs_enable refuses any other) */
        walks<true>(stream, tiles, t, msgs, fields, receiver, rx, filter_persistence, base, n, slot, in, out, dstats, nicrc,
                    reduce_interval, forward, sbs, rcode);
    else
        walks<false>(stream, tiles, t, msgs, fields, receiver, rx, filter_persistence, base, n, slot, in, out, dstats, nicrc,
                     reduce_interval, forward, nullptr, rcode);
}

void msd_pos_launch_expire(hipStream_t stream, msd_pos_table t, uint64_t now_ms, uint32_t *ctl)
{
    msd_pos_expire_kernel<<<blocks(t.cap), NT, 0, stream>>>(t, now_ms, ctl);
}

void msd_pos_launch_rebuild(hipStream_t stream, msd_pos_table from, msd_pos_table to)
{
    msd_pos_rebuild_kernel<<<blocks(from.cap), NT, 0, stream>>>(from, to);
}

/* the slots of the live aircraft in ascending key order: the live slots to the front, in slot order; then
 * least-significant-digit passes over those by their keys.  -> the one of idx_a / idx_b that holds them */
static const uint32_t *ordered_slots(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits, uint32_t *idx_a,
                                     uint32_t *idx_b, uint32_t *hist)
{
    counting_pass(stream, (const uint32_t *)nullptr, FreeDigit{t.keys}, t.cap, hist, idx_a);
    uint32_t *bufs[2] = {idx_a, idx_b};
    int w = 0;
    for (uint32_t shift = 0; shift < key_bits; shift += 8) {
        counting_pass(stream, (const uint32_t *)bufs[w], KeyDigit{t.keys, shift}, live, hist, bufs[w ^ 1]);
        w ^= 1;
    }
    return bufs[w];
}

void msd_pos_launch_snapshot(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits, uint32_t *idx_a,
                             uint32_t *idx_b, uint32_t *hist, msd_aircraft *out)
{
    const uint32_t *idx = ordered_slots(stream, t, live, key_bits, idx_a, idx_b, hist);
    msd_trk_gather_kernel<<<blocks(live), NT, 0, stream>>>(t, idx, live, out);
}

const uint32_t *msd_pos_launch_ordered_slots(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits,
                                             uint32_t *idx_a, uint32_t *idx_b, uint32_t *hist)
{
    return ordered_slots(stream, t, live, key_bits, idx_a, idx_b, hist);
}

void msd_pos_launch_modeac_count(hipStream_t stream, const msd_message *msgs, const msd_fields *fields,
                                 const uint32_t *receiver, uint32_t nrx, uint32_t n, uint32_t *ac)
{
    msd_modeac_count_kernel<<<blocks(n), NT, 0, stream>>>(msgs, fields, receiver, nrx, n, ac);
}

void msd_pos_launch_modeac_match(hipStream_t stream, msd_pos_table t, uint32_t nrx, uint64_t now_ms, uint64_t message_now_ms,
                                 const uint16_t *c_to_a, uint32_t *ac)
{
    const uint32_t codes = nrx * MSD_MODEAC_CODES; /* at most 65536 * 4096 = 2^28 */
    msd_modeac_clear_match_kernel<<<blocks(codes), NT, 0, stream>>>(ac, codes);
    msd_modeac_match_kernel<<<blocks(t.cap), NT, 0, stream>>>(t, nrx, now_ms, message_now_ms, c_to_a, ac);
    msd_modeac_age_kernel<<<blocks(codes), NT, 0, stream>>>(ac, codes);
}

void msd_pos_launch_modeac_codes(hipStream_t stream, const uint32_t *rx_ac, msd_modeac_code *out)
{
    msd_modeac_codes_kernel<<<blocks(MSD_MODEAC_CODES), NT, 0, stream>>>(rx_ac, out);
}

void msd_pos_launch_modeac_hits(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits, uint32_t *idx_a,
                                uint32_t *idx_b, uint32_t *hist, msd_modeac_hit *out)
{
    const uint32_t *idx = ordered_slots(stream, t, live, key_bits, idx_a, idx_b, hist);
    msd_modeac_gather_kernel<<<blocks(live), NT, 0, stream>>>(t, idx, live, out);
}

void msd_pos_launch_range(hipStream_t stream, msd_pos_table t, const msd_position *out, const uint32_t *receiver,
                          const msd_pos_receiver *rx, const uint32_t *slot, const uint8_t *rcode, uint32_t base, uint32_t n,
                          int polar, int combine, msd_range_state *rng, unsigned long long *margins)
{
    if (combine)
        msd_pos_range_kernel<true><<<blocks(n), NT, 0, stream>>>(t, out, receiver, rx, slot, rcode, base, n, polar, rng, margins);
    else
        msd_pos_range_kernel<false><<<blocks(n), NT, 0, stream>>>(t, out, receiver, rx, slot, rcode, base, n, polar, rng, margins);
}

void msd_pos_launch_range_read(hipStream_t stream, msd_range_state *rng, uint32_t first, uint32_t count, int take,
                               msd_range_receiver *out)
{
    msd_pos_range_read_kernel<<<blocks(count), NT, 0, stream>>>(rng, first, count, take, out);
}

void msd_pos_launch_range_distances(hipStream_t stream, msd_pos_table t, uint32_t live, uint32_t key_bits, uint32_t *idx_a,
                                    uint32_t *idx_b, uint32_t *hist, uint32_t *out)
{
    const uint32_t *idx = ordered_slots(stream, t, live, key_bits, idx_a, idx_b, hist);
    msd_pos_range_gather_kernel<<<blocks(live), NT, 0, stream>>>(t, idx, live, out);
}
