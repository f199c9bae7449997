/*
 * msd_group_beast.cpp -- host side of msd_group_accept_beast ("Beast input per receiver"): the pieces of
 * whole entries, the device scratch (made by the first call), the launches of msd_group_beast_kernels.hip, and what
 * stays on the host per receiver -- the kept incomplete frame, the pending gap, and the host copy of the ICAO filter,
 * on which every entry's new addresses are inserted again in the device's order before the flip.  The remote counters
 * are the group's (msd_gb_view.remote): the AVR input adds to the same ones.  A piece costs two host synchronisations and a fixed number of launches and copies, whatever its number of entries.
 */
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "msd_group_beast.h"
#include "msd_group_scratch.h"
#include "msd_kernels.h"

using namespace msd_group_scratch;

namespace {

struct Rx {
    uint8_t tail[MSD_FR_TAIL_MAX];
    uint32_t tl = 0;
    uint64_t pending_gap = 0;
};

struct State {
    std::vector<Rx> rx;
    Buf up, buf, first, nxt, succ, info, mark, exitl, entry, good, cnt, nodes, cls, addr, flags, off, scan_tmp, newlist,
        newaddr, hash, snaps, add_first, out, ctr, tot, tails_out, stage;
    Buf h_up{nullptr, 0, true}, h_ctr{nullptr, 0, true}, h_tot{nullptr, 0, true}, h_tails{nullptr, 0, true},
        h_out{nullptr, 0, true}, h_new{nullptr, 0, true}, h_stage{nullptr, 0, true}, h_snaps{nullptr, 0, true};
    OutBufs ob; /* of the fields and wire calls, made by the first of them */
    Buf *all[35] = {&up,      &buf,   &first,   &nxt,  &succ,      &info,      &mark,  &exitl, &entry,
                    &good,    &cnt,   &nodes,   &cls,  &addr,      &flags,     &off,   &scan_tmp, &newlist,
                    &newaddr, &hash,  &snaps,   &add_first, &out,  &ctr,       &tot,   &tails_out, &stage,
                    &h_up,    &h_ctr, &h_tot,   &h_tails,   &h_out, &h_new,    &h_stage, &h_snaps};
};

/* entries [a, b) of the call as one piece */
int run_piece(const msd_gb_view *v, State &s, const uint8_t *bytes, int on_device, const msd_gb_input *in, uint32_t a,
              uint32_t b, msd_group_message_fn sink, const msd_gb_out *out, void *user)
{
    hipStream_t st = static_cast<hipStream_t>(v->stream);
    const uint32_t n = b - a;
    int rc = 0;

    /* the upload block: entries | tile -> entry | kept frames | snapshot slots | flips */
    uint32_t ntiles = 0;
    size_t newbytes = 0;
    for (uint32_t i = a; i < b; ++i) {
        const uint32_t seg = in[i].nbytes ? s.rx[in[i].receiver].tl + in[i].nbytes : 0u;
        ntiles += (seg + MSD_FR_TILE - 1u) / MSD_FR_TILE;
        newbytes += in[i].nbytes;
    }
    const uint32_t len = ntiles * MSD_FR_TILE;
    const size_t o_ent = 0, o_tile = up8(sizeof(msd_gb_entry) * n), o_tails = o_tile + up8(sizeof(uint32_t) * ntiles),
                 o_slot = o_tails + (size_t)MSD_FR_TAIL_MAX * n, o_flip = o_slot + up8(sizeof(uint32_t) * n),
                 up_bytes = o_flip + up8(sizeof(uint32_t) * n);
    if ((rc = grow(v, s.h_up, up_bytes)) || (rc = grow(v, s.up, up_bytes)))
        return rc;
    if (!on_device && ((rc = grow(v, s.h_stage, newbytes + 1)) || (rc = grow(v, s.stage, newbytes + 1))))
        return rc;
    uint8_t *hu = as<uint8_t>(s.h_up);
    msd_gb_entry *ent = reinterpret_cast<msd_gb_entry *>(hu + o_ent);
    uint32_t *tile_ent = reinterpret_cast<uint32_t *>(hu + o_tile);
    uint8_t *tails = hu + o_tails;
    uint32_t *slot = reinterpret_cast<uint32_t *>(hu + o_slot), *flip = reinterpret_cast<uint32_t *>(hu + o_flip);
    uint32_t t = 0;
    size_t staged = 0;
    for (uint32_t i = a; i < b; ++i) {
        const msd_gb_input &I = in[i];
        Rx &r = s.rx[I.receiver];
        msd_gb_entry &E = ent[i - a];
        memset(&E, 0, sizeof E);
        E.tl = I.nbytes ? r.tl : 0u; /* an empty entry leaves its receiver's kept frame and gap alone */
        E.pending_gap = r.pending_gap;
        E.now_ms = I.now_ms;
        E.s0 = t * MSD_FR_TILE;
        E.s1 = E.s0 + (I.nbytes ? E.tl + I.nbytes : 0u);
        E.tile0 = t;
        E.ntiles = (E.s1 - E.s0 + MSD_FR_TILE - 1u) / MSD_FR_TILE;
        E.snap = v->d_snaps ? I.receiver : i - a;
        E.opt = (uint32_t)I.nfix | (I.mode_ac ? MSD_GB_OPT_MODEAC : 0u);
        if (on_device) {
            E.src = I.offset;
        } else { /* the call's bytes packed densely into one page-locked array: one copy to the device */
            E.src = staged;
            memcpy(as<uint8_t>(s.h_stage) + staged, bytes + I.offset, I.nbytes);
            staged += I.nbytes;
        }
        for (uint32_t k = 0; k < E.ntiles; ++k)
            tile_ent[t++] = i - a;
        memcpy(tails + (size_t)MSD_FR_TAIL_MAX * (i - a), r.tail, MSD_FR_TAIL_MAX);
        slot[i - a] = I.receiver;
        flip[i - a] = I.now_ms >= I.filter->next_flip ? 1u : 0u; /* icaoFilterExpire's own test (icao_filter.c:150-164) */
    }

    /* scratch: by the bytes of the piece (every byte can be a node), the records by its shortest frame (11 bytes) */
    const size_t words = (size_t)len + 2, nrec_max = (size_t)len / 11u + 2;
    if ((rc = grow(v, s.buf, len + 16)) || (rc = grow(v, s.first, 4 * (size_t)(ntiles + 1))) ||
        (rc = grow(v, s.nxt, 4 * (size_t)(ntiles + 1))) || (rc = grow(v, s.succ, 4 * words)) ||
        (rc = grow(v, s.info, 2 * words)) || (rc = grow(v, s.mark, words)) ||
        (rc = grow(v, s.exitl, 4 * (size_t)(ntiles + 1))) || (rc = grow(v, s.entry, 4 * (size_t)(ntiles + 1))) ||
        (rc = grow(v, s.good, ntiles + 1)) || (rc = grow(v, s.cnt, 4 * (size_t)(ntiles + 2))) ||
        (rc = grow(v, s.nodes, 4 * words)) || (rc = grow(v, s.cls, words)) || (rc = grow(v, s.addr, 4 * words)) ||
        (rc = grow(v, s.flags, 4 * words)) || (rc = grow(v, s.off, 4 * words)) ||
        (rc = grow(v, s.scan_tmp, 4 * msd_fr_scan_tmp_words((uint32_t)words))) ||
        (rc = grow(v, s.newlist, 4 * nrec_max)) || (rc = grow(v, s.newaddr, 4 * nrec_max)) ||
        (rc = grow(v, s.out, sizeof(msd_message) * nrec_max)) || (rc = grow(v, s.add_first, 4 * (size_t)(n + 1))) ||
        (rc = grow(v, s.ctr, 8 * (size_t)MSD_FR_CTR_WORDS * n)) || (rc = grow(v, s.tot, 8 * MSD_GB_TOT_WORDS)) ||
        (rc = grow(v, s.tails_out, (size_t)MSD_FR_TAIL_MAX * n)) ||
        (rc = grow(v, s.h_ctr, 8 * (size_t)MSD_FR_CTR_WORDS * n)) || (rc = grow(v, s.h_tot, 8 * MSD_GB_TOT_WORDS)) ||
        (rc = grow(v, s.h_tails, (size_t)MSD_FR_TAIL_MAX * n)))
        return rc;
    uint32_t *snaps = v->d_snaps;
    if (!snaps) { /* a group that resolves on the host keeps no snapshots on the device: those of this piece */
        const size_t sb = sizeof(uint32_t) * MSD_SNAP_WORDS * (size_t)n;
        if ((rc = grow(v, s.h_snaps, sb)) || (rc = grow(v, s.snaps, sb)))
            return rc;
        uint32_t *h = as<uint32_t>(s.h_snaps);
        for (uint32_t i = a; i < b; ++i, h += MSD_SNAP_WORDS)
            snapshot_of(in[i].filter, h);
        HCK(v, hipMemcpyAsync(s.snaps.p, s.h_snaps.p, sb, hipMemcpyHostToDevice, st));
        snaps = as<uint32_t>(s.snaps);
    }
    HCK(v, hipMemcpyAsync(s.up.p, s.h_up.p, up_bytes, hipMemcpyHostToDevice, st));
    if (!on_device && staged)
        HCK(v, hipMemcpyAsync(s.stage.p, s.h_stage.p, staged, hipMemcpyHostToDevice, st));

    msd_gb_scratch x{};
    uint8_t *du = as<uint8_t>(s.up);
    x.n = n;
    x.ntiles = ntiles;
    x.len = len;
    x.ent = reinterpret_cast<const msd_gb_entry *>(du + o_ent);
    x.tile_ent = reinterpret_cast<const uint32_t *>(du + o_tile);
    x.tails_in = du + o_tails;
    x.tails_out = as<uint8_t>(s.tails_out);
    x.buf = as<uint8_t>(s.buf);
    x.first = as<uint32_t>(s.first);
    x.nxt = as<uint32_t>(s.nxt);
    x.succ = as<uint32_t>(s.succ);
    x.info = as<uint16_t>(s.info);
    x.mark = as<uint8_t>(s.mark);
    x.exitl = as<uint32_t>(s.exitl);
    x.entry = as<uint32_t>(s.entry);
    x.good = as<uint8_t>(s.good);
    x.cnt = as<uint32_t>(s.cnt);
    x.nodes = as<uint32_t>(s.nodes);
    x.cls = as<uint8_t>(s.cls);
    x.addr = as<uint32_t>(s.addr);
    x.flags = as<uint32_t>(s.flags);
    x.off = as<uint32_t>(s.off);
    x.scan_tmp = as<uint32_t>(s.scan_tmp);
    x.newlist = as<uint32_t>(s.newlist);
    x.newaddr = as<uint32_t>(s.newaddr);
    x.snaps = snaps;
    x.add_first = as<uint32_t>(s.add_first);
    x.out = as<msd_message>(s.out);
    x.ctr = as<unsigned long long>(s.ctr);
    x.tot = as<unsigned long long>(s.tot);

    const uint8_t *src = on_device ? bytes : as<uint8_t>(s.stage);
    if ((rc = msd_gb_launch_chain_decode(src, &v->tables, &x, st)))
        return fail(v, rc, "Beast input: chain and decode kernels failed to launch");
    /* first synchronisation: the piece's nodes, adds and an upper bound of its records */
    HCK(v, hipMemcpyAsync(s.h_tot.p, s.tot.p, 8 * MSD_GB_TOT_WORDS, hipMemcpyDeviceToHost, st));
    HCK(v, hipStreamSynchronize(st));
    const unsigned long long *tot = as<unsigned long long>(s.h_tot);
    const uint32_t nnodes = (uint32_t)tot[MSD_GB_TOT_NODES], nadds = (uint32_t)tot[MSD_GB_TOT_ADDS],
                   ncand = (uint32_t)tot[MSD_GB_TOT_CAND];
    if (nnodes > len || ncand > nrec_max || nadds > nrec_max)
        return fail(v, -EIO, "Beast input: %u nodes, %u messages in a piece of %u bytes", nnodes, ncand, len);
    if (nadds) {
        uint32_t hs = 64;
        while (hs < 2u * nadds)
            hs <<= 1;
        if ((rc = grow(v, s.hash, (size_t)16 * hs)))
            return rc;
        HCK(v, hipMemsetAsync(s.hash.p, 0xff, (size_t)16 * hs, st));
        x.hash = as<unsigned long long>(s.hash);
        x.hslots = hs;
    }
    if ((rc = grow(v, s.h_out, sizeof(msd_message) * ((size_t)ncand + 1))) ||
        (rc = grow(v, s.h_new, sizeof(uint32_t) * ((size_t)nadds + 1))))
        return rc;
    if ((rc = out_errbits(v, s.ob, out, ncand, &x.errbits)))
        return rc;
    if ((rc = msd_gb_launch_filter(nnodes, nadds, &v->tables, &x, st)))
        return fail(v, rc, "Beast input: filter kernels failed to launch");
    if (v->d_snaps && /* the resident snapshots: every entry's inserts, then its flip */
        (rc = msd_launch_group_filter_apply(v->d_snaps, n, reinterpret_cast<const uint32_t *>(du + o_slot), x.add_first,
                                            x.newaddr, reinterpret_cast<const uint32_t *>(du + o_flip), st)))
        return fail(v, rc, "Beast input: group filter kernel launch failed");
    /* a fields or wire call: the output stage over the piece's records, whose number only the device knows */
    const bool queued = out && nnodes && ncand;
    if (queued && (rc = out_queue(v, s.ob, *out, x.out, x.off + nnodes, ncand, x.ctr, n, x.errbits, st)))
        return rc;
    /* second synchronisation: counters, kept frames, records and the new-address lists */
    HCK(v, hipMemcpyAsync(s.h_ctr.p, s.ctr.p, 8 * (size_t)MSD_FR_CTR_WORDS * n, hipMemcpyDeviceToHost, st));
    HCK(v, hipMemcpyAsync(s.h_tails.p, s.tails_out.p, (size_t)MSD_FR_TAIL_MAX * n, hipMemcpyDeviceToHost, st));
    if (nnodes && ncand)
        HCK(v, hipMemcpyAsync(s.h_out.p, s.out.p, sizeof(msd_message) * ncand, hipMemcpyDeviceToHost, st));
    if (nnodes && nadds)
        HCK(v, hipMemcpyAsync(s.h_new.p, s.newaddr.p, sizeof(uint32_t) * nadds, hipMemcpyDeviceToHost, st));
    HCK(v, hipStreamSynchronize(st));

    const unsigned long long *ctr = as<unsigned long long>(s.h_ctr);
    for (uint32_t i = a; i < b; ++i) { /* nothing is committed before every entry has been looked at */
        const unsigned long long *c = ctr + (size_t)MSD_FR_CTR_WORDS * (i - a);
        if (c[MSD_GB_CTR_NTL] > MSD_FR_TAIL_MAX)
            return fail(v, -EIO, "Beast input: receiver %u: incomplete frame of %llu bytes", in[i].receiver, c[MSD_GB_CTR_NTL]);
        if (c[MSD_GB_CTR_REC_FIRST] + c[MSD_FR_CTR_RECORDS] > ncand || c[MSD_GB_CTR_NEW_FIRST] + c[MSD_FR_CTR_NEW] > nadds)
            return fail(v, -EIO, "Beast input: receiver %u: record or address range outside the piece's", in[i].receiver);
        if (out && !out_range_ok(s.ob, *out, queued, i - a, ncand))
            return fail(v, -EIO, "Beast input: receiver %u: wire bytes outside the piece's", in[i].receiver);
    }
    const msd_message *recs = as<msd_message>(s.h_out);
    const uint32_t *newaddr = as<uint32_t>(s.h_new);
    for (uint32_t i = a; i < b; ++i) {
        const msd_gb_input &I = in[i];
        const msd_gb_entry &E = ent[i - a];
        const unsigned long long *c = ctr + (size_t)MSD_FR_CTR_WORDS * (i - a);
        Rx &r = s.rx[I.receiver];
        /* icaoFilterAdd of the entry's new addresses in order of first add, as the device inserted them; then the flip */
        for (uint32_t k = 0; k < (uint32_t)c[MSD_FR_CTR_NEW]; ++k)
            msd_filter_add(I.filter, newaddr[c[MSD_GB_CTR_NEW_FIRST] + k]);
        msd_filter_expire(I.filter, I.now_ms); /* readsb.c:331 */
        add_remote(v->remote[I.receiver], c);
        if (I.nbytes) { /* what its next entry starts with: the incomplete frame, or the bytes since the last frame as a gap */
            if ((uint32_t)c[MSD_FR_CTR_EXIT] & MSD_FR_INC) {
                r.tl = (uint32_t)c[MSD_GB_CTR_NTL];
                memcpy(r.tail, as<uint8_t>(s.h_tails) + (size_t)MSD_FR_TAIL_MAX * (i - a), r.tl);
                r.pending_gap = 0;
            } else {
                r.tl = 0;
                r.pending_gap = (c[MSD_FR_CTR_NODES] ? 0 : r.pending_gap) + ((E.s1 - E.s0) - c[MSD_FR_CTR_LAST_END]);
            }
        }
        if (out)
            out_deliver(s.ob, *out, queued, I.receiver, i - a, recs, (uint32_t)c[MSD_GB_CTR_REC_FIRST],
                        (uint32_t)c[MSD_FR_CTR_RECORDS], user);
        else if (sink)
            for (uint32_t k = 0; k < (uint32_t)c[MSD_FR_CTR_RECORDS]; ++k)
                sink(I.receiver, recs + c[MSD_GB_CTR_REC_FIRST] + k, user);
    }
    return 0;
}

} // namespace

extern "C" {

int msd_gb_accept(const msd_gb_view *v, const void *bytes, int on_device, const msd_gb_input *in, uint32_t n,
                  msd_group_message_fn sink, const msd_gb_out *out, void *user)
{
    State *s = static_cast<State *>(*v->state);
    if (!s) {
        s = new (std::nothrow) State();
        if (!s)
            return fail(v, -ENOMEM, "out of host memory");
        try {
            s->rx.resize(v->max_receivers);
        } catch (...) {
            delete s;
            return fail(v, -ENOMEM, "out of host memory");
        }
        *v->state = s;
    }
    HCK(v, hipSetDevice(v->device));
    /* pieces of whole entries: a piece is closed when the next entry would take its new bytes past MSD_FR_PIECE */
    for (uint32_t a = 0; a < n;) {
        uint32_t b = a;
        size_t sum = 0;
        while (b < n && (b == a || sum + in[b].nbytes <= MSD_FR_PIECE))
            sum += in[b++].nbytes;
        const int rc = run_piece(v, *s, static_cast<const uint8_t *>(bytes), on_device, in, a, b, sink, out, user);
        if (rc)
            return rc;
        a = b;
    }
    return 0;
}

void msd_gb_reset_receiver(void *state, uint32_t receiver)
{
    State *s = static_cast<State *>(state);
    if (s && receiver < s->rx.size())
        s->rx[receiver] = Rx();
}

void msd_gb_free(void *state)
{
    State *s = static_cast<State *>(state);
    if (!s)
        return;
    for (Buf *b : s->all)
        release(*b);
    for (Buf *b : s->ob.all)
        release(*b);
    delete s;
}

} // extern "C"
