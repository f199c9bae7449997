/* msd_wire_impl.h -- one msd_message as the Beast frame or AVR line readsb forwards (modesSendBeastOutput,
 * net_io.c:769-835; modesSendRawOutput, net_io.c:870-896): what host/msd_wire.c's msd_beast_frame_out and
 * msd_avr_line_out write, byte for byte.  Shared by the kernels of msd_wire_kernels.hip.  Device code only.
 *
 * A message is first brought into an msd_wire_src -- timestamp, level, payload words, byte count, and whether it
 * is forwarded at all --, from which the length and the bytes follow without looking at the record again.  The
 * payload sits in four little-endian words (byte k = w[k >> 2] >> 8 * (k & 3), as msd_emit_impl.h packs it) and
 * every loop over it is unrolled, so that nothing here is indexed at run time and nothing goes to scratch. */
#ifndef MSD_WIRE_IMPL_H
#define MSD_WIRE_IMPL_H

#include "modes_hip.h"

#define MSD_WIRE_MAX 44u /* MSD_BEAST_MAX: 2 + 2 * (7 + 14); an AVR line is at most 1 + 12 + 28 + 2 = 43 */

struct msd_wire_src {
    uint64_t ts;
    double level;
    uint32_t w[4];
    uint32_t nbytes;  /* msgbits / 8, at most 14 */
    uint32_t forward; /* msd_wire_forwards */
};

/* the syndromes of the 112 single bits of a 112-bit message (modesChecksum of a message with that bit alone); a
 * 56-bit message uses the last 56: a bit's syndrome depends on its distance from the end only */
struct msd_wire_syn_table {
    uint32_t v[112];
    constexpr msd_wire_syn_table() : v{}
    {
        for (int i = 0; i < 112; ++i) {
            uint32_t rem = 0;
            for (int byte = 0; byte < 11; ++byte) { /* crc.c:67-82 */
                if ((i >> 3) == byte)
                    rem ^= (uint32_t)(0x80u >> (i & 7)) << 16;
                for (int b = 0; b < 8; ++b)
                    rem = (rem & 0x800000u) ? ((rem << 1) ^ 0xfff409u) & 0xffffffu : (rem << 1) & 0xffffffu;
            }
            if (i >= 88)
                rem ^= 1u << (111 - i);
            v[i] = rem;
        }
    }
};
__constant__ const msd_wire_syn_table msd_wire_syn = msd_wire_syn_table();

/* bit b of the message (0 = the first bit sent) flipped in the payload words; b >= 112: nothing */
__device__ __forceinline__ void msd_wire_flip(uint32_t w[4], uint32_t b)
{
    const uint32_t mask = (0x80u >> (b & 7u)) << (8u * ((b >> 3) & 3u)); /* crc.c:417-425 */
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        w[j] ^= (b >> 5) == j ? mask : 0u;
}

/* msd_wire_verbatim: the repaired bits of a bare record found again -- the one or two positions in [5, msgbits)
 * whose single-bit syndromes xor to the syndrome the record carries -- and put back.  No pattern: the repaired
 * bytes stay, as on the host. */
__device__ inline void msd_wire_unrepair(const msd_message &mm, uint32_t w[4])
{
    const uint32_t nbits = mm.msgbits;
    if (mm.correctedbits == 0 || (nbits != 56 && nbits != 112))
        return;
    const uint32_t want = mm.msgtype == 11 ? (mm.crc & 0xffff80u) : mm.crc; /* mode_s.c:476-480 */
    const uint32_t *syn = msd_wire_syn.v + (112u - nbits);
    if (mm.correctedbits == 1) {
        for (uint32_t i = 5; i < nbits; ++i)
            if (syn[i] == want) {
                msd_wire_flip(w, i);
                return;
            }
        return;
    }
    for (uint32_t i = 5; i < nbits; ++i) {
        const uint32_t need = want ^ syn[i];
        for (uint32_t k = i + 1; k < nbits; ++k)
            if (syn[k] == need) {
                msd_wire_flip(w, i);
                msd_wire_flip(w, k);
                return;
            }
    }
}

/* a record as it goes out: wire_outgoing of host/msd_wire.c.  errbit / errbit2: where the encoder starts from a
 * resolve result, the repaired positions of the winning try (0xff: none) -- the received bytes are the repaired
 * ones with those bits flipped back; have_errbits = false: a bare record, searched (msd_wire_unrepair). */
__device__ __forceinline__ msd_wire_src msd_wire_source(const msd_message &mm, bool verbatim, bool have_errbits,
                                                        uint32_t errbit, uint32_t errbit2)
{
    msd_wire_src s;
    s.ts = mm.timestampMsg;
    s.level = mm.signalLevel;
    s.nbytes = min((uint32_t)mm.msgbits / 8u, 14u);
    s.forward = verbatim || mm.correctedbits < 2; /* net_io.c:1272-1285 */
#pragma unroll
    for (int j = 0; j < 4; ++j)
        s.w[j] = 0;
#pragma unroll
    for (int k = 0; k < 14; ++k)
        s.w[k >> 2] |= (uint32_t)mm.msg[k] << (8 * (k & 3));
    if (verbatim && mm.correctedbits) { /* net_io.c:775,874: msg = Modes.net_verbatim ? mm->verbatim : mm->msg */
        if (have_errbits) {
            if (errbit != 0xffu)
                msd_wire_flip(s.w, errbit);
            if (errbit2 != 0xffu)
                msd_wire_flip(s.w, errbit2);
        } else {
            msd_wire_unrepair(mm, s.w);
        }
    }
    return s;
}

/* net_io.c:819-823 in the host's double arithmetic: (int)round(sqrt(level) * 255), correctly rounded square root,
 * one rounded multiply (the build has neither fast-math nor contraction), round half away from zero; at least 1 for
 * a level above zero, at most 255 */
__device__ __forceinline__ uint32_t msd_wire_signal_byte(double level)
{
    const double r = sqrt(level) * 255.0;
    double t = trunc(r);
    if (r - t >= 0.5) /* exact: r and t are within a factor of two of each other or r < 1 */
        t += 1.0;
    uint32_t sig = t >= 255.0 ? 255u : (t >= 1.0 ? (uint32_t)t : 0u);
    if (level > 0 && sig < 1)
        sig = 1;
    return sig;
}

__device__ __forceinline__ uint32_t msd_wire_byte(const msd_wire_src &s, int k)
{
    return (s.w[k >> 2] >> (8 * (k & 3))) & 0xffu;
}

/* the Beast frame's bytes behind the type byte, before escaping: body[0..5] timestamp, [6] signal, [7..] payload */
__device__ __forceinline__ uint32_t msd_wire_beast_body(const msd_wire_src &s, uint32_t sig, int i)
{
    return i < 6 ? (uint32_t)(s.ts >> (40 - 8 * i)) & 0xffu : (i == 6 ? sig : msd_wire_byte(s, i - 7));
}

__device__ __forceinline__ uint32_t msd_wire_length(const msd_wire_src &s, int format)
{
    if (!s.forward)
        return 0;
    if (format != MSD_WIRE_BEAST)
        return 1u + (format == MSD_WIRE_AVR_MLAT && s.ts ? 12u : 0u) + 2u * s.nbytes + 2u;
    if (s.nbytes != 2 && s.nbytes != 7 && s.nbytes != 14)
        return 0; /* net_io.c:789-791 */
    const uint32_t sig = msd_wire_signal_byte(s.level);
    uint32_t len = 2u + 7u + s.nbytes;
#pragma unroll
    for (int i = 0; i < 21; ++i)
        len += (uint32_t)i < 7u + s.nbytes && msd_wire_beast_body(s, sig, i) == 0x1au ? 1u : 0u;
    return len;
}

__device__ __forceinline__ uint8_t msd_wire_hex(uint32_t v)
{
    return (uint8_t)(v < 10u ? '0' + v : 'A' + (v - 10u));
}

/* the msd_wire_length(s, format) bytes of the message to out (LDS) */
__device__ __forceinline__ void msd_wire_put(const msd_wire_src &s, int format, uint8_t *out)
{
    if (!s.forward)
        return;
    uint8_t *p = out;
    if (format != MSD_WIRE_BEAST) {
        const bool stamp = format == MSD_WIRE_AVR_MLAT && s.ts; /* net_io.c:877-881 */
        p[0] = stamp ? '@' : '*';
        if (stamp) {
#pragma unroll
            for (int d = 0; d < 12; ++d)
                p[1 + d] = msd_wire_hex((uint32_t)(s.ts >> (44 - 4 * d)) & 0xfu);
        }
        p += stamp ? 13 : 1;
#pragma unroll
        for (int k = 0; k < 14; ++k)
            if ((uint32_t)k < s.nbytes) {
                const uint32_t v = msd_wire_byte(s, k);
                p[2 * k] = msd_wire_hex(v >> 4);
                p[2 * k + 1] = msd_wire_hex(v & 0xfu);
            }
        p[2 * s.nbytes] = ';';
        p[2 * s.nbytes + 1] = '\n';
        return;
    }
    if (s.nbytes != 2 && s.nbytes != 7 && s.nbytes != 14)
        return;
    const uint32_t sig = msd_wire_signal_byte(s.level);
    *p++ = 0x1a;
    *p++ = s.nbytes == 7 ? '2' : (s.nbytes == 14 ? '3' : '1');
#pragma unroll
    for (int i = 0; i < 21; ++i)
        if ((uint32_t)i < 7u + s.nbytes) {
            const uint32_t v = msd_wire_beast_body(s, sig, i);
            *p++ = (uint8_t)v;
            if (v == 0x1au)
                *p++ = 0x1a;
        }
}

#endif
