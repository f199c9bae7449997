/*
 * msd_magbuf.c -- the signal power of accepted messages summed on the host, out of the caller's mag_buf views
 * (msd_demodulate_magbuf[s]).  Plain C, no GPU: tests/c/host_units.c links it.
 */
#include "modes_hip.h"
#include "msd_internal.h"

/* msd_demodulate_magbuf[s]: the caller's magnitudes are in host memory already -- the sums of squares of the few
 * accepted messages (demod_2400.c:386-399: m[j + 19 + k], k < msglen * 12 / 5) cost less here than a request upload, a
 * kernel, a download and a synchronisation (35 us of a 165 us call).  Position -> buffer: the batch is the buffers' new
 * samples one after the other; a message may run on into the next buffer's.  Samples no view holds count as zero. */
void msd_magbuf_power(const msd_magbuf_view *views, unsigned nviews, const uint64_t *req, size_t n, uint64_t *out)
{
    for (size_t i = 0; i < n; ++i) {
        const uint64_t rq = req[i];
        const int64_t first = (int64_t)(rq >> 16) - (int64_t)MSD_OVERLAP + 19; /* index into the batch's new samples */
        const uint64_t len = rq & 0xffffu;
        uint64_t acc = 0;
        if (first >= 0 && len) { /* nearly always the message lies inside one buffer's new samples: a plain sum of squares over
                                    consecutive u16 (the general walk below cost 0.9 ns a sample, a quarter of a twelve-buffer call) */
            const uint64_t b = (uint64_t)first / MSD_CHUNK_SAMPLES, o = (uint64_t)first % MSD_CHUNK_SAMPLES;
            if (b < nviews && o + len <= MSD_CHUNK_SAMPLES && o + len + MSD_OVERLAP <= views[b].validLength) {
                const uint16_t *m = views[b].data + MSD_OVERLAP + o;
                for (uint64_t k = 0; k < len; ++k)
                    acc += (uint64_t)((uint32_t)m[k] * (uint32_t)m[k]);
                out[i] = acc;
                continue;
            }
        }
        for (uint64_t k = 0; k < len; ++k) {
            const int64_t idx = first + (int64_t)k;
            uint64_t x = 0;
            if (idx < 0) {
                if (nviews && idx >= -(int64_t)MSD_OVERLAP)
                    x = views[0].data[(int64_t)MSD_OVERLAP + idx];
            } else {
                const uint64_t b = (uint64_t)idx / MSD_CHUNK_SAMPLES, o = (uint64_t)idx % MSD_CHUNK_SAMPLES;
                if (b < nviews && o + MSD_OVERLAP < views[b].validLength)
                    x = views[b].data[MSD_OVERLAP + o];
            }
            acc += x * x;
        }
        out[i] = acc;
    }
}
