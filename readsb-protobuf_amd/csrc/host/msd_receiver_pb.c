/* msd_receiver_pb.c -- receiver.pb (modes_hip.h "receiver.pb"): the Receiver message of readsb.proto as protobuf-c 1.3's
 * receiver__pack writes what generateReceiverProtoBuf (net_io.c:2342-2404) sets.  A dozen scalars: a plain sequential
 * encoder on the host, in both libraries. */
#include <errno.h>
#include <math.h>
#include <string.h>

#include "modes_hip.h"

typedef struct rpb {
    uint8_t *at; /* NULL: the size alone */
    size_t n;
} rpb;

static void rpb_byte(rpb *b, unsigned v)
{
    if (b->at)
        b->at[b->n] = (uint8_t)v;
    b->n++;
}

static void rpb_varint(rpb *b, uint64_t v)
{
    for (; v >= 0x80; v >>= 7)
        rpb_byte(b, (unsigned)(v & 0x7f) | 0x80);
    rpb_byte(b, (unsigned)v);
}

static void rpb_u32(rpb *b, unsigned field, uint32_t v)
{
    if (v) {
        rpb_varint(b, field << 3);
        rpb_varint(b, v);
    }
}

static void rpb_fixed(rpb *b, unsigned field, unsigned wire_type, const void *value, unsigned nbytes)
{
    uint64_t bits = 0;
    memcpy(&bits, value, nbytes); /* (the builds are little-endian: the low bytes) */
    rpb_varint(b, field << 3 | wire_type);
    for (unsigned i = 0; i < nbytes; ++i)
        rpb_byte(b, (unsigned)(bits >> (8 * i)) & 0xff);
}

static void receiver_pack(const msd_receiver_info *info, rpb *b)
{
    double lat = info->latitude, lon = info->longitude;
    /* net_io.c:2367-2374.  An accuracy of 0 leaves the location in the file: the reference removes it elsewhere, not here */
    if (info->location_accuracy == 1 && (lat != 0.0 || lon != 0.0)) {
        lat = round(lat * 100) / 100;
        lon = round(lon * 100) / 100;
    }
    if (info->version && info->version[0]) {
        const size_t k = strlen(info->version);
        rpb_varint(b, 1 << 3 | 2);
        rpb_varint(b, k);
        for (size_t i = 0; i < k; ++i)
            rpb_byte(b, (unsigned char)info->version[i]);
    }
    if (!(0 == info->refresh)) /* field_is_zeroish: -0.0 goes, NaN stays */
        rpb_fixed(b, 2, 5, &info->refresh, 4);
    if (!(0 == lat))
        rpb_fixed(b, 3, 1, &lat, 8);
    if (!(0 == lon))
        rpb_fixed(b, 4, 1, &lon, 8);
    rpb_u32(b, 5, info->altitude);
    rpb_u32(b, 6, info->antenna_serial);
    rpb_u32(b, 7, info->antenna_flags);
    rpb_u32(b, 8, info->antenna_gps_sats);
    rpb_u32(b, 9, info->antenna_gps_hdop);
    rpb_u32(b, 14, info->antenna_reserved);
    rpb_u32(b, 15, info->history);
}

int msd_receiver_pb(const msd_receiver_info *info, uint8_t *out, size_t cap, size_t *out_len)
{
    if (!info || !out_len || info->reserved != 0 || (!out && cap > 0))
        return -EINVAL;
    rpb size = {NULL, 0};
    receiver_pack(info, &size);
    *out_len = size.n;
    if (size.n > cap)
        return -ENOSPC;
    rpb b = {out, 0};
    if (size.n)
        receiver_pack(info, &b);
    return 0;
}
