/* msd_cpr_impl.h -- Compact Position Reporting, one implementation for the position kernels (device) and the host
 * twin (libmsd_host.so): the whole of the reference's cpr.c, restated.
 *   cprModInt :64-68, cprModDouble :70-74, cprNLFunction :82-143, cprNFunction :148-152, cprDlonFunction :157-159,
 *   decodeCPRairborne :170-221, decodeCPRsurface :223-319, decodeCPRrelative :332-375.
 * The arithmetic is double + - * /, floor, fmod and comparisons against constants, every operation in the reference's
 * order.  It is bit-exact on the device as long as no multiply-add pair is contracted: every object that includes this
 * file is built with -ffp-contract=off, and nothing here calls fma() or a fast-math form. */
#ifndef MSD_CPR_IMPL_H
#define MSD_CPR_IMPL_H

#include <math.h>
#include <stdint.h>

#ifndef MSD_HD
#ifdef __HIPCC__
#define MSD_HD __host__ __device__ static inline
#else
#define MSD_HD static inline
#endif
#endif

MSD_HD int msd_cpr_mod_int(int a, int b) /* cpr.c:64-68: always non-negative */
{
    int r = a % b;
    return r < 0 ? r + b : r;
}

MSD_HD double msd_cpr_mod_double(double a, double b) /* cpr.c:70-74 */
{
    double r = fmod(a, b);
    return r < 0 ? r + b : r;
}

/* cpr.c:82-143, the transition latitudes of 1090-WP-9-14: NL = 59 below the first, one less behind each, 1 from 87
 * degrees on.  The comparisons are the reference's `lat < t`, in its order. */
MSD_HD int msd_cpr_nl(double lat)
{
    const double t[58] = {
        10.47047130, 14.82817437, 18.18626357, 21.02939493, 23.54504487, 25.82924707, 27.93898710, 29.91135686,
        31.77209708, 33.53993436, 35.22899598, 36.85025108, 38.41241892, 39.92256684, 41.38651832, 42.80914012,
        44.19454951, 45.54626723, 46.86733252, 48.16039128, 49.42776439, 50.67150166, 51.89342469, 53.09516153,
        54.27817472, 55.44378444, 56.59318756, 57.72747354, 58.84763776, 59.95459277, 61.04917774, 62.13216659,
        63.20427479, 64.26616523, 65.31845310, 66.36171008, 67.39646774, 68.42322022, 69.44242631, 70.45451075,
        71.45986473, 72.45884545, 73.45177442, 74.43893416, 75.42056257, 76.39684391, 77.36789461, 78.33374083,
        79.29428225, 80.24923213, 81.19801349, 82.13956981, 83.07199445, 83.99173563, 84.89166191, 85.75541621,
        86.53536998, 87.00000000};
    if (lat < 0)
        lat = -lat;
    for (int i = 0; i < 58; ++i)
        if (lat < t[i])
            return 59 - i;
    return 1;
}

MSD_HD int msd_cpr_n(double lat, int fflag) /* cpr.c:148-152 */
{
    int nl = msd_cpr_nl(lat) - (fflag ? 1 : 0);
    return nl < 1 ? 1 : nl;
}

MSD_HD double msd_cpr_dlon(double lat, int fflag, int surface) /* cpr.c:157-159 */
{
    return (surface ? 90.0 : 360.0) / msd_cpr_n(lat, fflag);
}

/* the longitude half both global decoders share (cpr.c:199-212 and :290-303): rlat and rlon of the half fflag names */
MSD_HD void msd_cpr_global_lon(double rlat0, double rlat1, double lon0, double lon1, int fflag, int surface, double *rlat,
                               double *rlon)
{
    const double rl = fflag ? rlat1 : rlat0;
    const int ni = msd_cpr_n(rl, fflag);
    const int nl = msd_cpr_nl(rl);
    const int m = (int)floor((((lon0 * (nl - 1)) - (lon1 * nl)) / 131072.0) + 0.5);
    *rlon = msd_cpr_dlon(rl, fflag, surface) * (msd_cpr_mod_int(m, ni) + (fflag ? lon1 : lon0) / 131072);
    *rlat = rl;
}

/* cpr.c:170-221.  0, -1 (the halves lie in different latitude zones: try again later) or -2 (bad data) */
MSD_HD int msd_cpr_airborne(int even_lat, int even_lon, int odd_lat, int odd_lon, int fflag, double *out_lat, double *out_lon)
{
    const double dlat0 = 360.0 / 60.0, dlat1 = 360.0 / 59.0;
    const double lat0 = even_lat, lat1 = odd_lat, lon0 = even_lon, lon1 = odd_lon;
    const int j = (int)floor(((59 * lat0 - 60 * lat1) / 131072) + 0.5);
    double rlat0 = dlat0 * (msd_cpr_mod_int(j, 60) + lat0 / 131072);
    double rlat1 = dlat1 * (msd_cpr_mod_int(j, 59) + lat1 / 131072);
    double rlat, rlon;
    if (rlat0 >= 270)
        rlat0 -= 360;
    if (rlat1 >= 270)
        rlat1 -= 360;
    if (rlat0 < -90 || rlat0 > 90 || rlat1 < -90 || rlat1 > 90)
        return -2;
    if (msd_cpr_nl(rlat0) != msd_cpr_nl(rlat1))
        return -1;
    msd_cpr_global_lon(rlat0, rlat1, lon0, lon1, fflag, 0, &rlat, &rlon);
    rlon -= floor((rlon + 180) / 360) * 360; /* to -180 .. +180 */
    *out_lat = rlat;
    *out_lon = rlon;
    return 0;
}

/* cpr.c:264-280: the quadrant of a surface latitude that lies closest to the reference; -90, 0 and +90 all encode to 0 */
MSD_HD double msd_cpr_surface_quadrant(double rlat, double reflat)
{
    if (rlat == 0) {
        if (reflat < -45)
            rlat = -90;
        else if (reflat > 45)
            rlat = 90;
    } else if ((rlat - reflat) > 45) {
        rlat -= 90;
    }
    return rlat;
}

/* cpr.c:223-319 */
MSD_HD int msd_cpr_surface(double reflat, double reflon, int even_lat, int even_lon, int odd_lat, int odd_lon, int fflag,
                           double *out_lat, double *out_lon)
{
    const double dlat0 = 90.0 / 60.0, dlat1 = 90.0 / 59.0;
    const double lat0 = even_lat, lat1 = odd_lat, lon0 = even_lon, lon1 = odd_lon;
    const int j = (int)floor(((59 * lat0 - 60 * lat1) / 131072) + 0.5);
    double rlat0 = dlat0 * (msd_cpr_mod_int(j, 60) + lat0 / 131072);
    double rlat1 = dlat1 * (msd_cpr_mod_int(j, 59) + lat1 / 131072);
    double rlat, rlon;
    rlat0 = msd_cpr_surface_quadrant(rlat0, reflat);
    rlat1 = msd_cpr_surface_quadrant(rlat1, reflat);
    if (rlat0 < -90 || rlat0 > 90 || rlat1 < -90 || rlat1 > 90)
        return -2;
    if (msd_cpr_nl(rlat0) != msd_cpr_nl(rlat1))
        return -1;
    msd_cpr_global_lon(rlat0, rlat1, lon0, lon1, fflag, 1, &rlat, &rlon);
    rlon += floor((reflon - rlon + 45) / 90) * 90; /* a multiple of 90 degrees towards the reference (:311) */
    rlon -= floor((rlon + 180) / 360) * 360;
    *out_lat = rlat;
    *out_lon = rlon;
    return 0;
}

/* cpr.c:332-375: one half against a reference position; 0 or -1 */
MSD_HD int msd_cpr_relative(double reflat, double reflon, int cprlat, int cprlon, int fflag, int surface, double *out_lat,
                            double *out_lon)
{
    const double flat = cprlat / 131072.0, flon = cprlon / 131072.0;
    const double dlat = (surface ? 90.0 : 360.0) / (fflag ? 59.0 : 60.0);
    const int j = (int)(floor(reflat / dlat) + floor(0.5 + msd_cpr_mod_double(reflat, dlat) / dlat - flat));
    double rlat = dlat * (j + flat);
    if (rlat >= 270)
        rlat -= 360;
    if (rlat < -90 || rlat > 90)
        return -1;
    if (fabs(rlat - reflat) > (dlat / 2)) /* more than half a cell away */
        return -1;
    const double dlon = msd_cpr_dlon(rlat, fflag, surface);
    const int m = (int)(floor(reflon / dlon) + floor(0.5 + msd_cpr_mod_double(reflon, dlon) / dlon - flon));
    double rlon = dlon * (m + flon);
    if (rlon > 180)
        rlon -= 360;
    if (fabs(rlon - reflon) > (dlon / 2))
        return -1;
    *out_lat = rlat;
    *out_lon = rlon;
    return 0;
}

#endif
