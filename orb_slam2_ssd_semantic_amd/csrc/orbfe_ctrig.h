// orbfe_ctrig.h -- the library's canonical atan2 / sin / cos (DESIGN.md "Canonical trig"; tests/sim3_oracle.py c_atan2, c_sin,
// c_cos): fixed fp64 operation sequences -- fdlibm's polynomials, Cody-Waite reduction -- instead of the device library's or the
// host libm's, the same bits on the host and on the device.  For orbfe_sim3.hip (Horn's rotation) and orbfe_newpoints.h
// (CreateNewMapPoints' stereo parallax).  The files that include this are compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "orbfe_svd.h"   // ORBFE_HD

// the upper 32 bits of a double, and a double from them (lower word zero)
ORBFE_HD inline int hi_word(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __double2hiint(x);
#else
    uint64_t u;
    memcpy(&u, &x, 8);
    return (int)(uint32_t)(u >> 32);
#endif
}
ORBFE_HD inline double from_hi_word(int hi)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __hiloint2double(hi, 0);
#else
    const uint64_t u = (uint64_t)(uint32_t)hi << 32;
    double x;
    memcpy(&x, &u, 8);
    return x;
#endif
}

ORBFE_HD inline double c_atan_pos(double x)
{
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    const double aT[11] = {3.33333333333329318027e-01,  -1.99999999998764832476e-01, 1.42857142725034663711e-01,  -1.11111104054623557880e-01,
                           9.09088713343650656196e-02,  -7.69187620504482999495e-02, 6.66107313738753120669e-02,  -5.83357013379057348645e-02,
                           4.97687799461593236017e-02,  -3.65315727442169155270e-02, 1.62858201153657823623e-02};
    int id;
    if (x >= 7.378697629483821e19) return atanhi[3] + atanlo[3];
    if (x < 0.4375) {
        if (x < 1.862645149230957e-09) return x;
        id = -1;
    } else if (x < 1.1875) {
        if (x < 0.6875) {
            id = 0;
            x = (2.0 * x - 1.0) / (2.0 + x);
        } else {
            id = 1;
            x = (x - 1.0) / (x + 1.0);
        }
    } else if (x < 2.4375) {
        id = 2;
        x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
        id = 3;
        x = -1.0 / x;
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const double s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    return atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
}

ORBFE_HD inline double c_atan2(double y, double x)
{
    const double pi = 3.1415926535897931160e+00, pi_lo = 1.2246467991473531772e-16, pio2_hi = 1.57079632679489655800e+00;
    if (!(isfinite(x) && isfinite(y))) return (double)NAN;
    const bool xneg = signbit(x), yneg = signbit(y);
    if (y == 0) return !xneg ? y : yneg ? -pi : pi;
    if (x == 0) return yneg ? -pio2_hi : pio2_hi;
    const int ix = hi_word(x) & 0x7fffffff, iy = hi_word(y) & 0x7fffffff;
    const int k = (iy - ix) >> 20;
    double z;
    if (k > 60)
        z = pio2_hi + 0.5 * pi_lo;
    else if (xneg && k < -60)
        z = 0.0;
    else
        z = c_atan_pos(fabs(y / x));
    if (!xneg) return yneg ? -z : z;
    if (!yneg) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}

constexpr double C_TRIG_MAX = 823549.0;

// x >= 0 finite, x <= C_TRIG_MAX: n, y0, y1 with x = n * pi/2 + y0 + y1
ORBFE_HD inline int c_rem_pio2(double x, double &y0, double &y1)
{
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11,
                 pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    const int ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) {
        y0 = x;
        y1 = 0.0;
        return 0;
    }
    const int n = (int)(x * invpio2 + 0.5);
    const double fn = (double)n;
    double r = x - fn * pio2_1;
    double w = fn * pio2_1t;
    const int j = ix >> 20;
    y0 = r - w;
    int i = j - ((hi_word(y0) >> 20) & 0x7ff);
    if (i > 16) {
        double t = r;
        w = fn * pio2_2;
        r = t - w;
        w = fn * pio2_2t - ((t - r) - w);
        y0 = r - w;
        i = j - ((hi_word(y0) >> 20) & 0x7ff);
        if (i > 49) {
            t = r;
            w = fn * pio2_3;
            r = t - w;
            w = fn * pio2_3t - ((t - r) - w);
            y0 = r - w;
        }
    }
    y1 = (r - y0) - w;
    return n;
}

ORBFE_HD inline double c_ksin(double x, double y, int iy)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    if ((hi_word(x) & 0x7fffffff) < 0x3e400000) return x;
    const double z = x * x, v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

ORBFE_HD inline double c_kcos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const int ix = hi_word(x) & 0x7fffffff;
    if (ix < 0x3e400000) return 1.0;
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3fd33333) return 1.0 - (0.5 * z - (z * r - x * y));
    const double qx = ix > 0x3fe90000 ? 0.28125 : from_hi_word(ix - 0x00200000);
    const double hz = 0.5 * z - qx;
    const double a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}

ORBFE_HD inline double c_sin(double x)
{
    if (!isfinite(x) || fabs(x) > C_TRIG_MAX) return (double)NAN;
    const bool neg = signbit(x);
    double y0, y1, v;
    const int n = c_rem_pio2(fabs(x), y0, y1);
    if (n == 0) {
        v = c_ksin(y0, 0.0, 0);
    } else {
        const int q = n & 3;
        v = q == 0 ? c_ksin(y0, y1, 1) : q == 1 ? c_kcos(y0, y1) : q == 2 ? -c_ksin(y0, y1, 1) : -c_kcos(y0, y1);
    }
    return neg ? -v : v;
}

ORBFE_HD inline double c_cos(double x)
{
    if (!isfinite(x) || fabs(x) > C_TRIG_MAX) return (double)NAN;
    double y0, y1;
    const int n = c_rem_pio2(fabs(x), y0, y1);
    if (n == 0) return c_kcos(y0, 0.0);
    const int q = n & 3;
    return q == 0 ? c_kcos(y0, y1) : q == 1 ? -c_ksin(y0, y1, 1) : q == 2 ? -c_kcos(y0, y1) : c_ksin(y0, y1, 1);
}
