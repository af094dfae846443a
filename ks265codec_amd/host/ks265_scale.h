/* ks265_scale.h - the tables of the device-input scaler (tests/yuv_scale_ref.py is the specification): per axis the first source sample and the Q14
 * coefficients of every output sample, in int64 arithmetic, word for word what the specification's table() computes - and the size rules.  Like ks265_roi.h and ks265_recon.h
 * this header calls nothing: no allocation, no library - the caller owns every buffer (tests/scale_plan_main.c drives it alone under the sanitizers). */
#ifndef KS265_SCALE_H
#define KS265_SCALE_H
#include <stdint.h>

#define KS_SCALE_TRIANGLE 0
#define KS_SCALE_CATMULL_ROM 1
#define KS_SCALE_MAX_TAPS 36
#define KS_SCALE_MAX_DIM 8192
#define KS_SCALE_MAX_RATIO 8
#define KS_SCALE_ONE 16384

/* one axis: S source, D destination samples */
static inline int ks265_scale_axis_ok(int S, int D)
{
    return S > 0 && D > 0 && S <= KS_SCALE_MAX_DIM && D <= KS_SCALE_MAX_DIM && (long long)S <= (long long)KS_SCALE_MAX_RATIO * D && (long long)D <= (long long)KS_SCALE_MAX_RATIO * S;
}

/* the size rules of a picture: source width a multiple of 8 and height even, destination multiples of 8, all at most 8192, ratios at most 8 either way */
static inline int ks265_scale_size_ok(int sw, int sh, int dw, int dh)
{
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || (sw & 7) || (sh & 1) || (dw & 7) || (dh & 7)) return 0;
    return ks265_scale_axis_ok(sw, dw) && ks265_scale_axis_ok(sh, dh);
}

static inline long long ks_scale_floordiv(long long a, long long b) { long long d = a / b; if (a % b != 0 && ((a < 0) != (b < 0))) --d; return d; }   /* b > 0 */

/* the weight of |m| = x < support */
static inline long long ks_scale_weight(long long x, long long q, int filter)
{
    if (filter == KS_SCALE_TRIANGLE) return x < q ? q - x : 0;
    if (x < q) return 3 * x * x * x - 5 * q * x * x + 2 * q * q * q;
    if (x < 2 * q) return -x * x * x + 5 * q * x * x - 8 * q * q * x + 4 * q * q * q;
    return 0;
}

/* output j: its weights into n[KS_SCALE_MAX_TAPS + 4], leading and trailing zeros dropped; returns the count (0: more than the array holds), *first = the lowest tap */
static inline int ks_scale_row(int S, int D, int filter, int cosited, int j, long long *n, int *first)
{
    const long long q = 2LL * (S > D ? S : D), R = filter == KS_SCALE_TRIANGLE ? q : 2 * q, a = 2LL * D;
    const long long b = cosited ? -2LL * j * S : (long long)D - (2LL * j + 1) * S;      /* m = a k + b */
    long long lo = ks_scale_floordiv(-R - b, a) + 1, hi = -ks_scale_floordiv(b - R, a) - 1;
    if (lo < 0) lo = 0;
    if (hi > S - 1) hi = S - 1;
    while (lo <= hi) { const long long m = a * lo + b; if (ks_scale_weight(m < 0 ? -m : m, q, filter) != 0) break; ++lo; }
    while (hi >= lo) { const long long m = a * hi + b; if (ks_scale_weight(m < 0 ? -m : m, q, filter) != 0) break; --hi; }
    if (hi < lo || hi - lo + 1 > KS_SCALE_MAX_TAPS + 4) return 0;
    for (long long k = lo; k <= hi; ++k) { const long long m = a * k + b; n[k - lo] = ks_scale_weight(m < 0 ? -m : m, q, filter); }
    *first = (int)lo;
    return (int)(hi - lo + 1);
}

/* T of an axis, the largest tap count of its outputs; 0 when the axis, the filter or the count (above KS_SCALE_MAX_TAPS) is outside the rules */
static inline int ks265_scale_axis_taps(int S, int D, int filter, int cosited)
{
    if (!ks265_scale_axis_ok(S, D) || (filter != KS_SCALE_TRIANGLE && filter != KS_SCALE_CATMULL_ROM)) return 0;
    long long n[KS_SCALE_MAX_TAPS + 4];
    int T = 0, first;
    for (int j = 0; j < D; ++j) {
        const int c = ks_scale_row(S, D, filter, cosited, j, n, &first);
        if (c <= 0 || c > KS_SCALE_MAX_TAPS) return 0;
        if (c > T) T = c;
    }
    return T;
}

/* the table of an axis: first[D], coef[D * T] with T = ks265_scale_axis_taps(...).  0, or -1 when the axis is outside the rules or some output's sum |c| exceeds 2 * 16384 */
static inline int ks265_scale_axis_fill(int S, int D, int filter, int cosited, int T, int32_t *first, int16_t *coef)
{
    if (!first || !coef || T <= 0 || T != ks265_scale_axis_taps(S, D, filter, cosited)) return -1;
    long long n[KS_SCALE_MAX_TAPS + 4];
    for (int j = 0; j < D; ++j) {
        int f = 0;
        const int cnt = ks_scale_row(S, D, filter, cosited, j, n, &f);
        long long N = 0, sum = 0, abs_sum = 0;
        int best = 0;
        for (int i = 0; i < cnt; ++i) { N += n[i]; if (n[i] > n[best]) best = i; }
        if (N <= 0) return -1;
        long long c[KS_SCALE_MAX_TAPS];
        for (int i = 0; i < cnt; ++i) { c[i] = ks_scale_floordiv(2LL * KS_SCALE_ONE * n[i] + N, 2 * N); sum += c[i]; }
        c[best] += KS_SCALE_ONE - sum;
        for (int i = 0; i < cnt; ++i) abs_sum += c[i] < 0 ? -c[i] : c[i];
        if (abs_sum > 2 * KS_SCALE_ONE) return -1;
        first[j] = f;
        for (int i = 0; i < T; ++i) coef[(long long)j * T + i] = i < cnt ? (int16_t)c[i] : 0;
    }
    return 0;
}

/* the four axes of a picture in the order the plans keep them: luma x, luma y, chroma x (cosited), chroma y */
static inline void ks265_scale_axes(int sw, int sh, int dw, int dh, int S[4], int D[4], int cosited[4])
{
    S[0] = sw; S[1] = sh; S[2] = sw / 2; S[3] = sh / 2;
    D[0] = dw; D[1] = dh; D[2] = dw / 2; D[3] = dh / 2;
    cosited[0] = cosited[1] = cosited[3] = 0; cosited[2] = 1;
}

/* the specification's samples on a plane in host memory (the CPU stand-in's scaler): src S_w x S_h with `pitch` bytes between rows and `step` between samples,
 * dst D_w x D_h packed; tmp holds S_h * D_w int16 */
static inline void ks265_scale_plane_host(const uint8_t *src, long long pitch, int step, int sw, int sh, uint8_t *dst, int dw, int dh,
                                          const int32_t *fx, const int16_t *cx, int Tx, const int32_t *fy, const int16_t *cy, int Ty, int16_t *tmp)
{
    for (int y = 0; y < sh; ++y)
        for (int j = 0; j < dw; ++j) {
            int32_t acc = 0;
            for (int i = 0; i < Tx; ++i) { const int k = fx[j] + i < sw ? fx[j] + i : sw - 1; acc += (int32_t)cx[(long long)j * Tx + i] * src[y * pitch + (long long)k * step]; }
            tmp[(long long)y * dw + j] = (int16_t)((acc + 128) >> 8);
        }
    for (int r = 0; r < dh; ++r)
        for (int j = 0; j < dw; ++j) {
            int32_t v = 0;
            for (int i = 0; i < Ty; ++i) { const int k = fy[r] + i < sh ? fy[r] + i : sh - 1; v += (int32_t)cy[(long long)r * Ty + i] * tmp[(long long)k * dw + j]; }
            v = (v + (1 << 19)) >> 20;
            dst[(long long)r * dw + j] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
}

#endif
