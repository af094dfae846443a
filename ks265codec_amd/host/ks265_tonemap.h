/* ks265_tonemap.h - the tables and the arithmetic of tone mapping on the way in (tests/tonemap_ref.py is the specification): HDR10 - PQ, BT.2020 - of 10 to
 * 16 bits in 4:2:0 to the packed 8-bit I420 of BT.709 in limited range.  Three tables per (curve, peak, white), every entry from the C library's pow in the specification's
 * order of operations (no fused multiply-add: built for the baseline instruction set), so the integers are the specification's; the constants of the code step per
 * (depth, range); and the whole routine on a picture in host memory, which is what the CPU stand-in runs.  Like ks265_scale.h this header calls nothing but libm: no
 * allocation, no library - the caller owns every buffer (tests/tonemap_main.c drives it alone under the sanitizers). */
#ifndef KS265_TONEMAP_H
#define KS265_TONEMAP_H
#include <math.h>
#include <stdint.h>

#define KS_TM_TRANSFER_PQ 16
#define KS_TM_BT2390 0
#define KS_TM_REINHARD 1
#define KS_TM_CLIP 2
#define KS_TM_SH_CODE 17
#define KS_TM_O_LEN 4104                                                /* 4097 entries and padding to a multiple of 16 bytes */

/* E: linear light of PQ code i / 4095 in 1 / 2^20; G: the gain in 1 / 2^15 at that light; O: q of linear light i / 4096; M: BT.2020 -> BT.709 in 1 / 2^14, rows summing to 16384 */
typedef struct ks265_tm_tables { uint32_t E[4096]; uint16_t G[4096]; uint16_t O[KS_TM_O_LEN]; int32_t M[3][3]; } ks265_tm_tables;
/* the code step of a (depth, range): offsets and the coefficients of 4095 2^17 / range */
typedef struct ks265_tm_norm { int32_t yoff, coff, ky, krv, kgu, kgv, kbu; } ks265_tm_norm;

static inline int ks265_tm_cfg_ok(int transfer, int curve, double peak, double white)
{
    return transfer == KS_TM_TRANSFER_PQ && curve >= KS_TM_BT2390 && curve <= KS_TM_CLIP && peak >= 100.0 && peak <= 10000.0 && white >= 80.0 && white <= 1000.0 && white <= peak;
}
/* 4:2:0 of 10 .. 16 bits, planar or semi-planar, from the fields of a KS265_IN_YUV code */
static inline int ks265_tm_format_ok(int layout, int sub, int depth) { return (layout == 0 || layout == 1) && sub == 0 && depth >= 10 && depth <= 16; }

static inline double ks_tm_pq_eotf(double e)
{
    const double m1 = 0.1593017578125, m2 = 78.84375, c1 = 0.8359375, c2 = 18.8515625, c3 = 18.6875;
    const double p = pow(e, 1.0 / m2);
    double n = p - c1;
    if (n < 0.0) n = 0.0;
    return 10000.0 * pow(n / (c2 - c3 * p), 1.0 / m1);
}
static inline double ks_tm_pq_inv(double nits)
{
    const double m1 = 0.1593017578125, m2 = 78.84375, c1 = 0.8359375, c2 = 18.8515625, c3 = 18.6875;
    const double y = pow(nits / 10000.0, m1);
    return pow((c1 + c2 * y) / (1.0 + c3 * y), m2);
}
static inline double ks_tm_curve(double m, int curve, double peak, double white)
{
    if (curve == KS_TM_CLIP) return m < 1.0 ? m : 1.0;
    if (curve == KS_TM_REINHARD) { const double P = peak / white; return m * (1.0 + m / (P * P)) / (1.0 + m); }
    const double top = ks_tm_pq_inv(peak), e1 = ks_tm_pq_inv(m * white) / top, ml = ks_tm_pq_inv(white) / top, ks = 1.5 * ml - 0.5;
    double e2 = e1;
    if (e1 > ks && ks < 1.0) {
        const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
        e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * ml;
    }
    return ks_tm_pq_eotf(e2 * top) / white;
}
static inline long long ks_tm_rnd(double x) { return (long long)floor(x + 0.5); }

/* the tables of a configuration ks265_tm_cfg_ok accepts */
static inline void ks265_tm_tables_fill(int curve, double peak, double white, ks265_tm_tables *t)
{
    static const double prim[3][3] = {{1.660491, -0.587641, -0.072850}, {-0.124550, 1.132900, -0.008349}, {-0.018151, -0.100579, 1.118730}};
    for (int i = 0; i < 4096; ++i) {
        double L = ks_tm_pq_eotf(i / 4095.0);
        if (L > peak) L = peak;
        const double x = L / white;
        t->E[i] = (uint32_t)ks_tm_rnd(x * 1048576.0);
        const long long g = ks_tm_rnd((x > 0.0 ? ks_tm_curve(x, curve, peak, white) / x : 1.0) * 32768.0);
        t->G[i] = (uint16_t)(g < 0 ? 0 : g > 32768 ? 32768 : g);
    }
    for (int i = 0; i < KS_TM_O_LEN; ++i) {
        const double L = i / 4096.0;
        t->O[i] = i > 4096 ? 0 : (uint16_t)ks_tm_rnd(65280.0 * (L < 0.018 ? 4.5 * L : 1.099 * pow(L, 0.45) - 0.099));
    }
    for (int r = 0; r < 3; ++r) {
        int32_t sum = 0;
        for (int c = 0; c < 3; ++c) { t->M[r][c] = (int32_t)ks_tm_rnd(prim[r][c] * 16384.0); sum += t->M[r][c]; }
        t->M[r][r] += 16384 - sum;
    }
}

static inline void ks265_tm_norm_fill(int depth, int full_range, ks265_tm_norm *n)
{
    const int s = depth - 8;
    const double ys = full_range ? (double)((1 << depth) - 1) : (double)(219 << s), cs = full_range ? (double)((1 << depth) - 1) : (double)(224 << s);
    const double one = 4095.0 * (double)(1 << KS_TM_SH_CODE);
    n->yoff = full_range ? 0 : 16 << s; n->coff = 1 << (depth - 1);
    n->ky = (int32_t)ks_tm_rnd(one / ys);
    n->krv = (int32_t)ks_tm_rnd(1.4746 * one / cs); n->kgu = (int32_t)ks_tm_rnd(0.16455 * one / cs);
    n->kgv = (int32_t)ks_tm_rnd(0.57135 * one / cs); n->kbu = (int32_t)ks_tm_rnd(1.8814 * one / cs);
}

/* one pixel: the samples Y, Cb, Cr (chroma already at luma resolution) -> q[3] (R, G, B in 1 / 256 of an 8-bit code) */
static inline void ks265_tm_pixel(const ks265_tm_tables *t, const ks265_tm_norm *n, int32_t Y, int32_t Cb, int32_t Cr, int32_t q[3])
{
    const int32_t ly = n->ky * (Y - n->yoff) + (1 << (KS_TM_SH_CODE - 1)), cb = Cb - n->coff, cr = Cr - n->coff;
    int32_t code[3] = {(ly + n->krv * cr) >> KS_TM_SH_CODE, (ly - n->kgu * cb - n->kgv * cr) >> KS_TM_SH_CODE, (ly + n->kbu * cb) >> KS_TM_SH_CODE}, tl[3];
    for (int c = 0; c < 3; ++c) code[c] = code[c] < 0 ? 0 : code[c] > 4095 ? 4095 : code[c];
    const int32_t mx = code[0] > code[1] ? (code[0] > code[2] ? code[0] : code[2]) : (code[1] > code[2] ? code[1] : code[2]);
    const uint64_t g = t->G[mx];
    for (int c = 0; c < 3; ++c) { const uint64_t v = ((uint64_t)t->E[code[c]] * g + (1u << 18)) >> 19; tl[c] = v > 65536 ? 65536 : (int32_t)v; }
    for (int r = 0; r < 3; ++r) {
        int32_t v = (t->M[r][0] * tl[0] + t->M[r][1] * tl[1] + t->M[r][2] * tl[2] + (1 << 9)) >> 10;
        v = v < 0 ? 0 : v > (1 << 20) ? 1 << 20 : v;
        const int32_t i = v >> 8, f = v & 255;
        q[r] = ((int32_t)t->O[i] * (256 - f) + (int32_t)t->O[i + 1] * f + 128) >> 8;      /* (i = 4096: f = 0 and O[4097] is padding) */
    }
}

static inline int32_t ks_tm_sample(const uint8_t *p, int depth, int msb) { const int32_t w = p[0] | p[1] << 8; return msb ? w >> (16 - depth) : w & ((1 << depth) - 1); }
static inline uint8_t ks_tm_clip255(int64_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

/* the specification's bytes of a picture in host memory: planes and pitches as ks265_in_desc has them (layout 0: Y, U, V; 1: Y, UV), W x H even, into packed I420 at dst.
 * qrow: 6 W int32 of the caller's (two rows of q).  Reads the elements of the rows and nothing else.  The way from q to bytes is tests/yuv_float_ref.py's q_to_i420 with
 * the Q16 coefficients of BT.709 in limited range */
static inline void ks265_tm_picture_host(const ks265_tm_tables *t, int layout, int depth, int msb, int full_range, const uint8_t *const plane[3], const long long pitch[3],
                                         int W, int H, uint8_t *dst, int32_t *qrow)
{
    ks265_tm_norm n;
    ks265_tm_norm_fill(depth, full_range, &n);
    const double Kr = 0.2126, Kb = 0.0722, Kg = 1 - Kr - Kb, sy = 219.0 / 255.0, sc = 224.0 / 255.0;
    const int64_t cy[3] = {ks_tm_rnd(sy * Kr * 65536), ks_tm_rnd(sy * Kg * 65536), ks_tm_rnd(sy * Kb * 65536)};
    const int64_t cb[3] = {ks_tm_rnd(-sc * Kr / (2 * (1 - Kb)) * 65536), ks_tm_rnd(-sc * Kg / (2 * (1 - Kb)) * 65536), ks_tm_rnd(sc / 2 * 65536)};
    const int64_t cr[3] = {ks_tm_rnd(sc / 2 * 65536), ks_tm_rnd(-sc * Kg / (2 * (1 - Kr)) * 65536), ks_tm_rnd(-sc * Kb / (2 * (1 - Kr)) * 65536)};
    const uint8_t *ub = plane[1], *vb = layout ? plane[1] + 2 : plane[2];
    const long long up = pitch[1], vp = layout ? pitch[1] : pitch[2];
    const int cs = layout ? 4 : 2, cw = W / 2;
    uint8_t *U = dst + (size_t)W * H, *V = U + (size_t)W * H / 4;
    for (int i = 0; i < H / 2; ++i) {
        for (int dy = 0; dy < 2; ++dy)
            for (int x = 0; x < W; ++x) {
                const int k = x >> 1, k1 = (x & 1) && k + 1 < cw ? k + 1 : k;
                const int32_t Y = ks_tm_sample(plane[0] + (long long)(2 * i + dy) * pitch[0] + 2LL * x, depth, msb);
                const int32_t u0 = ks_tm_sample(ub + i * up + (long long)k * cs, depth, msb), u1 = ks_tm_sample(ub + i * up + (long long)k1 * cs, depth, msb);
                const int32_t v0 = ks_tm_sample(vb + i * vp + (long long)k * cs, depth, msb), v1 = ks_tm_sample(vb + i * vp + (long long)k1 * cs, depth, msb);
                int32_t *q = qrow + ((size_t)dy * W + x) * 3;
                ks265_tm_pixel(t, &n, Y, x & 1 ? (u0 + u1 + 1) >> 1 : u0, x & 1 ? (v0 + v1 + 1) >> 1 : v0, q);
                dst[(size_t)(2 * i + dy) * W + x] = ks_tm_clip255((cy[0] * q[0] + cy[1] * q[1] + cy[2] * q[2] + ((int64_t)16 << 24) + (1 << 23)) >> 24);
            }
        for (int j = 0; j < cw; ++j) {
            int64_t s[3] = {0, 0, 0};
            for (int dy = 0; dy < 2; ++dy)
                for (int c = 0; c < 3; ++c) {
                    const int32_t *q = qrow + (size_t)dy * W * 3 + c;
                    s[c] += q[3 * (2 * j > 0 ? 2 * j - 1 : 0)] + 2 * q[3 * (2 * j)] + q[3 * (2 * j + 1)];
                }
            const int64_t off = ((int64_t)128 << 27) + ((int64_t)1 << 26);
            U[(size_t)i * cw + j] = ks_tm_clip255((cb[0] * s[0] + cb[1] * s[1] + cb[2] * s[2] + off) >> 27);
            V[(size_t)i * cw + j] = ks_tm_clip255((cr[0] * s[0] + cr[1] * s[1] + cr[2] * s[2] + off) >> 27);
        }
    }
}

#endif
