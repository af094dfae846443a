/* TEST INFRASTRUCTURE: the device library's CPU stand-in with device input and the scaler (hip_stub_scale.c, included as it is, its picture entries under other names) plus the
 * float sample formats KS265_IN_RGB_F16 / _BF16 / _F32 (include/ks265_hip.h) in ks265_input_validate / ks265_input_convert / ks265_input_scale and the way back,
 * ks265_output_validate / ks265_output_convert (with ks265_set_stream, as hip_stub_recon.c has it), in plain C after tests/yuv_float_ref.py and tests/yuv_output_ref.py.
 * "Device memory" is the process's own.  Every other format goes to the entries of hip_stub_scale.c.  The two conversion routines, stub_float_to_i420 and
 * stub_i420_to_rgb, take nothing but pointers and numbers: -DKS265_STUB_FLOAT_ROUTINES_ONLY leaves them alone in the translation unit, for a program of its own. */
#ifndef KS265_STUB_FLOAT_ROUTINES_ONLY
#define ks265_input_validate ks265_u8_input_validate
#define ks265_input_convert ks265_u8_input_convert
#define ks265_input_scale_validate ks265_u8_input_scale_validate
#define ks265_input_scale ks265_u8_input_scale
#include "hip_stub_scale.c"
#undef ks265_input_validate
#undef ks265_input_convert
#undef ks265_input_scale_validate
#undef ks265_input_scale
#else
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "ks265_hip.h"
#endif

static int f_q16(double x) { return (int)floor(x * 65536 + 0.5); }

/* the sample at p as float32, exactly (float16 by hand: no compiler type is needed) */
static float f_sample(const uint8_t *p, int format)
{
    uint32_t b; float f;
    if (format == KS265_IN_RGB_F32) { memcpy(&b, p, 4); }
    else {
        uint16_t h; memcpy(&h, p, 2);
        if (format == KS265_IN_RGB_BF16) b = (uint32_t)h << 16;
        else {
            const uint32_t s = (uint32_t)(h & 0x8000) << 16, e = h >> 10 & 31, m = h & 0x3FF;
            if (e == 31) b = s | 0x7F800000u | m << 13;
            else if (e) b = s | (e + 112) << 23 | m << 13;
            else if (!m) b = s;
            else { f = (float)m * 5.9604644775390625e-8f; memcpy(&b, &f, 4); b |= s; }   /* a denormal: m x 2^-24, a normal float32 */
        }
    }
    memcpy(&f, &b, 4);
    return f;
}
/* q of the specification: one float32 multiply, NaN and everything below zero 0, ties to even (the default rounding mode) */
static int64_t f_q(float v)
{
    volatile float t = v * 65280.0f;                                   /* (volatile: a float32 product, whatever the compiler's evaluation precision) */
    float u = t;
    if (!(u > 0.0f)) u = 0.0f;
    if (!(u < 65280.0f)) u = 65280.0f;
    return (int64_t)lrintf(u);
}
static uint8_t f_clip255(int64_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

/* float RGB -> packed I420 (tests/yuv_float_ref.py rgbf_to_i420): reads the samples of the rows and nothing else */
static void stub_float_to_i420(int format, const uint8_t *const ch[3], long long pitch, int step, int W, int H, int matrix, int full_range, uint8_t *dst)
{
    const double Kr = matrix == KS265_MATRIX_BT601 ? 0.299 : 0.2126, Kb = matrix == KS265_MATRIX_BT601 ? 0.114 : 0.0722, Kg = 1 - Kr - Kb;
    const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
    const int64_t cy[3] = {f_q16(sy * Kr), f_q16(sy * Kg), f_q16(sy * Kb)}, cb[3] = {f_q16(-sc * Kr / (2 * (1 - Kb))), f_q16(-sc * Kg / (2 * (1 - Kb))), f_q16(sc / 2)};
    const int64_t cr[3] = {f_q16(sc / 2), f_q16(-sc * Kg / (2 * (1 - Kr))), f_q16(-sc * Kb / (2 * (1 - Kr)))};
    const int64_t yoff = ((int64_t)(full_range ? 0 : 16) << 24) + (1 << 23), coff = ((int64_t)128 << 27) + (1 << 26);
    uint8_t *u = dst + (size_t)W * H, *v = u + (size_t)W * H / 4;
#define FQ(k, y, x) f_q(f_sample(ch[k] + (long long)(y) * pitch + (long long)((x) < 0 ? 0 : (x) > W - 1 ? W - 1 : (x)) * step, format))
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) dst[(size_t)y * W + x] = f_clip255((cy[0] * FQ(0, y, x) + cy[1] * FQ(1, y, x) + cy[2] * FQ(2, y, x) + yoff) >> 24);
    for (int i = 0; i < H / 2; ++i)
        for (int j = 0; j < W / 2; ++j) {
            int64_t s[3];
            for (int k = 0; k < 3; ++k) {
                s[k] = 0;
                for (int dy = 0; dy < 2; ++dy) s[k] += FQ(k, 2 * i + dy, 2 * j - 1) + 2 * FQ(k, 2 * i + dy, 2 * j) + FQ(k, 2 * i + dy, 2 * j + 1);
            }
            u[(size_t)i * (W / 2) + j] = f_clip255((cb[0] * s[0] + cb[1] * s[1] + cb[2] * s[2] + coff) >> 27);
            v[(size_t)i * (W / 2) + j] = f_clip255((cr[0] * s[0] + cr[1] * s[1] + cr[2] * s[2] + coff) >> 27);
        }
#undef FQ
}

/* the sample of byte k into p: k / 255 as float32 (an IEEE division), for the 16-bit types rounded to nearest even */
static void f_put(uint8_t *p, int format, int k)
{
    volatile float q = (float)k / 255.0f;
    const float f = q;
    uint32_t b; memcpy(&b, &f, 4);
    if (format == KS265_IN_RGB_F32) { memcpy(p, &b, 4); return; }
    uint16_t h;
    if (format == KS265_IN_RGB_BF16) h = (uint16_t)((b + 0x7FFFu + (b >> 16 & 1u)) >> 16);
    else if (!k) h = 0;
    else {                                                              /* 1 / 255 .. 1: normal float16 values, exponent 127 - 8 .. 127 */
        const uint32_t e = (b >> 23) - 112, m = b & 0x7FFFFF;
        uint32_t r = e << 10 | m >> 13;
        const uint32_t rest = m & 0x1FFF;
        if (rest > 0x1000 || (rest == 0x1000 && (r & 1))) ++r;         /* (a carry out of the mantissa raises the exponent, as it must) */
        h = (uint16_t)r;
    }
    memcpy(p, &h, 2);
}

/* packed I420 -> RGB samples (tests/yuv_output_ref.py i420_to_rgb, then tests/yuv_float_ref.py code_to_sample); format KS265_IN_RGB writes the bytes.  one: where the
 * fourth element of pixel (0, 0) lies, or NULL */
static void stub_i420_to_rgb(int format, const uint8_t *src, uint8_t *const ch[3], uint8_t *one, long long pitch, int step, int W, int H, int matrix, int full_range)
{
    const double Kr = matrix == KS265_MATRIX_BT601 ? 0.299 : 0.2126, Kb = matrix == KS265_MATRIX_BT601 ? 0.114 : 0.0722, Kg = 1 - Kr - Kb;
    const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
    const int oy = full_range ? 0 : 16, ky8 = 8 * f_q16(1 / sy), rv = f_q16(2 * (1 - Kr) / sc), gu = f_q16(-2 * Kb * (1 - Kb) / (Kg * sc)), gv = f_q16(-2 * Kr * (1 - Kr) / (Kg * sc)),
              bu = f_q16(2 * (1 - Kb) / sc);
    const int w = W / 2, h = H / 2;
    const uint8_t *pl[2] = {src + (size_t)W * H, src + (size_t)W * H + (size_t)w * h};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int c8[2];
            for (int k = 0; k < 2; ++k) {
                const int i = y >> 1, i2 = (y & 1) ? (i + 1 < h ? i + 1 : h - 1) : (i > 0 ? i - 1 : 0), j = x >> 1, j1 = j + 1 < w ? j + 1 : w - 1;
                const int v0 = 3 * pl[k][(size_t)i * w + j] + pl[k][(size_t)i2 * w + j], v1 = 3 * pl[k][(size_t)i * w + j1] + pl[k][(size_t)i2 * w + j1];
                c8[k] = ((x & 1) ? v0 + v1 : 2 * v0) - 1024;
            }
            const int y8 = (src[(size_t)y * W + x] - oy) * ky8 + (1 << 18);
            const int px[3] = {(y8 + rv * c8[1]) >> 19, (y8 + gu * c8[0] + gv * c8[1]) >> 19, (y8 + bu * c8[0]) >> 19};
            const long long o = (long long)y * pitch + (long long)x * step;
            for (int k = 0; k < 3; ++k) {
                const int code = px[k] < 0 ? 0 : px[k] > 255 ? 255 : px[k];
                if (format == KS265_IN_RGB) ch[k][o] = (uint8_t)code; else f_put(ch[k] + o, format, code);
            }
            if (one) { if (format == KS265_IN_RGB) one[o] = 255; else f_put(one + o, format, 255); }
        }
}

#ifndef KS265_STUB_FLOAT_ROUTINES_ONLY
static int f_elem_size(int format) { return format == KS265_IN_RGB_F16 || format == KS265_IN_RGB_BF16 ? 2 : format == KS265_IN_RGB_F32 ? 4 : 0; }

/* the stand-in knows no allocations: NULL and a pitch below the row are a KS265_POINTER, what the description itself shows wrong a KS265_NOTSUPPORTED, as on the device */
static int stub_float_in_check(const ks265_in_desc *d)
{
    const int es = f_elem_size(d->format);
    if (d->width <= 0 || d->height <= 0 || (d->width & 7) || (d->height & 1)) return KS265_NOTSUPPORTED;
    if (d->pixel_step < es || d->pixel_step > 64 || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601)) return KS265_NOTSUPPORTED;
    if (((uintptr_t)d->plane[0] | (uintptr_t)d->plane[1] | (uintptr_t)d->plane[2] | (uintptr_t)d->pixel_step | (uintptr_t)d->pitch[0]) & (uintptr_t)(es - 1)) return KS265_NOTSUPPORTED;
    if (d->pitch[0] < (long long)d->width * d->pixel_step) return KS265_POINTER;
    return d->plane[0] && d->plane[1] && d->plane[2] ? KS265_OK : KS265_POINTER;
}

int ks265_input_validate(ks265_ctx *c, const ks265_in_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    return f_elem_size(d->format) ? stub_float_in_check(d) : ks265_u8_input_validate(c, d);
}

int ks265_input_convert(ks265_ctx *c, const ks265_in_desc *d, uint8_t *dst)
{
    if (!c || !d || !dst) return KS265_POINTER;
    if (!f_elem_size(d->format)) return ks265_u8_input_convert(c, d, dst);
    if (LOGC(c)) return KS265_FAIL;
    const int r = stub_float_in_check(d);
    if (r) return r;
    const uint8_t *ch[3] = {(const uint8_t *)d->plane[0], (const uint8_t *)d->plane[1], (const uint8_t *)d->plane[2]};
    stub_float_to_i420(d->format, ch, d->pitch[0], d->pixel_step, d->width, d->height, d->matrix, d->full_range, dst);
    return KS265_OK;
}

#ifndef KS265_STUB_NO_SCALE
int ks265_input_scale_validate(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s)
{
    if (!c || !p || !s) return KS265_POINTER;
    if (!f_elem_size(s->format)) return ks265_u8_input_scale_validate(c, p, s);
    if (s->width != p->sw || s->height != p->sh) return KS265_NOTSUPPORTED;
    return stub_float_in_check(s);
}

/* a float source: converted into the scratch picture at its own size, and that I420 picture is scaled - as the device library does it */
int ks265_input_scale(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s, uint8_t *scratch, uint8_t *dst)
{
    if (!c || !p || !s) return KS265_POINTER;
    if (!f_elem_size(s->format)) return ks265_u8_input_scale(c, p, s, scratch, dst);
    int r = ks265_input_scale_validate(c, p, s);
    if (r) return r;
    if (!dst || !scratch) return KS265_POINTER;
    const uint8_t *ch[3] = {(const uint8_t *)s->plane[0], (const uint8_t *)s->plane[1], (const uint8_t *)s->plane[2]};
    stub_float_to_i420(s->format, ch, s->pitch[0], s->pixel_step, s->width, s->height, s->matrix, s->full_range, scratch);
    const size_t sn = (size_t)p->sw * p->sh;
    ks265_in_desc i420 = {.format = KS265_IN_I420, .width = p->sw, .height = p->sh, .plane = {scratch, scratch + sn, scratch + sn + sn / 4}, .pitch = {p->sw, p->sw / 2, p->sw / 2}};
    return ks265_u8_input_scale(c, p, &i420, NULL, dst);
}
#endif

int ks265_set_stream(ks265_ctx *c, void *hip_stream) { LOGC(c); (void)hip_stream; return c ? KS265_OK : KS265_POINTER; }

int ks265_output_validate(ks265_ctx *c, const ks265_in_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    if (d->width <= 0 || d->height <= 0 || (d->width & 1) || (d->height & 1)) return KS265_NOTSUPPORTED;
    const int es = d->format == KS265_IN_RGB ? 1 : f_elem_size(d->format);
    if (es) {
        if ((d->pixel_step != es && d->pixel_step != 3 * es && d->pixel_step != 4 * es) || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601)) return KS265_NOTSUPPORTED;
        if (((uintptr_t)d->plane[0] | (uintptr_t)d->plane[1] | (uintptr_t)d->plane[2] | (uintptr_t)d->pitch[0]) & (uintptr_t)(es - 1)) return KS265_NOTSUPPORTED;
        if (d->pitch[0] < (long long)d->width * d->pixel_step || !d->plane[0] || !d->plane[1] || !d->plane[2]) return KS265_POINTER;
        if (d->pixel_step == 4 * es) {
            const uintptr_t p0 = (uintptr_t)d->plane[0], p1 = (uintptr_t)d->plane[1], p2 = (uintptr_t)d->plane[2];
            const uintptr_t lo = p0 < p1 ? (p0 < p2 ? p0 : p2) : (p1 < p2 ? p1 : p2), hi = p0 > p1 ? (p0 > p2 ? p0 : p2) : (p1 > p2 ? p1 : p2);
            if (hi - lo > (uintptr_t)(3 * es) || p0 == p1 || p0 == p2 || p1 == p2) return KS265_NOTSUPPORTED;
        }
        return KS265_OK;
    }
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12) return KS265_NOTSUPPORTED;
    const int nplanes = d->format == KS265_IN_I420 ? 3 : 2;
    for (int k = 0; k < nplanes; ++k) {
        const int row = k == 0 || d->format == KS265_IN_NV12 ? d->width : d->width / 2;
        if (!d->plane[k] || d->pitch[k] < row) return KS265_POINTER;
    }
    return KS265_OK;
}

int ks265_output_convert(ks265_ctx *c, const uint8_t *src, const ks265_in_desc *d)
{
    LOGC(c);
    const int r = src ? ks265_output_validate(c, d) : KS265_POINTER;
    if (r) return r;
    const int W = d->width, H = d->height;
    const int es = d->format == KS265_IN_RGB ? 1 : f_elem_size(d->format);
    if (es) {
        uint8_t *ch[3] = {(uint8_t *)d->plane[0], (uint8_t *)d->plane[1], (uint8_t *)d->plane[2]}, *one = NULL;
        if (d->pixel_step == 4 * es) {                                  /* the element of the pixel (it begins at the lowest channel) that no channel names */
            uint8_t *lo = ch[0] < ch[1] ? (ch[0] < ch[2] ? ch[0] : ch[2]) : (ch[1] < ch[2] ? ch[1] : ch[2]);
            for (int k = 1; k < 4 && !one; ++k) if (lo + k * es != ch[0] && lo + k * es != ch[1] && lo + k * es != ch[2]) one = lo + k * es;
        }
        stub_i420_to_rgb(d->format, src, ch, one, d->pitch[0], d->pixel_step, W, H, d->matrix, d->full_range);
        return KS265_OK;
    }
    const uint8_t *u = src + (size_t)W * H, *v = u + (size_t)W * H / 4;
    for (int y = 0; y < H; ++y) memcpy((uint8_t *)d->plane[0] + (size_t)y * d->pitch[0], src + (size_t)y * W, (size_t)W);
    for (int y = 0; y < H / 2; ++y) {
        if (d->format == KS265_IN_I420) {
            memcpy((uint8_t *)d->plane[1] + (size_t)y * d->pitch[1], u + (size_t)y * (W / 2), (size_t)W / 2);
            memcpy((uint8_t *)d->plane[2] + (size_t)y * d->pitch[2], v + (size_t)y * (W / 2), (size_t)W / 2);
        } else {
            uint8_t *uv = (uint8_t *)d->plane[1] + (size_t)y * d->pitch[1];
            for (int x = 0; x < W / 2; ++x) { uv[2 * x] = u[(size_t)y * (W / 2) + x]; uv[2 * x + 1] = v[(size_t)y * (W / 2) + x]; }
        }
    }
    return KS265_OK;
}
#endif
