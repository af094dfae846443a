/* TEST INFRASTRUCTURE: the device library's CPU stand-in with device input, the scaler and the float formats (hip_stub_float.c, included as it is, its picture entries under
 * other symbols) plus the YUV family KS265_IN_YUV(layout, sub, depth, msb) (include/ks265_hip.h) in ks265_input_validate / ks265_input_convert / ks265_input_scale, in plain C
 * after tests/yuv_hibit_ref.py.  "Device memory" is the process's own.  Every other format goes to the entries of hip_stub_float.c; KS265_IN_YUV(0 / 1, 0, 8, 0) go there as
 * KS265_IN_I420 / _NV12.  The conversion routine, stub_yuv_to_i420, takes nothing but pointers and numbers: -DKS265_STUB_YUV_ROUTINES_ONLY leaves it alone in the translation
 * unit, for a program of its own. */
#ifndef KS265_STUB_YUV_ROUTINES_ONLY
/* hip_stub_float.c renames the entries of the file IT includes with macros and takes them back, so macros cannot rename its own: its four picture entries get other SYMBOLS
 * instead (the identifiers stay, and its own calls among them still reach them), and this file's entries, defined under other identifiers, carry the public symbols */
#include "ks265_hip.h"
int ks265_input_validate(ks265_ctx *, const ks265_in_desc *) __asm__("ks265_f_input_validate");
int ks265_input_convert(ks265_ctx *, const ks265_in_desc *, uint8_t *) __asm__("ks265_f_input_convert");
int ks265_input_scale_validate(ks265_ctx *, const ks265_scale_plan *, const ks265_in_desc *) __asm__("ks265_f_input_scale_validate");
int ks265_input_scale(ks265_ctx *, const ks265_scale_plan *, const ks265_in_desc *, uint8_t *, uint8_t *) __asm__("ks265_f_input_scale");
#include "hip_stub_float.c"
#define ks265_f_input_validate ks265_input_validate
#define ks265_f_input_convert ks265_input_convert
#define ks265_f_input_scale_validate ks265_input_scale_validate
#define ks265_f_input_scale ks265_input_scale
int ks265_y_input_validate(ks265_ctx *, const ks265_in_desc *) __asm__("ks265_input_validate");
int ks265_y_input_convert(ks265_ctx *, const ks265_in_desc *, uint8_t *) __asm__("ks265_input_convert");
int ks265_y_input_scale_validate(ks265_ctx *, const ks265_scale_plan *, const ks265_in_desc *) __asm__("ks265_input_scale_validate");
int ks265_y_input_scale(ks265_ctx *, const ks265_scale_plan *, const ks265_in_desc *, uint8_t *, uint8_t *) __asm__("ks265_input_scale");
#else
#include <stdint.h>
#include <string.h>
#include "ks265_hip.h"
#endif

/* the sample of the element at p */
static int y_sample(const uint8_t *p, int depth, int msb)
{
    if (depth == 8) return *p;
    const int w = p[0] | p[1] << 8;
    return msb ? w >> (16 - depth) : w & ((1 << depth) - 1);
}
static uint8_t y_round(int v, int sh) { if (sh) v = (v + (1 << (sh - 1))) >> sh; return (uint8_t)(v > 255 ? 255 : v); }

/* a picture of the family -> packed I420 (tests/yuv_hibit_ref.py to_i420): reads the elements of the rows and nothing else */
static void stub_yuv_to_i420(int layout, int sub, int depth, int msb, const uint8_t *const plane[3], const long long pitch[3], int W, int H, uint8_t *dst)
{
    const int es = depth == 8 ? 1 : 2, s = depth - 8;
    /* where Y, U, V of luma column x / chroma column x lie in their row: base plane, byte offset of column 0, bytes between columns */
    const uint8_t *yb = plane[0], *ub, *vb;
    long long yp = pitch[0], up, vp;
    int y0 = 0, ys = es, u0, v0, cs;
    if (layout == 0) { ub = plane[1]; vb = plane[2]; up = pitch[1]; vp = pitch[2]; u0 = v0 = 0; cs = es; }
    else if (layout == 1) { ub = vb = plane[1]; up = vp = pitch[1]; u0 = 0; v0 = es; cs = 2 * es; }
    else { ub = vb = plane[0]; up = vp = pitch[0]; ys = 2 * es; cs = 4 * es; y0 = layout == 2 ? 0 : es; u0 = layout == 2 ? es : 0; v0 = layout == 2 ? 3 * es : 2 * es; }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) dst[(size_t)y * W + x] = y_round(y_sample(yb + y * yp + y0 + (long long)x * ys, depth, msb), s);
    uint8_t *u = dst + (size_t)W * H, *v = u + (size_t)W * H / 4;
#define YC(base, pit, off, x, y) y_sample((base) + (long long)(y) * (pit) + (off) + (long long)(x) * cs, depth, msb)
    for (int j = 0; j < H / 2; ++j)
        for (int i = 0; i < W / 2; ++i) {
            int su, sv, t;
            if (sub == 0) { su = YC(ub, up, u0, i, j); sv = YC(vb, vp, v0, i, j); t = 0; }
            else if (sub == 1) { su = YC(ub, up, u0, i, 2 * j) + YC(ub, up, u0, i, 2 * j + 1); sv = YC(vb, vp, v0, i, 2 * j) + YC(vb, vp, v0, i, 2 * j + 1); t = 1; }
            else {
                const int xl = 2 * i > 0 ? 2 * i - 1 : 0;
                su = sv = 0; t = 3;
                for (int dy = 0; dy < 2; ++dy) {
                    su += YC(ub, up, u0, xl, 2 * j + dy) + 2 * YC(ub, up, u0, 2 * i, 2 * j + dy) + YC(ub, up, u0, 2 * i + 1, 2 * j + dy);
                    sv += YC(vb, vp, v0, xl, 2 * j + dy) + 2 * YC(vb, vp, v0, 2 * i, 2 * j + dy) + YC(vb, vp, v0, 2 * i + 1, 2 * j + dy);
                }
            }
            u[(size_t)j * (W / 2) + i] = y_round(su, s + t);
            v[(size_t)j * (W / 2) + i] = y_round(sv, s + t);
        }
#undef YC
}

#ifndef KS265_STUB_YUV_ROUTINES_ONLY
/* the fields of a code: 1 valid, 0 no code of the family (below 0x1000), -1 refused */
static int y_decode(int format, int *layout, int *sub, int *depth, int *msb)
{
    if (!(format & ~0xFFF)) return 0;
    if ((format & ~0x3FF) != 0x1000) return -1;
    *layout = format >> 8 & 3; *sub = format >> 6 & 3; *msb = format >> 5 & 1; *depth = format & 31;
    if (*depth < 8 || *depth > 16 || *sub > 2 || (*depth == 8 && *msb) || (*layout >= 2 && *sub != 1)) return -1;
    return 1;
}

/* the stand-in knows no allocations: NULL and a pitch below the row are a KS265_POINTER, what the description itself shows wrong a KS265_NOTSUPPORTED, as on the device */
static int stub_yuv_in_check(const ks265_in_desc *d, int layout, int sub, int depth)
{
    if (d->width <= 0 || d->height <= 0 || (d->width & 7) || (d->height & 1)) return KS265_NOTSUPPORTED;
    const int es = depth == 8 ? 1 : 2, np = layout == 0 ? 3 : layout == 1 ? 2 : 1;
    const long long W = d->width, cw = sub == 2 ? W : W / 2;
    for (int k = 0; k < np && es == 2; ++k) if (((uintptr_t)d->plane[k] | (uintptr_t)d->pitch[k]) & 1) return KS265_NOTSUPPORTED;
    for (int k = 0; k < np; ++k) {
        const long long row = layout >= 2 ? 2 * W * es : k == 0 ? W * es : layout == 1 ? 2 * cw * es : cw * es;
        if (!d->plane[k] || d->pitch[k] < row) return KS265_POINTER;
    }
    return KS265_OK;
}

/* 0: not the family's (d as it is, or under its other name in *loc), 1: the family's, judged in *r */
static int y_route(const ks265_in_desc **d, ks265_in_desc *loc, int f[4], int *r)
{
    const int fam = y_decode((*d)->format, &f[0], &f[1], &f[2], &f[3]);
    if (fam < 0) { *r = KS265_NOTSUPPORTED; return 1; }
    if (!fam) return 0;
    if (f[2] == 8 && f[1] == 0 && f[0] < 2) { *loc = **d; loc->format = f[0] ? KS265_IN_NV12 : KS265_IN_I420; *d = loc; return 0; }
    *r = stub_yuv_in_check(*d, f[0], f[1], f[2]);
    return 1;
}

static void y_convert(const ks265_in_desc *d, const int f[4], uint8_t *dst)
{
    const uint8_t *pl[3] = {(const uint8_t *)d->plane[0], (const uint8_t *)d->plane[1], (const uint8_t *)d->plane[2]};
    const long long pitch[3] = {d->pitch[0], d->pitch[1], d->pitch[2]};
    stub_yuv_to_i420(f[0], f[1], f[2], f[3], pl, pitch, d->width, d->height, dst);
}

int ks265_y_input_validate(ks265_ctx *c, const ks265_in_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    ks265_in_desc loc; int f[4], r;
    return y_route(&d, &loc, f, &r) ? r : ks265_f_input_validate(c, d);
}

int ks265_y_input_convert(ks265_ctx *c, const ks265_in_desc *d, uint8_t *dst)
{
    if (!c || !d || !dst) return KS265_POINTER;
    ks265_in_desc loc; int f[4], r;
    if (!y_route(&d, &loc, f, &r)) return ks265_f_input_convert(c, d, dst);
    if (call_log("ks265_input_convert", c, NULL, NULL, 0)) return KS265_FAIL;                /* (LOGC would write this function's identifier) */
    if (r) return r;
    y_convert(d, f, dst);
    return KS265_OK;
}

#ifndef KS265_STUB_NO_SCALE
int ks265_y_input_scale_validate(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s)
{
    if (!c || !p || !s) return KS265_POINTER;
    ks265_in_desc loc; int f[4], r;
    if (!y_route(&s, &loc, f, &r)) return ks265_f_input_scale_validate(c, p, s);
    if (s->width != p->sw || s->height != p->sh) return KS265_NOTSUPPORTED;
    return r;
}

/* a source of the family: converted into the scratch picture at its own size, and that I420 picture is scaled - as the device library does it */
int ks265_y_input_scale(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s, uint8_t *scratch, uint8_t *dst)
{
    if (!c || !p || !s) return KS265_POINTER;
    ks265_in_desc loc; int f[4], r;
    if (!y_route(&s, &loc, f, &r)) return ks265_f_input_scale(c, p, s, scratch, dst);
    if (s->width != p->sw || s->height != p->sh) return KS265_NOTSUPPORTED;
    if (r) return r;
    if (!dst || !scratch) return KS265_POINTER;
    y_convert(s, f, scratch);
    const size_t sn = (size_t)p->sw * p->sh;
    ks265_in_desc i420 = {.format = KS265_IN_I420, .width = p->sw, .height = p->sh, .plane = {scratch, scratch + sn, scratch + sn + sn / 4}, .pitch = {p->sw, p->sw / 2, p->sw / 2}};
    return ks265_f_input_scale(c, p, &i420, NULL, dst);
}
#endif
#endif
