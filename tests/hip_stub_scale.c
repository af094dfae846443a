/* TEST INFRASTRUCTURE: the device library's CPU stand-in with the ROI entries (hip_stub_roi.c, which includes hip_stub.c as it is) plus what device input and
 * ks265_enc_enable_device_scale (include/ks265_enc.h) ask of a device library, in plain C after the specifications: ks265_input_validate / ks265_input_convert (I420 and NV12
 * repacked, RGB after tests/yuv_convert_ref.py) and ks265_scale_plan_create / _destroy / ks265_input_scale_validate / ks265_input_scale after tests/yuv_scale_ref.py, with the
 * tables of ../ks265codec_amd/host/ks265_scale.h.  "Device memory" is the process's own.  A plan counts as device memory alive (ks265_stub_live), its creation is a creating
 * call; ks265_input_convert and ks265_input_scale show in the call log.  The host tests of the switch link this file instead of hip_stub.c
 * (with -DKS265_STUB_NO_SCALE: device input alone, no scaler). */
#include "hip_stub_roi.c"
#include "../ks265codec_amd/host/ks265_scale.h"

struct ks265_scale_plan { int sw, sh, dw, dh, filter, T[4]; int32_t *first[4]; int16_t *coef[4]; };

static int stub_in_check(const ks265_in_desc *d)
{
    if (d->width <= 0 || d->height <= 0 || (d->width & 7) || (d->height & 1)) return KS265_NOTSUPPORTED;
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12 && d->format != KS265_IN_RGB) return KS265_NOTSUPPORTED;
    if (d->format == KS265_IN_RGB && (d->pixel_step < 1 || d->pixel_step > 16 || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601))) return KS265_NOTSUPPORTED;
    const int np = d->format == KS265_IN_NV12 ? 2 : 3;
    for (int k = 0; k < np; ++k) {
        const long long row = d->format == KS265_IN_RGB ? (long long)d->width * d->pixel_step : (k == 0 || d->format == KS265_IN_NV12) ? d->width : d->width / 2;
        if (!d->plane[k] || d->pitch[d->format == KS265_IN_RGB ? 0 : k] < row) return KS265_POINTER;
    }
    return KS265_OK;
}
int ks265_input_validate(ks265_ctx *c, const ks265_in_desc *d) { return c && d ? stub_in_check(d) : KS265_POINTER; }

static int q16(double x) { return (int)floor(x * 65536 + 0.5); }
static uint8_t clip255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

int ks265_input_convert(ks265_ctx *c, const ks265_in_desc *d, uint8_t *dst)
{
    if (LOGC(c)) return KS265_FAIL;
    if (!c || !d || !dst) return KS265_POINTER;
    const int r = stub_in_check(d);
    if (r) return r;
    const int W = d->width, H = d->height;
    uint8_t *u = dst + (size_t)W * H, *v = u + (size_t)W * H / 4;
    const uint8_t *p0 = (const uint8_t *)d->plane[0], *p1 = (const uint8_t *)d->plane[1], *p2 = (const uint8_t *)d->plane[2];
    if (d->format != KS265_IN_RGB) {
        for (int y = 0; y < H; ++y) memcpy(dst + (size_t)y * W, p0 + (size_t)y * d->pitch[0], (size_t)W);
        for (int y = 0; y < H / 2; ++y)
            for (int x = 0; x < W / 2; ++x) {
                u[(size_t)y * (W / 2) + x] = d->format == KS265_IN_NV12 ? p1[(size_t)y * d->pitch[1] + 2 * x] : p1[(size_t)y * d->pitch[1] + x];
                v[(size_t)y * (W / 2) + x] = d->format == KS265_IN_NV12 ? p1[(size_t)y * d->pitch[1] + 2 * x + 1] : p2[(size_t)y * d->pitch[2] + x];
            }
        return KS265_OK;
    }
    const double Kr = d->matrix == KS265_MATRIX_BT601 ? 0.299 : 0.2126, Kb = d->matrix == KS265_MATRIX_BT601 ? 0.114 : 0.0722, Kg = 1 - Kr - Kb;
    const double sy = d->full_range ? 1.0 : 219.0 / 255.0, sc = d->full_range ? 1.0 : 224.0 / 255.0;
    const int cy[3] = {q16(sy * Kr), q16(sy * Kg), q16(sy * Kb)}, cb[3] = {q16(-sc * Kr / (2 * (1 - Kb))), q16(-sc * Kg / (2 * (1 - Kb))), q16(sc / 2)};
    const int cr[3] = {q16(sc / 2), q16(-sc * Kg / (2 * (1 - Kr))), q16(-sc * Kb / (2 * (1 - Kr)))}, yoff = ((d->full_range ? 0 : 16) << 16) + 32768;
    const uint8_t *ch[3] = {p0, p1, p2};
#define PX(k, y, x) ((int)ch[k][(size_t)(y) * d->pitch[0] + (size_t)((x) < 0 ? 0 : (x) > W - 1 ? W - 1 : (x)) * d->pixel_step])
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) dst[(size_t)y * W + x] = clip255((cy[0] * PX(0, y, x) + cy[1] * PX(1, y, x) + cy[2] * PX(2, y, x) + yoff) >> 16);
    for (int i = 0; i < H / 2; ++i)
        for (int j = 0; j < W / 2; ++j) {
            int s[3];
            for (int k = 0; k < 3; ++k) {
                s[k] = 0;
                for (int dy = 0; dy < 2; ++dy) s[k] += PX(k, 2 * i + dy, 2 * j - 1) + 2 * PX(k, 2 * i + dy, 2 * j) + PX(k, 2 * i + dy, 2 * j + 1);
            }
            const int rnd = (128 << 19) + (1 << 18);
            u[(size_t)i * (W / 2) + j] = clip255((cb[0] * s[0] + cb[1] * s[1] + cb[2] * s[2] + rnd) >> 19);
            v[(size_t)i * (W / 2) + j] = clip255((cr[0] * s[0] + cr[1] * s[1] + cr[2] * s[2] + rnd) >> 19);
        }
#undef PX
    return KS265_OK;
}

#ifndef KS265_STUB_NO_SCALE                                            /* -DKS265_STUB_NO_SCALE: a device library with device input and without the scaler */
int ks265_scale_plan_destroy(ks265_ctx *c, ks265_scale_plan *p)
{
    if (!c) return KS265_POINTER;
    if (!p) return KS265_OK;
    for (int k = 0; k < 4; ++k) { free(p->first[k]); free(p->coef[k]); }
    free(p); live(LIVE_DEV, -1);
    return KS265_OK;
}

int ks265_scale_plan_create(ks265_ctx *c, int sw, int sh, int dw, int dh, int filter, ks265_scale_plan **out)
{
    if (!c || !out) return KS265_POINTER;
    *out = NULL;
    if (!ks265_scale_size_ok(sw, sh, dw, dh) || (filter != KS_SCALE_TRIANGLE && filter != KS_SCALE_CATMULL_ROM)) return KS265_NOTSUPPORTED;
    if (creating_fails("scale_plan c%d %dx%d -> %dx%d filter %d", ctx_ordinal(c), sw, sh, dw, dh, filter)) return KS265_OUTOFMEMORY;
    ks265_scale_plan *p = (ks265_scale_plan *)calloc(1, sizeof *p);
    if (!p) return KS265_OUTOFMEMORY;
    live(LIVE_DEV, 1);
    p->sw = sw; p->sh = sh; p->dw = dw; p->dh = dh; p->filter = filter;
    int S[4], D[4], cos[4];
    ks265_scale_axes(sw, sh, dw, dh, S, D, cos);
    for (int k = 0; k < 4; ++k) {
        p->T[k] = ks265_scale_axis_taps(S[k], D[k], filter, cos[k]);
        p->first[k] = (int32_t *)malloc((size_t)D[k] * sizeof(int32_t));
        p->coef[k] = (int16_t *)malloc((size_t)D[k] * (size_t)(p->T[k] ? p->T[k] : 1) * sizeof(int16_t));
        if (!p->T[k] || !p->first[k] || !p->coef[k] || ks265_scale_axis_fill(S[k], D[k], filter, cos[k], p->T[k], p->first[k], p->coef[k])) { (void)ks265_scale_plan_destroy(c, p); return KS265_NOTSUPPORTED; }
    }
    *out = p;
    return KS265_OK;
}

int ks265_input_scale_validate(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s)
{
    if (!c || !p || !s) return KS265_POINTER;
    if (s->width != p->sw || s->height != p->sh) return KS265_NOTSUPPORTED;
    return stub_in_check(s);
}

int ks265_input_scale(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s, uint8_t *scratch, uint8_t *dst)
{
    int r = ks265_input_scale_validate(c, p, s);
    if (r) return r;
    if (!dst || (s->format == KS265_IN_RGB && !scratch)) return KS265_POINTER;
    const size_t sn = (size_t)p->sw * p->sh, dn = (size_t)p->dw * p->dh;
    const uint8_t *src[3] = {(const uint8_t *)s->plane[0], (const uint8_t *)s->plane[1], (const uint8_t *)s->plane[2]};
    long long pitch[3] = {s->pitch[0], s->pitch[1], s->pitch[2]};
    int step[3] = {1, 1, 1};
    if (s->format == KS265_IN_RGB) {
        if ((r = ks265_input_convert(c, s, scratch))) return r;
        src[0] = scratch; src[1] = scratch + sn; src[2] = scratch + sn + sn / 4;
        pitch[0] = p->sw; pitch[1] = pitch[2] = p->sw / 2;
    } else if (s->format == KS265_IN_NV12) { src[2] = src[1] + 1; pitch[2] = pitch[1]; step[1] = step[2] = 2; }
    if (LOGC(c)) return KS265_FAIL;
    int16_t *tmp = (int16_t *)malloc((size_t)p->sh * p->dw * sizeof(int16_t));
    if (!tmp) return KS265_OUTOFMEMORY;
    for (int k = 0; k < 3; ++k) {
        const int a = k ? 2 : 0;
        ks265_scale_plane_host(src[k], pitch[k], step[k], k ? p->sw / 2 : p->sw, k ? p->sh / 2 : p->sh, dst + (k == 0 ? 0 : k == 1 ? dn : dn + dn / 4), k ? p->dw / 2 : p->dw, k ? p->dh / 2 : p->dh,
                               p->first[a], p->coef[a], p->T[a], p->first[a + 1], p->coef[a + 1], p->T[a + 1], tmp);
    }
    free(tmp);
    return KS265_OK;
}
#endif
