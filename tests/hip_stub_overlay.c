/* TEST INFRASTRUCTURE: the device library's CPU stand-in with everything hip_stub_hdr.c has (included as it is) plus the two entries of the overlay stage
 * (include/ks265_hip.h: ks265_input_overlay[_validate]), in plain C after tests/overlay_ref.py.  "Device memory" is the process's own, so no extent can be judged: pointers
 * are refused for NULL and a pitch below the row alone.  Every ks265_input_overlay call is logged like the others (arg: the number of overlays) and kept - sizes, window and
 * per overlay its place, opacity and format - for ks265_stub_overlay_calls; ks265_stub_overlay_dump makes every call append the slot it leaves behind to a file. */
#include "hip_stub_hdr.c"

typedef struct { int32_t w, h, win_w, win_h, n, ow[8], oh[8], x[8], y[8], opacity[8], format[8]; } StubOvCall;
static pthread_mutex_t g_ov_mu = PTHREAD_MUTEX_INITIALIZER;
static StubOvCall g_ov[1024]; static int g_nov;
/* the calls so far (at most cap of them, oldest first) into out; returns how many there were.  ks265_stub_overlay_reset forgets them */
int ks265_stub_overlay_calls(StubOvCall *out, int cap)
{
    pthread_mutex_lock(&g_ov_mu);
    const int n = g_nov;
    for (int i = 0; i < n && i < cap && i < 1024; ++i) out[i] = g_ov[i];
    pthread_mutex_unlock(&g_ov_mu);
    return n;
}
void ks265_stub_overlay_reset(void) { pthread_mutex_lock(&g_ov_mu); g_nov = 0; pthread_mutex_unlock(&g_ov_mu); }
/* from now on every call appends the picture it leaves behind - the input slot as the encoder will read it, W x H x 3 / 2 bytes - to the file at `path` (NULL: no more) */
static char g_ov_dump[1024];
void ks265_stub_overlay_dump(const char *path) { pthread_mutex_lock(&g_ov_mu); snprintf(g_ov_dump, sizeof g_ov_dump, "%s", path ? path : ""); pthread_mutex_unlock(&g_ov_mu); }

static int ov_elem_size(int format) { return format == KS265_IN_RGB ? 1 : f_elem_size(format); }

int ks265_input_overlay_validate(ks265_ctx *c, const ks265_overlay_desc *ov, int n, int W, int H, int win_w, int win_h)
{
    if (!c || !ov) return KS265_POINTER;
    if (n < 1 || n > KS265_OVERLAY_MAX) return KS265_NOTSUPPORTED;
    if (W <= 0 || H <= 0 || (W & 7) || (H & 7) || W > 8192 || H > 8192 || win_w < 2 || win_h < 2 || ((win_w | win_h) & 1) || win_w > W || win_h > H) return KS265_NOTSUPPORTED;
    for (int k = 0; k < n; ++k) {
        const ks265_in_desc *d = &ov[k].rgb;
        const int es = ov_elem_size(d->format);
        if (!es) return KS265_NOTSUPPORTED;
        if (d->width < 2 || d->height < 2 || ((d->width | d->height | ov[k].x | ov[k].y) & 1) || d->width > 8192 || d->height > 8192) return KS265_NOTSUPPORTED;
        if (ov[k].x < -16384 || ov[k].x > 16384 || ov[k].y < -16384 || ov[k].y > 16384 || ov[k].opacity < 0 || ov[k].opacity > 256) return KS265_NOTSUPPORTED;
        if (d->pixel_step < es || d->pixel_step > (es == 1 ? 16 : 64) || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601)) return KS265_NOTSUPPORTED;
        if (((uintptr_t)d->plane[0] | (uintptr_t)d->plane[1] | (uintptr_t)d->plane[2] | (uintptr_t)ov[k].alpha | (uintptr_t)d->pixel_step | (uintptr_t)d->pitch[0]) & (uintptr_t)(es - 1)) return KS265_NOTSUPPORTED;
        if (d->pitch[0] < (long long)d->width * d->pixel_step || !d->plane[0] || !d->plane[1] || !d->plane[2]) return KS265_POINTER;
    }
    return KS265_OK;
}

/* the 8-bit code of the sample at p */
static int64_t ov_code(const uint8_t *p, int format) { return format == KS265_IN_RGB ? *p : (f_q(f_sample(p, format)) + 128) >> 8; }
static int64_t ov_floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return a % b < 0 ? q - 1 : q; }

static void stub_overlay_one(const ks265_overlay_desc *o, int W, int H, int win_w, int win_h, uint8_t *pic)
{
    const ks265_in_desc *d = &o->rgb;
    const int w = d->width, h = d->height, fmt = d->format, x0 = o->x, y0 = o->y;
    const double Kr = d->matrix == KS265_MATRIX_BT601 ? 0.299 : 0.2126, Kb = d->matrix == KS265_MATRIX_BT601 ? 0.114 : 0.0722, Kg = 1 - Kr - Kb;
    const double sy = d->full_range ? 1.0 : 219.0 / 255.0, sc = d->full_range ? 1.0 : 224.0 / 255.0;
    const int64_t cy[3] = {f_q16(sy * Kr), f_q16(sy * Kg), f_q16(sy * Kb)}, cb[3] = {f_q16(-sc * Kr / (2 * (1 - Kb))), f_q16(-sc * Kg / (2 * (1 - Kb))), f_q16(sc / 2)};
    const int64_t cr[3] = {f_q16(sc / 2), f_q16(-sc * Kg / (2 * (1 - Kr))), f_q16(-sc * Kb / (2 * (1 - Kr)))};
    const int64_t oy = d->full_range ? 0 : 16, D = (int64_t)2040 * 65536;
    uint8_t *U = pic + (size_t)W * H, *V = U + (size_t)W * H / 4;
#define OVS(p, r, c) ov_code((const uint8_t *)(p) + (long long)(r) * d->pitch[0] + (long long)((c) < 0 ? 0 : (c) > w - 1 ? w - 1 : (c)) * d->pixel_step, fmt)
#define OVA(r, c) (((o->alpha ? OVS(o->alpha, r, c) : 255) * o->opacity + 128) >> 8)
    for (int r = 0; r < h; ++r) {
        const int py = y0 + r;
        if (py < 0 || py >= win_h) continue;
        for (int cc = 0; cc < w; ++cc) {
            const int px = x0 + cc;
            if (px < 0 || px >= win_w) continue;
            const int64_t A = OVA(r, cc), lum = cy[0] * OVS(d->plane[0], r, cc) + cy[1] * OVS(d->plane[1], r, cc) + cy[2] * OVS(d->plane[2], r, cc) + (oy << 16);
            uint8_t *y = pic + (size_t)py * W + px;
            *y = f_clip255(ov_floor_div((int64_t)*y * (255 - A) * 65536 + A * lum + 255 * 32768, (int64_t)255 * 65536));
        }
    }
    for (int i = 0; i < h / 2; ++i) {
        const int py = y0 / 2 + i;                                      /* (y0 even: exact) */
        if (2 * py < 0 || 2 * py >= win_h) continue;
        for (int j = 0; j < w / 2; ++j) {
            const int px = x0 / 2 + j;
            if (2 * px < 0 || 2 * px >= win_w) continue;
            int64_t sa = 0, s[3] = {0, 0, 0};
            for (int dy = 0; dy < 2; ++dy)
                for (int t = -1; t <= 1; ++t) {
                    const int64_t A = (t ? 1 : 2) * OVA(2 * i + dy, 2 * j + t);
                    sa += A;
                    for (int k = 0; k < 3; ++k) s[k] += A * OVS(d->plane[k], 2 * i + dy, 2 * j + t);
                }
            const size_t at = (size_t)py * (W / 2) + px;
            const int64_t keep = (2040 - sa) * 65536, mid = (int64_t)128 * 65536 * sa + D / 2;
            U[at] = f_clip255(ov_floor_div(U[at] * keep + cb[0] * s[0] + cb[1] * s[1] + cb[2] * s[2] + mid, D));
            V[at] = f_clip255(ov_floor_div(V[at] * keep + cr[0] * s[0] + cr[1] * s[1] + cr[2] * s[2] + mid, D));
        }
    }
#undef OVA
#undef OVS
}

int ks265_input_overlay(ks265_ctx *c, const ks265_overlay_desc *ov, int n, int W, int H, int win_w, int win_h, uint8_t *pic)
{
    const int r = ks265_input_overlay_validate(c, ov, n, W, H, win_w, win_h);
    if (r) return r;
    if (!pic) return KS265_POINTER;
    if ((uintptr_t)pic & 15) return KS265_NOTSUPPORTED;
    if (call_log(__func__, c, NULL, NULL, n)) return KS265_FAIL;
    pthread_mutex_lock(&g_ov_mu);
    if (g_nov < 1024) {
        StubOvCall *k = &g_ov[g_nov];
        memset(k, 0, sizeof *k);
        k->w = W; k->h = H; k->win_w = win_w; k->win_h = win_h; k->n = n;
        for (int i = 0; i < n; ++i) { k->ow[i] = ov[i].rgb.width; k->oh[i] = ov[i].rgb.height; k->x[i] = ov[i].x; k->y[i] = ov[i].y; k->opacity[i] = ov[i].opacity; k->format[i] = ov[i].rgb.format; }
    }
    ++g_nov;
    pthread_mutex_unlock(&g_ov_mu);
    for (int k = 0; k < n; ++k) stub_overlay_one(&ov[k], W, H, win_w, win_h, pic);
    pthread_mutex_lock(&g_ov_mu);
    int bad = 0;
    if (g_ov_dump[0]) {
        FILE *f = fopen(g_ov_dump, "ab");
        bad = !f || fwrite(pic, 1, (size_t)W * H * 3 / 2, f) != (size_t)W * H * 3 / 2;
        if (f) fclose(f);
    }
    pthread_mutex_unlock(&g_ov_mu);
    return bad ? KS265_FAIL : KS265_OK;
}
