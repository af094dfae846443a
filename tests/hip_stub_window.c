/* TEST INFRASTRUCTURE: the device library's CPU stand-in with everything hip_stub_yuv.c has (included as it is) plus the three entries of picture sizes that are no multiple of 8
 * (include/ks265_hip.h: ks265_input_pad[_validate], ks265_output_crop, ks265_sse_window), in plain C after tests/picture_window_ref.py.  "Device memory" is the process's own.
 * Every ks265_input_pad call is kept - source size, coded size, format, pitches - for ks265_stub_pad_calls; the stand-in's SSE is a constant per picture, so ks265_sse_window
 * only shows in the call log. */
#include "hip_stub_yuv.c"

typedef struct { int32_t format, w, h, cw, ch, pitch[3]; } StubPadCall;
static pthread_mutex_t g_pad_mu = PTHREAD_MUTEX_INITIALIZER;
static StubPadCall g_pad[4096]; static int g_npad;
/* the calls so far (at most cap of them, oldest first) into out; returns how many there were.  ks265_stub_pad_reset forgets them */
int ks265_stub_pad_calls(StubPadCall *out, int cap)
{
    pthread_mutex_lock(&g_pad_mu);
    const int n = g_npad;
    for (int i = 0; i < n && i < cap && i < 4096; ++i) out[i] = g_pad[i];
    pthread_mutex_unlock(&g_pad_mu);
    return n;
}
void ks265_stub_pad_reset(void) { pthread_mutex_lock(&g_pad_mu); g_npad = 0; pthread_mutex_unlock(&g_pad_mu); }

static int window_sizes_ok(int w, int h, int cw, int ch)
{
    return w > 0 && h > 0 && !(w & 1) && !(h & 1) && !(cw & 7) && !(ch & 7) && cw >= w && cw < w + 8 && ch >= h && ch < h + 8;
}

int ks265_input_pad_validate(ks265_ctx *c, const ks265_in_desc *d, int cw, int ch)
{
    if (!c || !d) return KS265_POINTER;
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12) return KS265_NOTSUPPORTED;
    if (!window_sizes_ok(d->width, d->height, cw, ch)) return KS265_NOTSUPPORTED;
    const int nv12 = d->format == KS265_IN_NV12;
    if (d->pitch[0] < d->width || d->pitch[1] < (nv12 ? d->width : d->width / 2) || (!nv12 && d->pitch[2] < d->width / 2)) return KS265_NOTSUPPORTED;
    if (!d->plane[0] || !d->plane[1] || (!nv12 && !d->plane[2])) return KS265_POINTER;
    return KS265_OK;
}

/* np.pad(..., mode="edge") per plane: column and row clamped to the source's last */
static void stub_pad_plane(const uint8_t *src, long long pitch, int step, int w, int h, int cw, int ch, uint8_t *dst)
{
    for (int y = 0; y < ch; ++y) {
        const uint8_t *row = src + (long long)(y < h ? y : h - 1) * pitch;
        for (int x = 0; x < cw; ++x) dst[(size_t)y * cw + x] = row[(size_t)(x < w ? x : w - 1) * step];
    }
}

int ks265_input_pad(ks265_ctx *c, const ks265_in_desc *d, int cw, int ch, uint8_t *dst)
{
    const int r = ks265_input_pad_validate(c, d, cw, ch);
    if (r) return r;
    if (!dst) return KS265_POINTER;
    if (call_log(__func__, c, NULL, NULL, d->format)) return KS265_FAIL;
    pthread_mutex_lock(&g_pad_mu);
    if (g_npad < 4096) g_pad[g_npad] = (StubPadCall){d->format, d->width, d->height, cw, ch, {d->pitch[0], d->pitch[1], d->pitch[2]}};
    ++g_npad;
    pthread_mutex_unlock(&g_pad_mu);
    const int w = d->width, h = d->height;
    const size_t npx = (size_t)cw * ch;
    stub_pad_plane((const uint8_t *)d->plane[0], d->pitch[0], 1, w, h, cw, ch, dst);
    if (d->format == KS265_IN_NV12) {
        stub_pad_plane((const uint8_t *)d->plane[1], d->pitch[1], 2, w / 2, h / 2, cw / 2, ch / 2, dst + npx);
        stub_pad_plane((const uint8_t *)d->plane[1] + 1, d->pitch[1], 2, w / 2, h / 2, cw / 2, ch / 2, dst + npx + npx / 4);
    } else {
        stub_pad_plane((const uint8_t *)d->plane[1], d->pitch[1], 1, w / 2, h / 2, cw / 2, ch / 2, dst + npx);
        stub_pad_plane((const uint8_t *)d->plane[2], d->pitch[2], 1, w / 2, h / 2, cw / 2, ch / 2, dst + npx + npx / 4);
    }
    return KS265_OK;
}

int ks265_output_crop(ks265_ctx *c, const uint8_t *src, int cw, int ch, int w, int h, uint8_t *dst)
{
    if (!c || !src || !dst) return KS265_POINTER;
    if (!window_sizes_ok(w, h, cw, ch)) return KS265_NOTSUPPORTED;
    call_log(__func__, c, NULL, NULL, 0);
    for (int p = 0; p < 3; ++p) {
        const int s = p ? 2 : 1;
        for (int y = 0; y < h / s; ++y) memcpy(dst + (size_t)y * (w / s), src + (size_t)y * (cw / s), (size_t)(w / s));
        src += (size_t)(cw / s) * (ch / s); dst += (size_t)(w / s) * (h / s);
    }
    return KS265_OK;
}

int ks265_sse_window(ks265_ctx *c, ks265_frame *f, ks265_pic a, ks265_pic b, int w, int h, uint64_t *sse3)
{
    (void)a; (void)b;
    if (!c || !f || !sse3) return KS265_POINTER;
    if (!window_sizes_ok(w, h, f->cfg.width, f->cfg.height)) return KS265_NOTSUPPORTED;
    call_log(__func__, c, f, NULL, 0);
    return KS265_OK;
}
