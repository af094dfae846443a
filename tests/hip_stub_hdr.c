/* TEST INFRASTRUCTURE: the device library's CPU stand-in with everything hip_stub_enhance.c has (included as it is) plus the three entries of the local-contrast filter
 * (include/ks265_hip.h: ks265_input_hdr[_validate|_work_bytes]), in plain C after tests/hdr_ref.py.  "Device memory" is the process's own.  Every ks265_input_hdr call is
 * logged like the others (arg: iters) and kept - size, cfg, and which work buffer it was given, as the ordinal of that buffer's first appearance since the last reset (a
 * lane owns one: one lane shows 0 throughout) - for ks265_stub_hdr_calls. */
#include "hip_stub_enhance.c"

typedef struct { int32_t w, h, gain, iters, slope, radius[3], work_no, work_ok; } StubHdrCall;
static pthread_mutex_t g_hdr_mu = PTHREAD_MUTEX_INITIALIZER;
static StubHdrCall g_hdr[4096]; static int g_nhdr;
static const void *g_hdr_buf[64]; static int g_nhdr_buf;
/* the calls so far (at most cap of them, oldest first) into out; returns how many there were.  ks265_stub_hdr_reset forgets them */
int ks265_stub_hdr_calls(StubHdrCall *out, int cap)
{
    pthread_mutex_lock(&g_hdr_mu);
    const int n = g_nhdr;
    for (int i = 0; i < n && i < cap && i < 4096; ++i) out[i] = g_hdr[i];
    pthread_mutex_unlock(&g_hdr_mu);
    return n;
}
void ks265_stub_hdr_reset(void) { pthread_mutex_lock(&g_hdr_mu); g_nhdr = 0; g_nhdr_buf = 0; pthread_mutex_unlock(&g_hdr_mu); }

int ks265_input_hdr_validate(ks265_ctx *c, const ks265_hdr_cfg *cfg, int w, int h)
{
    if (!c || !cfg) return KS265_POINTER;
    if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || w > 8192 || h > 8192) return KS265_NOTSUPPORTED;
    if (cfg->gain < 1 || cfg->gain > 80 || (cfg->iters != 2 && cfg->iters != 3) || cfg->slope < 0 || cfg->slope > 4096) return KS265_NOTSUPPORTED;
    for (int i = 0; i < cfg->iters; ++i) if (cfg->radius[i] < 16 || cfg->radius[i] > 2480) return KS265_NOTSUPPORTED;
    return KS265_OK;
}

size_t ks265_input_hdr_work_bytes(int w, int h)
{
    if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || w > 8192 || h > 8192) return 0;
    return (size_t)5 * w * h;
}

/* one pass over a line of n samples `step` apart: y the guidance, j in, o out (o != j), ct / ps the caller's n + 1 each */
static void hdr_line(const uint8_t *y, const uint16_t *j, uint16_t *o, int n, size_t step, int slope, int r, int64_t *ct, int64_t *ps)
{
    ct[0] = 0; ps[0] = 0;
    for (int x = 0; x < n; ++x) {
        if (x) { const int d = y[x * step] - y[(x - 1) * step]; ct[x] = ct[x - 1] + 16 + (int64_t)slope * (d < 0 ? -d : d); }
        ps[x + 1] = ps[x] + j[x * step];
    }
    int lo = 0, hi = 0;
    for (int x = 0; x < n; ++x) {
        while (ct[x] - ct[lo] > r) ++lo;
        if (hi < x) hi = x;
        while (hi + 1 < n && ct[hi + 1] - ct[x] <= r) ++hi;
        const int64_t S = ps[hi + 1] - ps[lo], cnt = hi - lo + 1;
        o[x * step] = (uint16_t)((2 * S + cnt) / (2 * cnt));
    }
}

int ks265_input_hdr(ks265_ctx *c, const ks265_hdr_cfg *cfg, int w, int h, uint8_t *pic, void *work, size_t work_bytes)
{
    const int r = ks265_input_hdr_validate(c, cfg, w, h);
    if (r) return r;
    const size_t npx = (size_t)w * h, n = npx * 3 / 2, need = 5 * npx;
    if (!pic || !work || work_bytes < need) return KS265_POINTER;
    if (((uintptr_t)pic | (uintptr_t)work) & 3) return KS265_NOTSUPPORTED;
    if ((uint8_t *)work < pic + n && pic < (uint8_t *)work + need) return KS265_POINTER;
    if (call_log(__func__, c, NULL, NULL, cfg->iters)) return KS265_FAIL;
    pthread_mutex_lock(&g_hdr_mu);
    int no = 0;
    while (no < g_nhdr_buf && g_hdr_buf[no] != work) ++no;
    if (no == g_nhdr_buf && g_nhdr_buf < 64) g_hdr_buf[g_nhdr_buf++] = work;
    const StubHdrCall k = {w, h, cfg->gain, cfg->iters, cfg->slope, {cfg->radius[0], cfg->radius[1], cfg->iters > 2 ? cfg->radius[2] : 0}, no, work_bytes == need};
    if (g_nhdr < 4096) g_hdr[g_nhdr] = k;
    ++g_nhdr;
    pthread_mutex_unlock(&g_hdr_mu);
    uint16_t *a = (uint16_t *)((uint8_t *)work + npx), *b = a + npx;    /* (the layout is the stand-in's own business, as the kernel's is the kernel's) */
    const int longest = w > h ? w : h;
    int64_t *ct = (int64_t *)malloc(2 * (size_t)(longest + 1) * sizeof *ct), *ps = ct ? ct + longest + 1 : NULL;
    if (!ct) return KS265_OUTOFMEMORY;
    for (size_t i = 0; i < npx; ++i) a[i] = (uint16_t)(16 * pic[i]);
    for (int it = 0; it < cfg->iters; ++it) {
        for (int y = 0; y < h; ++y) hdr_line(pic + (size_t)y * w, a + (size_t)y * w, b + (size_t)y * w, w, 1, cfg->slope, cfg->radius[it], ct, ps);
        for (int x = 0; x < w; ++x) hdr_line(pic + x, b + x, a + x, h, (size_t)w, cfg->slope, cfg->radius[it], ct, ps);
    }
    free(ct);
    for (size_t i = 0; i < npx; ++i) {
        const int y = pic[i], gd = cfg->gain * (16 * y - (int)a[i]), m = ((gd < 0 ? -gd : gd) + 128) >> 8, o = gd < 0 ? y - m : y + m;
        pic[i] = (uint8_t)(o < 0 ? 0 : o > 255 ? 255 : o);
    }
    return KS265_OK;
}
