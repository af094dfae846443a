/* TEST INFRASTRUCTURE: the device library's CPU stand-in with everything hip_stub_denoise.c has (included as it is) plus the two entries of the edge / colour enhancement
 * (include/ks265_hip.h: ks265_input_enhance[_validate]), in plain C after tests/enhance_ref.py.  "Device memory" is the process's own.  Every ks265_input_enhance call is logged
 * like the others (arg: 1 = a luma source was handed over) and kept - size, cfg, and whether the luma source was one of the denoiser's history buffers - for
 * ks265_stub_enhance_calls. */
#include "hip_stub_denoise.c"

typedef struct { int32_t w, h, edge_gain, edge_core, edge_limit, edge_over, color_gain, has_src, src_is_hist; } StubEnCall;
static pthread_mutex_t g_en_mu = PTHREAD_MUTEX_INITIALIZER;
static StubEnCall g_en[4096]; static int g_nen;
/* the calls so far (at most cap of them, oldest first) into out; returns how many there were.  ks265_stub_enhance_reset forgets them */
int ks265_stub_enhance_calls(StubEnCall *out, int cap)
{
    pthread_mutex_lock(&g_en_mu);
    const int n = g_nen;
    for (int i = 0; i < n && i < cap && i < 4096; ++i) out[i] = g_en[i];
    pthread_mutex_unlock(&g_en_mu);
    return n;
}
void ks265_stub_enhance_reset(void) { pthread_mutex_lock(&g_en_mu); g_nen = 0; pthread_mutex_unlock(&g_en_mu); }

int ks265_input_enhance_validate(ks265_ctx *c, const ks265_enhance_cfg *cfg, int w, int h)
{
    if (!c || !cfg) return KS265_POINTER;
    if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || w > 8192 || h > 8192) return KS265_NOTSUPPORTED;
    if (cfg->edge_gain < 0 || cfg->edge_gain > 64 || cfg->edge_core < 0 || cfg->edge_core > 16 || cfg->edge_over < 0 || cfg->edge_over > 32 || cfg->color_gain < 0 || cfg->color_gain > 32) return KS265_NOTSUPPORTED;
    if (cfg->edge_gain > 0 && (cfg->edge_limit < 1 || cfg->edge_limit > 64)) return KS265_NOTSUPPORTED;
    if (!cfg->edge_gain && !cfg->color_gain) return KS265_NOTSUPPORTED;
    return KS265_OK;
}

static int en_at(const uint8_t *s, int W, int H, int x, int y)         /* coordinates clamped into the plane */
{
    x = x < 0 ? 0 : x >= W ? W - 1 : x; y = y < 0 ? 0 : y >= H ? H - 1 : y;
    return s[(size_t)y * W + x];
}

static void en_luma(const uint8_t *s, int W, int H, const ks265_enhance_cfg *g, uint8_t *out)
{
    static const int k[5] = {1, 4, 6, 4, 1};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int v = 0, mn = 255, mx = 0;
            for (int j = 0; j < 5; ++j) {
                int hsum = 0;
                for (int i = 0; i < 5; ++i) hsum += k[i] * en_at(s, W, H, x + i - 2, y + j - 2);
                v += k[j] * hsum;
            }
            for (int j = -1; j <= 1; ++j)
                for (int i = -1; i <= 1; ++i) { const int q = en_at(s, W, H, x + i, y + j); if (q < mn) mn = q; if (q > mx) mx = q; }
            const int S = s[(size_t)y * W + x], d = 256 * S - v, ad = d < 0 ? -d : d;
            const int a = ad - 256 * g->edge_core > 0 ? ad - 256 * g->edge_core : 0;
            int e = (g->edge_gain * a + 2048) >> 12;
            if (e > g->edge_limit) e = g->edge_limit;
            int o = d < 0 ? S - e : S + e;
            const int lo = mn - g->edge_over > 0 ? mn - g->edge_over : 0, hi = mx + g->edge_over < 255 ? mx + g->edge_over : 255;
            out[(size_t)y * W + x] = (uint8_t)(o < lo ? lo : o > hi ? hi : o);
        }
}

static int en_color1(int s, int K)
{
    const int c = s - 128, m = ((c < 0 ? -c : c) * K + 4096) >> 13, o = c < 0 ? 128 - m : 128 + m;
    return o < 0 ? 0 : o > 255 ? 255 : o;
}

int ks265_input_enhance(ks265_ctx *c, const ks265_enhance_cfg *cfg, int w, int h, const uint8_t *luma_src, uint8_t *pic)
{
    const int r = ks265_input_enhance_validate(c, cfg, w, h);
    if (r) return r;
    const size_t npx = (size_t)w * h, n = npx * 3 / 2;
    if (!cfg->edge_gain) luma_src = NULL;
    if (!pic || (cfg->edge_gain && !luma_src)) return KS265_POINTER;
    if (luma_src && luma_src < pic + n && pic < luma_src + npx) return KS265_POINTER;
    if (call_log(__func__, c, NULL, NULL, luma_src != NULL)) return KS265_FAIL;
    pthread_mutex_lock(&g_dn_mu);
    int is_hist = 0;
    for (int i = 0; i < g_ndn_buf; ++i) if (luma_src && g_dn_buf[i] == luma_src) is_hist = 1;
    pthread_mutex_unlock(&g_dn_mu);
    pthread_mutex_lock(&g_en_mu);
    const StubEnCall k = {w, h, cfg->edge_gain, cfg->edge_core, cfg->edge_limit, cfg->edge_over, cfg->color_gain, luma_src != NULL, is_hist};
    if (g_nen < 4096) g_en[g_nen] = k;
    ++g_nen;
    pthread_mutex_unlock(&g_en_mu);
    if (cfg->edge_gain) en_luma(luma_src, w, h, cfg, pic);
    if (cfg->color_gain) {
        uint8_t *u = pic + npx, *v = u + npx / 4;
        for (size_t i = 0; i < npx / 4; ++i) {
            const int cu = u[i] - 128, cv = v[i] - 128, au = cu < 0 ? -cu : cu, av = cv < 0 ? -cv : cv;
            const int K = 8192 + cfg->color_gain * (128 - (au > av ? au : av));
            u[i] = (uint8_t)en_color1(u[i], K); v[i] = (uint8_t)en_color1(v[i], K);
        }
    }
    return KS265_OK;
}
