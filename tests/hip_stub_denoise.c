/* TEST INFRASTRUCTURE: the device library's CPU stand-in with everything hip_stub_window.c has (included as it is) plus the two entries of the temporal denoiser
 * (include/ks265_hip.h: ks265_input_denoise[_validate]), in plain C after tests/denoise_ref.py.  "Device memory" is the process's own.  Every ks265_input_denoise call is kept -
 * size, cfg, whether there was a history, and which buffers the history came from and went to (numbered in the order the stand-in first saw them) - for
 * ks265_stub_denoise_calls. */
#include "hip_stub_window.c"

typedef struct { int32_t w, h, thr, weight, has_hist, hist_in, hist_out; } StubDnCall;     /* hist_in / hist_out: the buffer's number (from 0), -1 = NULL */
static pthread_mutex_t g_dn_mu = PTHREAD_MUTEX_INITIALIZER;
static StubDnCall g_dn[4096]; static int g_ndn;
static const void *g_dn_buf[64]; static int g_ndn_buf;
/* the calls so far (at most cap of them, oldest first) into out; returns how many there were.  ks265_stub_denoise_reset forgets them and the buffers' numbers */
int ks265_stub_denoise_calls(StubDnCall *out, int cap)
{
    pthread_mutex_lock(&g_dn_mu);
    const int n = g_ndn;
    for (int i = 0; i < n && i < cap && i < 4096; ++i) out[i] = g_dn[i];
    pthread_mutex_unlock(&g_dn_mu);
    return n;
}
void ks265_stub_denoise_reset(void) { pthread_mutex_lock(&g_dn_mu); g_ndn = 0; g_ndn_buf = 0; pthread_mutex_unlock(&g_dn_mu); }
static int dn_buf_number(const void *p)                                  /* (g_dn_mu held) */
{
    if (!p) return -1;
    for (int i = 0; i < g_ndn_buf; ++i) if (g_dn_buf[i] == p) return i;
    if (g_ndn_buf < 64) g_dn_buf[g_ndn_buf++] = p;
    return g_ndn_buf - 1;
}

int ks265_input_denoise_validate(ks265_ctx *c, const ks265_denoise_cfg *cfg, int w, int h)
{
    if (!c || !cfg) return KS265_POINTER;
    if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || w > 8192 || h > 8192) return KS265_NOTSUPPORTED;
    if (cfg->thr < 1 || cfg->thr > 64 || cfg->weight < 1 || cfg->weight > 30) return KS265_NOTSUPPORTED;
    return KS265_OK;
}

static int dn_blend(int c, int p, int thr, int wmax)
{
    const int d = c > p ? c - p : p - c, t = thr - d > 0 ? thr - d : 0;
    int w = 2 * wmax * t / thr;
    if (w > wmax) w = wmax;
    return (c * (32 - w) + p * w + 16) >> 5;
}

/* one picture, block by block; out receives the filtered picture (cur stays) */
static void dn_filter(const uint8_t *cur, const uint8_t *hist, int W, int H, int thr, int wmax, uint8_t *out, int32_t *blocks)
{
    const size_t npx = (size_t)W * H;
    memcpy(out, cur, npx * 3 / 2);
    int nb = 0;
    for (int by = 0; by < H; by += 16)
        for (int bx = 0; bx < W; bx += 16, ++nb) {
            const int bw = W - bx < 16 ? W - bx : 16, bh = H - by < 16 ? H - by : 16;
            if (!hist) { if (blocks) { blocks[2 * nb] = 8 | 8 << 8 | 1 << 16; blocks[2 * nb + 1] = 0; } continue; }
            long best[4] = {0, 0, 0, 0}; int have = 0, bsad = 0;            /* (cost, l1, dy, dx): the candidates in any order, the smallest tuple wins */
            for (int dy = -8; dy <= 8; ++dy)
                for (int dx = -8; dx <= 8; ++dx) {
                    if (bx + dx < 0 || bx + dx + bw > W || by + dy < 0 || by + dy + bh > H) continue;
                    int sad = 0;
                    for (int y = 0; y < bh; ++y)
                        for (int x = 0; x < bw; ++x) sad += abs((int)cur[(size_t)(by + y) * W + bx + x] - (int)hist[(size_t)(by + dy + y) * W + bx + dx + x]);
                    const long l1 = abs(dx) + abs(dy), k[4] = {sad + 16 * l1, l1, dy, dx};
                    int less = !have;
                    for (int i = 0; i < 4 && !less; ++i) { if (k[i] != best[i]) { less = k[i] < best[i]; break; } }
                    if (less) { memcpy(best, k, sizeof best); bsad = sad; have = 1; }
                }
            const int dx = (int)best[3], dy = (int)best[2], gated = bsad >= thr * bw * bh;
            if (blocks) { blocks[2 * nb] = (dx + 8) | (dy + 8) << 8 | gated << 16; blocks[2 * nb + 1] = bsad; }
            if (gated) continue;
            for (int y = 0; y < bh; ++y)
                for (int x = 0; x < bw; ++x) {
                    const size_t at = (size_t)(by + y) * W + bx + x;
                    out[at] = (uint8_t)dn_blend(cur[at], hist[(size_t)(by + dy + y) * W + bx + dx + x], thr, wmax);
                }
            const int cw = W / 2, fx = dx & 1, fy = dy & 1, mx = dx >> 1, my = dy >> 1;      /* (>> of a negative int: arithmetic with gcc and clang, as the test's compilers) */
            for (int pl = 0; pl < 2; ++pl) {
                const uint8_t *cp = cur + npx + (pl ? npx / 4 : 0), *hp = hist + npx + (pl ? npx / 4 : 0);
                uint8_t *op = out + npx + (pl ? npx / 4 : 0);
                for (int y = 0; y < bh / 2; ++y)
                    for (int x = 0; x < bw / 2; ++x) {
                        const size_t at = (size_t)(by / 2 + y) * cw + bx / 2 + x;
                        const uint8_t *q = hp + (size_t)(by / 2 + my + y) * cw + bx / 2 + mx + x;
                        const int p = (q[0] + q[fx] + q[(size_t)fy * cw] + q[(size_t)fy * cw + fx] + 2) >> 2;
                        op[at] = (uint8_t)dn_blend(cp[at], p, (thr + 1) >> 1, wmax);
                    }
            }
        }
}

int ks265_input_denoise(ks265_ctx *c, const ks265_denoise_cfg *cfg, int w, int h, uint8_t *pic, const uint8_t *hist_in, uint8_t *hist_out, int32_t *blocks)
{
    const int r = ks265_input_denoise_validate(c, cfg, w, h);
    if (r) return r;
    if (!pic || !hist_out) return KS265_POINTER;
    const size_t n = (size_t)w * h * 3 / 2;
    if ((pic < hist_out + n && hist_out < pic + n) || (hist_in && ((hist_in < hist_out + n && hist_out < hist_in + n) || (hist_in < pic + n && pic < hist_in + n)))) return KS265_POINTER;
    if (call_log(__func__, c, NULL, NULL, hist_in != NULL)) return KS265_FAIL;
    pthread_mutex_lock(&g_dn_mu);
    const int from = dn_buf_number(hist_in), to = dn_buf_number(hist_out);
    const StubDnCall k = {w, h, cfg->thr, cfg->weight, hist_in != NULL, from, to};
    if (g_ndn < 4096) g_dn[g_ndn] = k;
    ++g_ndn;
    pthread_mutex_unlock(&g_dn_mu);
    dn_filter(pic, hist_in, w, h, cfg->thr, cfg->weight, hist_out, blocks);
    memcpy(pic, hist_out, n);
    return KS265_OK;
}
