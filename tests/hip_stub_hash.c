/* TEST INFRASTRUCTURE: the device library's CPU stand-in (hip_stub.c, included as it is) plus ks265_picture_hash / ks265_picture_hash_on, computed byte by byte in plain C from
 * the stand-in's pictures: picture_crc as the standard's bit loop, picture_checksum as its double loop (H.265 D.3.19; the specification the tests hold the values to is
 * tests/picture_hash_ref.py).  The host tests of the `hash` switch link this file instead of hip_stub.c.
 * A call inside a capture is kept with the capture and runs behind the replayed calls of ks265_graph_launch, like the stand-in's own recorded calls: for that the stand-in's
 * ks265_capture_end and ks265_graph_launch and ks265_graph_destroy are compiled under other names and wrapped below. */
#define ks265_capture_end stub_base_capture_end
#define ks265_graph_launch stub_base_graph_launch
#define ks265_graph_destroy stub_base_graph_destroy
#include "hip_stub.c"
#undef ks265_capture_end
#undef ks265_graph_launch
#undef ks265_graph_destroy
int ks265_capture_end(ks265_ctx *c, void **exec);
int ks265_graph_launch(ks265_ctx *c, void *exec);
int ks265_graph_destroy(ks265_ctx *c, void *exec);

static void plane_hash(const uint8_t *p, long stride, int w, int h, uint32_t *crc_out, uint32_t *sum_out)
{
    uint32_t crc = 0xFFFF, sum = 0;
    for (long i = 0; i < (long)w * h + 2; ++i) {
        const int y = (int)(i / w), x = (int)(i - (long)y * w);
        const uint32_t byte = y < h ? p[(long)y * stride + x] : 0;      /* the two zero bytes behind the plane */
        for (int k = 7; k >= 0; --k) {
            const uint32_t msb = crc >> 15 & 1;
            crc = (((crc << 1) + (byte >> k & 1)) & 0xFFFF) ^ (msb * 0x1021);
        }
        if (y < h) sum += byte ^ (uint32_t)((x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8));
    }
    *crc_out = crc; *sum_out = sum;
}
/* the stand-in's picture is what its ks265_store_i420 hands out: the luma plane, and flat 128 for both chroma planes (it keeps none) */
static void hash_now(const ks265_frame *f, ks265_pic p, uint32_t *h6)
{
    const int W = f->cfg.width, H = f->cfg.height;
    uint8_t *flat = (uint8_t *)malloc((size_t)(W / 2) * (H / 2));
    if (!flat) { memset(h6, 0, 24); return; }
    memset(flat, 128, (size_t)(W / 2) * (H / 2));
    plane_hash(luma0(f, p), f->g.stride_y, W, H, h6 + 0, h6 + 3);
    plane_hash(flat, W / 2, W / 2, H / 2, h6 + 1, h6 + 4);
    h6[2] = h6[1]; h6[5] = h6[4];
    free(flat);
}

/* hash calls met inside a capture: first with their context (exec = NULL), from ks265_capture_end on with the graph they belong to */
typedef struct HashOp { ks265_ctx *c; void *exec; ks265_frame *f; ks265_pic p; uint32_t *dst; } HashOp;
static HashOp g_hops[1024]; static int g_nhops; static pthread_mutex_t g_hmu = PTHREAD_MUTEX_INITIALIZER;

int ks265_picture_hash_on(ks265_ctx *c, ks265_frame *f, ks265_pic p, uint32_t *dev_hash6)
{
    LOGF(c, f, 0);
    if (!f || !c || !dev_hash6) return KS265_POINTER;
    if (f->ctx->capturing) {                                            /* (the stand-in records on the frame's context whichever stream the call names) */
        int r = KS265_OK;
        pthread_mutex_lock(&g_hmu);
        if (g_nhops < (int)(sizeof g_hops / sizeof g_hops[0])) { const HashOp o = {f->ctx, NULL, f, p, dev_hash6}; g_hops[g_nhops++] = o; } else r = KS265_OUTOFMEMORY;
        pthread_mutex_unlock(&g_hmu);
        return r;
    }
    hash_now(f, p, dev_hash6);
    return KS265_OK;
}
int ks265_picture_hash(ks265_frame *f, ks265_pic p, uint32_t *dev_hash6) { return f ? ks265_picture_hash_on(f->ctx, f, p, dev_hash6) : KS265_POINTER; }

int ks265_capture_end(ks265_ctx *c, void **exec)
{
    const int r = stub_base_capture_end(c, exec);
    pthread_mutex_lock(&g_hmu);
    int n = 0;
    for (int i = 0; i < g_nhops; ++i) {
        if (g_hops[i].c == c && !g_hops[i].exec) { if (r || !*exec) continue; g_hops[i].exec = *exec; }    /* a capture that failed: its calls go */
        g_hops[n++] = g_hops[i];
    }
    g_nhops = n;
    pthread_mutex_unlock(&g_hmu);
    return r;
}
int ks265_graph_launch(ks265_ctx *c, void *exec)
{
    const int r = stub_base_graph_launch(c, exec);
    pthread_mutex_lock(&g_hmu);
    for (int i = 0; i < g_nhops; ++i) if (g_hops[i].exec == exec) hash_now(g_hops[i].f, g_hops[i].p, g_hops[i].dst);
    pthread_mutex_unlock(&g_hmu);
    return r;
}
int ks265_graph_destroy(ks265_ctx *c, void *exec)
{
    pthread_mutex_lock(&g_hmu);
    int n = 0;
    for (int i = 0; i < g_nhops; ++i) if (g_hops[i].exec != exec) g_hops[n++] = g_hops[i];
    g_nhops = n;
    pthread_mutex_unlock(&g_hmu);
    return stub_base_graph_destroy(c, exec);
}
