/* TEST INFRASTRUCTURE (tests/test_input_order_cpu.py, tests/test_lane_put_cpu.py): hands pictures to the encoder host (ks265codec_amd/host/ks265_enc.c) on the device library's
 * stand-in (tests/hip_stub_window.c: every way in there is) by every way a picture can reach a lane.  A program of its own, so that it can be built with sanitizers and run as it is.
 *   lane_put_main run  OUT W H N WAYS [name value]...   one handle, N pictures handed in by the ways of WAYS in turn, then the flush; the stream goes to the file OUT, one line
 *                                                        `rc <way> <code>` per call of the API goes to stdout, then `live <objects of the stand-in alive after the close>`
 *   lane_put_main walk W H WAYS [name value]...         the k-th call the calling thread makes to the device library while it hands in the LAST picture of WAYS fails
 *                                                        (ks265_stub_fail_call), for every k of such a call: `k <k> <code>`; the call must fail, nothing more is handed in, the
 *                                                        handle is closed, and no object of the stand-in may be alive then
 * WAYS, a letter per picture (the pictures' content does not depend on it):
 *   c  host, planes packed in one buffer      p  host, packed planes in three buffers      s  host, strides wider than the rows
 *   a  host, written into an acquired slot    u  host, a slot acquired and NOT used (the picture comes in a buffer of the caller's; the slot stays acquired)
 *   d  device I420 at pitches of its own      n  device NV12      r  device RGBA      y  device KS265_IN_I010      f  device RGB float32
 *   z  device I420 of 2W x 2H, scaled (triangle)
 * and letters that hand in no picture:
 *   h / g  a ROI map (int8, blocks of 16) for the next picture, from host / device memory
 *   X  a device picture with a chroma pitch below its row      Y  a scaled picture of 4W x 4H, over the enabled 2W x 2H      Z  a device RGB picture (a ragged handle refuses it)
 * name value: `latency zerolatency`, a QY265ConfigParse pair, or one of ks265_enc_set_default (roi, ...).  The configuration starts as -preset medium with `threads 4`, `log 1`,
 * `rc 0`, `qp 34`.  KS265_* variables act as always. */
#include "ks265_enc.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void ks265_stub_fail_call(long k);
long ks265_stub_thread_calls(void);
void ks265_stub_mark(void);
long ks265_stub_live(int kind);

typedef struct Run {
    int W, H; void *h; FILE *out; long fed;
    uint8_t *img, *buf, *sep[3]; int8_t *map;
    int arm;                                                             /* walk: the picture's call runs with the k-th call failing (0: counted only) */
    long calls; int last_rc;
} Run;

static void emit(Run *r, char way, int rc, QY265Nal *nal, int nn)
{
    if (r->out) {
        printf("rc %c %d\n", way, rc);
        for (int i = 0; i < nn && rc == QY_OK; ++i) if (nal[i].iSize > 0) fwrite(nal[i].pPayload, 1, (size_t)nal[i].iSize, r->out);
    }
    r->last_rc = rc;
}

/* picture t as packed I420 of w x h */
static void picture(uint8_t *p, int w, int h, long t)
{
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) p[(size_t)y * w + x] = (uint8_t)(x * 3 + y * 5 + t * 29 + ((x ^ y) & 8));
    uint8_t *c = p + (size_t)w * h;
    for (size_t i = 0; i < (size_t)w * h / 2; ++i) c[i] = (uint8_t)(128 + (int)((i * 7 + (size_t)t * 11) % 61) - 30);
}
static void rows(uint8_t *d, long long dp, int dstep, const uint8_t *s, int w, int h)
{
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) d[y * dp + (long long)x * dstep] = s[(size_t)y * w + x];
}

static int encode(Run *r, char way, QY265Picture *in, const ks265_dev_picture *dp, int sw, int sh)
{
    QY265Nal *nal = NULL; int nn = 0; QY265Picture outp;
    memset(&outp, 0, sizeof outp);
    if (r->arm >= 0) ks265_stub_fail_call(r->arm);
    const int rc = !dp ? QY265EncoderEncodeFrame(r->h, &nal, &nn, in, &outp, 0) : sw ? ks265_enc_encode_device_frame_scaled(r->h, &nal, &nn, dp, sw, sh, 0, &outp)
                                                                                     : ks265_enc_encode_device_frame(r->h, &nal, &nn, dp, &outp);
    if (r->arm >= 0) { r->calls = ks265_stub_thread_calls(); ks265_stub_fail_call(0); }
    emit(r, way, rc, nal, nn);
    return rc;
}

static void step(Run *r, char way, int armed)
{
    const int W = r->W, H = r->H;
    const size_t ny = (size_t)W * H, nc = ny / 4;
    const uint8_t *pl[3] = {r->img, r->img + ny, r->img + ny + nc};
    r->arm = armed;
    if (way == 'h' || way == 'g') {
        const int cols = (W + 15) / 16, rws = (H + 15) / 16;
        for (int i = 0; i < cols * rws; ++i) r->map[i] = (int8_t)((i * 5 + r->fed) % 13 - 6);
        const ks265_roi roi = {KS265_ROI_INT8, 4, way == 'g' ? 0 : -1, r->map, cols, NULL};
        emit(r, way, ks265_enc_set_next_roi(r->h, &roi), NULL, 0);
        return;
    }
    picture(r->img, W, H, r->fed);
    if (strchr("cpsau", way)) {
        QY265YUV yuv; QY265Picture pic;
        memset(&yuv, 0, sizeof yuv); memset(&pic, 0, sizeof pic);
        int got = 0;
        if (way == 'a' || way == 'u') got = ks265_enc_acquire_input(r->h, &yuv) == QY_OK;
        if (way == 'a' && got) memcpy(yuv.pData[0], r->img, ny + 2 * nc);
        else {
            const int ex = way == 's' ? 16 : 0;
            yuv.iWidth = W; yuv.iHeight = H;
            yuv.iStride[0] = W + ex; yuv.iStride[1] = yuv.iStride[2] = W / 2 + ex / 2;
            yuv.pData[0] = way == 'p' ? r->sep[0] : r->buf;
            yuv.pData[1] = way == 'p' ? r->sep[1] : yuv.pData[0] + (size_t)yuv.iStride[0] * H;
            yuv.pData[2] = way == 'p' ? r->sep[2] : yuv.pData[1] + (size_t)yuv.iStride[1] * (H / 2);
            for (int k = 0; k < 3; ++k) rows(yuv.pData[k], yuv.iStride[k], 1, pl[k], k ? W / 2 : W, k ? H / 2 : H);
        }
        pic.yuv = &yuv; pic.pts = r->fed;
        if (encode(r, way, &pic, NULL, 0, 0) == QY_OK) ++r->fed;
        return;
    }
    ks265_dev_picture d;
    memset(&d, 0, sizeof d);
    d.pts = r->fed;
    int sw = 0, sh = 0, good = 1;
    if (way == 'd' || way == 'X') {
        d.format = KS265_IN_I420;
        d.pitch[0] = W + 5; d.pitch[1] = d.pitch[2] = W / 2 + 5;
        d.plane[0] = r->buf; d.plane[1] = r->buf + (size_t)d.pitch[0] * H; d.plane[2] = (const uint8_t *)d.plane[1] + (size_t)d.pitch[1] * (H / 2);
        for (int k = 0; k < 3; ++k) rows((uint8_t *)d.plane[k], d.pitch[k], 1, pl[k], k ? W / 2 : W, k ? H / 2 : H);
        if (way == 'X') { d.pitch[1] = W / 2 - 1; good = 0; }
    } else if (way == 'n') {
        d.format = KS265_IN_NV12;
        d.pitch[0] = d.pitch[1] = W + 6;
        d.plane[0] = r->buf; d.plane[1] = r->buf + (size_t)d.pitch[0] * H;
        rows((uint8_t *)d.plane[0], d.pitch[0], 1, pl[0], W, H);
        rows((uint8_t *)d.plane[1], d.pitch[1], 2, pl[1], W / 2, H / 2); rows((uint8_t *)d.plane[1] + 1, d.pitch[1], 2, pl[2], W / 2, H / 2);
    } else if (way == 'r' || way == 'Z') {
        d.format = KS265_IN_RGB; d.pixel_step = 4; d.pitch[0] = 4 * W;
        for (int k = 0; k < 3; ++k) d.plane[k] = r->buf + k;
        for (size_t i = 0; i < 4 * ny; ++i) r->buf[i] = (uint8_t)(i * 3 + (size_t)r->fed * 17);
        good = way == 'r';
    } else if (way == 'y') {
        d.format = KS265_IN_I010;
        d.pitch[0] = 2 * W; d.pitch[1] = d.pitch[2] = W;
        d.plane[0] = r->buf; d.plane[1] = r->buf + 2 * ny; d.plane[2] = r->buf + 2 * ny + 2 * nc;
        uint16_t *q = (uint16_t *)r->buf;
        for (size_t i = 0; i < ny + 2 * nc; ++i) q[i] = (uint16_t)(r->img[i] << 2 | (i & 3));
    } else if (way == 'f') {
        d.format = KS265_IN_RGB_F32; d.pixel_step = 12; d.pitch[0] = 12 * W;
        for (int k = 0; k < 3; ++k) d.plane[k] = r->buf + 4 * k;
        float *q = (float *)r->buf;
        for (size_t i = 0; i < 3 * ny; ++i) q[i] = (float)((i * 5 + (size_t)r->fed * 23) & 255) / 255.0f;
    } else if (way == 'z' || way == 'Y') {
        const int m = way == 'z' ? 2 : 4;
        sw = m * W; sh = m * H; good = way == 'z';
        d.format = KS265_IN_I420;
        d.pitch[0] = sw; d.pitch[1] = d.pitch[2] = sw / 2;
        d.plane[0] = r->buf; d.plane[1] = r->buf + (size_t)sw * sh; d.plane[2] = r->buf + (size_t)sw * sh * 5 / 4;
        if (good) picture(r->buf, sw, sh, r->fed);                       /* (the refused one is judged by its size: its planes are never read) */
    } else { fprintf(stderr, "way %c?\n", way); exit(2); }
    if (encode(r, way, NULL, &d, sw, sh) == QY_OK && good) ++r->fed;
}

static int open_run(Run *r, const QY265EncConfig *cfg, const char *ways)
{
    int err = 0;
    QY265EncConfig c = *cfg;
    r->h = QY265EncoderOpen(&c, &err);
    if (!r->h) { printf("FAIL: open %d\n", err); return 1; }
    r->fed = 0;
    if (strpbrk(ways, "dnryfzXYZ")) emit(r, 'D', ks265_enc_enable_device_input(r->h), NULL, 0);
    if (strpbrk(ways, "zY")) emit(r, 'S', ks265_enc_enable_device_scale(r->h, 2 * r->W, 2 * r->H), NULL, 0);
    return 0;
}

static int close_run(Run *r, const char *when)
{
    int bad = 0;
    QY265EncoderClose(r->h); r->h = NULL;
    for (int k = 0; k < 5; ++k) if (ks265_stub_live(k)) { printf("FAIL %s: %ld objects of kind %d alive\n", when, ks265_stub_live(k), k); bad = 1; }
    return bad;
}

int main(int argc, char **argv)
{
    const int walk = argc > 1 && !strcmp(argv[1], "walk"), a0 = walk ? 2 : 3;
    if (argc < a0 + 3 || ((argc - a0 - (walk ? 3 : 4)) & 1) || (!walk && strcmp(argv[1], "run"))) { fprintf(stderr, "usage: lane_put_main run OUT W H N WAYS [name value]... | walk W H WAYS [name value]...\n"); return 2; }
    Run r;
    memset(&r, 0, sizeof r);
    r.W = atoi(argv[a0]); r.H = atoi(argv[a0 + 1]);
    const long n = walk ? 0 : atol(argv[a0 + 2]);
    const char *ways = argv[a0 + (walk ? 2 : 3)];
    const int opt = a0 + (walk ? 3 : 4);
    int latency = QY265LATENCY_DEFAULT;
    for (int i = opt; i + 1 < argc; i += 2) if (!strcmp(argv[i], "latency") && !strcmp(argv[i + 1], "zerolatency")) latency = QY265LATENCY_ZERO;
    QY265EncConfig cfg;
    QY265ConfigDefault(&cfg, QY265PRESET_MEDIUM, QY265TUNE_DEFAULT, latency);
    cfg.picWidth = r.W; cfg.picHeight = r.H; cfg.threads = 4; cfg.logLevel = 1; cfg.rc = 0; cfg.qp = 34;
    for (int i = opt; i + 1 < argc; i += 2) {
        if (!strcmp(argv[i], "latency")) continue;
        int e = QY265ConfigParse(&cfg, argv[i], argv[i + 1]);
        if (e == QY265_PARAM_BAD_NAME) e = ks265_enc_set_default(argv[i], atoi(argv[i + 1]));
        if (e) { fprintf(stderr, "%s %s: refused (%d)\n", argv[i], argv[i + 1], e); return 2; }
    }
    const size_t ny = (size_t)r.W * r.H;
    r.img = (uint8_t *)malloc(ny * 3 / 2); r.buf = (uint8_t *)malloc(ny * 24 + 4096); r.map = (int8_t *)malloc((size_t)((r.W + 15) / 16) * ((r.H + 15) / 16));
    r.sep[0] = (uint8_t *)malloc(ny); r.sep[1] = (uint8_t *)malloc(ny / 4); r.sep[2] = (uint8_t *)malloc(ny / 4);
    if (!r.img || !r.buf || !r.map || !r.sep[0] || !r.sep[1] || !r.sep[2]) return 2;
    ks265_stub_mark();                                                   /* (the thread that hands the pictures in) */
    int bad = 0;
    const size_t nw = strlen(ways);
    if (!walk) {
        r.out = fopen(argv[2], "wb");
        if (!r.out) return 2;
        if (open_run(&r, &cfg, ways)) return 1;
        for (size_t i = 0; r.fed < n && i < 64 * nw; ++i) step(&r, ways[i % nw], -1);
        for (int k = 0; k < 4096 && QY265EncoderDelayedFrames(r.h) > 0; ++k) {
            QY265Nal *nal = NULL; int nn = 0; QY265Picture outp;
            const int rc = QY265EncoderEncodeFrame(r.h, &nal, &nn, NULL, &outp, 0);
            emit(&r, '-', rc, nal, nn);
            if (rc) break;
        }
        bad = close_run(&r, "after the close");
        fclose(r.out);
        printf("live %s\n", bad ? "FAIL" : "0");
    } else {
        long ncalls = 0;
        for (long k = 0; k <= ncalls; ++k) {                             /* k = 0: nothing fails, the picture's calls are counted */
            char when[32]; snprintf(when, sizeof when, "k = %ld", k);
            if (open_run(&r, &cfg, ways)) return 1;
            for (size_t i = 0; i < nw; ++i) step(&r, ways[i], i + 1 < nw ? -1 : (int)k);
            if (!k) { ncalls = r.calls; printf("calls %ld\n", ncalls); if (r.last_rc != QY_OK) { printf("FAIL: the plain picture: %d\n", r.last_rc); bad = 1; } }
            else { printf("k %ld %d\n", k, r.last_rc); if (r.last_rc == QY_OK) { printf("FAIL %s: the call succeeded\n", when); bad = 1; } }
            bad |= close_run(&r, when);
        }
        printf("walk: %s\n", bad ? "FAIL" : "ok");
    }
    free(r.img); free(r.buf); free(r.map); free(r.sep[0]); free(r.sep[1]); free(r.sep[2]);
    return bad;
}
