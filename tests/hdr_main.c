/* TEST INFRASTRUCTURE: a handle with the local-contrast filter on (`hdr=1`, strength 2, 2 iterations, sigma_s 30, sigma_r at its default; with a sixth argument also
 * `denoise=2` and `edge=2` around it) at a size that is no multiple of 8, in a program of its own, for a build with -fsanitize=address,undefined against the host sources and
 * the stand-in tests/hip_stub_hdr.c (tests/test_hdr_host_cpu.py): open, encode N pictures - every third one through an acquired slot, every third one strided - flush, close.
 *   hdr_main WIDTH HEIGHT N STREAM_FILE LATENCY [all]    LATENCY: zerolatency | default.  Exit status 0 = every call succeeded and the stand-in saw one hdr call per picture at
 *                                                        the coded size with the derived integers (32, 2, 13, 744 / 372), always with the same work buffer of exactly
 *                                                        ks265_input_hdr_work_bytes; prints `hdr calls N` */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ks265_enc.h"

typedef struct { int32_t w, h, gain, iters, slope, radius[3], work_no, work_ok; } StubHdrCall;
int ks265_stub_hdr_calls(StubHdrCall *out, int cap);

static int put(FILE *f, QY265Nal *nal, int n) { for (int i = 0; i < n; ++i) if (nal[i].iSize > 0 && fwrite(nal[i].pPayload, 1, (size_t)nal[i].iSize, f) != (size_t)nal[i].iSize) return 1; return 0; }

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), N = atoi(argv[3]), all = argc > 6;
    char preset[] = "medium", tune[] = "default";
    QY265EncConfig cfg;
    if (QY265ConfigDefaultPreset(&cfg, preset, tune, argv[5])) return 3;
    cfg.picWidth = W; cfg.picHeight = H; cfg.frameRate = 50; cfg.rc = 0; cfg.qp = 34; cfg.threads = 2; cfg.logLevel = 1; cfg.calcPsnr = 1;
    if (QY265ConfigParse(&cfg, "hdr", "1") || cfg.vpp_hdr != 1 || QY265ConfigParse(&cfg, "hdr-strength", "2") || QY265ConfigParse(&cfg, "hdr-iter", "2") || cfg.vpp_hdr_iter != 2 ||
        QY265ConfigParse(&cfg, "hdr-sigma-s", "30") || cfg.vpp_hdr_sigma_r != 0) return 3;
    if (all && (QY265ConfigParse(&cfg, "denoise", "2") || QY265ConfigParse(&cfg, "edge", "2"))) return 3;
    int err = 0;
    void *h = QY265EncoderOpen(&cfg, &err);
    if (!h) { fprintf(stderr, "open: %x\n", (unsigned)err); return 4; }
    FILE *fs = fopen(argv[4], "wb");
    if (!fs) return 6;
    const size_t ny = (size_t)W * H, fsz = ny * 3 / 2;
    const int pitch = W + 10;                                          /* the strided pictures: every row ends exactly where its bytes end (the last one with the block) */
    uint8_t *packed = (uint8_t *)malloc(fsz), *sy = (uint8_t *)malloc((size_t)pitch * (H - 1) + W), *su = (uint8_t *)malloc((size_t)(pitch / 2) * (H / 2 - 1) + W / 2),
            *sv = (uint8_t *)malloc((size_t)(pitch / 2) * (H / 2 - 1) + W / 2);
    if (!packed || !sy || !su || !sv) return 7;
    QY265Nal *nal = NULL; int nn = 0;
    QY265Picture out; memset(&out, 0, sizeof out);
    for (int t = 0; t < N; ++t) {
        QY265YUV yuv; memset(&yuv, 0, sizeof yuv);
        QY265Picture pic; memset(&pic, 0, sizeof pic);
        uint8_t *dy = packed, *du = packed + ny, *dv = du + ny / 4; int py = W, pc = W / 2;
        if (t % 3 == 1 && ks265_enc_acquire_input(h, &yuv) == 0) { dy = yuv.pData[0]; du = yuv.pData[1]; dv = yuv.pData[2]; py = yuv.iStride[0]; pc = yuv.iStride[1]; }
        else {
            if (t % 3 == 2) { dy = sy; du = su; dv = sv; py = pitch; pc = pitch / 2; }
            yuv.iWidth = W; yuv.iHeight = H; yuv.pData[0] = dy; yuv.pData[1] = du; yuv.pData[2] = dv; yuv.iStride[0] = py; yuv.iStride[1] = yuv.iStride[2] = pc;
        }
        if (yuv.iWidth != W || yuv.iHeight != H) return 8;
        /* moving edges with a little texture */
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) dy[(size_t)y * py + x] = (uint8_t)(128 + 60 * ((x + 2 * t) / 16 % 2) - 40 * ((y + t) / 8 % 2) + (x * 7 + y * 13 + t * 5) % 5);
        for (int y = 0; y < H / 2; ++y) for (int x = 0; x < W / 2; ++x) { du[(size_t)y * pc + x] = (uint8_t)((x * 5 + t) % 256); dv[(size_t)y * pc + x] = (uint8_t)(255 - (y * 7 + t) % 256); }
        pic.yuv = &yuv; pic.pts = t;
        if (QY265EncoderEncodeFrame(h, &nal, &nn, &pic, &out, 0)) return 9;
        if (put(fs, nal, nn)) return 10;
    }
    while (QY265EncoderDelayedFrames(h) > 0) {
        if (QY265EncoderEncodeFrame(h, &nal, &nn, NULL, &out, 0)) return 11;
        if (put(fs, nal, nn)) return 10;
    }
    ks265_enc_quality q;
    if (ks265_enc_get_quality(h, &q) || q.frames != N) return 12;
    QY265EncoderClose(h);
    fclose(fs);
    free(packed); free(sy); free(su); free(sv);
    StubHdrCall calls[64];
    const int n = ks265_stub_hdr_calls(calls, 64);
    printf("hdr calls %d\n", n);
    if (n != N) return 13;
    for (int t = 0; t < n && t < 64; ++t)
        if (calls[t].w != ((W + 7) & ~7) || calls[t].h != ((H + 7) & ~7) || calls[t].gain != 32 || calls[t].iters != 2 || calls[t].slope != 13 || calls[t].radius[0] != 744 ||
            calls[t].radius[1] != 372 || calls[t].work_no != 0 || !calls[t].work_ok) return 14;
    return 0;
}
