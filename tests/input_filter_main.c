/* TEST INFRASTRUCTURE: a handle with filters on the way in at a size that is no multiple of 8, in a program of its own, for a build with -fsanitize=address,undefined against
 * the host sources and a stand-in of the chain tests/hip_stub_window.c .. tests/hip_stub_hdr.c (tests/test_window_host_cpu.py, test_denoise_host_cpu.py,
 * test_enhance_host_cpu.py, test_hdr_host_cpu.py): open, encode N pictures - every third one through an acquired slot, every third one strided - flush, close.
 *   input_filter_main WIDTH HEIGHT N STREAM_FILE LATENCY [name=value ...]    LATENCY: zerolatency | default.  Every name=value goes through QY265ConfigParse, but
 *                                                                            recon=FILE: the reconstruction is dumped there (ks265_enc_set_recon_file).
 * Exit status 0 = every call succeeded and nothing of the stand-in's is alive behind the close.  Then one line per call the stand-in recorded, every field as name=value:
 * `pad ..`, `denoise ..`, `enhance ..`, `hdr ..` - the readers are weak, a stand-in further up the chain prints fewer kinds.  What the records must be is the tests' business. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ks265_enc.h"

typedef struct { int32_t format, w, h, cw, ch, pitch[3]; } StubPadCall;
typedef struct { int32_t w, h, thr, weight, has_hist, hist_in, hist_out; } StubDnCall;
typedef struct { int32_t w, h, edge_gain, edge_core, edge_limit, edge_over, color_gain, has_src, src_is_hist; } StubEnCall;
typedef struct { int32_t w, h, gain, iters, slope, radius[3], work_no, work_ok; } StubHdrCall;
long ks265_stub_live(int kind);                                       /* contexts, frame objects, events, device and pinned blocks alive */
__attribute__((weak)) int ks265_stub_pad_calls(StubPadCall *out, int cap);
__attribute__((weak)) int ks265_stub_denoise_calls(StubDnCall *out, int cap);
__attribute__((weak)) int ks265_stub_enhance_calls(StubEnCall *out, int cap);
__attribute__((weak)) int ks265_stub_hdr_calls(StubHdrCall *out, int cap);

static int put(FILE *f, QY265Nal *nal, int n) { for (int i = 0; i < n; ++i) if (nal[i].iSize > 0 && fwrite(nal[i].pPayload, 1, (size_t)nal[i].iSize, f) != (size_t)nal[i].iSize) return 1; return 0; }

#define CAP 64
static void print_calls(void)
{
    static StubPadCall pad[CAP]; static StubDnCall dn[CAP]; static StubEnCall en[CAP]; static StubHdrCall hdr[CAP];
    int n = ks265_stub_pad_calls ? ks265_stub_pad_calls(pad, CAP) : 0;
    for (int t = 0; t < n && t < CAP; ++t)
        printf("pad format=%d w=%d h=%d cw=%d ch=%d pitch0=%d pitch1=%d pitch2=%d\n", pad[t].format, pad[t].w, pad[t].h, pad[t].cw, pad[t].ch, pad[t].pitch[0], pad[t].pitch[1], pad[t].pitch[2]);
    n = ks265_stub_denoise_calls ? ks265_stub_denoise_calls(dn, CAP) : 0;
    for (int t = 0; t < n && t < CAP; ++t)
        printf("denoise w=%d h=%d thr=%d weight=%d has_hist=%d hist_in=%d hist_out=%d\n", dn[t].w, dn[t].h, dn[t].thr, dn[t].weight, dn[t].has_hist, dn[t].hist_in, dn[t].hist_out);
    n = ks265_stub_enhance_calls ? ks265_stub_enhance_calls(en, CAP) : 0;
    for (int t = 0; t < n && t < CAP; ++t)
        printf("enhance w=%d h=%d edge_gain=%d edge_core=%d edge_limit=%d edge_over=%d color_gain=%d has_src=%d src_is_hist=%d\n", en[t].w, en[t].h, en[t].edge_gain, en[t].edge_core,
               en[t].edge_limit, en[t].edge_over, en[t].color_gain, en[t].has_src, en[t].src_is_hist);
    n = ks265_stub_hdr_calls ? ks265_stub_hdr_calls(hdr, CAP) : 0;
    for (int t = 0; t < n && t < CAP; ++t)
        printf("hdr w=%d h=%d gain=%d iters=%d slope=%d radius0=%d radius1=%d radius2=%d work_no=%d work_ok=%d\n", hdr[t].w, hdr[t].h, hdr[t].gain, hdr[t].iters, hdr[t].slope,
               hdr[t].radius[0], hdr[t].radius[1], hdr[t].radius[2], hdr[t].work_no, hdr[t].work_ok);
}

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), N = atoi(argv[3]);
    const char *recon = NULL;
    char preset[] = "medium", tune[] = "default";
    QY265EncConfig cfg;
    if (QY265ConfigDefaultPreset(&cfg, preset, tune, argv[5])) return 3;
    cfg.picWidth = W; cfg.picHeight = H; cfg.frameRate = 50; cfg.rc = 0; cfg.qp = 34; cfg.threads = 2; cfg.logLevel = 1; cfg.calcPsnr = 1;
    for (int a = 6; a < argc; ++a) {
        char *eq = strchr(argv[a], '=');
        if (!eq) return 2;
        *eq = 0;
        if (!strcmp(argv[a], "recon")) recon = eq + 1;
        else if (QY265ConfigParse(&cfg, argv[a], eq + 1)) return 3;
    }
    int err = 0;
    void *h = QY265EncoderOpen(&cfg, &err);
    if (!h) { fprintf(stderr, "open: %x\n", (unsigned)err); return 4; }
    if (recon && ks265_enc_set_recon_file(h, recon)) return 5;
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
        /* moving edges with a little texture: blocks that follow the motion and blocks that do not; chroma over its whole range */
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
    for (int k = 0; k < 5; ++k) if (ks265_stub_live(k)) { fprintf(stderr, "alive behind the close: kind %d, %ld\n", k, ks265_stub_live(k)); return 13; }
    print_calls();
    return 0;
}
