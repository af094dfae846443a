/* TEST INFRASTRUCTURE: overlays through the host and the stand-in tests/hip_stub_overlay.c in a program of its own, for a build with -fsanitize=address,undefined
 * (tests/test_overlay_host_cpu.py): open, run the script below over the N >= 6 pictures of CLIP, flush, close.
 *   overlay_main WIDTH HEIGHT N CLIP STREAM_FILE SLOTS_FILE LATENCY LOGO LW LH
 *     CLIP        N packed I420 pictures of WIDTH x HEIGHT;  LOGO: LW x LH pixels of R G B A bytes;  LATENCY: zerolatency | default
 *     SLOTS_FILE  the stand-in appends every input slot as its overlay call leaves it (ks265_stub_overlay_dump): what the encoder codes
 * The script (tests/test_overlay_host_cpu.py mirrors it with tests/overlay_ref.py):
 *   before picture 0   slot 0 = LOGO from host memory as RGBA at (8, 4), opacity 256 - and the buffer it came from is written over at once;
 *                      slot 5 = LOGO in "device" memory read as BGRA at (WIDTH - LW + 6, HEIGHT - LH + 2), opacity 128, BT.601 full range, KS265_OV_FORCED_ONLY
 *   before picture 2   slot 0 = LOGO from host memory without its alpha (pixel_step 4) at (-4, -2), opacity 200
 *   before picture 4   slot 0 cleared; slot 1 = LOGO from host memory as RGBA at (40, 20), never cleared: the close frees it
 *   picture t          handed in with bForceLogo = t & 1
 * Refusals along the way leave the slots as they are.  Exit status 0 = every call did what it should and nothing of the stand-in's is alive behind the close. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ks265_enc.h"

long ks265_stub_live(int kind);
void ks265_stub_overlay_dump(const char *path);

static int put(FILE *f, QY265Nal *nal, int n) { for (int i = 0; i < n; ++i) if (nal[i].iSize > 0 && fwrite(nal[i].pPayload, 1, (size_t)nal[i].iSize, f) != (size_t)nal[i].iSize) return 1; return 0; }

static ks265_overlay rgba(const uint8_t *p, int lw, int lh, int device, int bgr, int alpha, int x, int y, int opacity)
{
    ks265_overlay o; memset(&o, 0, sizeof o);
    o.rgb.format = KS265_IN_RGB; o.rgb.device = device; o.rgb.pixel_step = 4; o.rgb.pitch[0] = 4 * lw;
    o.rgb.plane[0] = p + (bgr ? 2 : 0); o.rgb.plane[1] = p + 1; o.rgb.plane[2] = p + (bgr ? 0 : 2);
    o.width = lw; o.height = lh; o.alpha = alpha ? p + 3 : NULL; o.x = x; o.y = y; o.opacity = opacity;
    return o;
}

int main(int argc, char **argv)
{
    if (argc != 11) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), N = atoi(argv[3]), LW = atoi(argv[9]), LH = atoi(argv[10]);
    const size_t fsz = (size_t)W * H * 3 / 2, lsz = (size_t)LW * LH * 4;
    uint8_t *clip = (uint8_t *)malloc(fsz * (size_t)N), *logo = (uint8_t *)malloc(lsz), *tmp = (uint8_t *)malloc(lsz);
    if (N < 6 || !clip || !logo || !tmp) return 2;
    FILE *f = fopen(argv[4], "rb");
    if (!f || fread(clip, 1, fsz * (size_t)N, f) != fsz * (size_t)N) return 2;
    fclose(f);
    f = fopen(argv[8], "rb");
    if (!f || fread(logo, 1, lsz, f) != lsz) return 2;
    fclose(f);
    char preset[] = "medium", tune[] = "default";
    QY265EncConfig cfg;
    if (QY265ConfigDefaultPreset(&cfg, preset, tune, argv[7])) return 3;
    cfg.picWidth = W; cfg.picHeight = H; cfg.frameRate = 50; cfg.rc = 0; cfg.qp = 34; cfg.threads = 2; cfg.logLevel = 1;
    int err = 0;
    void *h = QY265EncoderOpen(&cfg, &err);
    if (!h) { fprintf(stderr, "open: %x\n", (unsigned)err); return 4; }
    ks265_stub_overlay_dump(argv[6]);
    FILE *fs = fopen(argv[5], "wb");
    if (!fs) return 6;
    QY265Nal *nal = NULL; int nn = 0;
    QY265Picture out; memset(&out, 0, sizeof out);
    ks265_overlay o;
    for (int t = 0; t < N; ++t) {
        if (t == 0) {
            memcpy(tmp, logo, lsz);
            o = rgba(tmp, LW, LH, -1, 0, 1, 8, 4, 256);
            if (ks265_enc_set_overlay(h, 0, &o)) return 20;
            memset(tmp, 0x77, lsz);                                     /* the host buffer is the caller's again */
            o = rgba(logo, LW, LH, 0, 1, 1, W - LW + 6, H - LH + 2, 128);
            o.rgb.matrix = KS265_MATRIX_BT601; o.rgb.full_range = 1; o.flags = KS265_OV_FORCED_ONLY;
            if (ks265_enc_set_overlay(h, 5, &o)) return 21;
            /* refusals: the slots keep what they have */
            o = rgba(logo, LW, LH, 0, 0, 1, 9, 4, 256);
            if (ks265_enc_set_overlay(h, 0, &o) != QY_NOTSUPPORTED) return 22;      /* an odd x */
            o = rgba(logo, LW, LH, 0, 0, 1, 8, 4, 257);
            if (ks265_enc_set_overlay(h, 5, &o) != QY_NOTSUPPORTED) return 23;      /* opacity */
            o = rgba(logo, LW, LH, 0, 0, 1, 8, 4, 256);
            if (ks265_enc_set_overlay(h, 8, &o) != QY_NOTSUPPORTED || ks265_enc_set_overlay(h, -1, NULL) != QY_NOTSUPPORTED) return 24;   /* the slot */
            o.rgb.plane[1] = NULL;
            if (ks265_enc_set_overlay(h, 0, &o) != QY_POINTER || ks265_enc_set_overlay(NULL, 0, NULL) != QY_POINTER) return 25;
        }
        if (t == 2) {
            memcpy(tmp, logo, lsz);
            o = rgba(tmp, LW, LH, -1, 0, 0, -4, -2, 200);
            if (ks265_enc_set_overlay(h, 0, &o)) return 26;
            memset(tmp, 0x11, lsz);
        }
        if (t == 4) {
            if (ks265_enc_set_overlay(h, 0, NULL) || ks265_enc_set_overlay(h, 3, NULL)) return 27;   /* (an empty slot clears to nothing) */
            memcpy(tmp, logo, lsz);
            o = rgba(tmp, LW, LH, -1, 0, 1, 40, 20, 256);
            if (ks265_enc_set_overlay(h, 1, &o)) return 28;
            memset(tmp, 0xEE, lsz);
        }
        QY265YUV yuv; memset(&yuv, 0, sizeof yuv);
        QY265Picture pic; memset(&pic, 0, sizeof pic);
        uint8_t *p = clip + fsz * (size_t)t;
        yuv.iWidth = W; yuv.iHeight = H; yuv.pData[0] = p; yuv.pData[1] = p + (size_t)W * H; yuv.pData[2] = p + (size_t)W * H * 5 / 4;
        yuv.iStride[0] = W; yuv.iStride[1] = yuv.iStride[2] = W / 2;
        pic.yuv = &yuv; pic.pts = t;
        if (QY265EncoderEncodeFrame(h, &nal, &nn, &pic, &out, t & 1)) return 9;
        if (put(fs, nal, nn)) return 10;
    }
    while (QY265EncoderDelayedFrames(h) > 0) {
        if (QY265EncoderEncodeFrame(h, &nal, &nn, NULL, &out, 1)) return 11;
        if (put(fs, nal, nn)) return 10;
    }
    QY265EncoderClose(h);
    ks265_stub_overlay_dump(NULL);
    fclose(fs);
    free(clip); free(logo); free(tmp);
    for (int k = 0; k < 5; ++k) if (ks265_stub_live(k)) { fprintf(stderr, "alive behind the close: kind %d, %ld\n", k, ks265_stub_live(k)); return 13; }
    return 0;
}
