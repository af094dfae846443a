/* TEST INFRASTRUCTURE: the scaler's table builder (ks265codec_amd/host/ks265_scale.h) alone, as a program of its own that tests/test_scale_plan_cpu.py builds with
 * -fsanitize=address,undefined and runs: every table sits in a heap block of exactly its extent, so a write past a table is a sanitizer report.
 *   scale_plan_main axis OUT S D filter cosited [S D filter cosited ...]   per axis: "axis S D filter cosited T" + D int32 first + D * T int16 coefficients (binary, appended to OUT), or
 *                                                              "refused S D filter cosited" on stdout
 *   scale_plan_main size sw sh dw dh                       prints "ok" or "refused" after the size rules
 *   scale_plan_main plane OUT sw sh dw dh filter cosited_x IN    one plane through ks265_scale_plane_host (IN: sw * sh bytes; OUT: dw * dh) */
#include "ks265_scale.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
    if (argc >= 6 && !strcmp(argv[1], "size")) {
        puts(ks265_scale_size_ok(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])) ? "ok" : "refused");
        return 0;
    }
    if (argc >= 7 && !strcmp(argv[1], "axis")) {
        FILE *fp = fopen(argv[2], "wb");
        if (!fp) return 2;
        for (int i = 3; i + 3 < argc; i += 4) {
            const int S = atoi(argv[i]), D = atoi(argv[i + 1]), filter = atoi(argv[i + 2]), cos = atoi(argv[i + 3]);
            const int T = ks265_scale_axis_taps(S, D, filter, cos);
            if (!T) { printf("refused %d %d %d %d\n", S, D, filter, cos); continue; }
            int32_t *first = (int32_t *)malloc((size_t)D * sizeof *first);
            int16_t *coef = (int16_t *)malloc((size_t)D * T * sizeof *coef);
            if (!first || !coef) return 2;
            if (ks265_scale_axis_fill(S, D, filter, cos, T, first, coef)) printf("refused %d %d %d %d\n", S, D, filter, cos);
            else {
                printf("axis %d %d %d %d %d\n", S, D, filter, cos, T);
                if (fwrite(first, sizeof *first, (size_t)D, fp) != (size_t)D || fwrite(coef, sizeof *coef, (size_t)D * T, fp) != (size_t)D * T) return 2;
            }
            free(first); free(coef);
        }
        return fclose(fp) ? 2 : 0;
    }
    if (argc == 10 && !strcmp(argv[1], "plane")) {
        const int sw = atoi(argv[3]), sh = atoi(argv[4]), dw = atoi(argv[5]), dh = atoi(argv[6]), filter = atoi(argv[7]), cos = atoi(argv[8]);
        const int Tx = ks265_scale_axis_taps(sw, dw, filter, cos), Ty = ks265_scale_axis_taps(sh, dh, filter, 0);
        if (!Tx || !Ty) { puts("refused"); return 0; }
        uint8_t *src = (uint8_t *)malloc((size_t)sw * sh), *dst = (uint8_t *)malloc((size_t)dw * dh);
        int32_t *fx = (int32_t *)malloc((size_t)dw * 4), *fy = (int32_t *)malloc((size_t)dh * 4);
        int16_t *cx = (int16_t *)malloc((size_t)dw * Tx * 2), *cy = (int16_t *)malloc((size_t)dh * Ty * 2), *tmp = (int16_t *)malloc((size_t)sh * dw * 2);
        FILE *in = fopen(argv[9], "rb");
        if (!src || !dst || !fx || !fy || !cx || !cy || !tmp || !in || fread(src, 1, (size_t)sw * sh, in) != (size_t)sw * sh) return 2;
        fclose(in);
        if (ks265_scale_axis_fill(sw, dw, filter, cos, Tx, fx, cx) || ks265_scale_axis_fill(sh, dh, filter, 0, Ty, fy, cy)) { puts("refused"); return 0; }
        ks265_scale_plane_host(src, sw, 1, sw, sh, dst, dw, dh, fx, cx, Tx, fy, cy, Ty, tmp);
        FILE *out = fopen(argv[2], "wb");
        if (!out || fwrite(dst, 1, (size_t)dw * dh, out) != (size_t)dw * dh || fclose(out)) return 2;
        free(src); free(dst); free(fx); free(fy); free(cx); free(cy); free(tmp);
        puts("ok");
        return 0;
    }
    fprintf(stderr, "usage: scale_plan_main axis|size|plane ...\n");
    return 2;
}
