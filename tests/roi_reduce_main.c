/* roi_reduce_main.c - ks265codec_amd/host/ks265_roi.h driven alone (tests/test_roi_host_cpu.py builds this with -fsanitize=address,undefined and runs it as a child process).
 *   roi_reduce_main reduce TYPE LOG2 WIDTH HEIGHT PITCH OFFSET IN OUT
 *       IN holds exactly OFFSET + PITCH * (rows - 1) + row bytes: the map starts OFFSET bytes into a heap block of exactly that size, so a read past either end of the
 *       map's extent is a sanitizer report.  OUT receives the records, int32 each.
 *   roi_reduce_main raster WIDTH HEIGHT PITCH OUT X:Y:W:H:DQP ...
 *       OUT receives the map's rows without the pitch; the bytes behind every row are checked to be untouched. */
#include <stdio.h>
#include <stdlib.h>
#include "ks265_roi.h"

static int fail(const char *what) { fprintf(stderr, "roi_reduce_main: %s\n", what); return 2; }

int main(int argc, char **argv)
{
    if (argc >= 10 && !strcmp(argv[1], "reduce")) {
        const int type = atoi(argv[2]), lb = atoi(argv[3]), W = atoi(argv[4]), H = atoi(argv[5]);
        const long long pitch = atoll(argv[6]), off = atoll(argv[7]);
        if (ks265_roi_check(type, lb, pitch, W, H)) { printf("refused\n"); return 0; }
        const long long ext = off + pitch * (ks265_roi_map_rows(H, lb) - 1) + (long long)ks265_roi_map_cols(W, lb) * ks265_roi_elem_size(type);
        unsigned char *buf = malloc((size_t)ext);
        FILE *f = fopen(argv[8], "rb");
        if (!buf || !f || fread(buf, 1, (size_t)ext, f) != (size_t)ext || fgetc(f) != EOF) return fail("input file");
        fclose(f);
        const int n = ((W + 63) / 64) * ((H + 63) / 64);
        int32_t *rec = malloc((size_t)n * sizeof *rec);
        if (!rec || ks265_roi_reduce_host(type, lb, buf + off, pitch, W, H, rec)) return fail("reduce");
        f = fopen(argv[9], "wb");
        if (!f || fwrite(rec, sizeof *rec, (size_t)n, f) != (size_t)n || fclose(f)) return fail("output file");
        free(rec); free(buf);
        printf("ok %d\n", n);
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "raster")) {
        const int W = atoi(argv[2]), H = atoi(argv[3]);
        const long long pitch = atoll(argv[4]);
        ks265_roi_rect rect[KS265_ROI_MAX_RECTS + 1];
        int nrect = 0;
        for (int i = 6; i < argc; ++i) {
            if (nrect > KS265_ROI_MAX_RECTS) break;
            ks265_roi_rect *r = &rect[nrect++];
            if (sscanf(argv[i], "%d:%d:%d:%d:%d", &r->x, &r->y, &r->w, &r->h, &r->dqp) != 5) return fail("rectangle");
        }
        if (ks265_roi_check(KS265_ROI_TYPE_INT8, KS265_ROI_RECT_LOG2, pitch, W, H)) { printf("refused\n"); return 0; }
        const int mw = ks265_roi_map_cols(W, KS265_ROI_RECT_LOG2), mh = ks265_roi_map_rows(H, KS265_ROI_RECT_LOG2);
        const size_t ext = (size_t)(pitch * (mh - 1) + mw);                /* the last row has nothing behind it */
        int8_t *map = malloc(ext);
        if (!map) return fail("memory");
        memset(map, 0x5a, ext);
        if (ks265_roi_rasterise(rect, nrect, W, H, map, pitch)) { printf("refused\n"); free(map); return 0; }
        FILE *f = fopen(argv[5], "wb");
        if (!f) return fail("output file");
        for (int r = 0; r < mh; ++r) {
            if (fwrite(map + r * pitch, 1, (size_t)mw, f) != (size_t)mw) return fail("output file");
            for (long long c = mw; r < mh - 1 && c < pitch; ++c) if (map[r * pitch + c] != 0x5a) return fail("a byte behind a row was written");
        }
        if (fclose(f)) return fail("output file");
        free(map);
        printf("ok %d\n", mw * mh);
        return 0;
    }
    return fail("usage");
}
