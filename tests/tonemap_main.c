/* TEST INFRASTRUCTURE: a program of its own around the stand-in's tone-mapping routine (tests/hip_stub_tonemap.c, -DKS265_STUB_TONEMAP_ROUTINES_ONLY) and the host's table
 * builder (ks265codec_amd/host/ks265_tonemap.h), built with -fsanitize=address,undefined and run as it is (tests/test_tonemap_host_cpu.py, tests/test_tonemap_ref_cpu.py).
 *   tonemap_main layout depth msb full_range curve peak white W H behind in out tables
 * `in` holds the stored elements of the planes one after another, rows packed.  Every plane goes into a heap block of its own with `behind` elements behind every row but
 * the last - the block ends with the last row's last element, so a read past a row's end in the last row, or in front of a plane, is the sanitizer's.  `out` gets the packed
 * I420 picture (from a block of exactly W x H x 3 / 2 bytes); `tables` gets E (uint32[4096]), G (uint16[4096]), O (uint16[4097]) and M (int32[9]) as the builder made them. */
#define KS265_STUB_TONEMAP_ROUTINES_ONLY
#include "hip_stub_tonemap.c"
#include <stdio.h>

int main(int argc, char **argv)
{
    if (argc != 14) { fprintf(stderr, "usage: %s layout depth msb full_range curve peak white W H behind in out tables\n", argv[0]); return 2; }
    const int layout = atoi(argv[1]), depth = atoi(argv[2]), msb = atoi(argv[3]), full = atoi(argv[4]), curve = atoi(argv[5]);
    const double peak = atof(argv[6]), white = atof(argv[7]);
    const int W = atoi(argv[8]), H = atoi(argv[9]), behind = atoi(argv[10]);
    if (!ks265_tm_cfg_ok(KS_TM_TRANSFER_PQ, curve, peak, white) || !ks265_tm_format_ok(layout, 0, depth) || W <= 0 || H <= 0 || (W & 1) || (H & 1) || behind < 0) return 2;
    ks265_tm_tables *t = (ks265_tm_tables *)malloc(sizeof *t);
    if (!t) return 1;
    ks265_tm_tables_fill(curve, peak, white, t);
    FILE *f = fopen(argv[13], "wb");
    if (!f || fwrite(t->E, 4, 4096, f) != 4096 || fwrite(t->G, 2, 4096, f) != 4096 || fwrite(t->O, 2, 4097, f) != 4097 || fwrite(t->M, 4, 9, f) != 9 || fclose(f)) return 1;
    const int np = layout ? 2 : 3;
    uint8_t *block[3] = {NULL, NULL, NULL};
    const uint8_t *plane[3] = {NULL, NULL, NULL};
    long long pitch[3] = {0, 0, 0};
    f = fopen(argv[11], "rb");
    if (!f) return 1;
    for (int k = 0; k < np; ++k) {
        const int rows = k ? H / 2 : H, n = k == 0 || layout ? W : W / 2;
        pitch[k] = (long long)(n + behind) * 2;
        block[k] = (uint8_t *)malloc((size_t)(rows - 1) * (size_t)pitch[k] + (size_t)n * 2);
        if (!block[k]) return 1;
        for (int r = 0; r < rows; ++r) {
            if (fread(block[k] + (size_t)r * (size_t)pitch[k], 2, (size_t)n, f) != (size_t)n) return 1;
            if (r + 1 < rows) memset(block[k] + (size_t)r * (size_t)pitch[k] + (size_t)n * 2, 0xEE, (size_t)behind * 2);
        }
        plane[k] = block[k];
    }
    fclose(f);
    uint8_t *dst = (uint8_t *)malloc((size_t)W * H * 3 / 2);
    if (!dst || stub_tonemap_to_i420(t, layout, depth, msb, full, plane, pitch, W, H, dst)) return 1;
    f = fopen(argv[12], "wb");
    if (!f || fwrite(dst, 1, (size_t)W * H * 3 / 2, f) != (size_t)W * H * 3 / 2 || fclose(f)) return 1;
    free(dst); free(t);
    for (int k = 0; k < np; ++k) free(block[k]);
    return 0;
}
