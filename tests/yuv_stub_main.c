/* TEST INFRASTRUCTURE: the conversion routine of tests/hip_stub_yuv.c in a program of its own, for a build with -fsanitize=address,undefined
 * (tests/test_yuv_in_host_cpu.py): every plane is a file read into a block of exactly its size, so that a byte read outside a row's bytes is a report.
 *   yuv_stub_main LAYOUT SUB DEPTH MSB W H DST_FILE  PLANE_FILE OFF PITCH  [PLANE_FILE OFF PITCH [PLANE_FILE OFF PITCH]]      the planes -> packed I420 in DST_FILE */
#define KS265_STUB_YUV_ROUTINES_ONLY
#include "hip_stub_yuv.c"
#include <stdio.h>
#include <stdlib.h>

static uint8_t *slurp(const char *path, size_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *p = (uint8_t *)malloc(*n ? *n : 1);
    if (p && fread(p, 1, *n, f) != *n) { free(p); p = NULL; }
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 11 || (argc - 8) % 3) return 2;
    const int layout = atoi(argv[1]), sub = atoi(argv[2]), depth = atoi(argv[3]), msb = atoi(argv[4]), W = atoi(argv[5]), H = atoi(argv[6]);
    const int np = (argc - 8) / 3;
    if (np != (layout == 0 ? 3 : layout == 1 ? 2 : 1)) return 2;
    uint8_t *buf[3] = {NULL, NULL, NULL};
    const uint8_t *plane[3] = {NULL, NULL, NULL};
    long long pitch[3] = {0, 0, 0};
    for (int k = 0; k < np; ++k) {
        size_t n = 0;
        if (!(buf[k] = slurp(argv[8 + 3 * k], &n))) return 3;
        plane[k] = buf[k] + atoll(argv[9 + 3 * k]);
        pitch[k] = atoll(argv[10 + 3 * k]);
    }
    const size_t dn = (size_t)W * H * 3 / 2;
    uint8_t *dst = (uint8_t *)malloc(dn);
    if (!dst) return 4;
    stub_yuv_to_i420(layout, sub, depth, msb, plane, pitch, W, H, dst);
    FILE *f = fopen(argv[7], "wb");
    if (!f || fwrite(dst, 1, dn, f) != dn) return 5;
    fclose(f);
    free(dst);
    for (int k = 0; k < np; ++k) free(buf[k]);
    return 0;
}
