/* TEST INFRASTRUCTURE: the two conversion routines of tests/hip_stub_float.c in a program of their own, for a build with -fsanitize=address,undefined
 * (tests/test_float_io_host_cpu.py): every buffer is allocated at exactly its extent, so that a byte read or written outside a row's bytes is a report.
 *   float_stub_main in  FORMAT W H STEP PITCH OFF_R OFF_G OFF_B MATRIX FULL SRC_FILE DST_FILE        the samples in SRC_FILE -> packed I420 in DST_FILE
 *   float_stub_main out FORMAT W H STEP PITCH OFF_R OFF_G OFF_B MATRIX FULL SRC_FILE DST_FILE BYTES ONE_OFF   packed I420 -> a destination of BYTES bytes (0xA5 before) */
#define KS265_STUB_FLOAT_ROUTINES_ONLY
#include "hip_stub_float.c"
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
    if (argc < 14) return 2;
    const int out = argv[1][0] == 'o', format = atoi(argv[2]), W = atoi(argv[3]), H = atoi(argv[4]), step = atoi(argv[5]), matrix = atoi(argv[10]), full = atoi(argv[11]);
    const long long pitch = atoll(argv[6]), off[3] = {atoll(argv[7]), atoll(argv[8]), atoll(argv[9])};
    size_t n = 0;
    uint8_t *src = slurp(argv[12], &n), *dst;
    if (!src) return 3;
    size_t dn = (size_t)W * H * 3 / 2;
    if (!out) {
        const uint8_t *ch[3] = {src + off[0], src + off[1], src + off[2]};
        if (!(dst = (uint8_t *)malloc(dn))) return 4;
        stub_float_to_i420(format, ch, pitch, step, W, H, matrix, full, dst);
    } else {
        if (argc < 16 || n != dn) return 2;
        dn = (size_t)atoll(argv[14]);
        const long long one = atoll(argv[15]);
        if (!(dst = (uint8_t *)malloc(dn))) return 4;
        memset(dst, 0xA5, dn);
        uint8_t *ch[3] = {dst + off[0], dst + off[1], dst + off[2]};
        stub_i420_to_rgb(format, src, ch, one < 0 ? NULL : dst + one, pitch, step, W, H, matrix, full);
    }
    FILE *f = fopen(argv[13], "wb");
    if (!f || fwrite(dst, 1, dn, f) != dn) return 5;
    fclose(f);
    free(dst); free(src);
    return 0;
}
