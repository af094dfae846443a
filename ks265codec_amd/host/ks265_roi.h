/* ks265_roi.h - ROI quantiser offset maps in host memory (tests/roi_map_ref.py is the specification): the plain-C reducer of a map to one record per CTU,
 * word for word what ks265_roi_reduce computes on the device, and the rasteriser of the command line's -roi rectangles.  Like ks265_recon.h and ks265_gop.h this header calls
 * nothing: no allocation, no library, no lock - the caller owns every buffer (tests/roi_reduce_main.c drives it alone under the sanitizers). */
#ifndef KS265_ROI_H
#define KS265_ROI_H
#include <stdint.h>
#include <string.h>

#define KS265_ROI_TYPE_INT8 0
#define KS265_ROI_TYPE_FLOAT32 1
#define KS265_ROI_MAX_RECTS 8
#define KS265_ROI_RECT_LOG2 4                  /* the rasteriser's block: 16 x 16 luma samples */

typedef struct { int x, y, w, h, dqp; } ks265_roi_rect;

/* an element's size in bytes; 0: not a type */
static inline int ks265_roi_elem_size(int type) { return type == KS265_ROI_TYPE_INT8 ? 1 : type == KS265_ROI_TYPE_FLOAT32 ? 4 : 0; }
/* the map's size in elements for a width x height picture */
static inline int ks265_roi_map_cols(int width, int log2_block) { return (width + (1 << log2_block) - 1) >> log2_block; }
static inline int ks265_roi_map_rows(int height, int log2_block) { return (height + (1 << log2_block) - 1) >> log2_block; }

/* 0 when (type, log2_block, pitch) describe a map of a width x height picture, else -1: pitch in bytes, at least the row and a multiple of the element size */
static inline int ks265_roi_check(int type, int log2_block, long long pitch, int width, int height)
{
    const int es = ks265_roi_elem_size(type);
    if (!es || log2_block < 0 || log2_block > 6 || width <= 0 || height <= 0) return -1;
    if (pitch < (long long)ks265_roi_map_cols(width, log2_block) * es || pitch % es) return -1;
    return 0;
}

/* int8: clip(v, -51, 51) * 256 */
static inline int32_t ks265_roi_q8_i8(int8_t v) { const int x = v; return (x < -51 ? -51 : x > 51 ? 51 : x) * 256; }
/* float32 by its bits: a non-finite value counts 0; else clip to [-51, 51] and v * 256 rounded to the nearest integer, half to even.  Integer arithmetic on the bit pattern:
 * the result does not depend on the rounding mode of the calling thread or on how the compiler evaluates float expressions */
static inline int32_t ks265_roi_q8_f32(uint32_t bits)
{
    const int e = (int)(bits >> 23 & 255), neg = (int)(bits >> 31);
    if (e == 255) return 0;                                             /* NaN, +-Inf */
    if (e < 127 - 9) return 0;                                          /* |v| < 2^-9: |v * 256| < 0.5 (zeros and denormals too) */
    if (e >= 127 + 6) return neg ? -13056 : 13056;                      /* |v| >= 64 */
    const uint32_t m = (bits & 0x7fffffu) | 0x800000u;                  /* |v| = m * 2^(e - 150), so |v * 256| = m * 2^(e - 142) with e - 142 in [-24, -10] */
    const int sh = 142 - e;
    uint32_t q = m >> sh;
    const uint32_t rem = m & ((1u << sh) - 1), half = 1u << (sh - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    if (q > 13056) q = 13056;
    return neg ? -(int32_t)q : (int32_t)q;
}

/* floor((2 S + cnt) / (2 cnt)) */
static inline int32_t ks265_roi_record(int32_t S, int32_t cnt)
{
    const int32_t num = 2 * S + cnt, den = 2 * cnt;
    int32_t q = num / den;
    if (num % den != 0 && num < 0) --q;
    return q;
}

/* the records of a map in host memory: rec[ceil(width / 64) * ceil(height / 64)], raster order.  data may have any alignment (elements are read bytewise);
 * -1 when ks265_roi_check refuses the description */
static inline int ks265_roi_reduce_host(int type, int log2_block, const void *data, long long pitch, int width, int height, int32_t *rec)
{
    if (!data || !rec || ks265_roi_check(type, log2_block, pitch, width, height)) return -1;
    const int mw = ks265_roi_map_cols(width, log2_block), mh = ks265_roi_map_rows(height, log2_block), n = 64 >> log2_block;
    const int cols = (width + 63) / 64, rows = (height + 63) / 64;
    const unsigned char *base = (const unsigned char *)data;
    for (int cy = 0; cy < rows; ++cy)
        for (int cx = 0; cx < cols; ++cx) {
            const int x0 = cx * n, y0 = cy * n, w = mw - x0 < n ? mw - x0 : n, h = mh - y0 < n ? mh - y0 : n;
            int32_t S = 0;
            for (int r = 0; r < h; ++r) {
                const unsigned char *row = base + (long long)(y0 + r) * pitch;
                if (type == KS265_ROI_TYPE_INT8) {
                    for (int c = 0; c < w; ++c) S += ks265_roi_q8_i8((int8_t)row[x0 + c]);
                } else {
                    for (int c = 0; c < w; ++c) { uint32_t u; memcpy(&u, row + 4 * (long long)(x0 + c), 4); S += ks265_roi_q8_f32(u); }
                }
            }
            rec[cy * cols + cx] = ks265_roi_record(S, w * h);
        }
    return 0;
}

/* the -roi rectangles (luma samples) as an int8 map of 16 x 16 blocks, ceil(width / 16) x ceil(height / 16) elements with `pitch` bytes between rows: a block takes the
 * offset (clipped to [-51, 51]) of the LAST rectangle that covers any of its samples inside the picture, 0 where none does.  -1: more than KS265_ROI_MAX_RECTS, or a bad size */
static inline int ks265_roi_rasterise(const ks265_roi_rect *rect, int nrect, int width, int height, int8_t *map, long long pitch)
{
    if (nrect < 0 || nrect > KS265_ROI_MAX_RECTS || (nrect && !rect) || !map || ks265_roi_check(KS265_ROI_TYPE_INT8, KS265_ROI_RECT_LOG2, pitch, width, height)) return -1;
    const int mw = ks265_roi_map_cols(width, KS265_ROI_RECT_LOG2), mh = ks265_roi_map_rows(height, KS265_ROI_RECT_LOG2);
    for (int r = 0; r < mh; ++r) memset(map + (long long)r * pitch, 0, (size_t)mw);
    for (int i = 0; i < nrect; ++i) {
        const long long x0 = rect[i].x > 0 ? rect[i].x : 0, y0 = rect[i].y > 0 ? rect[i].y : 0;
        long long x1 = (long long)rect[i].x + rect[i].w, y1 = (long long)rect[i].y + rect[i].h;
        if (x1 > width) x1 = width;
        if (y1 > height) y1 = height;
        if (x1 <= x0 || y1 <= y0) continue;
        const int d = rect[i].dqp < -51 ? -51 : rect[i].dqp > 51 ? 51 : rect[i].dqp;
        for (long long by = y0 >> 4; by <= (y1 - 1) >> 4; ++by) memset(map + by * pitch + (x0 >> 4), d, (size_t)(((x1 - 1) >> 4) - (x0 >> 4) + 1));
    }
    return 0;
}

#endif
