// input_yuv.hip — the YUV family of the device input (include/ks265_hip.h KS265_IN_YUV(layout, sub, depth, msb)): 8- to 16-bit 4:2:0 / 4:2:2 / 4:4:4 pictures, planar,
// semi-planar or packed, reduced to the packed 8-bit I420 of the encoder's input slots.  tests/yuv_hibit_ref.py is the specification: luma rounded to 8 bits, chroma summed at
// full depth - 4:2:2 by (1, 1) vertically, 4:4:4 by (1, 2, 1) x (1, 1) with the left edge clamped - and rounded ONCE with the depth reduction, ties up, clipped to 255; no
// dither, no range or matrix conversion.  Memory-bound, on convert_dev.h's cell: one thread owns 8 luma columns across the two rows of one chroma row, every chroma sample is
// made from registers (no LDS, no scratch: every register array is indexed by unrolled constants).  A run is loaded as exactly its own bytes (convert_dev.h load_run), so no load
// leaves [row start, row start + row bytes); the stores are aligned words (width a multiple of 8, the destination on 16 bytes).  Templates: (layout shape, subsampling, element size); depth, alignment and the packed byte order are arguments.
#include "convert_dev.h"

namespace {

struct YuvArgs {
    const uint8_t *p[3];          // planar: Y, U, V; semi-planar: Y, UV; packed: the one plane
    long long pitch[3];
    int W, H;
    int nsh, mask;                // the sample of a stored element w: (w >> nsh) & mask
    int s, rl, rc;                // s = depth - 8; the rounding terms of luma (shift s) and chroma (shift s + t)
    int uyvy;                     // packed: U Y0 V Y1 instead of Y0 U Y1 V
    uint8_t *dst;
};

enum { SH_PLANAR = 0, SH_SEMI = 1, SH_PACKED = 2 };

template <int ES> __device__ inline uint32_t one_elem(const uint8_t *p) { return ES == 2 ? (uint32_t)*(const uint16_t *)p : (uint32_t)*p; }
// the sample of a stored element
template <int ES> __device__ inline uint32_t norm(const YuvArgs &a, uint32_t w) { return ES == 1 ? w : (w >> a.nsh) & (uint32_t)a.mask; }

// SHAPE x SUB x ES: 8 luma columns x the two rows of chroma row i -> 16 Y, 4 Cb, 4 Cr
template <int SHAPE, int SUB, int ES> __global__ __launch_bounds__(256) void yuvx_to_i420_kernel(YuvArgs a)
{
    int x0, i;
    if (!ks_cell<8>(a.W, a.H, x0, i)) return;
    constexpr int T = SUB == 0 ? 0 : SUB == 1 ? 1 : 3;                 // log2 of the chroma filter's weight
    uint32_t su[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const long long y = 2 * i + dy;
        uint32_t yw[2] = {0, 0};
        if constexpr (SHAPE == SH_PACKED) {                            // 16 elements: four pixel pairs; after the swap Y0 U Y1 V
            uint32_t w[4 * ES];
            load_run<16 * ES, ES>(a.p[0] + y * a.pitch[0] + (long long)x0 * (2 * ES), w);
            if (a.uyvy) {
#pragma unroll
                for (int k = 0; k < 4 * ES; ++k) w[k] = ES == 2 ? (w[k] << 16 | w[k] >> 16) : ((w[k] & 0x00ff00ffu) << 8 | (w[k] >> 8 & 0x00ff00ffu));
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) yw[k >> 2] |= shr_clip255<uint32_t>(norm<ES>(a, run_elem<ES>(w, 2 * k)) + a.rl, a.s) << 8 * (k & 3);
#pragma unroll
            for (int k = 0; k < 4; ++k) { su[k] += norm<ES>(a, run_elem<ES>(w, 4 * k + 1)); sv[k] += norm<ES>(a, run_elem<ES>(w, 4 * k + 3)); }
        } else {
            uint32_t w[2 * ES];
            load_run<8 * ES, ES>(a.p[0] + y * a.pitch[0] + (long long)x0 * ES, w);
            if constexpr (ES == 1) { yw[0] = w[0]; yw[1] = w[1]; }
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) yw[k >> 2] |= shr_clip255<uint32_t>(norm<ES>(a, run_elem<ES>(w, k)) + a.rl, a.s) << 8 * (k & 3);
            }
            if (SUB != 0 || dy == 0) {                                  // 4:2:0: the one chroma row i
                const long long cy = SUB == 0 ? i : y;
                if constexpr (SHAPE == SH_PLANAR && SUB != 2) {         // 4 samples of each plane
                    uint32_t cu[ES], cv[ES];
                    load_run<4 * ES, ES>(a.p[1] + cy * a.pitch[1] + (long long)(x0 / 2) * ES, cu);
                    load_run<4 * ES, ES>(a.p[2] + cy * a.pitch[2] + (long long)(x0 / 2) * ES, cv);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { su[k] += norm<ES>(a, run_elem<ES>(cu, k)); sv[k] += norm<ES>(a, run_elem<ES>(cv, k)); }
                } else if constexpr (SHAPE == SH_SEMI && SUB != 2) {    // 4 pairs U, V
                    uint32_t c[2 * ES];
                    load_run<8 * ES, ES>(a.p[1] + cy * a.pitch[1] + (long long)x0 * ES, c);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { su[k] += norm<ES>(a, run_elem<ES>(c, 2 * k)); sv[k] += norm<ES>(a, run_elem<ES>(c, 2 * k + 1)); }
                } else {                                                // 4:4:4: columns x0 - 1 (clamped to 0) .. x0 + 7 as entries 0 .. 8, (1, 2, 1) at the even columns
                    const long long xl = x0 > 0 ? x0 - 1 : 0;
                    uint32_t eu[9], ev[9];
                    if constexpr (SHAPE == SH_PLANAR) {
                        uint32_t cu[2 * ES], cv[2 * ES];
                        const uint8_t *ru = a.p[1] + cy * a.pitch[1], *rv = a.p[2] + cy * a.pitch[2];
                        eu[0] = norm<ES>(a, one_elem<ES>(ru + xl * ES)); ev[0] = norm<ES>(a, one_elem<ES>(rv + xl * ES));
                        load_run<8 * ES, ES>(ru + (long long)x0 * ES, cu);
                        load_run<8 * ES, ES>(rv + (long long)x0 * ES, cv);
#pragma unroll
                        for (int k = 0; k < 8; ++k) { eu[k + 1] = norm<ES>(a, run_elem<ES>(cu, k)); ev[k + 1] = norm<ES>(a, run_elem<ES>(cv, k)); }
                    } else {
                        uint32_t c[4 * ES];
                        const uint8_t *r = a.p[1] + cy * a.pitch[1];
                        eu[0] = norm<ES>(a, one_elem<ES>(r + xl * (2 * ES))); ev[0] = norm<ES>(a, one_elem<ES>(r + xl * (2 * ES) + ES));
                        load_run<16 * ES, ES>(r + (long long)x0 * (2 * ES), c);
#pragma unroll
                        for (int k = 0; k < 8; ++k) { eu[k + 1] = norm<ES>(a, run_elem<ES>(c, 2 * k)); ev[k + 1] = norm<ES>(a, run_elem<ES>(c, 2 * k + 1)); }
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) { su[k] += eu[2 * k] + 2 * eu[2 * k + 1] + eu[2 * k + 2]; sv[k] += ev[2 * k] + 2 * ev[2 * k + 1] + ev[2 * k + 2]; }
                }
            }
        }
        store_words<8>(a.dst + (size_t)y * a.W + x0, yw);
    }
    uint32_t u[1] = {0}, v[1] = {0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u[0] |= shr_clip255<uint32_t>(su[k] + a.rc, a.s + T) << 8 * k;
        v[0] |= shr_clip255<uint32_t>(sv[k] + a.rc, a.s + T) << 8 * k;
    }
    store_chroma(a.dst, a.W, a.H, i, x0, u, v);
}

template <int SHAPE, int SUB> void launch_es(hipStream_t st, int es, const YuvArgs &a)
{
    const KsCellLaunch l = ks_cell_launch(a.W, a.H, 8);
    if (es == 2) hipLaunchKernelGGL((yuvx_to_i420_kernel<SHAPE, SUB, 2>), l.grid, l.blk, 0, st, a);
    else hipLaunchKernelGGL((yuvx_to_i420_kernel<SHAPE, SUB, 1>), l.grid, l.blk, 0, st, a);
}

}  // namespace

int ks265_yuv_check_desc(ks265_ctx *c, const ks265_in_desc *d, const ks265_yuv_fmt &f)
{
    if (d->width <= 0 || d->height <= 0 || (d->width & 7) || (d->height & 1)) { c->last_error = "input: width a multiple of 8, height even"; return KS265_NOTSUPPORTED; }
    const int nplanes = f.layout == 0 ? 3 : f.layout == 1 ? 2 : 1;
    if (f.es == 2) {
        uintptr_t bits = 0;
        for (int k = 0; k < nplanes; ++k) bits |= (uintptr_t)d->plane[k] | (uintptr_t)d->pitch[k];
        if (bits & 1) { c->last_error = "input: planes and pitches of a two-byte format are even"; return KS265_NOTSUPPORTED; }
    }
    const long long W = d->width, H = d->height, es = f.es;
    const long long cw = f.sub == 2 ? W : W / 2, ch = f.sub == 0 ? H / 2 : H;
    if (f.layout >= 2) return ks265_check_extent(c, d->plane[0], d->pitch[0], (int)H, 2 * W * es, "YUYV");
    int r = ks265_check_extent(c, d->plane[0], d->pitch[0], (int)H, W * es, "Y");
    if (!r && f.layout == 1) r = ks265_check_extent(c, d->plane[1], d->pitch[1], (int)ch, 2 * cw * es, "UV");
    for (int k = 1; k < 3 && !r && f.layout == 0; ++k) r = ks265_check_extent(c, d->plane[k], d->pitch[k], (int)ch, cw * es, k == 1 ? "U" : "V");
    return r;
}

int ks265_yuv_launch(ks265_ctx *c, const ks265_in_desc *d, const ks265_yuv_fmt &f, uint8_t *dst)
{
    YuvArgs a = {};
    for (int k = 0; k < 3; ++k) { a.p[k] = (const uint8_t *)d->plane[k]; a.pitch[k] = d->pitch[k]; }
    a.W = d->width; a.H = d->height; a.dst = dst;
    const int t = f.sub == 0 ? 0 : f.sub == 1 ? 1 : 3;
    a.s = f.depth - 8;
    a.nsh = f.msb ? 16 - f.depth : 0; a.mask = (1 << f.depth) - 1;
    a.rl = a.s ? 1 << (a.s - 1) : 0; a.rc = a.s + t ? 1 << (a.s + t - 1) : 0;
    a.uyvy = f.layout == 3;
    if (f.layout >= 2) launch_es<SH_PACKED, 1>(c->stream, f.es, a);
    else if (f.layout == 1) {
        if (f.sub == 0) launch_es<SH_SEMI, 0>(c->stream, f.es, a);
        else if (f.sub == 1) launch_es<SH_SEMI, 1>(c->stream, f.es, a);
        else launch_es<SH_SEMI, 2>(c->stream, f.es, a);
    } else {
        if (f.sub == 0) launch_es<SH_PLANAR, 0>(c->stream, f.es, a);
        else if (f.sub == 1) launch_es<SH_PLANAR, 1>(c->stream, f.es, a);
        else launch_es<SH_PLANAR, 2>(c->stream, f.es, a);
    }
    return ks265_check_launch(c);
}
