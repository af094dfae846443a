// output_convert.hip — a packed I420 picture of the encoder (its reconstruction) into the caller's picture in device memory (include/ks265_hip.h ks265_output_convert):
// an I420 repack onto arbitrary pitches, an NV12 interleave, and YCbCr -> RGB (RGB24, RGBA / BGRA, planar) in exact integer arithmetic (tests/yuv_output_ref.py is the
// specification).  The mirror image of input_convert.hip on the same cell (convert_dev.h): one thread owns a run of 8 luma columns across the two luma rows of one chroma row - the
// rows that share their vertical chroma neighbours - so the three chroma rows it interpolates from are 2 x 3 x 5 bytes in registers (no LDS round trip).  Wide accesses where the address allows, a
// byte path for the rest; nothing is written outside [row start, row start + row bytes) of any destination row.  The RGB picture also goes out as float16 / bfloat16 / float32
// samples byte / 255 (tests/yuv_float_ref.py).
#include "convert_dev.h"

namespace {

struct OutArgs {
    const uint8_t *src;           // packed I420: Y W x H, U and V W/2 x H/2
    uint8_t *p[3];                // I420: Y, U, V; NV12: Y, UV; RGB: R, G, B of pixel (0, 0)
    long long pitch[3];           // RGB: pitch[0] for all three
    int step, W, H;               // step in bytes
    int ky8, rv, gu, gv, bu, oy;  // Q16 coefficients (ky8 = 8 ky)
    int mode;                     // RGB bytes: 0 byte by byte, 1 planar (8-byte stores per channel), 2 four-byte pixels on word addresses (16-byte stores)
    uint8_t *px0;                 // a pixel of 3 / 4 elements: the first byte of pixel (0, 0) = the lowest channel pointer; the channels are its elements off[c]
    int off[3], asel;             // the element none names: bytes get 255 at bit asel of the pixel's word, float samples 1.0
};

// n (8, or an even number below it at the right edge) bytes at p
__device__ inline void load_ragged(const uint8_t *p, int n, int (&b)[8])
{
    const uintptr_t a = (uintptr_t)p;
    if (n == 8 && !(a & 3)) {
        uint32_t lo, hi;
        if (!(a & 7)) { const uint2 v = *(const uint2 *)p; lo = v.x; hi = v.y; }
        else { lo = ((const uint32_t *)p)[0]; hi = ((const uint32_t *)p)[1]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { b[k] = (int)(lo >> 8 * k & 255); b[4 + k] = (int)(hi >> 8 * k & 255); }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = k < n ? p[k] : 0;
    }
}
// chroma columns j0 .. j0 + 4 of one row, clamped to the plane's last column w - 1: four bytes of the run and the right neighbour
__device__ inline void load_chroma(const uint8_t *row, int j0, int w, int nc, int (&b)[5])
{
    const uint8_t *p = row + j0;
    if (nc == 4 && !((uintptr_t)p & 3)) {
        const uint32_t v = *(const uint32_t *)p;
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = (int)(v >> 8 * k & 255);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = row[j0 + k < w ? j0 + k : w - 1];
    }
    b[4] = row[j0 + 4 < w ? j0 + 4 : w - 1];
}
// the n lowest bytes of w[0], w[1] to p
__device__ inline void store_run(uint8_t *p, int n, uint32_t w0, uint32_t w1)
{
    const uintptr_t a = (uintptr_t)p;
    if (n == 8 && !(a & 7)) *(uint2 *)p = make_uint2(w0, w1);
    else if (n == 8 && !(a & 3)) { ((uint32_t *)p)[0] = w0; ((uint32_t *)p)[1] = w1; }
    else {
#pragma unroll
        for (int k = 0; k < 8; ++k) if (k < n) p[k] = (uint8_t)((k < 4 ? w0 >> 8 * k : w1 >> 8 * (k - 4)) & 255);
    }
}
__device__ inline void store_half(uint8_t *p, int n, uint32_t w)
{
    if (n == 4 && !((uintptr_t)p & 3)) *(uint32_t *)p = w;
    else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < n) p[k] = (uint8_t)(w >> 8 * k & 255);
    }
}
__device__ inline uint32_t pack4(const int *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }

// I420 / NV12: 8 luma columns x the two rows of chroma row i; 4 samples of U and of V
template <bool NV12> __global__ __launch_bounds__(256) void i420_to_yuv_kernel(OutArgs a)
{
    int x0, i;
    if (!ks_cell<8>(a.W, a.H, x0, i)) return;
    const size_t W = (size_t)a.W, npx = W * a.H;
    const int n = a.W - x0 < 8 ? a.W - x0 : 8, w = a.W / 2, j0 = x0 / 2;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        int y[8];
        load_ragged(a.src + (2 * i + dy) * W + x0, n, y);
        store_run(a.p[0] + (2 * i + dy) * a.pitch[0] + x0, n, pack4(y), pack4(y + 4));
    }
    int u[5], v[5];
    load_chroma(a.src + npx + (size_t)i * w, j0, w, n / 2, u);
    load_chroma(a.src + npx + npx / 4 + (size_t)i * w, j0, w, n / 2, v);
    if constexpr (NV12) {
        const int uv[8] = {u[0], v[0], u[1], v[1], u[2], v[2], u[3], v[3]};
        store_run(a.p[1] + i * a.pitch[1] + x0, n, pack4(uv), pack4(uv + 4));
    } else {
        store_half(a.p[1] + i * a.pitch[1] + j0, n / 2, pack4(u));
        store_half(a.p[2] + i * a.pitch[2] + j0, n / 2, pack4(v));
    }
}

// YCbCr -> RGB of one cell (8 luma columns x the two rows of chroma row i -> 16 pixels) in three pieces.  The chroma rows i - 1, i, i + 1 (clamped), columns j0 .. j0 + 4 (clamped) of
// both planes
__device__ inline void load_chroma_rows(const OutArgs &a, int x0, int i, int n, int (&cu)[3][5], int (&cv)[3][5])
{
    const size_t npx = (size_t)a.W * a.H;
    const int w = a.W / 2, h = a.H / 2;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int ci = i + r - 1 < 0 ? 0 : i + r - 1 > h - 1 ? h - 1 : i + r - 1;
        load_chroma(a.src + npx + (size_t)ci * w, x0 / 2, w, n / 2, cu[r]);
        load_chroma(a.src + npx + npx / 4 + (size_t)ci * w, x0 / 2, w, n / 2, cv[r]);
    }
}
// the horizontal step at luma column k of the run, from the vertical step's samples v (weight 4): the chroma at weight 8, minus 128 x 8
__device__ inline int chroma8(const int (&v)[5], int k) { return (k & 1 ? v[k >> 1] + v[(k >> 1) + 1] : 2 * v[k >> 1]) - 1024; }
// and the three matrix rows: R, G, B of one pixel as bytes.  (The two kernels keep the loops over a row's pixels to themselves and take these pieces by value: one function that
// fills px[3][8] for both costs the float kernels their eighth wave per SIMD)
struct Rgb8 { uint32_t c[3]; };
__device__ inline Rgb8 pixel_to_rgb(const OutArgs &a, int y, int us, int vs)
{
    const int y8 = (y - a.oy) * a.ky8 + (1 << 18);
    return {{shr_clip255(y8 + a.rv * vs, 19), shr_clip255(y8 + a.gu * us + a.gv * vs, 19), shr_clip255(y8 + a.bu * us, 19)}};
}

// RGB as bytes
__global__ __launch_bounds__(256) void i420_to_rgb_kernel(OutArgs a)
{
    int x0, i;
    if (!ks_cell<8>(a.W, a.H, x0, i)) return;
    const int n = a.W - x0 < 8 ? a.W - x0 : 8;
    int cu[3][5], cv[3][5];
    load_chroma_rows(a, x0, i, n, cu, cv);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        int y[8];
        load_ragged(a.src + (2 * i + dy) * (size_t)a.W + x0, n, y);
        int vu[5], vv[5];                                              // vertical step, weight 4: the row's own chroma row x 3 + the nearer neighbour
#pragma unroll
        for (int k = 0; k < 5; ++k) { vu[k] = 3 * cu[1][k] + cu[2 * dy][k]; vv[k] = 3 * cv[1][k] + cv[2 * dy][k]; }
        uint32_t px[3][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const Rgb8 q = pixel_to_rgb(a, y[k], chroma8(vu, k), chroma8(vv, k));
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px[ch][k] = q.c[ch];
        }
        const long long ro = (long long)(2 * i + dy) * a.pitch[0];
        if (a.mode == 2) {                                             // one word per pixel, the fourth byte 255
            uint32_t wd[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) wd[k] = px[0][k] << 8 * a.off[0] | px[1][k] << 8 * a.off[1] | px[2][k] << 8 * a.off[2] | 255u << a.asel;
            uint8_t *q = a.px0 + ro + (long long)x0 * 4;
            if (n == 8 && !((uintptr_t)q & 15)) store_words<32>(q, wd);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k < n) ((uint32_t *)q)[k] = wd[k];
            }
        } else if (a.mode == 1) {                                      // planar
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                store_run(a.p[ch] + ro + x0, n, px[ch][0] | px[ch][1] << 8 | px[ch][2] << 16 | px[ch][3] << 24, px[ch][4] | px[ch][5] << 8 | px[ch][6] << 16 | px[ch][7] << 24);
        } else {                                                       // bytes: RGB24, and four-byte pixels that lie on no word address
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k >= n) continue;
                const long long o = ro + (long long)(x0 + k) * a.step;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) a.p[ch][o] = (uint8_t)px[ch][k];
                if (a.step == 4) a.px0[o + (a.asel >> 3)] = 255;
            }
        }
    }
}

// the first n of NE elements (bit patterns) to p: 16-byte stores where all NE are there and p is on 16 bytes, else element by element
template <int ES, int NE> __device__ inline void store_elems(uint8_t *p, int n, const uint32_t (&e)[NE])
{
    if (n == NE && !((uintptr_t)p & 15)) {
        if constexpr (ES == 4) store_words<4 * NE>(p, e);
        else {
            uint32_t w[NE / 2];
#pragma unroll
            for (int k = 0; k < NE / 2; ++k) w[k] = e[2 * k] | e[2 * k + 1] << 16;
            store_words<2 * NE>(p, w);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            if (k >= n) continue;
            if constexpr (ES == 4) ((uint32_t *)p)[k] = e[k]; else ((uint16_t *)p)[k] = (uint16_t)e[k];
        }
    }
}

// RGB as float samples (KS265_IN_RGB_F16 / _BF16 / _F32; tests/yuv_float_ref.py is the specification): the picture i420_to_rgb_kernel makes, each byte k as the sample k / 255.
// NPIX 1: planar; 3 / 4: the channels are elements of one pixel of 3 / 4 elements that begins at px0 (a run of 8 pixels is one contiguous store); 0: three channels that share no
// pixel (step 3 elements), element by element
template <int FMT, int NPIX> __global__ __launch_bounds__(256) void i420_to_rgbf_kernel(OutArgs a)
{
    typedef typename FElem<FMT>::type E;
    constexpr int ES = (int)sizeof(E);
    int x0, i;
    if (!ks_cell<8>(a.W, a.H, x0, i)) return;
    const int n = a.W - x0 < 8 ? a.W - x0 : 8;
    int cu[3][5], cv[3][5];
    load_chroma_rows(a, x0, i, n, cu, cv);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        int y[8];
        load_ragged(a.src + (2 * i + dy) * (size_t)a.W + x0, n, y);
        int vu[5], vv[5];                                              // vertical step, weight 4: the row's own chroma row x 3 + the nearer neighbour
#pragma unroll
        for (int k = 0; k < 5; ++k) { vu[k] = 3 * cu[1][k] + cu[2 * dy][k]; vv[k] = 3 * cv[1][k] + cv[2 * dy][k]; }
        uint32_t px[3][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const Rgb8 q = pixel_to_rgb(a, y[k], chroma8(vu, k), chroma8(vv, k));
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px[ch][k] = code_bits<FMT>(q.c[ch]);
        }
        const long long ro = (long long)(2 * i + dy) * a.pitch[0];
        if constexpr (NPIX == 1) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) store_elems<ES, 8>(a.p[ch] + ro + (long long)x0 * ES, n, px[ch]);
        } else if constexpr (NPIX >= 3) {
            uint32_t e[8 * NPIX];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
#pragma unroll
                for (int j = 0; j < NPIX; ++j) e[k * NPIX + j] = j == a.off[0] ? px[0][k] : j == a.off[1] ? px[1][k] : j == a.off[2] ? px[2][k] : one_bits<FMT>();
            }
            store_elems<ES, 8 * NPIX>(a.px0 + ro + (long long)x0 * (NPIX * ES), n * NPIX, e);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k >= n) continue;
                const long long o = ro + (long long)(x0 + k) * a.step;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) *(E *)(a.p[ch] + o) = (E)px[ch][k];
            }
        }
    }
}

template <int FMT> void launch_rgbf(hipStream_t st, const KsCellLaunch &l, int npix, const OutArgs &a)
{
    if (npix == 1) hipLaunchKernelGGL((i420_to_rgbf_kernel<FMT, 1>), l.grid, l.blk, 0, st, a);
    else if (npix == 3) hipLaunchKernelGGL((i420_to_rgbf_kernel<FMT, 3>), l.grid, l.blk, 0, st, a);
    else if (npix == 4) hipLaunchKernelGGL((i420_to_rgbf_kernel<FMT, 4>), l.grid, l.blk, 0, st, a);
    else hipLaunchKernelGGL((i420_to_rgbf_kernel<FMT, 0>), l.grid, l.blk, 0, st, a);
}

int check_out_desc(ks265_ctx *c, const ks265_in_desc *d)
{
    if (d->width <= 0 || d->height <= 0 || (d->width & 1) || (d->height & 1)) { c->last_error = "output: width and height even"; return KS265_NOTSUPPORTED; }
    const int es = ks265_rgb_elem_size(d->format);
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12 && !es) { c->last_error = "output: unknown format"; return KS265_NOTSUPPORTED; }
    if (!es) return ks_check_planes_420(c, d, d->format == KS265_IN_NV12);
    // RGB: bytes (es 1) or float samples; steps and offsets in elements of es bytes
    const long long W = d->width;
    if ((d->pixel_step != es && d->pixel_step != 3 * es && d->pixel_step != 4 * es) || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601)) {
        c->last_error = "output: RGB pixel step 1, 3 or 4 elements, matrix BT.709 or BT.601"; return KS265_NOTSUPPORTED;
    }
    if (((uintptr_t)d->plane[0] | (uintptr_t)d->plane[1] | (uintptr_t)d->plane[2] | (uintptr_t)d->pitch[0]) & (uintptr_t)(es - 1)) {
        c->last_error = "output: float RGB pointers and pitch are multiples of the element size"; return KS265_NOTSUPPORTED;
    }
    if (d->pitch[0] < W * d->pixel_step) { c->last_error = "output: RGB pitch below width x pixel step"; return KS265_POINTER; }
    if (d->pixel_step == 4 * es) {                                     // the three channels are three different elements of one four-element pixel, which begins at the lowest of them
        if (!d->plane[0] || !d->plane[1] || !d->plane[2]) { c->last_error = "output: NULL"; return KS265_POINTER; }
        const KsChannels ch = ks_channels(d, es);
        if (__builtin_popcount(ch.used & 15u) != 3) { c->last_error = "output: pixel step 4 needs the three channels inside one four-element pixel"; return KS265_NOTSUPPORTED; }
        return ks265_check_extent(c, (const void *)ch.lo, d->pitch[0], d->height, W * 4 * es, "RGBA");
    }
    int r = KS265_OK;
    for (int k = 0; k < 3 && !r; ++k) r = ks265_check_extent(c, d->plane[k], d->pitch[0], d->height, (W - 1) * d->pixel_step + es, k == 0 ? "R" : k == 1 ? "G" : "B");
    return r;
}

}  // namespace

extern "C" {

int ks265_output_validate(ks265_ctx *c, const ks265_in_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    return check_out_desc(c, d);
}

int ks265_output_convert(ks265_ctx *c, const uint8_t *src, const ks265_in_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    int r = check_out_desc(c, d);
    if (r) return r;
    const long long W = d->width, H = d->height;
    if ((r = ks265_check_extent(c, src, W * H * 3 / 2, 1, W * H * 3 / 2, "source"))) return r;
    OutArgs a = {};
    a.src = src;
    for (int k = 0; k < 3; ++k) { a.p[k] = (uint8_t *)d->plane[k]; a.pitch[k] = d->pitch[k]; }
    a.W = (int)W; a.H = (int)H; a.step = d->pixel_step;
    const KsCellLaunch l = ks_cell_launch(W, H, 8);
    const int es = ks265_rgb_elem_size(d->format);
    if (!es) {
        if (d->format == KS265_IN_NV12) hipLaunchKernelGGL((i420_to_yuv_kernel<true>), l.grid, l.blk, 0, c->stream, a);
        else hipLaunchKernelGGL((i420_to_yuv_kernel<false>), l.grid, l.blk, 0, c->stream, a);
        return ks265_check_launch(c);
    }
    const KsRgbCoef k = ks_rgb_coef(d->matrix, d->full_range);
    a.oy = k.oy; a.ky8 = k.ky8; a.rv = k.rv; a.gu = k.gu; a.gv = k.gv; a.bu = k.bu;
    // the pixel shape: planar (1), the channels as elements of one pixel of 4 (checked above) or of 3 (float samples: R, G, B are its three elements), or anything else (0)
    const KsChannels ch = ks_channels(d, es);
    int npix = d->pixel_step == es ? 1 : 0;
    if (d->pixel_step == 4 * es || (d->pixel_step == 3 * es && es > 1 && ch.hi - ch.lo == (uintptr_t)(2 * es) && ch.used == 7)) npix = d->pixel_step / es;
    a.px0 = (uint8_t *)ch.lo;
    for (int j = 0; j < 3; ++j) a.off[j] = ch.off[j];
    a.asel = 8 * (ch.used == 7 ? 3 : ch.used == 11 ? 2 : 1);            // bytes: the byte of the pixel no channel names (byte 0 is always one: the pixel begins at a channel)
    if (es == 1) {
        a.mode = npix == 4 ? (!(ch.lo & 3) && !(d->pitch[0] & 3) ? 2 : 0) : npix;
        hipLaunchKernelGGL(i420_to_rgb_kernel, l.grid, l.blk, 0, c->stream, a);
    } else if (d->format == KS265_IN_RGB_F16) launch_rgbf<KS265_IN_RGB_F16>(c->stream, l, npix, a);
    else if (d->format == KS265_IN_RGB_BF16) launch_rgbf<KS265_IN_RGB_BF16>(c->stream, l, npix, a);
    else launch_rgbf<KS265_IN_RGB_F32>(c->stream, l, npix, a);
    return ks265_check_launch(c);
}

}  // extern "C"
