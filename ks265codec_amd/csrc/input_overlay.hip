// input_overlay.hip — overlays on the way in (include/ks265_hip.h ks265_input_overlay; tests/overlay_ref.py is the specification of every byte): up to 8 pictures
// of RGB plus alpha blended IN PLACE onto the packed I420 picture of an input slot by one launch, the descriptors by value in the kernel's argument.  No state, no scratch, no
// atomics.
//
// The cell is the conversion kernels' (convert_dev.h ks_cell<2>): a thread owns 2 luma columns across the two rows of one chroma row, and the Cb and the Cr sample under them.
// Two columns, not the converters' eight: a logo is a few thousand samples on a device of 256 CUs, and a thread's work per overlay is a dependent chain of loads and 64-bit
// sums - the narrowest cell spreads it widest (measurement builds with cells of 8 / 4 / 2 columns, profiles/overlay.txt: a 256x128 logo 10.0 / 6.8 / 5.1 us, eight of them 44.5 / 19.4 /
// 9.3 us, a whole 2160p picture of float16 35.9 / 31.8 / 32.2 us; this kernel: 4.7, 8.6 and 38.6 us).  Positions, sizes and the window are even, so a cell lies wholly inside an overlay's columns and rows or
// wholly outside: no sample of a cell is masked.
// The grid covers the bounding box of the clipped rectangles, not the picture.  A thread walks the overlays in slot order; the first one that covers its cell makes it load the
// cell (two aligned 2-byte runs of luma, one byte of each chroma plane) into registers, every one that does blends there, and at the end a cell that was loaded is stored the
// same way - every byte once.  A thread no overlay covers touches no memory.
//
// Per overlay and row the thread reads the overlay's columns c0 - 1, c0, c0 + 1 (c0 = x0 - x, even, 0 .. w - 2): column c0 - 1 is the left neighbour of the chroma filter
// ((1, 2, 1) over the overlay as a picture of its own - at c0 = 0 it clamps to column 0; the last column never needs a right neighbour: w is even).  Every address lies inside
// the validated extent.  In an overlay of four-element pixels that hold all four channels (RGBA in any order) the two pixels come as one load_run; anything else element by
// element.  Samples become 8-bit codes at once (floats through sample_q), A = (a opacity + 128) >> 8.
//
// Arithmetic: the luma numerator Y (255 - A) 65536 + A (cy . RGB + oy 65536) + 255 * 32768 and the chroma numerator Cb (2040 - SA) 65536 + cb . (SAR, SAG, SAB) + 128 * 65536 SA + D / 2
// are 64-bit (cb . S needs 35 bits and a sign); the sums under them that fit 32 bits are 32-bit.  The quotient is convert_dev.h's shr_div_clip255: the clamp in front of the
// shift, then a 32-bit division by the constant.  It runs over overlay samples only.  Nothing here may be built with fast-math.
#include "convert_dev.h"

namespace {

struct OvK {
    const uint8_t *p[4];          // R, G, B, alpha of pixel (0, 0); p[3] NULL: opaque
    const uint8_t *base;          // fast: where pixel (0, 0) of four elements begins; the channels are its elements off[c]
    long long pitch;
    int step, fmt, w, h, x, y, opacity, fast;
    int off[4];
    int cy[3], cb[3], cr[3], oy;
};
struct OvArgs {
    OvK o[KS265_OVERLAY_MAX];
    int n, W, H;
    int bx, bi, bw, bh;           // the bounding box of the clipped rectangles: first luma column (even), first chroma row, size in luma samples
    uint8_t *pic;
};

constexpr int OV_RUN = 2;                                               // luma columns a thread owns

template <int FMT> __device__ inline int ov_code(uint32_t bits)
{
    if constexpr (FMT == KS265_IN_RGB) return (int)bits;
    else return (sample_q(sample_f32<FMT>(bits)) + 128) >> 8;
}
template <int ES> __device__ inline uint32_t ov_elem(const uint8_t *p)
{
    if constexpr (ES == 1) return *p;
    else if constexpr (ES == 2) return *(const uint16_t *)p;
    else return *(const uint32_t *)p;
}

// one row of an overlay: the codes of its columns max(c0 - 1, 0), c0, c0 + 1 into c[ch][0..2] (R, G, B) and the effective alpha into al[0..2]
template <int FMT> __device__ inline void ov_load_row(const OvK &o, int row, int c0, int (&c)[3][3], int (&al)[3])
{
    constexpr int ES = FMT == KS265_IN_RGB ? 1 : (int)sizeof(typename FElem<FMT>::type);
    const long long ro = (long long)row * o.pitch, xl = (long long)(c0 > 0 ? c0 - 1 : 0) * o.step;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][0] = ov_code<FMT>(ov_elem<ES>(o.p[ch] + ro + xl));
    al[0] = o.p[3] ? ov_code<FMT>(ov_elem<ES>(o.p[3] + ro + xl)) : 255;
    if (o.fast) {
        uint32_t w[2 * ES];                                             // 2 pixels of 4 elements
        load_run<8 * ES, ES>(o.base + ro + (long long)c0 * (4 * ES), w);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint32_t e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = run_elem<ES>(w, 4 * k + j);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = ov_code<FMT>(o.off[ch] == 0 ? e[0] : o.off[ch] == 1 ? e[1] : o.off[ch] == 2 ? e[2] : e[3]);
            al[k + 1] = ov_code<FMT>(o.off[3] == 0 ? e[0] : o.off[3] == 1 ? e[1] : o.off[3] == 2 ? e[2] : e[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long xo = (long long)(c0 + k) * o.step;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = ov_code<FMT>(ov_elem<ES>(o.p[ch] + ro + xo));
            al[k + 1] = o.p[3] ? ov_code<FMT>(ov_elem<ES>(o.p[3] + ro + xo)) : 255;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) al[k] = (al[k] * o.opacity + 128) >> 8;
}

// one overlay onto the cell it covers at luma column x0, chroma row i: Y[dy][k], U, V in registers
template <int FMT> __device__ inline void ov_blend(const OvK &o, int x0, int i, int (&Y)[2][2], int &U, int &V)
{
    const int c0 = x0 - o.x, r0 = 2 * i - o.y;                          // the overlay's column and row under the cell's first sample: even, in [0, w - 2] and [0, h - 2]
    int sa = 0, sr = 0, sg = 0, sb = 0;                                 // (at most 8 * 255 and 8 * 255 * 255)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        int c[3][3], al[3];
        ov_load_row<FMT>(o, r0 + dy, c0, c, al);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int A = al[k + 1];
            const int lum = o.cy[0] * c[0][k + 1] + o.cy[1] * c[1][k + 1] + o.cy[2] * c[2][k + 1] + (o.oy << 16);     // (24 bits and a bit: the conversion's own 32-bit sum)
            Y[dy][k] = (int)shr_div_clip255<255>(((long long)(Y[dy][k] * (255 - A)) << 16) + (long long)A * lum + 255 * 32768, 16);
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int A = (t == 1 ? 2 : 1) * al[t];
            sa += A; sr += A * c[0][t]; sg += A * c[1][t]; sb += A * c[2][t];
        }
    }
    const long long mid = ((long long)(128 * sa) << 16) + (long long)2040 * 32768;
    const int keep = 2040 - sa;
    U = (int)shr_div_clip255<2040>(((long long)(U * keep) << 16) + (long long)o.cb[0] * sr + (long long)o.cb[1] * sg + (long long)o.cb[2] * sb + mid, 16);
    V = (int)shr_div_clip255<2040>(((long long)(V * keep) << 16) + (long long)o.cr[0] * sr + (long long)o.cr[1] * sg + (long long)o.cr[2] * sb + mid, 16);
}

__global__ __launch_bounds__(256) void input_overlay_kernel(OvArgs a)
{
    int x0, i;
    if (!ks_cell<OV_RUN>(a.bw, a.bh, x0, i)) return;
    x0 += a.bx; i += a.bi;                                               // (inside the window: the box is)
    const size_t npx = (size_t)a.W * a.H;
    uint8_t *const py = a.pic + (size_t)(2 * i) * a.W + x0, *const pu = a.pic + npx + (size_t)i * (a.W / 2) + x0 / 2, *const pv = pu + npx / 4;
    int Y[2][2], U = 0, V = 0;
    bool loaded = false;
    for (int n = 0; n < a.n; ++n) {
        const OvK &o = a.o[n];
        if (2 * i < o.y || 2 * i >= o.y + o.h || x0 < o.x || x0 >= o.x + o.w) continue;   // (everything even: both rows and both columns are covered, or none)
        if (!loaded) {
            loaded = true;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) { const uint32_t w = *(const uint16_t *)(py + (size_t)dy * a.W); Y[dy][0] = (int)(w & 255u); Y[dy][1] = (int)(w >> 8); }
            U = *pu; V = *pv;
        }
        if (o.fmt == KS265_IN_RGB) ov_blend<KS265_IN_RGB>(o, x0, i, Y, U, V);
        else if (o.fmt == KS265_IN_RGB_F16) ov_blend<KS265_IN_RGB_F16>(o, x0, i, Y, U, V);
        else if (o.fmt == KS265_IN_RGB_BF16) ov_blend<KS265_IN_RGB_BF16>(o, x0, i, Y, U, V);
        else ov_blend<KS265_IN_RGB_F32>(o, x0, i, Y, U, V);
    }
    if (!loaded) return;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) *(uint16_t *)(py + (size_t)dy * a.W) = (uint16_t)(Y[dy][0] | Y[dy][1] << 8);
    *pu = (uint8_t)U; *pv = (uint8_t)V;
}

constexpr int OV_MAX_DIM = 8192, OV_MAX_POS = 16384;

int ov_check(ks265_ctx *c, const ks265_overlay_desc *ov, int n, int W, int H, int win_w, int win_h)
{
    if (n < 1 || n > KS265_OVERLAY_MAX) { c->last_error = "overlay: 1 .. 8 overlays"; return KS265_NOTSUPPORTED; }
    if (W <= 0 || H <= 0 || (W & 7) || (H & 7) || W > OV_MAX_DIM || H > OV_MAX_DIM || win_w < 2 || win_h < 2 || ((win_w | win_h) & 1) || win_w > W || win_h > H) {
        c->last_error = "overlay: picture width and height positive multiples of 8, at most 8192; window even, 2 .. the picture's size"; return KS265_NOTSUPPORTED;
    }
    for (int k = 0; k < n; ++k) {
        const ks265_in_desc *d = &ov[k].rgb;
        const int es = ks265_rgb_elem_size(d->format);
        if (!es) { c->last_error = "overlay: format RGB as bytes, float16, bfloat16 or float32"; return KS265_NOTSUPPORTED; }
        if (d->width < 2 || d->height < 2 || ((d->width | d->height | ov[k].x | ov[k].y) & 1) || d->width > OV_MAX_DIM || d->height > OV_MAX_DIM || ov[k].x < -OV_MAX_POS || ov[k].x > OV_MAX_POS ||
            ov[k].y < -OV_MAX_POS || ov[k].y > OV_MAX_POS) { c->last_error = "overlay: width, height, x, y even; size 2 .. 8192; position -16384 .. 16384"; return KS265_NOTSUPPORTED; }
        if (ov[k].opacity < 0 || ov[k].opacity > 256) { c->last_error = "overlay: opacity 0 .. 256"; return KS265_NOTSUPPORTED; }
        if (d->pixel_step < es || d->pixel_step > (es == 1 ? 16 : 64) || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601)) {
            c->last_error = "overlay: pixel step element size .. 16 (bytes) / 64 (floats), matrix BT.709 or BT.601"; return KS265_NOTSUPPORTED;
        }
        if (((uintptr_t)d->plane[0] | (uintptr_t)d->plane[1] | (uintptr_t)d->plane[2] | (uintptr_t)ov[k].alpha | (uintptr_t)d->pixel_step | (uintptr_t)d->pitch[0]) & (uintptr_t)(es - 1)) {
            c->last_error = "overlay: float pointers, pixel step and pitch are multiples of the element size"; return KS265_NOTSUPPORTED;
        }
        const long long w = d->width, rb = (w - 1) * d->pixel_step + es;
        if (d->pitch[0] < w * d->pixel_step) { c->last_error = "overlay: pitch below width x pixel step"; return KS265_POINTER; }
        int r = KS265_OK;
        for (int j = 0; j < 3 && !r; ++j) r = ks265_check_extent(c, d->plane[j], d->pitch[0], d->height, rb, j == 0 ? "overlay R" : j == 1 ? "overlay G" : "overlay B");
        if (!r && ov[k].alpha) r = ks265_check_extent(c, ov[k].alpha, d->pitch[0], d->height, rb, "overlay alpha");
        if (r) return r;
    }
    return KS265_OK;
}

}  // namespace

extern "C" {

int ks265_input_overlay_validate(ks265_ctx *c, const ks265_overlay_desc *ov, int n, int coded_w, int coded_h, int win_w, int win_h)
{
    if (!c || !ov) return KS265_POINTER;
    ks_use_device(c);
    return ov_check(c, ov, n, coded_w, coded_h, win_w, win_h);
}

int ks265_input_overlay(ks265_ctx *c, const ks265_overlay_desc *ov, int n, int coded_w, int coded_h, int win_w, int win_h, uint8_t *dev_i420)
{
    if (!c || !ov) return KS265_POINTER;
    ks_use_device(c);
    int r = ov_check(c, ov, n, coded_w, coded_h, win_w, win_h);
    if (r) return r;
    if ((r = ks_check_slot(c, dev_i420, (long long)coded_w * coded_h * 3 / 2, "overlay", "picture"))) return r;
    OvArgs a = {};
    a.n = n; a.W = coded_w; a.H = coded_h; a.pic = dev_i420;
    int bx0 = coded_w, by0 = coded_h, bx1 = 0, by1 = 0;                 // the union of the rectangles clipped to the window (all even)
    for (int k = 0; k < n; ++k) {
        const ks265_in_desc *d = &ov[k].rgb;
        const int es = ks265_rgb_elem_size(d->format);
        OvK &o = a.o[k];
        for (int j = 0; j < 3; ++j) o.p[j] = (const uint8_t *)d->plane[j];
        o.p[3] = (const uint8_t *)ov[k].alpha;
        o.pitch = d->pitch[0]; o.step = d->pixel_step; o.fmt = d->format; o.w = d->width; o.h = d->height; o.x = ov[k].x; o.y = ov[k].y; o.opacity = ov[k].opacity;
        const KsRgbCoef q = ks_rgb_coef(d->matrix, d->full_range);
        for (int j = 0; j < 3; ++j) { o.cy[j] = q.cy[j]; o.cb[j] = q.cb[j]; o.cr[j] = q.cr[j]; }
        o.oy = q.oy;
        // four-element pixels that hold all four channels: a run of pixels is then whole pixels of validated bytes, and wide loads may take it
        const KsChannels ch = ks_channels(d, es);
        if (o.p[3] && d->pixel_step == 4 * es) {
            const uintptr_t pa = (uintptr_t)o.p[3], lo = pa < ch.lo ? pa : ch.lo, hi = pa > ch.hi ? pa : ch.hi;
            unsigned used = 0;
            for (int j = 0; j < 4; ++j) { o.off[j] = (int)(((uintptr_t)o.p[j] - lo) / (uintptr_t)es); if (o.off[j] < 4) used |= 1u << o.off[j]; }
            if (hi - lo < (uintptr_t)(4 * es) && used == 15u) { o.fast = 1; o.base = (const uint8_t *)lo; }
        }
        const int x0 = o.x > 0 ? o.x : 0, y0 = o.y > 0 ? o.y : 0, x1 = o.x + o.w < win_w ? o.x + o.w : win_w, y1 = o.y + o.h < win_h ? o.y + o.h : win_h;
        if (x0 >= x1 || y0 >= y1) continue;
        bx0 = x0 < bx0 ? x0 : bx0; by0 = y0 < by0 ? y0 : by0; bx1 = x1 > bx1 ? x1 : bx1; by1 = y1 > by1 ? y1 : by1;
    }
    if (bx0 >= bx1 || by0 >= by1) return KS265_OK;                      // every overlay lies outside the window: nothing to do
    a.bx = bx0; a.bi = by0 / 2; a.bw = bx1 - a.bx; a.bh = by1 - by0;
    const KsCellLaunch l = ks_cell_launch(a.bw, a.bh, OV_RUN);
    hipLaunchKernelGGL(input_overlay_kernel, l.grid, l.blk, 0, c->stream, a);
    return ks265_check_launch(c);
}

}  // extern "C"
