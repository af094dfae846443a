// input_convert.hip — pictures already in device memory into the packed I420 layout of the encoder's input slots (include/ks265_hip.h ks265_input_convert):
// an I420 repack with arbitrary pitches, an NV12 deinterleave, and RGB (any pixel step: RGB24, RGBA, BGRA, planar) -> YCbCr in exact integer arithmetic
// (tests/yuv_convert_ref.py is the specification).  Memory-bound with no reuse beyond the neighbouring columns: the cell, the run loaders and the aligned stores are convert_dev.h's
// (width a multiple of 8, the destination 16-byte aligned).  RGB as float16 / bfloat16 / float32 in [0, 1] goes the same way in one pass over the
// samples, with 64-bit sums (tests/yuv_float_ref.py).  YUV of more bits or more chroma (KS265_IN_YUV) is judged here first (check_any) and converted by input_yuv.hip.
#include "convert_dev.h"

namespace {

// everything is in bytes except off[] (elements of the sample type)
struct CvtArgs {
    const uint8_t *p[3];          // I420: Y, U, V; NV12: Y, UV; RGB: R, G, B of pixel (0, 0)
    long long pitch[3];           // RGB: pitch[0] for all three
    int step, W, H;               // RGB: bytes between horizontally adjacent samples
    int cy[3], cb[3], cr[3], oy;  // Q16 coefficients
    int mode;                     // RGB bytes: 0 byte by byte, 1 planar (8-byte loads per channel), 2 four-byte pixels (16-byte loads, all three channels from one word)
    const uint8_t *base;          // mode 2, float NPIX 3 / 4: where the run of pixel (0, 0) begins (four elements: the lowest channel pointer rounded down to a pixel); the channels are its elements off[c]
    int off[3];
    const uint8_t *lo; long long ext;   // with base: the union of the channels' extents in row 0 is [lo, lo + ext) - a wide load must lie inside it
    uint8_t *dst;
};

// I420 / NV12: RUN luma columns (16 when the width allows, else 8) x the two rows of chroma row i; RUN / 2 samples of U and of V
template <int RUN, bool NV12> __global__ __launch_bounds__(256) void yuv_to_i420_kernel(CvtArgs a)
{
    int x0, i;
    if (!ks_cell<RUN>(a.W, a.H, x0, i)) return;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        uint32_t w[RUN / 4];
        load_run<RUN, 1>(a.p[0] + (2 * i + dy) * a.pitch[0] + x0, w);
        store_words<RUN>(a.dst + (2 * i + dy) * (size_t)a.W + x0, w);
    }
    uint32_t u[RUN / 8], v[RUN / 8];
    if constexpr (NV12) {
        uint32_t w[RUN / 4];
        load_run<RUN, 1>(a.p[1] + i * a.pitch[1] + x0, w);
#pragma unroll
        for (int k = 0; k < RUN / 8; ++k) {                            // bytes U0 V0 U1 V1 | U2 V2 U3 V3 -> U0 U1 U2 U3, V0 V1 V2 V3
            const uint32_t lo = w[2 * k], hi = w[2 * k + 1];
            u[k] = (lo & 0xff) | (lo >> 8 & 0xff00) | (hi & 0xff) << 16 | (hi >> 16 & 0xff) << 24;
            v[k] = (lo >> 8 & 0xff) | (lo >> 16 & 0xff00) | (hi >> 8 & 0xff) << 16 | (hi >> 24) << 24;
        }
    } else {
        load_run<RUN / 2, 1>(a.p[1] + i * a.pitch[1] + x0 / 2, u);
        load_run<RUN / 2, 1>(a.p[2] + i * a.pitch[2] + x0 / 2, v);
    }
    store_chroma(a.dst, a.W, a.H, i, x0, u, v);
}

// a wide load of the pixels x0 .. x0 + 7 of row offset ro, NB bytes at q: on 16 bytes and inside the row's own bytes
template <int NB> __device__ inline bool pixels_inside(const CvtArgs &a, const uint8_t *q, long long ro) { return !((uintptr_t)q & 15) && q >= a.lo + ro && q + NB <= a.lo + ro + a.ext; }

// one row of an RGB picture: columns x0 - 1 (clamped to 0) .. x0 + 7 into c[0][0..8] (R), c[1] (G), c[2] (B)
__device__ inline void load_rgb_row(const CvtArgs &a, int y, int x0, int (&c)[3][9])
{
    const long long ro = (long long)y * a.pitch[0];
    const long long xl = (long long)(x0 > 0 ? x0 - 1 : 0) * a.step;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][0] = a.p[ch][ro + xl];
    const uint8_t *q = a.base + ro + (long long)x0 * 4;
    if (a.mode == 2 && pixels_inside<32>(a, q, ro)) {
        uint32_t w[8];
        load_aligned<32, 16>(q, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = (int)(w[k] >> 8 * a.off[ch] & 255);
        }
    } else if (a.mode == 1 && !(((uintptr_t)(a.p[0] + ro + x0) | (uintptr_t)(a.p[1] + ro + x0) | (uintptr_t)(a.p[2] + ro + x0)) & 7)) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            uint32_t w[2];
            load_aligned<8, 8>(a.p[ch] + ro + x0, w);
#pragma unroll
            for (int k = 0; k < 8; ++k) c[ch][k + 1] = (int)run_elem<1>(w, k);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = a.p[ch][ro + (long long)(x0 + k) * a.step];
        }
    }
}

// one row of a float RGB picture (everything in ELEMENTS of the type except the pointers, pitch and step): q of columns x0 - 1 (clamped to 0) .. x0 + 7 into c[0][0..8] (R), c[1] (G),
// c[2] (B).  NPIX 1: planar; 3 / 4: the three channels are elements of one pixel of 3 / 4 elements; 0: anything else.  16-byte loads where the run's address is on 16 bytes and the run inside the row; else element by element
template <int FMT, int NPIX> __device__ inline void load_rgbf_row(const CvtArgs &a, int y, int x0, int (&c)[3][9])
{
    typedef typename FElem<FMT>::type E;
    constexpr int ES = (int)sizeof(E);
    const long long ro = (long long)y * a.pitch[0];
    const long long xl = (long long)(x0 > 0 ? x0 - 1 : 0) * a.step;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][0] = sample_q(sample_f32<FMT>(*(const E *)(a.p[ch] + ro + xl)));
    if constexpr (NPIX == 1) {
        const uint8_t *q[3] = {a.p[0] + ro + (long long)x0 * ES, a.p[1] + ro + (long long)x0 * ES, a.p[2] + ro + (long long)x0 * ES};
        if (!(((uintptr_t)q[0] | (uintptr_t)q[1] | (uintptr_t)q[2]) & 15)) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                uint32_t w[2 * ES];
                load_aligned<8 * ES, 16>(q[ch], w);
#pragma unroll
                for (int k = 0; k < 8; ++k) c[ch][k + 1] = sample_q(sample_f32<FMT>(run_elem<ES>(w, k)));
            }
            return;
        }
    } else if constexpr (NPIX >= 3) {
        const uint8_t *q = a.base + ro + (long long)x0 * (NPIX * ES);
        if (pixels_inside<8 * NPIX * ES>(a, q, ro)) {
            uint32_t w[2 * NPIX * ES];                                  // 8 pixels of NPIX elements
            load_aligned<8 * NPIX * ES, 16>(q, w);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                uint32_t e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = j < NPIX ? run_elem<ES>(w, k * NPIX + j) : 0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = sample_q(sample_f32<FMT>(a.off[ch] == 0 ? e[0] : a.off[ch] == 1 ? e[1] : a.off[ch] == 2 ? e[2] : e[3]));
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = sample_q(sample_f32<FMT>(*(const E *)(a.p[ch] + ro + (long long)(x0 + k) * a.step)));
    }
}

// (the three pieces of RGB -> YCbCr of one cell - rgb_store_luma, rgb_sum121, rgb_store_chroma - are convert_dev.h's: input_tonemap.hip ends in them too)
// bytes: 32-bit sums throughout; both rows are loaded before anything is stored
__global__ __launch_bounds__(256) void rgb_to_i420_kernel(CvtArgs a)
{
    int x0, i;
    if (!ks_cell<8>(a.W, a.H, x0, i)) return;
    int c[2][3][9], s[3][4] = {};
    load_rgb_row(a, 2 * i, x0, c[0]);
    load_rgb_row(a, 2 * i + 1, x0, c[1]);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        rgb_store_luma<int, 16>(a, 2 * i + dy, x0, c[dy]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s[ch][k] += rgb_sum121(c[dy][ch], k);
        }
    }
    rgb_store_chroma<int, 16>(a, i, x0, s);
}
// float samples (KS265_IN_RGB_F16 / _BF16 / _F32): q in 1 / 256 of a code (17 bits) and 64-bit sums.  A row's q live only until its luma is stored and its chroma sums are taken
template <int FMT, int NPIX> __global__ __launch_bounds__(256) void rgbf_to_i420_kernel(CvtArgs a)
{
    int x0, i;
    if (!ks_cell<8>(a.W, a.H, x0, i)) return;
    int s[3][4] = {};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        int c[3][9];
        load_rgbf_row<FMT, NPIX>(a, 2 * i + dy, x0, c);
        rgb_store_luma<long long, 24>(a, 2 * i + dy, x0, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s[ch][k] += rgb_sum121(c[ch], k);
        }
    }
    rgb_store_chroma<long long, 24>(a, i, x0, s);
}

template <int FMT> void launch_rgbf(hipStream_t st, const KsCellLaunch &l, int npix, const CvtArgs &a)
{
    if (npix == 1) hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 1>), l.grid, l.blk, 0, st, a);
    else if (npix == 3) hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 3>), l.grid, l.blk, 0, st, a);
    else if (npix == 4) hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 4>), l.grid, l.blk, 0, st, a);
    else hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 0>), l.grid, l.blk, 0, st, a);
}

int check_desc(ks265_ctx *c, const ks265_in_desc *d)
{
    if (d->width <= 0 || d->height <= 0 || (d->width & 7) || (d->height & 1)) { c->last_error = "input: width a multiple of 8, height even"; return KS265_NOTSUPPORTED; }
    const int es = ks265_rgb_elem_size(d->format);
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12 && !es) { c->last_error = "input: unknown format"; return KS265_NOTSUPPORTED; }
    if (d->format == KS265_IN_RGB && (d->pixel_step < 1 || d->pixel_step > 16 || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601))) {
        c->last_error = "input: RGB pixel step 1 .. 16, matrix BT.709 or BT.601"; return KS265_NOTSUPPORTED;
    }
    if (es > 1) {
        if (d->pixel_step < es || d->pixel_step > 64 || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601)) {
            c->last_error = "input: float RGB pixel step element size .. 64, matrix BT.709 or BT.601"; return KS265_NOTSUPPORTED;
        }
        if (((uintptr_t)d->plane[0] | (uintptr_t)d->plane[1] | (uintptr_t)d->plane[2] | (uintptr_t)d->pixel_step | (uintptr_t)d->pitch[0]) & (uintptr_t)(es - 1)) {
            c->last_error = "input: float RGB pointers, pixel step and pitch are multiples of the element size"; return KS265_NOTSUPPORTED;
        }
    }
    if (!es) return ks_check_planes_420(c, d, d->format == KS265_IN_NV12);
    const long long W = d->width, rb = (W - 1) * d->pixel_step + es;
    if (d->pitch[0] < W * d->pixel_step) { c->last_error = "input: RGB pitch below width x pixel step"; return KS265_POINTER; }
    int r = KS265_OK;
    for (int k = 0; k < 3 && !r; ++k) r = ks265_check_extent(c, d->plane[k], d->pitch[0], d->height, rb, k == 0 ? "R" : k == 1 ? "G" : "B");
    return r;
}

// a description judged whichever family it belongs to.  *fam = 1: the YUV family (input_yuv.hip), the fields in *f; 0: a format of this file - KS265_IN_YUV(0 / 1, 0, 8, 0)
// are KS265_IN_I420 / _NV12, and *d then points at `loc`, the description under that code
int check_any(ks265_ctx *c, const ks265_in_desc *&d, ks265_in_desc &loc, ks265_yuv_fmt *f, int *fam)
{
    *fam = ks265_yuv_decode(d->format, f);
    if (*fam < 0) { c->last_error = "input: unknown format"; return KS265_NOTSUPPORTED; }
    if (*fam && f->alias) { loc = *d; loc.format = f->layout ? KS265_IN_NV12 : KS265_IN_I420; d = &loc; *fam = 0; }
    return *fam ? ks265_yuv_check_desc(c, d, *f) : check_desc(c, d);
}

}  // namespace

// [p, p + pitch (rows - 1) + row_bytes) inside one device allocation on the context's device
int ks265_check_extent(ks265_ctx *c, const void *p, long long pitch, int rows, long long row_bytes, const char *what)
{
    if (!p) { c->last_error = std::string(what) + ": NULL"; return KS265_POINTER; }
    if (rows <= 0 || row_bytes <= 0 || pitch < row_bytes) { c->last_error = std::string(what) + ": pitch below the row's bytes"; return KS265_POINTER; }
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); c->last_error = std::string(what) + ": not memory of the HIP runtime"; return KS265_POINTER; }
    if (at.type != hipMemoryTypeDevice || at.isManaged) { c->last_error = std::string(what) + ": not device memory"; return KS265_POINTER; }
    if (at.device != c->device) { c->last_error = std::string(what) + ": memory of another device"; return KS265_POINTER; }
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); c->last_error = std::string(what) + ": no allocation found"; return KS265_POINTER; }
    const uintptr_t b = (uintptr_t)base, q = (uintptr_t)p;
    const unsigned long long ext = (unsigned long long)pitch * (unsigned long long)(rows - 1) + (unsigned long long)row_bytes;
    if (q < b || q - b >= size || ext > size - (q - b)) { c->last_error = std::string(what) + ": extends past the end of its allocation"; return KS265_POINTER; }
    return KS265_OK;
}

extern "C" {

int ks265_wait_external(ks265_ctx *c, void *s)
{
    if (!c) return KS265_POINTER;
    ks_use_device(c);
    int r = ks265_hip(c, hipEventRecord(c->ev_ext, (hipStream_t)s));
    if (!r) r = ks265_hip(c, hipStreamWaitEvent(c->stream, c->ev_ext, 0));
    return r;
}
int ks265_external_wait_event(ks265_ctx *c, void *s, void *ev)
{
    if (!c || !ev) return KS265_POINTER;
    ks_use_device(c);
    return ks265_hip(c, hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)ev, 0));
}

int ks265_input_validate(ks265_ctx *c, const ks265_in_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    ks265_in_desc loc; ks265_yuv_fmt f; int fam;
    return check_any(c, d, loc, &f, &fam);
}

int ks265_input_convert(ks265_ctx *c, const ks265_in_desc *d, uint8_t *dst)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    ks265_in_desc loc; ks265_yuv_fmt yf; int fam;
    int r = check_any(c, d, loc, &yf, &fam);
    if (r) return r;
    const long long W = d->width, H = d->height;
    if ((r = ks_check_slot(c, dst, W * H * 3 / 2, "input", "destination"))) return r;
    if (fam) return ks265_yuv_launch(c, d, yf, dst);
    CvtArgs a = {};
    for (int k = 0; k < 3; ++k) { a.p[k] = (const uint8_t *)d->plane[k]; a.pitch[k] = d->pitch[k]; }
    a.W = (int)W; a.H = (int)H; a.dst = dst; a.step = d->pixel_step;
    const int es = ks265_rgb_elem_size(d->format);
    if (!es) {
        const int run = W % 16 == 0 ? 16 : 8;
        const KsCellLaunch l = ks_cell_launch(W, H, run);
        if (d->format == KS265_IN_NV12) {
            if (run == 16) hipLaunchKernelGGL((yuv_to_i420_kernel<16, true>), l.grid, l.blk, 0, c->stream, a);
            else hipLaunchKernelGGL((yuv_to_i420_kernel<8, true>), l.grid, l.blk, 0, c->stream, a);
        } else {
            if (run == 16) hipLaunchKernelGGL((yuv_to_i420_kernel<16, false>), l.grid, l.blk, 0, c->stream, a);
            else hipLaunchKernelGGL((yuv_to_i420_kernel<8, false>), l.grid, l.blk, 0, c->stream, a);
        }
        return ks265_check_launch(c);
    }
    const KsRgbCoef k = ks_rgb_coef(d->matrix, d->full_range);
    for (int j = 0; j < 3; ++j) { a.cy[j] = k.cy[j]; a.cb[j] = k.cb[j]; a.cr[j] = k.cr[j]; }
    a.oy = k.oy;
    // the pixel shape: planar (1), or the three channels inside one pixel of 3 / 4 elements that a run of wide loads can take whole (for bytes: 4 only), or anything else (0).
    // A four-element pixel lies on its own size, `skew` bytes below the lowest channel; one of three begins at its lowest channel
    const KsChannels ch = ks_channels(d, es);
    const uintptr_t step = (uintptr_t)d->pixel_step, skew = step == (uintptr_t)(4 * es) ? ch.lo & (uintptr_t)(4 * es - 1) : 0;
    int npix = d->pixel_step == es ? 1 : 0;
    if ((step == (uintptr_t)(4 * es) || (step == (uintptr_t)(3 * es) && es > 1)) && ch.hi - ch.lo + skew < step) {
        npix = d->pixel_step / es;
        a.base = (const uint8_t *)(ch.lo - skew);
        for (int j = 0; j < 3; ++j) a.off[j] = ch.off[j] + (int)skew / es;
        a.lo = (const uint8_t *)ch.lo; a.ext = (long long)(ch.hi - ch.lo) + (W - 1) * d->pixel_step + es;
    }
    const KsCellLaunch l = ks_cell_launch(W, H, 8);
    if (es == 1) {
        a.mode = npix == 4 ? 2 : npix;
        hipLaunchKernelGGL(rgb_to_i420_kernel, l.grid, l.blk, 0, c->stream, a);
    } else if (d->format == KS265_IN_RGB_F16) launch_rgbf<KS265_IN_RGB_F16>(c->stream, l, npix, a);
    else if (d->format == KS265_IN_RGB_BF16) launch_rgbf<KS265_IN_RGB_BF16>(c->stream, l, npix, a);
    else launch_rgbf<KS265_IN_RGB_F32>(c->stream, l, npix, a);
    return ks265_check_launch(c);
}

}  // extern "C"
