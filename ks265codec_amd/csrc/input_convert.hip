// input_convert.hip — pictures already in device memory into the packed I420 layout of the encoder's input slots (include/ks265_hip.h ks265_input_convert):
// an I420 repack with arbitrary pitches, an NV12 deinterleave, and RGB (any pixel step: RGB24, RGBA, BGRA, planar) -> YCbCr in exact integer arithmetic
// (tests/yuv_convert_ref.py is the specification).  Memory-bound with no reuse beyond the neighbouring columns: one thread owns a run of luma columns across the
// two rows of one chroma row, so every chroma sample is made from registers (no LDS round trip).  Wide loads where the address allows, a byte path for the rest;
// the stores are always aligned (width a multiple of 8, the destination 16-byte aligned).  RGB as float16 / bfloat16 / float32 in [0, 1] goes the same way in one pass over the
// samples, with 64-bit sums (tests/yuv_float_ref.py).  YUV of more bits or more chroma (KS265_IN_YUV) is judged here first (check_any) and converted by input_yuv.hip.
#include "ks265_internal.h"
#include <cmath>

namespace {

struct CvtArgs {
    const uint8_t *p[3];          // I420: Y, U, V; NV12: Y, UV; RGB: R, G, B of pixel (0, 0)
    long long pitch[3];           // RGB: pitch[0] for all three
    int step, W, H;               // RGB: bytes between horizontally adjacent samples
    int cy[3], cb[3], cr[3], yoff; // Q16 coefficients; yoff = (oy << 16) + 32768
    int mode;                     // RGB: 0 bytes, 1 planar (8-byte loads per channel), 2 four-byte pixels (16-byte loads, all three channels from one word)
    const uint8_t *base4;         // mode 2: the lowest channel pointer rounded down to 4 bytes; the channels are bytes sh[c] / 8 of each pixel's word
    int sh[3];
    const uint8_t *lo; long long ext;   // mode 2: the union of the channels' extents in row 0 is [lo, lo + ext) - a wide load must lie inside it
    uint8_t *dst;
};

template <int N> __device__ inline void load_words(const uint8_t *p, uint32_t (&w)[N / 4])
{
    const uintptr_t a = (uintptr_t)p;
    if (N % 16 == 0 && !(a & 15)) {
#pragma unroll
        for (int k = 0; k < N / 16; ++k) { const uint4 v = ((const uint4 *)p)[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
    } else if (N % 8 == 0 && !(a & 7)) {
#pragma unroll
        for (int k = 0; k < N / 8; ++k) { const uint2 v = ((const uint2 *)p)[k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
    } else if (!(a & 3)) {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) w[k] = ((const uint32_t *)p)[k];
    } else {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
    }
}
// N bytes to an address aligned to min(N, 16)
template <int N> __device__ inline void store_words(uint8_t *p, const uint32_t (&w)[N / 4])
{
    if constexpr (N % 16 == 0) {
#pragma unroll
        for (int k = 0; k < N / 16; ++k) ((uint4 *)p)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else if constexpr (N % 8 == 0) {
#pragma unroll
        for (int k = 0; k < N / 8; ++k) ((uint2 *)p)[k] = make_uint2(w[2 * k], w[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) ((uint32_t *)p)[k] = w[k];
    }
}

// I420 / NV12: RUN luma columns (16 when the width allows, else 8) x the two rows of chroma row i; RUN / 2 samples of U and of V
template <int RUN, bool NV12> __global__ __launch_bounds__(256) void yuv_to_i420_kernel(CvtArgs a)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * RUN, i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.W || 2 * i >= a.H) return;
    const size_t W = (size_t)a.W, npx = W * a.H;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        uint32_t w[RUN / 4];
        load_words<RUN>(a.p[0] + (2 * i + dy) * a.pitch[0] + x0, w);
        store_words<RUN>(a.dst + (2 * i + dy) * W + x0, w);
    }
    uint32_t u[RUN / 8], v[RUN / 8];
    if constexpr (NV12) {
        uint32_t w[RUN / 4];
        load_words<RUN>(a.p[1] + i * a.pitch[1] + x0, w);
#pragma unroll
        for (int k = 0; k < RUN / 8; ++k) {                            // bytes U0 V0 U1 V1 | U2 V2 U3 V3 -> U0 U1 U2 U3, V0 V1 V2 V3
            const uint32_t lo = w[2 * k], hi = w[2 * k + 1];
            u[k] = (lo & 0xff) | (lo >> 8 & 0xff00) | (hi & 0xff) << 16 | (hi >> 16 & 0xff) << 24;
            v[k] = (lo >> 8 & 0xff) | (lo >> 16 & 0xff00) | (hi >> 8 & 0xff) << 16 | (hi >> 24) << 24;
        }
    } else {
        load_words<RUN / 2>(a.p[1] + i * a.pitch[1] + x0 / 2, u);
        load_words<RUN / 2>(a.p[2] + i * a.pitch[2] + x0 / 2, v);
    }
    uint8_t *dc = a.dst + npx + (size_t)i * (W / 2) + x0 / 2;
    store_words<RUN / 2>(dc, u);
    store_words<RUN / 2>(dc + npx / 4, v);
}

// one row of an RGB picture: columns x0 - 1 (clamped to 0) .. x0 + 7 into c[0][0..8] (R), c[1] (G), c[2] (B)
__device__ inline void load_rgb_row(const CvtArgs &a, int y, int x0, int (&c)[3][9])
{
    const long long ro = (long long)y * a.pitch[0];
    const long long xl = (long long)(x0 > 0 ? x0 - 1 : 0) * a.step;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][0] = a.p[ch][ro + xl];
    if (a.mode == 2) {
        const uint8_t *q = a.base4 + ro + (long long)x0 * 4;
        if (!((uintptr_t)q & 15) && q >= a.lo + ro && q + 32 <= a.lo + ro + a.ext) {
            const uint4 v0 = ((const uint4 *)q)[0], v1 = ((const uint4 *)q)[1];
            const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = (int)(w[k] >> a.sh[ch] & 255);
            }
            return;
        }
    } else if (a.mode == 1) {
        const uint8_t *q0 = a.p[0] + ro + x0, *q1 = a.p[1] + ro + x0, *q2 = a.p[2] + ro + x0;
        if (!(((uintptr_t)q0 | (uintptr_t)q1 | (uintptr_t)q2) & 7)) {
            const uint2 v[3] = {*(const uint2 *)q0, *(const uint2 *)q1, *(const uint2 *)q2};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
                for (int k = 0; k < 8; ++k) c[ch][k + 1] = (int)((k < 4 ? v[ch].x >> 8 * k : v[ch].y >> 8 * (k - 4)) & 255);
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][k + 1] = a.p[ch][ro + (long long)(x0 + k) * a.step];
    }
}

// clip255(v >> sh), written as a clamp of v before a logical shift: hipcc for gfx950 folds clip255(v >> sh) of two samples into v_ashr_pk_u8_i32 and then ORs the
// packed pair into the output word as if the instruction's upper 16 bits were zero (measured on the MI355X: output bytes = the right value OR stray bits).  This form
// compiles to med3 + shift and is exact.
__device__ inline uint32_t shr_clip255(int v, int sh)
{
    const int hi = (256 << sh) - 1;
    return (uint32_t)(v < 0 ? 0 : v > hi ? hi : v) >> sh;
}

// RGB: 8 luma columns x the two rows of chroma row i -> 16 Y, 4 Cb, 4 Cr
__global__ __launch_bounds__(256) void rgb_to_i420_kernel(CvtArgs a)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8, i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.W || 2 * i >= a.H) return;
    const size_t W = (size_t)a.W, npx = W * a.H;
    int c0[3][9], c1[3][9];
    load_rgb_row(a, 2 * i, x0, c0);
    load_rgb_row(a, 2 * i + 1, x0, c1);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int (&c)[3][9] = dy ? c1 : c0;
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k >> 2] |= shr_clip255(a.cy[0] * c[0][k + 1] + a.cy[1] * c[1][k + 1] + a.cy[2] * c[2][k + 1] + a.yoff, 16) << 8 * (k & 3);
        *(uint2 *)(a.dst + (2 * i + dy) * W + x0) = make_uint2(w[0], w[1]);
    }
    uint32_t u = 0, v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                      // chroma column x0 / 2 + k: luma columns x0 + 2k - 1, x0 + 2k, x0 + 2k + 1 = entries 2k, 2k + 1, 2k + 2
        int s[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            s[ch] = c0[ch][2 * k] + 2 * c0[ch][2 * k + 1] + c0[ch][2 * k + 2] + c1[ch][2 * k] + 2 * c1[ch][2 * k + 1] + c1[ch][2 * k + 2];
        const int rnd = (128 << 19) + (1 << 18);
        u |= shr_clip255(a.cb[0] * s[0] + a.cb[1] * s[1] + a.cb[2] * s[2] + rnd, 19) << 8 * k;
        v |= shr_clip255(a.cr[0] * s[0] + a.cr[1] * s[1] + a.cr[2] * s[2] + rnd, 19) << 8 * k;
    }
    uint8_t *dc = a.dst + npx + (size_t)i * (W / 2) + x0 / 2;
    *(uint32_t *)dc = u;
    *(uint32_t *)(dc + npx / 4) = v;
}

// ---- float RGB (KS265_IN_RGB_F16 / _BF16 / _F32; tests/yuv_float_ref.py is the specification): the shape of rgb_to_i420_kernel with samples q in 1 / 256 of a code (17 bits)
// and 64-bit sums.  Everything below is in ELEMENTS of the type except the pointers, pitch and step (bytes).
struct CvtFArgs {
    const uint8_t *p[3];          // R, G, B of pixel (0, 0)
    long long pitch;
    int step, W, H;
    int cy[3], cb[3], cr[3], oy;  // Q16 coefficients
    const uint8_t *base;          // NPIX 3 / 4: where the run of pixel (0, 0) begins (NPIX 4: the lowest channel pointer rounded down to a pixel); the channels are its elements off[c]
    int off[3];
    const uint8_t *lo; long long ext;   // NPIX 3 / 4: the union of the channels' extents in row 0 is [lo, lo + ext) - a wide load must lie inside it
    uint8_t *dst;
};

template <int FMT> struct FElem { typedef uint16_t type; };
template <> struct FElem<KS265_IN_RGB_F32> { typedef uint32_t type; };

// the bit pattern of a sample -> float32, exactly
template <int FMT> __device__ inline float sample_f32(uint32_t bits)
{
    if constexpr (FMT == KS265_IN_RGB_F32) return __uint_as_float(bits);
    else if constexpr (FMT == KS265_IN_RGB_BF16) return __uint_as_float(bits << 16);
    else { const uint16_t b = (uint16_t)bits; _Float16 h; __builtin_memcpy(&h, &b, 2); return (float)h; }
}
// q of the specification: ONE IEEE multiply (this translation unit is built without fast-math), NaN and everything below zero 0 (both comparisons are false for NaN), ties to even.
// A denormal times 65280 stays below 1 / 2 whether or not it is flushed.
__device__ inline int sample_q(float v)
{
    float t = v * 65280.0f;
    t = t > 0.0f ? t : 0.0f;
    t = t < 65280.0f ? t : 65280.0f;
    return (int)rintf(t);
}
// element k of a run of 16-byte loads
template <int ES> __device__ inline uint32_t run_elem(const uint32_t *w, int k) { return ES == 4 ? w[k] : w[k >> 1] >> 16 * (k & 1) & 0xffff; }

// one row of a float RGB picture: q of columns x0 - 1 (clamped to 0) .. x0 + 7 into c[0][0..8] (R), c[1] (G), c[2] (B).  NPIX 1: planar, 3 / 4: the three channels are elements of
// one pixel of 3 / 4 elements, 0: anything else.  16-byte loads where the run's address is on 16 bytes and the run inside the row; else element by element.
template <int FMT, int NPIX> __device__ inline void load_rgbf_row(const CvtFArgs &a, int y, int x0, int (&c)[3][9])
{
    typedef typename FElem<FMT>::type E;
    constexpr int ES = (int)sizeof(E);
    const long long ro = (long long)y * a.pitch;
    const long long xl = (long long)(x0 > 0 ? x0 - 1 : 0) * a.step;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][0] = sample_q(sample_f32<FMT>(*(const E *)(a.p[ch] + ro + xl)));
    if constexpr (NPIX == 1) {
        const uint8_t *q[3] = {a.p[0] + ro + (long long)x0 * ES, a.p[1] + ro + (long long)x0 * ES, a.p[2] + ro + (long long)x0 * ES};
        if (!(((uintptr_t)q[0] | (uintptr_t)q[1] | (uintptr_t)q[2]) & 15)) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                uint32_t w[2 * ES];
#pragma unroll
                for (int k = 0; k < ES / 2; ++k) { const uint4 v = ((const uint4 *)q[ch])[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
#pragma unroll
                for (int k = 0; k < 8; ++k) c[ch][k + 1] = sample_q(sample_f32<FMT>(run_elem<ES>(w, k)));
            }
            return;
        }
    } else if constexpr (NPIX >= 3) {
        const uint8_t *q = a.base + ro + (long long)x0 * (NPIX * ES);
        if (!((uintptr_t)q & 15) && q >= a.lo + ro && q + 8 * NPIX * ES <= a.lo + ro + a.ext) {
            uint32_t w[2 * NPIX * ES];                                  // 8 pixels of NPIX elements: NPIX * ES / 2 loads of 16 bytes
#pragma unroll
            for (int k = 0; k < NPIX * ES / 2; ++k) { const uint4 v = ((const uint4 *)q)[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
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

// clip255(v >> sh) of a 64-bit sum, in shr_clip255's form: the clamp in front of a logical shift
__device__ inline uint32_t shr_clip255_64(long long v, int sh)
{
    const long long hi = (256LL << sh) - 1;
    return (uint32_t)((unsigned long long)(v < 0 ? 0 : v > hi ? hi : v) >> sh);
}

// float RGB: 8 luma columns x the two rows of chroma row i -> 16 Y, 4 Cb, 4 Cr.  A row's q live only until its luma is stored and its (1, 2, 1) sums are taken.
template <int FMT, int NPIX> __global__ __launch_bounds__(256) void rgbf_to_i420_kernel(CvtFArgs a)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8, i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.W || 2 * i >= a.H) return;
    const size_t W = (size_t)a.W, npx = W * a.H;
    const long long yoff = ((long long)a.oy << 24) + (1 << 23);
    int s[3][4] = {};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        int c[3][9];
        load_rgbf_row<FMT, NPIX>(a, 2 * i + dy, x0, c);
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k)
            w[k >> 2] |= shr_clip255_64((long long)a.cy[0] * c[0][k + 1] + (long long)a.cy[1] * c[1][k + 1] + (long long)a.cy[2] * c[2][k + 1] + yoff, 24) << 8 * (k & 3);
        *(uint2 *)(a.dst + (2 * i + dy) * W + x0) = make_uint2(w[0], w[1]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                  // chroma column x0 / 2 + k: entries 2k, 2k + 1, 2k + 2
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s[ch][k] += c[ch][2 * k] + 2 * c[ch][2 * k + 1] + c[ch][2 * k + 2];
        }
    }
    uint32_t u = 0, v = 0;
    const long long rnd = (128LL << 27) + (1 << 26);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u |= shr_clip255_64((long long)a.cb[0] * s[0][k] + (long long)a.cb[1] * s[1][k] + (long long)a.cb[2] * s[2][k] + rnd, 27) << 8 * k;
        v |= shr_clip255_64((long long)a.cr[0] * s[0][k] + (long long)a.cr[1] * s[1][k] + (long long)a.cr[2] * s[2][k] + rnd, 27) << 8 * k;
    }
    uint8_t *dc = a.dst + npx + (size_t)i * (W / 2) + x0 / 2;
    *(uint32_t *)dc = u;
    *(uint32_t *)(dc + npx / 4) = v;
}

template <int FMT> void launch_rgbf(hipStream_t st, dim3 grid, dim3 blk, int npix, const CvtFArgs &a)
{
    if (npix == 1) hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 1>), grid, blk, 0, st, a);
    else if (npix == 3) hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 3>), grid, blk, 0, st, a);
    else if (npix == 4) hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 4>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((rgbf_to_i420_kernel<FMT, 0>), grid, blk, 0, st, a);
}

// [p, p + pitch (rows - 1) + row_bytes) inside one device allocation on the context's device
int check_extent(ks265_ctx *c, const void *p, long long pitch, int rows, long long row_bytes, const char *what)
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
    const long long W = d->width, H = d->height;
    int r = KS265_OK;
    if (es) {
        const long long rb = (W - 1) * d->pixel_step + es;
        if (d->pitch[0] < W * d->pixel_step) { c->last_error = "input: RGB pitch below width x pixel step"; return KS265_POINTER; }
        for (int k = 0; k < 3 && !r; ++k) r = check_extent(c, d->plane[k], d->pitch[0], (int)H, rb, k == 0 ? "R" : k == 1 ? "G" : "B");
    } else {
        r = check_extent(c, d->plane[0], d->pitch[0], (int)H, W, "Y");
        if (!r && d->format == KS265_IN_NV12) r = check_extent(c, d->plane[1], d->pitch[1], (int)(H / 2), W, "UV");
        for (int k = 1; k < 3 && !r && d->format == KS265_IN_I420; ++k) r = check_extent(c, d->plane[k], d->pitch[k], (int)(H / 2), W / 2, k == 1 ? "U" : "V");
    }
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

int q16(double x) { return (int)std::floor(x * 65536 + 0.5); }

}  // namespace

// check_extent for the other translation units that take pictures of the application (output_convert.hip)
int ks265_check_extent(ks265_ctx *c, const void *p, long long pitch, int rows, long long row_bytes, const char *what) { return check_extent(c, p, pitch, rows, row_bytes, what); }

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
    if ((uintptr_t)dst & 15) { c->last_error = "input: destination not 16-byte aligned"; return KS265_NOTSUPPORTED; }
    if ((r = check_extent(c, dst, W * H * 3 / 2, 1, W * H * 3 / 2, "destination"))) return r;
    if (fam) return ks265_yuv_launch(c, d, yf, dst);
    CvtArgs a = {};
    for (int k = 0; k < 3; ++k) { a.p[k] = (const uint8_t *)d->plane[k]; a.pitch[k] = d->pitch[k]; }
    a.W = (int)W; a.H = (int)H; a.dst = dst; a.step = d->pixel_step;
    const dim3 blk(64, 4);
    const int es = ks265_rgb_elem_size(d->format);
    if (!es) {
        const int run = W % 16 == 0 ? 16 : 8;
        const dim3 grid((unsigned)((W / run + 63) / 64), (unsigned)((H / 2 + 3) / 4));
        if (d->format == KS265_IN_NV12) {
            if (run == 16) hipLaunchKernelGGL((yuv_to_i420_kernel<16, true>), grid, blk, 0, c->stream, a);
            else hipLaunchKernelGGL((yuv_to_i420_kernel<8, true>), grid, blk, 0, c->stream, a);
        } else {
            if (run == 16) hipLaunchKernelGGL((yuv_to_i420_kernel<16, false>), grid, blk, 0, c->stream, a);
            else hipLaunchKernelGGL((yuv_to_i420_kernel<8, false>), grid, blk, 0, c->stream, a);
        }
        return ks265_check_launch(c);
    }
    const double Kr = d->matrix == KS265_MATRIX_BT601 ? 0.299 : 0.2126, Kb = d->matrix == KS265_MATRIX_BT601 ? 0.114 : 0.0722, Kg = 1 - Kr - Kb;
    const double sy = d->full_range ? 1.0 : 219.0 / 255.0, sc = d->full_range ? 1.0 : 224.0 / 255.0;
    const int oy = d->full_range ? 0 : 16;
    a.cy[0] = q16(sy * Kr); a.cy[1] = q16(sy * Kg); a.cy[2] = q16(sy * Kb);
    a.cb[0] = q16(-sc * Kr / (2 * (1 - Kb))); a.cb[1] = q16(-sc * Kg / (2 * (1 - Kb))); a.cb[2] = q16(sc / 2);
    a.cr[0] = q16(sc / 2); a.cr[1] = q16(-sc * Kg / (2 * (1 - Kr))); a.cr[2] = q16(-sc * Kb / (2 * (1 - Kr)));
    a.yoff = (oy << 16) + 32768;
    const uintptr_t p0 = (uintptr_t)d->plane[0], p1 = (uintptr_t)d->plane[1], p2 = (uintptr_t)d->plane[2];
    const uintptr_t lo = p0 < p1 ? (p0 < p2 ? p0 : p2) : (p1 < p2 ? p1 : p2), hi = p0 > p1 ? (p0 > p2 ? p0 : p2) : (p1 > p2 ? p1 : p2);
    const dim3 grid((unsigned)((W / 8 + 63) / 64), (unsigned)((H / 2 + 3) / 4));
    if (es > 1) {                                                      // float samples: the kernel by type and pixel shape
        CvtFArgs f = {};
        for (int k = 0; k < 3; ++k) { f.p[k] = a.p[k]; f.cy[k] = a.cy[k]; f.cb[k] = a.cb[k]; f.cr[k] = a.cr[k]; }
        f.pitch = d->pitch[0]; f.step = d->pixel_step; f.W = (int)W; f.H = (int)H; f.oy = oy; f.dst = dst;
        int npix = d->pixel_step == es ? 1 : 0;
        const uintptr_t base = d->pixel_step == 4 * es ? lo & ~(uintptr_t)(4 * es - 1) : lo;   // a four-element pixel lies on its own size; one of three begins at its lowest channel
        if ((d->pixel_step == 3 * es || d->pixel_step == 4 * es) && hi - base < (uintptr_t)d->pixel_step) {
            npix = d->pixel_step / es;
            f.base = (const uint8_t *)base;
            for (int k = 0; k < 3; ++k) f.off[k] = (int)(((uintptr_t)d->plane[k] - base) / (uintptr_t)es);
            f.lo = (const uint8_t *)lo; f.ext = (long long)(hi - lo) + (W - 1) * d->pixel_step + es;
        }
        if (d->format == KS265_IN_RGB_F16) launch_rgbf<KS265_IN_RGB_F16>(c->stream, grid, blk, npix, f);
        else if (d->format == KS265_IN_RGB_BF16) launch_rgbf<KS265_IN_RGB_BF16>(c->stream, grid, blk, npix, f);
        else launch_rgbf<KS265_IN_RGB_F32>(c->stream, grid, blk, npix, f);
        return ks265_check_launch(c);
    }
    a.mode = d->pixel_step == 1 ? 1 : 0;
    if (d->pixel_step == 4 && hi - (lo & ~(uintptr_t)3) < 4) {         // the three channels are bytes of one 32-bit word per pixel (RGBA, BGRA, ARGB, ...)
        a.mode = 2;
        a.base4 = (const uint8_t *)(lo & ~(uintptr_t)3);
        for (int k = 0; k < 3; ++k) a.sh[k] = 8 * (int)((uintptr_t)d->plane[k] - (lo & ~(uintptr_t)3));
        a.lo = (const uint8_t *)lo; a.ext = (long long)(hi - lo) + (W - 1) * 4 + 1;
    }
    hipLaunchKernelGGL(rgb_to_i420_kernel, grid, blk, 0, c->stream, a);
    return ks265_check_launch(c);
}

}  // extern "C"
