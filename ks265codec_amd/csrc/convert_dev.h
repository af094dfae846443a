// convert_dev.h — what the picture conversion kernels share (input_convert.hip, input_yuv.hip, output_convert.hip, picture_window.hip, input_scale.hip): the cell a thread owns, the run
// loaders and stores, the clamp in front of a shift, the float sample types, and on the host side the RGB matrices, the analysis of an RGB description's three channel pointers and the
// checks of 4:2:0 planes and of an input slot.  Each of these exists here and nowhere else.
#pragma once
#include "ks265_internal.h"
#include <cmath>
#include <type_traits>

// ---- the cell.  The picture kernels run 64 x 4 work-groups in which one thread owns RUN luma columns (from x0 on) across the two rows of chroma row i: every chroma sample is made
// from registers.  false: the thread lies outside the W x H picture
template <int RUN> __device__ inline bool ks_cell(int W, int H, int &x0, int &i)
{
    x0 = (blockIdx.x * 64 + threadIdx.x) * RUN; i = blockIdx.y * 4 + threadIdx.y;
    return x0 < W && 2 * i < H;
}
struct KsCellLaunch { dim3 grid, blk; };
static inline KsCellLaunch ks_cell_launch(long long W, long long H, int run)
{
    return {dim3((unsigned)(((W + run - 1) / run + 63) / 64), (unsigned)((H / 2 + 3) / 4)), dim3(64, 4)};
}

// ---- runs.  NB bytes at an address that is known to be on A = 16, 8 or 4 bytes, into words, little-endian
template <int NB, int A> __device__ inline void load_aligned(const uint8_t *p, uint32_t (&w)[NB / 4])
{
#pragma unroll
    for (int k = 0; k < NB / A; ++k) {
        if constexpr (A == 16) { const uint4 v = ((const uint4 *)p)[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
        else if constexpr (A == 8) { const uint2 v = ((const uint2 *)p)[k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
        else w[k] = ((const uint32_t *)p)[k];
    }
}
// NB bytes at p (a multiple of ES) as exactly those bytes: 16, 8 or 4 at a time where the address allows, element by element otherwise
template <int NB, int ES> __device__ inline void load_run(const uint8_t *p, uint32_t (&w)[NB / 4])
{
    const uintptr_t a = (uintptr_t)p;
    if (NB % 16 == 0 && !(a & 15)) load_aligned<NB, 16>(p, w);
    else if (NB % 8 == 0 && !(a & 7)) load_aligned<NB, 8>(p, w);
    else if (ES == 4 || !(a & 3)) load_aligned<NB, 4>(p, w);
    else if (ES == 2) {
#pragma unroll
        for (int k = 0; k < NB / 4; ++k) w[k] = (uint32_t)((const uint16_t *)p)[2 * k] | (uint32_t)((const uint16_t *)p)[2 * k + 1] << 16;
    } else {
#pragma unroll
        for (int k = 0; k < NB / 4; ++k) w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
    }
}
// stored element k (a constant after unrolling) of a run
template <int ES> __device__ inline uint32_t run_elem(const uint32_t *w, int k) { return ES == 4 ? w[k] : ES == 2 ? w[k >> 1] >> 16 * (k & 1) & 0xffffu : w[k >> 2] >> 8 * (k & 3) & 0xffu; }
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
// the cell's chroma into a packed I420 picture of W x H at dst (W a multiple of 8, dst on 16 bytes): NW words of Cb and NW of Cr (4 samples each) from column x0 / 2 of chroma row i
template <int NW> __device__ inline void store_chroma(uint8_t *dst, size_t W, size_t H, int i, int x0, const uint32_t (&u)[NW], const uint32_t (&v)[NW])
{
    const size_t npx = W * H;
    uint8_t *dc = dst + npx + (size_t)i * (W / 2) + x0 / 2;
    store_words<4 * NW>(dc, u);
    store_words<4 * NW>(dc + npx / 4, v);
}

// ---- the clamp.  clip255(v >> sh), written as a clamp of v in front of a logical shift: hipcc for gfx950 folds clip255(v >> sh) of two samples into v_ashr_pk_u8_i32 and then ORs
// the packed pair into the output word as if the instruction's upper 16 bits were zero (measured on the MI355X: output bytes = the right value OR stray bits).  This form compiles to
// med3 + shift and is exact.  No kernel may clip a shifted value; T = int, long long, or uint32_t (min(255, v >> sh): no lower branch)
template <typename T> __device__ inline uint32_t shr_clip255(T v, int sh)
{
    const T hi = ((T)256 << sh) - 1;
    if constexpr (std::is_signed<T>::value) v = v < 0 ? 0 : v;          // (two steps, the upper bound last: written as one nested conditional it compiles to compare + select + min)
    return (uint32_t)((typename std::make_unsigned<T>::type)(v > hi ? hi : v) >> sh);
}
// the same rule where a constant divides as well: clip255(floor(v / (DEN << sh))) of a 64-bit v - the clamp to [0, 256 DEN << sh) in front of the shift, and what remains
// (below 256 DEN, 32 bits) divided by the constant.  floor(floor(v / 2^sh) / DEN) = floor(v / (DEN 2^sh)) for v >= 0; a negative v clips to 0 either way
template <int DEN> __device__ inline uint32_t shr_div_clip255(long long v, int sh)
{
    const long long hi = ((long long)(256 * DEN) << sh) - 1;
    v = v < 0 ? 0 : v;
    return (uint32_t)((unsigned long long)(v > hi ? hi : v) >> sh) / (uint32_t)DEN;
}

// ---- float RGB samples (KS265_IN_RGB_F16 / _BF16 / _F32; tests/yuv_float_ref.py is the specification).  Nothing here may be built with fast-math
template <int FMT> struct FElem { typedef uint16_t type; };
template <> struct FElem<KS265_IN_RGB_F32> { typedef uint32_t type; };
// the bit pattern of a sample -> float32, exactly
template <int FMT> __device__ inline float sample_f32(uint32_t bits)
{
    if constexpr (FMT == KS265_IN_RGB_F32) return __uint_as_float(bits);
    else if constexpr (FMT == KS265_IN_RGB_BF16) return __uint_as_float(bits << 16);
    else { const uint16_t b = (uint16_t)bits; _Float16 h; __builtin_memcpy(&h, &b, 2); return (float)h; }
}
// q of the specification (the sample in 1 / 256 of a code): ONE IEEE multiply, NaN and everything below zero 0 (both comparisons are false for NaN), ties to even.
// A denormal times 65280 stays below 1 / 2 whether or not it is flushed.
__device__ inline int sample_q(float v)
{
    float t = v * 65280.0f;
    t = t > 0.0f ? t : 0.0f;
    t = t < 65280.0f ? t : 65280.0f;
    return (int)rintf(t);
}
// the bit pattern of the sample of byte k: the correctly rounded float32 of k / 255 - an IEEE division (hipcc keeps float32 division correctly rounded;
// tests/test_gpu_float_recon.py drives all 256 codes through every channel) - and for the 16-bit types that value rounded to nearest even
template <int FMT> __device__ inline uint32_t code_bits(uint32_t k)
{
    const float f = (float)k / 255.0f;
    if constexpr (FMT == KS265_IN_RGB_F32) return __float_as_uint(f);
    else if constexpr (FMT == KS265_IN_RGB_BF16) { const uint32_t b = __float_as_uint(f); return (b + 0x7fffu + (b >> 16 & 1u)) >> 16; }
    else { const _Float16 h = (_Float16)f; uint16_t b; __builtin_memcpy(&b, &h, 2); return b; }
}
template <int FMT> __device__ constexpr uint32_t one_bits() { return FMT == KS265_IN_RGB_F32 ? 0x3f800000u : FMT == KS265_IN_RGB_BF16 ? 0x3f80u : 0x3c00u; }

// ---- RGB -> YCbCr of one cell (8 luma columns x the two rows of chroma row i -> 16 Y, 4 Cb, 4 Cr) in three pieces, for every kernel whose arguments ARGS carry W, H, dst and the Q16 coefficients cy, cb, cr, oy.  c holds a row's samples of SH - 16 fraction bits, columns x0 - 1 .. x0 + 7;
// the sums are of type A, the luma shifted by SH and the (1, 2, 1) x (1, 1) chroma sums (weight 8) by SH + 3
template <typename A, int SH, typename ARGS> __device__ inline void rgb_store_luma(const ARGS &a, int y, int x0, const int (&c)[3][9])
{
    const A yoff = ((A)a.oy << SH) + ((A)1 << (SH - 1));
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k >> 2] |= shr_clip255<A>((A)a.cy[0] * c[0][k + 1] + (A)a.cy[1] * c[1][k + 1] + (A)a.cy[2] * c[2][k + 1] + yoff, SH) << 8 * (k & 3);
    store_words<8>(a.dst + y * (size_t)a.W + x0, w);
}
// chroma column x0 / 2 + k of one row and channel, weight 4: luma columns x0 + 2k - 1, x0 + 2k, x0 + 2k + 1 = entries 2k, 2k + 1, 2k + 2.  (Returned by value on purpose: the same sum
// added inside a function that takes the 3 x 4 accumulator by reference costs the float kernels up to 10 VGPRs and a wave per SIMD)
__device__ inline int rgb_sum121(const int (&c)[9], int k) { return c[2 * k] + 2 * c[2 * k + 1] + c[2 * k + 2]; }
template <typename A, int SH, typename ARGS> __device__ inline void rgb_store_chroma(const ARGS &a, int i, int x0, const int (&s)[3][4])
{
    const A rnd = ((A)128 << (SH + 3)) + ((A)1 << (SH + 2));
    uint32_t u[1] = {0}, v[1] = {0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u[0] |= shr_clip255<A>((A)a.cb[0] * s[0][k] + (A)a.cb[1] * s[1][k] + (A)a.cb[2] * s[2][k] + rnd, SH + 3) << 8 * k;
        v[0] |= shr_clip255<A>((A)a.cr[0] * s[0][k] + (A)a.cr[1] * s[1][k] + (A)a.cr[2] * s[2][k] + rnd, SH + 3) << 8 * k;
    }
    store_chroma(a.dst, a.W, a.H, i, x0, u, v);
}

// ---- host side
// the Q16 coefficients of an RGB description, both ways (tests/yuv_convert_ref.py, tests/yuv_output_ref.py): forward cy, cb, cr (R, G, B) and the luma offset oy; inverse ky8 = 8 ky, rv, gu, gv, bu
struct KsRgbCoef { int cy[3], cb[3], cr[3], oy, ky8, rv, gu, gv, bu; };
static inline KsRgbCoef ks_rgb_coef(int matrix, int full_range)
{
    const auto q16 = [](double x) { return (int)std::floor(x * 65536 + 0.5); };
    const double Kr = matrix == KS265_MATRIX_BT601 ? 0.299 : 0.2126, Kb = matrix == KS265_MATRIX_BT601 ? 0.114 : 0.0722, Kg = 1 - Kr - Kb;
    const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
    KsRgbCoef k;
    k.cy[0] = q16(sy * Kr); k.cy[1] = q16(sy * Kg); k.cy[2] = q16(sy * Kb);
    k.cb[0] = q16(-sc * Kr / (2 * (1 - Kb))); k.cb[1] = q16(-sc * Kg / (2 * (1 - Kb))); k.cb[2] = q16(sc / 2);
    k.cr[0] = q16(sc / 2); k.cr[1] = q16(-sc * Kg / (2 * (1 - Kr))); k.cr[2] = q16(-sc * Kb / (2 * (1 - Kr)));
    k.oy = full_range ? 0 : 16;
    k.ky8 = 8 * q16(1 / sy);
    k.rv = q16(2 * (1 - Kr) / sc); k.gu = q16(-2 * Kb * (1 - Kb) / (Kg * sc)); k.gv = q16(-2 * Kr * (1 - Kr) / (Kg * sc)); k.bu = q16(2 * (1 - Kb) / sc);
    return k;
}
// the three channel pointers of an RGB description of es-byte elements: the lowest and the highest, each channel's offset from the lowest in elements (4 for anything beyond 3),
// the mask of those offsets, and whether all three lie inside one pixel of pixel_step bytes that begins at the lowest
struct KsChannels { uintptr_t lo, hi; int off[3]; unsigned used; bool one_pixel; };
static inline KsChannels ks_channels(const ks265_in_desc *d, int es)
{
    const uintptr_t p0 = (uintptr_t)d->plane[0], p1 = (uintptr_t)d->plane[1], p2 = (uintptr_t)d->plane[2];
    KsChannels c = {p0 < p1 ? (p0 < p2 ? p0 : p2) : (p1 < p2 ? p1 : p2), p0 > p1 ? (p0 > p2 ? p0 : p2) : (p1 > p2 ? p1 : p2), {0, 0, 0}, 0, false};
    for (int k = 0; k < 3; ++k) { const uintptr_t o = ((uintptr_t)d->plane[k] - c.lo) / (uintptr_t)es; c.off[k] = o < 4 ? (int)o : 4; c.used |= 1u << c.off[k]; }
    c.one_pixel = c.hi - c.lo < (uintptr_t)d->pixel_step;
    return c;
}
// the planes of an 8-bit 4:2:0 description, I420 or NV12, each inside one device allocation (ks265_check_extent)
static inline int ks_check_planes_420(ks265_ctx *c, const ks265_in_desc *d, bool nv12)
{
    const long long W = d->width, H = d->height;
    int r = ks265_check_extent(c, d->plane[0], d->pitch[0], (int)H, W, "Y");
    if (!r && nv12) r = ks265_check_extent(c, d->plane[1], d->pitch[1], (int)(H / 2), W, "UV");
    for (int k = 1; k < 3 && !r && !nv12; ++k) r = ks265_check_extent(c, d->plane[k], d->pitch[k], (int)(H / 2), W / 2, k == 1 ? "U" : "V");
    return r;
}
// a packed picture the kernels store aligned words into (an input slot, the scaler's scratch): on 16 bytes, `bytes` inside one device allocation.  who: the call, what: the pointer
static inline int ks_check_slot(ks265_ctx *c, const void *p, long long bytes, const char *who, const char *what)
{
    if ((uintptr_t)p & 15) { c->last_error = std::string(who) + ": " + what + " not 16-byte aligned"; return KS265_NOTSUPPORTED; }
    return ks265_check_extent(c, p, bytes, 1, bytes, what);
}
