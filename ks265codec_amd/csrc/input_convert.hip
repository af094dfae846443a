// input_convert.hip — pictures already in device memory into the packed I420 layout of the encoder's input slots (include/ks265_hip.h ks265_input_convert):
// an I420 repack with arbitrary pitches, an NV12 deinterleave, and RGB (any pixel step: RGB24, RGBA, BGRA, planar) -> YCbCr in exact integer arithmetic
// (tests/yuv_convert_ref.py is the specification).  Memory-bound with no reuse beyond the neighbouring columns: one thread owns a run of luma columns across the
// two rows of one chroma row, so every chroma sample is made from registers (no LDS round trip).  Wide loads where the address allows, a byte path for the rest;
// the stores are always aligned (width a multiple of 8, the destination 16-byte aligned).
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
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12 && d->format != KS265_IN_RGB) { c->last_error = "input: unknown format"; return KS265_NOTSUPPORTED; }
    if (d->format == KS265_IN_RGB && (d->pixel_step < 1 || d->pixel_step > 16 || (d->matrix != KS265_MATRIX_BT709 && d->matrix != KS265_MATRIX_BT601))) {
        c->last_error = "input: RGB pixel step 1 .. 16, matrix BT.709 or BT.601"; return KS265_NOTSUPPORTED;
    }
    const long long W = d->width, H = d->height;
    int r = KS265_OK;
    if (d->format == KS265_IN_RGB) {
        const long long rb = (W - 1) * d->pixel_step + 1;
        if (d->pitch[0] < W * d->pixel_step) { c->last_error = "input: RGB pitch below width x pixel step"; return KS265_POINTER; }
        for (int k = 0; k < 3 && !r; ++k) r = check_extent(c, d->plane[k], d->pitch[0], (int)H, rb, k == 0 ? "R" : k == 1 ? "G" : "B");
    } else {
        r = check_extent(c, d->plane[0], d->pitch[0], (int)H, W, "Y");
        if (!r && d->format == KS265_IN_NV12) r = check_extent(c, d->plane[1], d->pitch[1], (int)(H / 2), W, "UV");
        for (int k = 1; k < 3 && !r && d->format == KS265_IN_I420; ++k) r = check_extent(c, d->plane[k], d->pitch[k], (int)(H / 2), W / 2, k == 1 ? "U" : "V");
    }
    return r;
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
    return check_desc(c, d);
}

int ks265_input_convert(ks265_ctx *c, const ks265_in_desc *d, uint8_t *dst)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    int r = check_desc(c, d);
    if (r) return r;
    const long long W = d->width, H = d->height;
    if ((uintptr_t)dst & 15) { c->last_error = "input: destination not 16-byte aligned"; return KS265_NOTSUPPORTED; }
    if ((r = check_extent(c, dst, W * H * 3 / 2, 1, W * H * 3 / 2, "destination"))) return r;
    CvtArgs a = {};
    for (int k = 0; k < 3; ++k) { a.p[k] = (const uint8_t *)d->plane[k]; a.pitch[k] = d->pitch[k]; }
    a.W = (int)W; a.H = (int)H; a.dst = dst; a.step = d->pixel_step;
    const dim3 blk(64, 4);
    if (d->format != KS265_IN_RGB) {
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
    a.mode = d->pixel_step == 1 ? 1 : 0;
    if (d->pixel_step == 4 && hi - (lo & ~(uintptr_t)3) < 4) {         // the three channels are bytes of one 32-bit word per pixel (RGBA, BGRA, ARGB, ...)
        a.mode = 2;
        a.base4 = (const uint8_t *)(lo & ~(uintptr_t)3);
        for (int k = 0; k < 3; ++k) a.sh[k] = 8 * (int)((uintptr_t)d->plane[k] - (lo & ~(uintptr_t)3));
        a.lo = (const uint8_t *)lo; a.ext = (long long)(hi - lo) + (W - 1) * 4 + 1;
    }
    const dim3 grid((unsigned)((W / 8 + 63) / 64), (unsigned)((H / 2 + 3) / 4));
    hipLaunchKernelGGL(rgb_to_i420_kernel, grid, blk, 0, c->stream, a);
    return ks265_check_launch(c);
}

}  // extern "C"
