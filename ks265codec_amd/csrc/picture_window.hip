// picture_window.hip — pictures whose size is no multiple of 8 (tests/picture_window_ref.py is the specification of every byte).  The encoder codes
// cW x cH = the source size W x H rounded up to the minimum CU size and signals a conformance window; these three kernels are the only code that sees both sizes:
//   ks265_input_pad    8-bit I420 / NV12 of W x H with its own pitches -> the packed I420 of cW x cH of an input slot, last column and last row replicated (np.pad mode="edge")
//   ks265_output_crop  packed I420 of cW x cH -> packed I420 of W x H (the top-left corner)
//   ks265_sse_window   takes the padding strips' squared error out of the three plane sums of ks265_sse_picture / ks265_ssim_picture
// Pad and crop are memory-bound and run on convert_dev.h's cell: one thread owns 8 luma columns across the two rows of one chroma row, no LDS.  A source row of 854
// bytes starts at any address, so a run is copied out of the row as exactly its own bytes (memcpy of 8 or 4: the hardware takes a dword load at any byte address) and a run
// that crosses the row's end is read byte by byte with the column clamped; nothing outside [row start, row start + row bytes) is read.  The coded rows are multiples of 8 / 4
// bytes and the slot is 16-byte aligned, so the pad's stores are aligned words.  The thread of the LAST source row pair also writes the rows below it: the source is read once.
#include "frame_common.h"
#include "convert_dev.h"

namespace {

struct PadArgs {
    const uint8_t *p[3];          // I420: Y, U, V; NV12: Y, UV
    long long pitch[3];
    int W, H, cW, cH;
    uint8_t *dst;
};

__device__ inline uint2 ld8(const uint8_t *p) { uint2 v; __builtin_memcpy(&v, p, 8); return v; }
__device__ inline uint32_t ld4(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
// bytes x0 .. x0 + 7 of a row of w bytes, the column clamped to w - 1 (x0 < w)
__device__ inline uint2 ld8_edge(const uint8_t *row, int x0, int w)
{
    if (x0 + 8 <= w) return ld8(row + x0);
    uint32_t v[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int x = x0 + k < w ? x0 + k : w - 1; v[k >> 2] |= (uint32_t)row[x] << 8 * (k & 3); }
    return make_uint2(v[0], v[1]);
}
__device__ inline uint32_t ld4_edge(const uint8_t *row, int x0, int w)
{
    if (x0 + 4 <= w) return ld4(row + x0);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int x = x0 + k < w ? x0 + k : w - 1; v |= (uint32_t)row[x] << 8 * k; }
    return v;
}
// four U, V pairs from pair x0 on of an interleaved row of w pairs, the pair clamped to w - 1: u = the four U bytes, v = the four V bytes
__device__ inline void ld4_pairs_edge(const uint8_t *row, int x0, int w, uint32_t &u, uint32_t &v)
{
    if (x0 + 4 <= w) {
        const uint2 c = ld8(row + 2 * x0);
        u = (c.x & 0xffu) | (c.x >> 8 & 0xff00u) | (c.y << 16 & 0xff0000u) | (c.y << 8 & 0xff000000u);
        v = (c.x >> 8 & 0xffu) | (c.x >> 16 & 0xff00u) | (c.y << 8 & 0xff0000u) | (c.y & 0xff000000u);
        return;
    }
    u = v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k < w ? x0 + k : w - 1;
        u |= (uint32_t)row[2 * x] << 8 * k; v |= (uint32_t)row[2 * x + 1] << 8 * k;
    }
}

// a thread: luma columns x0 .. x0 + 7 of source rows 2 i and 2 i + 1, chroma columns x0 / 2 .. + 3 of chroma row i; for the last source row pair also every row below
template <bool NV12> __global__ __launch_bounds__(256) void input_pad_kernel(PadArgs a)
{
    int x0, i;
    if (!ks_cell<8>(a.cW, a.H, x0, i)) return;
    const size_t cW = (size_t)a.cW;
    // x0 < W: cW - 8 < W, so every run holds at least one source column
    const uint2 y0 = ld8_edge(a.p[0] + (long long)(2 * i) * a.pitch[0], x0, a.W);
    const uint2 y1 = ld8_edge(a.p[0] + (long long)(2 * i + 1) * a.pitch[0], x0, a.W);
    uint32_t u[1], v[1];
    if (NV12) ld4_pairs_edge(a.p[1] + (long long)i * a.pitch[1], x0 / 2, a.W / 2, u[0], v[0]);
    else {
        u[0] = ld4_edge(a.p[1] + (long long)i * a.pitch[1], x0 / 2, a.W / 2);
        v[0] = ld4_edge(a.p[2] + (long long)i * a.pitch[2], x0 / 2, a.W / 2);
    }
    uint8_t *dy = a.dst + (size_t)(2 * i) * cW + x0;
    *(uint2 *)dy = y0;
    *(uint2 *)(dy + cW) = y1;
    store_chroma(a.dst, cW, a.cH, i, x0, u, v);
    if (2 * i + 2 == a.H) {                                                // at most 6 luma and 3 chroma rows
        for (int y = a.H; y < a.cH; ++y) *(uint2 *)(a.dst + (size_t)y * cW + x0) = y1;
        for (int y = a.H / 2; y < a.cH / 2; ++y) store_chroma(a.dst, cW, a.cH, y, x0, u, v);
    }
}

// the way back: a thread copies luma columns x0 .. x0 + 7 of rows 2 i, 2 i + 1 and chroma columns x0 / 2 .. + 3 of chroma row i that lie inside w x h.  The source's rows are
// aligned; the destination's rows (w bytes, w / 2 bytes) start anywhere: whole runs are stored as one unaligned word pair / word, the run across the row's end byte by byte
__device__ inline void st_run8(uint8_t *row, int x0, int w, uint2 v)
{
    if (x0 + 8 <= w) { __builtin_memcpy(row + x0, &v, 8); return; }
    const uint32_t q[2] = {v.x, v.y};
#pragma unroll
    for (int k = 0; k < 8; ++k) if (x0 + k < w) row[x0 + k] = (uint8_t)(q[k >> 2] >> 8 * (k & 3));
}
__device__ inline void st_run4(uint8_t *row, int x0, int w, uint32_t v)
{
    if (x0 + 4 <= w) { __builtin_memcpy(row + x0, &v, 4); return; }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (x0 + k < w) row[x0 + k] = (uint8_t)(v >> 8 * k);
}
__global__ __launch_bounds__(256) void output_crop_kernel(const uint8_t *src, int cW, int cH, int w, int h, uint8_t *dst)
{
    int x0, i;
    if (!ks_cell<8>(w, h, x0, i)) return;
    const size_t sW = (size_t)cW, snpx = sW * cH, dW = (size_t)w, dnpx = dW * h;
    const uint8_t *sy = src + (size_t)(2 * i) * sW + x0, *sc = src + snpx + (size_t)i * (sW / 2) + x0 / 2;
    const uint2 y0 = *(const uint2 *)sy, y1 = *(const uint2 *)(sy + sW);
    const uint32_t u = *(const uint32_t *)sc, v = *(const uint32_t *)(sc + snpx / 4);
    st_run8(dst + (size_t)(2 * i) * dW, x0, w, y0);
    st_run8(dst + (size_t)(2 * i + 1) * dW, x0, w, y1);
    st_run4(dst + dnpx + (size_t)i * (dW / 2), x0 / 2, w / 2, u);
    st_run4(dst + dnpx + dnpx / 4 + (size_t)i * (dW / 2), x0 / 2, w / 2, v);
}

// blockIdx.y = the plane.  The strips of a plane of pw x ph whose window is ww x wh: columns ww .. pw - 1 of every row, then rows wh .. ph - 1 of columns 0 .. ww - 1; at most
// 7 columns and 7 rows, a few thousand samples per work-group.  out[plane] -= the strips' squared error: a 64-bit atomic add of the two's complement, exact in any order
__global__ __launch_bounds__(256) void sse_window_kernel(KsGeom g, const uint8_t *ay, const uint8_t *au, const uint8_t *av, const uint8_t *by, const uint8_t *bu, const uint8_t *bv,
                                                         int w, int h, unsigned long long *out)
{
    const int pl = blockIdx.y;
    const int pw = pl ? g.W / 2 : g.W, ph = pl ? g.H / 2 : g.H, ww = pl ? w / 2 : w, wh = pl ? h / 2 : h;
    const long stride = pl ? g.sc : g.sy, org = pl ? g.org_c : g.org_y;
    const uint8_t *a = (pl == 0 ? ay : pl == 1 ? au : av) + org, *b = (pl == 0 ? by : pl == 1 ? bu : bv) + org;
    const int nc = pw - ww, ncol = ph * nc, nbot = (ph - wh) * ww;
    unsigned long long s = 0;
    for (int k = blockIdx.x * 256 + (int)threadIdx.x; k < ncol + nbot; k += gridDim.x * 256) {
        int x, y;
        if (k < ncol) { y = k / nc; x = ww + (k - y * nc); }
        else { const int j = k - ncol; y = wh + j / ww; x = j - (j / ww) * ww; }
        const int d = (int)a[y * stride + x] - (int)b[y * stride + x];
        s += (unsigned)(d * d);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd(out + pl, 0ull - t);
    }
}

int pad_check(ks265_ctx *c, const ks265_in_desc *d, int cw, int ch)
{
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12) { c->last_error = "pad: 8-bit I420 or NV12 only"; return KS265_NOTSUPPORTED; }
    const long long W = d->width, H = d->height;
    if (W <= 0 || H <= 0 || (W & 1) || (H & 1) || (cw & 7) || (ch & 7) || cw < W || cw >= W + 8 || ch < H || ch >= H + 8) {
        c->last_error = "pad: width and height even, the coded size theirs rounded up to a multiple of 8"; return KS265_NOTSUPPORTED;
    }
    const bool nv12 = d->format == KS265_IN_NV12;
    if (d->pitch[0] < W || d->pitch[1] < (nv12 ? W : W / 2) || (!nv12 && d->pitch[2] < W / 2)) { c->last_error = "pad: pitch below the row's bytes"; return KS265_NOTSUPPORTED; }
    return ks_check_planes_420(c, d, nv12);
}

}  // namespace

extern "C" {

int ks265_input_pad_validate(ks265_ctx *c, const ks265_in_desc *d, int coded_w, int coded_h)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    return pad_check(c, d, coded_w, coded_h);
}

int ks265_input_pad(ks265_ctx *c, const ks265_in_desc *d, int coded_w, int coded_h, uint8_t *dst)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    int r = pad_check(c, d, coded_w, coded_h);
    if (r) return r;
    if ((r = ks_check_slot(c, dst, (long long)coded_w * coded_h * 3 / 2, "pad", "destination"))) return r;
    PadArgs a = {};
    for (int k = 0; k < 3; ++k) { a.p[k] = (const uint8_t *)d->plane[k]; a.pitch[k] = d->pitch[k]; }
    a.W = d->width; a.H = d->height; a.cW = coded_w; a.cH = coded_h; a.dst = dst;
    const KsCellLaunch l = ks_cell_launch(coded_w, d->height, 8);
    if (d->format == KS265_IN_NV12) hipLaunchKernelGGL(input_pad_kernel<true>, l.grid, l.blk, 0, c->stream, a);
    else hipLaunchKernelGGL(input_pad_kernel<false>, l.grid, l.blk, 0, c->stream, a);
    return ks265_check_launch(c);
}

int ks265_output_crop(ks265_ctx *c, const uint8_t *src, int coded_w, int coded_h, int w, int h, uint8_t *dst)
{
    if (!c) return KS265_POINTER;
    ks_use_device(c);
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || (coded_w & 7) || (coded_h & 7) || coded_w < w || coded_w >= w + 8 || coded_h < h || coded_h >= h + 8) {
        c->last_error = "crop: width and height even, the coded size theirs rounded up to a multiple of 8"; return KS265_NOTSUPPORTED;
    }
    if ((uintptr_t)src & 7) { c->last_error = "crop: source not 8-byte aligned"; return KS265_NOTSUPPORTED; }
    const long long sb = (long long)coded_w * coded_h * 3 / 2, db = (long long)w * h * 3 / 2;
    int r = ks265_check_extent(c, src, sb, 1, sb, "source");
    if (!r) r = ks265_check_extent(c, dst, db, 1, db, "destination");
    if (r) return r;
    const KsCellLaunch l = ks_cell_launch(w, h, 8);
    hipLaunchKernelGGL(output_crop_kernel, l.grid, l.blk, 0, c->stream, src, coded_w, coded_h, w, h, dst);
    return ks265_check_launch(c);
}

int ks265_sse_window(ks265_ctx *c, ks265_frame *f, ks265_pic a, ks265_pic b, int w, int h, uint64_t *dev_sse3)
{
    KS_FRAME_CHECK(f);
    if (!c || !dev_sse3 || !a.y || !a.u || !a.v || !b.y || !b.u || !b.v) return KS265_POINTER;
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || w > f->g.W || f->g.W >= w + 8 || h > f->g.H || f->g.H >= h + 8) {
        c->last_error = "sse window: width and height even, the frame's size theirs rounded up to a multiple of 8"; return KS265_NOTSUPPORTED;
    }
    if (w == f->g.W && h == f->g.H) return KS265_OK;                   // no strips
    ks_use_device(c);
    hipLaunchKernelGGL(sse_window_kernel, dim3(8, 3), dim3(256), 0, c->stream, f->g, a.y, a.u, a.v, b.y, b.u, b.v, w, h, (unsigned long long *)dev_sse3);
    return ks265_check_launch(c);
}

}  // extern "C"
