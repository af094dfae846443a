// roi_map.hip — the caller's per-picture quantiser offset map (include/ks265_hip.h ks265_roi_*; tests/roi_map_ref.py is the specification):
//   ks265_roi_reduce   the map (int8 or float32, one element per b x b luma block, b = 1 .. 64) -> one int32 per CTU, the CTU's mean offset in 1/256 QP.  Integer sums
//                      only, so the result does not depend on the order of summation.  Bandwidth-shaped (a per-pixel float mask at 2160p is 33 MB read for 2 040 words
//                      written): one work-group per CTU, every lane's loads issued before their first use, 16-byte loads where base and pitch allow (chosen per launch),
//                      a wave reduction by shuffles and one LDS step across the waves; no atomics.  Maps of 16 x 16 blocks and coarser (<= 16 elements per CTU): a lane per CTU.
//   ks265_roi_ctu_map  the CTU's QP from the record and the mean of the CTU's AQ / cuTree block offsets: without a record bit for bit aq_ctu_map_kernel / qoff_ctu_map_kernel.
#include "ks265_internal.h"

namespace {

struct RoiArgs {
    const uint8_t *data; long long pitch;
    int mw, mh;                   // the map's size in elements
    int n;                        // elements per CTU side, 64 >> log2_block
    int cols, rows;               // CTUs
    int32_t *rec;
};

__device__ __forceinline__ int q8_of(int8_t v) { const int x = v; return (x < -51 ? -51 : x > 51 ? 51 : x) * 256; }
__device__ __forceinline__ int q8_of_bits(uint32_t u)
{
    if ((u & 0x7f800000u) == 0x7f800000u) return 0;                    // NaN, +-Inf
    float v = __uint_as_float(u);
    v = v < -51.0f ? -51.0f : v > 51.0f ? 51.0f : v;
    return (int)rintf(v * 256.0f);                                      // the product is exact; half to even
}
__device__ __forceinline__ int q8_of(float v) { return q8_of_bits(__float_as_uint(v)); }
template <typename T> __device__ __forceinline__ int q8_of_word(uint32_t w);
template <> __device__ __forceinline__ int q8_of_word<float>(uint32_t w) { return q8_of_bits(w); }
template <> __device__ __forceinline__ int q8_of_word<int8_t>(uint32_t w)
{
    return q8_of((int8_t)(w & 255)) + q8_of((int8_t)(w >> 8 & 255)) + q8_of((int8_t)(w >> 16 & 255)) + q8_of((int8_t)(w >> 24));
}

// floor((2 S + cnt) / (2 cnt))
__device__ __forceinline__ int record_of(int S, int cnt)
{
    const int num = 2 * S + cnt, den = 2 * cnt;
    int q = num / den;
    if (num % den != 0 && num < 0) --q;
    return q;
}

// the work-group's sum: shuffles inside a wave, one LDS step across the waves (every thread of the group calls it)
__device__ __forceinline__ int group_sum(int v, int *part)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    const int nw = (int)blockDim.x >> 6;
    if (nw == 1) return v;
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int k = 0; k < nw; ++k) s += part[k];
    return s;
}

// One work-group (64 .. 256 threads) per CTU, log2_block 0 .. 3 (n = 64 .. 8).  VEC: base and pitch are multiples of 16 and so is a CTU's row (n * sizeof(T)): the CTU is
// n * n * sizeof(T) / 16 chunks of 16 bytes, at most 4 per thread; a chunk that the map's right edge cuts is read element by element.  Otherwise one element per load,
// at most 16 per thread.  No load reaches beyond [row start, row start + mw * sizeof(T)) of a row below mh.
template <typename T, bool VEC> __global__ __launch_bounds__(256) void roi_reduce_kernel(RoiArgs a)
{
    __shared__ int part[4];
    const int cx = blockIdx.x, cy = blockIdx.y, n = a.n, t = threadIdx.x, nt = blockDim.x;
    const int x0 = cx * n, y0 = cy * n;
    const int w = min(n, a.mw - x0), h = min(n, a.mh - y0);            // >= 1 each: the grid is the CTUs of the picture
    int sum = 0;
    if constexpr (VEC) {
        constexpr int EPC = 16 / (int)sizeof(T);                       // elements per chunk
        const int cpr = n / EPC, total = cpr * h;                      // chunks per CTU row; rows beyond the map are no chunks at all
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = t + k * nt;
            v[k] = make_uint4(0, 0, 0, 0);
            if (idx < total) {
                const int r = idx / cpr, c = (idx - r * cpr) * EPC;
                const uint8_t *p = a.data + (long long)(y0 + r) * a.pitch + (long long)(x0 + c) * (long long)sizeof(T);
                if (c + EPC <= w) v[k] = *(const uint4 *)p;
                else if (c < w) {                                      // the right edge's chunk: the elements inside the map only, v[k] stays zero
                    const T *e = (const T *)p;
                    for (int i = 0; i < w - c; ++i) sum += q8_of(e[i]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)                                    // (a chunk that was not loaded is zeros: int8 0 and float +0.0 both count 0)
            sum += q8_of_word<T>(v[k].x) + q8_of_word<T>(v[k].y) + q8_of_word<T>(v[k].z) + q8_of_word<T>(v[k].w);
    } else {
        const int total = n * h;
        T v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int idx = t + k * nt;
            v[k] = (T)0;
            if (idx < total) {
                const int r = idx / n, c = idx - r * n;
                if (c < w) v[k] = *(const T *)(a.data + (long long)(y0 + r) * a.pitch + (long long)(x0 + c) * (long long)sizeof(T));
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) sum += q8_of(v[k]);
    }
    const int S = group_sum(sum, part);
    if (t == 0) a.rec[cy * a.cols + cx] = record_of(S, w * h);
}

// log2_block 4 .. 6: 16, 4 or 1 elements per CTU - a lane per CTU
template <typename T> __global__ __launch_bounds__(64) void roi_reduce_coarse_kernel(RoiArgs a)
{
    const int ctu = blockIdx.x * 64 + threadIdx.x;
    if (ctu >= a.cols * a.rows) return;
    const int cx = ctu % a.cols, cy = ctu / a.cols, n = a.n;
    const int x0 = cx * n, y0 = cy * n, w = min(n, a.mw - x0), h = min(n, a.mh - y0);
    T v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = k >> 2, c = k & 3;
        v[k] = (T)0;
        if (r < h && c < w) v[k] = *(const T *)(a.data + (long long)(y0 + r) * a.pitch + (long long)(x0 + c) * (long long)sizeof(T));
    }
    int S = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) S += q8_of(v[k]);
    a.rec[ctu] = record_of(S, w * h);
}

// tests/roi_map_ref.py ctu_map: the sum in the loop order of aq_ctu_map_kernel / qoff_ctu_map_kernel, the record (if any) added to the mean before the rounding
__global__ __launch_bounds__(64) void roi_ctu_map_kernel(const int32_t *rec, const double *off, int nx, int ny, int bpc, int cols, int rows, int base_qp, int lo, int hi, int8_t *map)
{
    const int ctu = blockIdx.x * 64 + threadIdx.x;
    if (ctu >= cols * rows) return;
    const int cx = ctu % cols, cy = ctu / cols;
    double sum = 0.0; int cnt = 0;
    if (off)
        for (int by = cy * bpc; by < min(cy * bpc + bpc, ny); ++by)
            for (int bx = cx * bpc; bx < min(cx * bpc + bpc, nx); ++bx) { sum += off[by * nx + bx]; ++cnt; }
    const double mean = cnt ? sum / (double)cnt : 0.0;
    int d = rec ? (int)floor(mean + (double)rec[ctu] / 256.0 + 0.5) : (int)floor(mean + 0.5);
    d = d < -12 ? -12 : d > 12 ? 12 : d;                               // CuQpDeltaVal stays inside [-26, 25] (7.4.9.14)
    const int q = base_qp + d;
    map[ctu] = (int8_t)(q < lo ? lo : q > hi ? hi : q);
}

int elem_size(int type) { return type == KS265_ROI_INT8 ? 1 : type == KS265_ROI_FLOAT32 ? 4 : 0; }

int check_roi(ks265_ctx *c, const ks265_roi_desc *d)
{
    const int es = elem_size(d->type);
    if (!es) { c->last_error = "roi: element type int8 or float32"; return KS265_NOTSUPPORTED; }
    if (d->log2_block < 0 || d->log2_block > 6) { c->last_error = "roi: log2_block 0 .. 6"; return KS265_NOTSUPPORTED; }
    if (d->cols <= 0 || d->rows <= 0 || d->cols > 65536 || d->rows > 65536) { c->last_error = "roi: map size"; return KS265_NOTSUPPORTED; }
    if (d->pitch < (long long)d->cols * es || d->pitch % es) { c->last_error = "roi: pitch at least the row and a multiple of the element size"; return KS265_NOTSUPPORTED; }
    if (!d->data) { c->last_error = "roi: NULL"; return KS265_POINTER; }
    if ((uintptr_t)d->data % (uintptr_t)es) { c->last_error = "roi: map not aligned to its element size"; return KS265_POINTER; }
    return ks265_check_extent(c, d->data, d->pitch, d->rows, (long long)d->cols * es, "roi map");
}

}  // namespace

extern "C" {

int ks265_roi_validate(ks265_ctx *c, const ks265_roi_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    return check_roi(c, d);
}

int ks265_roi_reduce(ks265_ctx *c, const ks265_roi_desc *d, int width, int height, int32_t *dev_records)
{
    if (!c || !d || !dev_records) return KS265_POINTER;
    ks_use_device(c);
    int r = check_roi(c, d);
    if (r) return r;
    if (width <= 0 || height <= 0 || width > 65536 || height > 65536) { c->last_error = "roi: picture size"; return KS265_NOTSUPPORTED; }
    const int b = 1 << d->log2_block;
    if (d->cols != (width + b - 1) / b || d->rows != (height + b - 1) / b) { c->last_error = "roi: the map is not ceil(width / block) x ceil(height / block)"; return KS265_NOTSUPPORTED; }
    RoiArgs a = {};
    a.data = (const uint8_t *)d->data; a.pitch = d->pitch; a.mw = d->cols; a.mh = d->rows; a.n = 64 >> d->log2_block;
    a.cols = (width + 63) / 64; a.rows = (height + 63) / 64; a.rec = dev_records;
    if ((uintptr_t)dev_records & 3) { c->last_error = "roi: records not 4-byte aligned"; return KS265_POINTER; }
    if ((r = ks265_check_extent(c, dev_records, (long long)a.cols * a.rows * 4, 1, (long long)a.cols * a.rows * 4, "roi records"))) return r;
    const bool f32 = d->type == KS265_ROI_FLOAT32;
    if (d->log2_block >= 4) {
        const dim3 grid((unsigned)((a.cols * a.rows + 63) / 64)), blk(64);
        if (f32) hipLaunchKernelGGL(roi_reduce_coarse_kernel<float>, grid, blk, 0, c->stream, a);
        else hipLaunchKernelGGL(roi_reduce_coarse_kernel<int8_t>, grid, blk, 0, c->stream, a);
        return ks265_check_launch(c);
    }
    const int es = f32 ? 4 : 1, row_bytes = a.n * es;
    const bool vec = row_bytes % 16 == 0 && !((uintptr_t)d->data & 15) && d->pitch % 16 == 0;
    const int items = vec ? a.n * (row_bytes / 16) : a.n * a.n;           // chunks or elements of a whole CTU: at most 4 / 16 per thread of 256
    const int nt = items >= 256 ? 256 : items <= 64 ? 64 : (items + 63) / 64 * 64;
    const dim3 grid((unsigned)a.cols, (unsigned)a.rows), blk((unsigned)nt);
    if (f32) {
        if (vec) hipLaunchKernelGGL((roi_reduce_kernel<float, true>), grid, blk, 0, c->stream, a);
        else hipLaunchKernelGGL((roi_reduce_kernel<float, false>), grid, blk, 0, c->stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((roi_reduce_kernel<int8_t, true>), grid, blk, 0, c->stream, a);
        else hipLaunchKernelGGL((roi_reduce_kernel<int8_t, false>), grid, blk, 0, c->stream, a);
    }
    return ks265_check_launch(c);
}

int ks265_roi_ctu_map(ks265_ctx *c, const int32_t *dev_records, const double *dev_base, int nx, int ny, int blocks_per_ctu_side, int ctu_cols, int ctu_rows,
                      int base_qp, int qp_lo, int qp_hi, int8_t *dev_map)
{
    if (!c || !dev_map) return KS265_POINTER;
    if (ctu_cols <= 0 || ctu_rows <= 0 || qp_lo > qp_hi) return KS265_NOTSUPPORTED;
    if (dev_base && (nx <= 0 || ny <= 0 || blocks_per_ctu_side < 1 || blocks_per_ctu_side > 64)) return KS265_NOTSUPPORTED;
    ks_use_device(c);
    const int n = ctu_cols * ctu_rows;
    hipLaunchKernelGGL(roi_ctu_map_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, dev_records, dev_base, nx, ny, blocks_per_ctu_side, ctu_cols, ctu_rows, base_qp, qp_lo, qp_hi, dev_map);
    return ks265_check_launch(c);
}

}  // extern "C"
