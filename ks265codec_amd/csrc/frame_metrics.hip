// frame_metrics.hip — picture quality figures beside the SSE of frame_util.hip: the reference's `-ssim`, with the SSE from the same read of the two pictures.
//
// Definition (pinned on the reference's printed numbers, tests/ssim_ref.py): per plane 8x8 windows, non-overlapping, from sample (0, 0); a window that is not wholly inside the
// plane is dropped; per window, from the integer sums sa, sb, saa, sbb, sab of its 64 samples,
//     ssim = (2 sa sb + K1) (2 (64 sab - sa sb) + K2) / ((sa^2 + sb^2 + K1) (64 (saa + sbb) - sa^2 - sb^2 + K2)),   K1 = 4096 C1, K2 = 4096 C2
// (the textbook form times 64^2 top and bottom: every term but the constants is an exact integer).  The kernel sums llrint(ssim x 2^30) per plane in 64-bit integers.
#include "frame_common.h"

using namespace ks265;

#define KS_SSIM_K1 (4096.0 * (0.01 * 255) * (0.01 * 255))
#define KS_SSIM_K2 (4096.0 * (0.03 * 255) * (0.03 * 255))

// v_sad_u8 against zero = the sum of four bytes; v_dot4_u32_u8 = the sum of four byte products
__device__ __forceinline__ unsigned sum_u8x4(unsigned v, unsigned acc) { return __builtin_amdgcn_sad_u8(v, 0u, acc); }
__device__ __forceinline__ unsigned dot_u8x4(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_udot4(a, b, acc, false); }

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// A lane owns a window, a wave 64 horizontally adjacent windows of a window row (each of the 8 rows is one contiguous 512-byte read per picture), the (window row, 64-window
// chunk) items of a plane are dealt round-robin to the waves of the plane's work-groups.  One launch for the three planes: the first nb_y work-groups take luma, then nb_c
// each for Cb and Cr - luma has four times the windows, and a plane per blockIdx.y would leave the chroma work-groups idle three quarters of the time.
// acc: [0..2] SSE, [3..5] SSIM sums (two's complement), [6] work-groups done; all zero between calls.
__global__ __launch_bounds__(256) void ssim_picture_kernel(KsGeom g, const uint8_t *ay, const uint8_t *au, const uint8_t *av, const uint8_t *by, const uint8_t *bu, const uint8_t *bv,
                                                           int nb_y, int nb_c, unsigned long long *acc, unsigned long long *out_sse /* may be null */, long long *out_ssim)
{
    const int pl = (int)blockIdx.x < nb_y ? 0 : (int)blockIdx.x < nb_y + nb_c ? 1 : 2;
    const int blk = (int)blockIdx.x - (pl == 0 ? 0 : pl == 1 ? nb_y : nb_y + nb_c), nblk = pl ? nb_c : nb_y;
    const int w = pl ? g.W / 2 : g.W, h = pl ? g.H / 2 : g.H;
    const long stride = pl ? g.sc : g.sy, org = pl ? g.org_c : g.org_y;
    const uint8_t *a = (pl == 0 ? ay : pl == 1 ? au : av) + org, *b = (pl == 0 ? by : pl == 1 ? bu : bv) + org;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwx = w >> 3, nwy = h >> 3, chunks = (nwx + 63) >> 6;
    // a window's rows start 8 x its column into 8-byte aligned rows - or, a plane base or stride that is only 4-byte aligned (chroma in general), as two dwords
    const bool wide = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)stride) & 7) == 0;
    unsigned long long sse = 0;
    long long fix = 0;
    for (int it = blk * 4 + wave; it < nwy * chunks; it += nblk * 4) {
        const int wy = it / chunks, wx = (it - wy * chunks) * 64 + lane;
        if (wx >= nwx) continue;                                       // the last chunk of a row: the samples right of the last whole window (and the border) enter no sum
        const uint8_t *pa = a + (long)(wy * 8) * stride + wx * 8, *pb = b + (long)(wy * 8) * stride + wx * 8;
        // all 16 loads of the window are issued before the first use: the kernel is a latency chain otherwise (as sse_picture_kernel)
        uint2 va[8], vb[8];
        if (wide) {
#pragma unroll
            for (int r = 0; r < 8; ++r) { va[r] = *(const uint2 *)(pa + r * stride); vb[r] = *(const uint2 *)(pb + r * stride); }
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                va[r] = make_uint2(*(const unsigned *)(pa + r * stride), *(const unsigned *)(pa + r * stride + 4));
                vb[r] = make_uint2(*(const unsigned *)(pb + r * stride), *(const unsigned *)(pb + r * stride + 4));
            }
        }
        unsigned sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;            // <= 64 x 255 and <= 64 x 255^2 < 2^22
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            sa = sum_u8x4(va[r].y, sum_u8x4(va[r].x, sa)); sb = sum_u8x4(vb[r].y, sum_u8x4(vb[r].x, sb));
            saa = dot_u8x4(va[r].y, va[r].y, dot_u8x4(va[r].x, va[r].x, saa));
            sbb = dot_u8x4(vb[r].y, vb[r].y, dot_u8x4(vb[r].x, vb[r].x, sbb));
            sab = dot_u8x4(va[r].y, vb[r].y, dot_u8x4(va[r].x, vb[r].x, sab));
        }
        sse += saa + sbb - 2u * sab;                                   // sum (a - b)^2 of the window
        // sa sb and sa^2 + sb^2 fit 32 bits unsigned ((64 x 255)^2 < 2^28); the covariance term is signed, |64 sab - sa sb| and 64 (saa + sbb) < 2^29.1: int
        const unsigned pab = sa * sb, paa = sa * sa + sb * sb;
        const int cov = (int)(64u * sab) - (int)pab, var = (int)(64u * (saa + sbb)) - (int)paa;
        const double num = (2.0 * (double)pab + KS_SSIM_K1) * (2.0 * (double)cov + KS_SSIM_K2);
        const double den = ((double)paa + KS_SSIM_K1) * ((double)var + KS_SSIM_K2);
        fix += __double2ll_rn(num / den * 1073741824.0);              // IEEE division (no fast-math in this build); x 2^30 is exact
    }
    // the SSE also counts what the window rule leaves out: the columns right of the last whole window (all rows) and the rows below the last window row (the columns of
    // whole windows); plane widths are multiples of 4 (picture sizes are multiples of 8), rows at least 4-byte aligned
    {
        const int x0 = nwx * 8, y0 = nwy * 8, cw = (w - x0) >> 2, bw = x0 >> 2;
        const int ncol = h * cw, nbot = (h - y0) * bw;
        unsigned s = 0;
        for (int i = blk * 256 + (int)threadIdx.x; i < ncol + nbot; i += nblk * 256) {
            int x, y;
            if (i < ncol) { y = i / cw; x = x0 + (i - y * cw) * 4; }
            else { const int j = i - ncol; y = y0 + j / bw; x = (j - (j / bw) * bw) * 4; }
            const unsigned p = *(const unsigned *)(a + y * stride + x), q = *(const unsigned *)(b + y * stride + x);
            s = dot_u8x4(p, p, s); s = dot_u8x4(q, q, s); s -= 2u * dot_u8x4(p, q, 0u);
        }
        sse += s;
    }
    const unsigned long long sse_w = wave_sum64(sse), fix_w = wave_sum64((unsigned long long)fix);
    __shared__ unsigned long long part[4][2];
    if (lane == 0) { part[wave][0] = sse_w; part[wave][1] = fix_w; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = part[0][0] + part[1][0] + part[2][0] + part[3][0], u = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (t) atomicAdd(acc + pl, t);
        if (u) atomicAdd(acc + 3 + pl, u);
        __threadfence();
        // the last work-group to finish hands the sums out and leaves the accumulators zeroed for the next call (no memset launch per picture)
        if (atomicAdd(acc + 6, 1ull) == (unsigned long long)gridDim.x - 1ull) {
            __threadfence();
            for (int i = 0; i < 3; ++i) {
                const unsigned long long s = atomicExch(acc + i, 0ull), v = atomicExch(acc + 3 + i, 0ull);
                if (out_sse) out_sse[i] = s;
                out_ssim[i] = (long long)v;
            }
            atomicExch(acc + 6, 0ull);
        }
    }
}

extern "C" int ks265_ssim_picture_on(ks265_ctx *cx, ks265_frame *f, ks265_pic a, ks265_pic b, uint64_t *sse3, int64_t *ssim3)
{
    KS_FRAME_CHECK(f);
    if (!ssim3 || !cx) return KS265_POINTER;
    ks_use_device(cx);
    // few work-groups, each over many window rows (every work-group ends in three atomics on the same words); never more than a plane has items for four waves
    const int items_y = (f->g.H / 8) * ((f->g.W / 8 + 63) / 64), items_c = (f->g.H / 16) * ((f->g.W / 16 + 63) / 64);
    const int nb_y = items_y >= 512 ? 128 : items_y >= 4 ? (items_y + 3) / 4 : 1, nb_c = items_c >= 128 ? 32 : items_c >= 4 ? (items_c + 3) / 4 : 1;
    hipLaunchKernelGGL(ssim_picture_kernel, dim3(nb_y + 2 * nb_c), dim3(256), 0, cx->stream, f->g, a.y, a.u, a.v, b.y, b.u, b.v, nb_y, nb_c, f->ssim_acc,
                       (unsigned long long *)sse3, (long long *)ssim3);
    return ks265_check_launch(cx);
}
extern "C" int ks265_ssim_picture(ks265_frame *f, ks265_pic a, ks265_pic b, uint64_t *sse3, int64_t *ssim3) { return f ? ks265_ssim_picture_on(f->ctx, f, a, b, sse3, ssim3) : KS265_POINTER; }
