// frame_metrics.hip — picture quality figures beside the SSE of frame_util.hip: the reference's `-ssim`, with the SSE from the same read of the two pictures.
//
// Definition (pinned on the reference's printed numbers, tests/ssim_ref.py): per plane 8x8 windows, non-overlapping, from sample (0, 0); a window that is not wholly inside the
// plane is dropped; per window, from the integer sums sa, sb, saa, sbb, sab of its 64 samples,
//     ssim = (2 sa sb + K1) (2 (64 sab - sa sb) + K2) / ((sa^2 + sb^2 + K1) (64 (saa + sbb) - sa^2 - sb^2 + K2)),   K1 = 4096 C1, K2 = 4096 C2
// (the textbook form times 64^2 top and bottom: every term but the constants is an exact integer).  The kernel sums llrint(ssim x 2^30) per plane in 64-bit integers.
//
// Second half: the decoded picture hash of H.265 D.3.19 (picture_crc and picture_checksum of the three planes) from one read of one picture.
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

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------------------
// Decoded picture hash (H.265 D.3.19, 8-bit samples; specification: tests/picture_hash_ref.py).
//
// picture_checksum of a plane = sum over its samples of sample ^ (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8), modulo 2^32: a sum, order-free.
//
// picture_crc of a plane of n bytes (raster order) is the standard's bit loop with P = x^16 + x^12 + x^5 + 1, register preset 0xFFFF, two zero bytes appended.  Over GF(2) that is
//     0xFFFF x^(8 (n + 2))  +  M(x) x^16        (mod P),
// the second term being the zero-preset CRC ("XMODEM") of the bytes, linear in M: a piece of the plane that r more bytes follow contributes xmodem(piece) x^(8 r), and the
// contributions add (XOR) in any order.  A piece that does not exist contributes nothing, wherever it would lie.
//
// Shape.  A lane owns KS_HASH_LANE_BYTES contiguous bytes of a row, a wave a row item of KS_HASH_WAVE_BYTES; the items of a row are aligned to the row's END, so the lanes in
// front of a ragged row's start simply do not exist (nothing is loaded, the border enters nothing) and every distance inside a wave is a constant:
//   - between lanes: x^(8 LANE_BYTES 2^s) at step s of a log-step tree - compile-time constants;
//   - between the items of a row: ka = x^(8 WAVE_BYTES); from a row's last item to the next row's first: kb = x^(8 (w - (items - 1) WAVE_BYTES)).
// A wave takes R consecutive rows and walks their items in raster order keeping ONE running value per lane (acc = acc k + own: every lane multiplies by the same constants, so
// the lane tree can wait until the end of the walk).  Wave slots are aligned to the END of the plane as well (the rows in front of row 0 do not exist), so a work-group's four
// slots are x^(8 w R) = kr apart, and block b of nblocks lies (kr^4)^(nblocks - 1 - b) in front of the plane's end: the one general power, once per work-group.
// A work-group's four waves take different rows: per row item a work-group covers what a wave covers (KS_HASH_WAVE_BYTES samples).
#define KS_HASH_LANE_BYTES 32
#define KS_HASH_WAVE_BYTES (64 * KS_HASH_LANE_BYTES)
#define KS_HASH_MAX_WG_Y 256                                           // work-groups dealt to luma at most; each chroma plane: a quarter
#define KS_HASH_POLY 0x1021u

// a b mod P for 16-bit a, b.  With a wave-uniform or constant b the chain of b x^j leaves the vector unit: what remains per lane is a 16-term XOR
__host__ __device__ constexpr unsigned gf16_mul(unsigned a, unsigned b)
{
    unsigned r = 0;
    for (int j = 0; j < 16; ++j) {
        r ^= (0u - ((a >> j) & 1u)) & b;
        b = ((b << 1) & 0xFFFFu) ^ ((0u - ((b >> 15) & 1u)) & KS_HASH_POLY);
    }
    return r;
}
// x^(8 nbytes) mod P
__host__ __device__ constexpr unsigned gf16_xpow8(unsigned long long nbytes)
{
    unsigned r = 1, q = 0x100u;                                        // x^8
    for (; nbytes; nbytes >>= 1) { if (nbytes & 1) r = gf16_mul(r, q); q = gf16_mul(q, q); }
    return r;
}

template <int M> struct KsHashLaneK { static constexpr unsigned v = gf16_xpow8((unsigned long long)KS_HASH_LANE_BYTES * M); };

// per plane kind (luma, chroma) what the host works out from the plane's size
struct KsHashPlane { unsigned ka, kb, kr, kr4, init; int rows, nwaves, nblocks; };

// zero-preset CRC over the four bytes of a dword, lowest address first; crc's bits above 15 are don't-care on entry and on exit
__device__ __forceinline__ unsigned xmodem_dword(unsigned crc, unsigned d)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned t = ((crc >> 8) ^ (d >> (8 * k))) & 0xFFu;
        t ^= t >> 4;
        crc = (crc << 8) ^ (t << 12) ^ (t << 5) ^ t;
    }
    return crc;
}

// 16 bytes from an address that is 16-, 8- or only 4-byte aligned (mode 2, 1, 0; uniform for a plane)
__device__ __forceinline__ uint4 hash_load16(const uint8_t *p, int mode)
{
    if (mode == 2) return *(const uint4 *)p;
    if (mode == 1) { const uint2 a = *(const uint2 *)p, b = *(const uint2 *)(p + 8); return make_uint4(a.x, a.y, b.x, b.y); }
    return make_uint4(*(const unsigned *)p, *(const unsigned *)(p + 4), *(const unsigned *)(p + 8), *(const unsigned *)(p + 12));
}

// acc: [0..2] CRC parts (XOR), [3..5] checksums (add), [6] work-groups done; all zero between calls.  out: [0..2] picture_crc, [3..5] picture_checksum of Y, Cb, Cr
__global__ __launch_bounds__(256) void picture_hash_kernel(KsGeom g, const uint8_t *py, const uint8_t *pu, const uint8_t *pv, KsHashPlane ky, KsHashPlane kc, unsigned *acc, unsigned *out)
{
    const int nb_y = ky.nblocks, nb_c = kc.nblocks;
    const int pl = (int)blockIdx.x < nb_y ? 0 : (int)blockIdx.x < nb_y + nb_c ? 1 : 2;
    const int b = (int)blockIdx.x - (pl == 0 ? 0 : pl == 1 ? nb_y : nb_y + nb_c);
    const int w = pl ? g.W / 2 : g.W, h = pl ? g.H / 2 : g.H;
    const long stride = pl ? g.sc : g.sy;
    const uint8_t *base = (pl == 0 ? py : pl == 1 ? pu : pv) + (pl ? g.org_c : g.org_y);
    const unsigned ka = pl ? kc.ka : ky.ka, kb = pl ? kc.kb : ky.kb, kr = pl ? kc.kr : ky.kr, kr4 = pl ? kc.kr4 : ky.kr4;
    const int R = pl ? kc.rows : ky.rows, NW = pl ? kc.nwaves : ky.nwaves, nblocks = pl ? kc.nblocks : ky.nblocks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int items = (w + KS_HASH_WAVE_BYTES - 1) / KS_HASH_WAVE_BYTES;
    // a lane's bytes start w - items x WAVE_BYTES + lane x LANE_BYTES + ... into the row: every address is congruent to base + w modulo 16 (strides are multiples of 64)
    const unsigned al = (unsigned)((uintptr_t)base | (uintptr_t)stride | (uintptr_t)w);
    const int mode = (al & 15u) == 0 ? 2 : (al & 7u) == 0 ? 1 : 0;

    // the wave's slot, counted from the plane's end: slot NW - 1 ends with the last row; slots in front of the first (the last block is the full one) do not exist
    const int slot = 4 * b + wave - (4 * nblocks - NW);
    const int r_end = h - (NW - 1 - slot) * R;                          // one past the slot's last row
    const int r_beg = max(r_end - R, 0);
    const int nit = slot >= 0 ? (r_end - r_beg) * items : 0;
    unsigned crc = 0, sum = 0;
    uint4 n0 = make_uint4(0, 0, 0, 0), n1 = n0;
    // item it of the walk: row r_beg + it / items, item it % items; x = where the lane's bytes start in the row (< 0: in front of the row - those bytes do not exist)
    auto load = [&](int it, uint4 &a0, uint4 &a1) {
        const int rr = it / items, c = it - rr * items;
        const int x = w - (items - c) * KS_HASH_WAVE_BYTES + lane * KS_HASH_LANE_BYTES;
        const uint8_t *p = base + (long)(r_beg + rr) * stride + x;
        a0 = a1 = make_uint4(0, 0, 0, 0);
        if (x + 16 > 0) a0 = hash_load16(p, mode);                      // (a half that starts in front of the row reaches at most 12 bytes into the border: inside the padding)
        if (x + 32 > 0) a1 = hash_load16(p + 16, mode);
    };
    if (nit > 0) load(0, n0, n1);
    for (int it = 0; it < nit; ++it) {
        const uint4 c0 = n0, c1 = n1;
        if (it + 1 < nit) load(it + 1, n0, n1);                         // the next item's loads are in flight while this one is hashed
        const int rr = it / items, c = it - rr * items;
        const int y = r_beg + rr, x = w - (items - c) * KS_HASH_WAVE_BYTES + lane * KS_HASH_LANE_BYTES;
        const unsigned d[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const unsigned ym = (unsigned)((y & 0xFF) ^ (y >> 8));
        unsigned own = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int xi = x + 4 * i;                                   // a multiple of 4: the four samples' masks differ in their low two bits only
            const bool there = xi >= 0;
            const unsigned v = there ? d[i] : 0u;
            own = xmodem_dword(own, v);                                 // (zero bytes in front leave a zero-preset CRC as it is)
            const unsigned m = ((unsigned)((xi & 0xFF) ^ (xi >> 8)) ^ ym) & 0xFFu;
            if (there) sum = sum_u8x4(v ^ (m * 0x01010101u ^ 0x03020100u), sum);
        }
        crc = gf16_mul(crc & 0xFFFFu, c == 0 ? kb : ka) ^ (own & 0xFFFFu);   // (the walk's first item multiplies zero)
    }
    // lanes: lane i's bytes end (63 - i) x LANE_BYTES in front of the item's end
    auto lanes = [&](int m, unsigned k) {                             // k = x^(8 LANE_BYTES m), a compile-time constant
        const unsigned t = (unsigned)__shfl_xor((int)crc, m, 64);
        const bool upper = (lane & m) != 0;
        crc = gf16_mul(upper ? t : crc, k) ^ (upper ? crc : t);
    };
    lanes(1, KsHashLaneK<1>::v); lanes(2, KsHashLaneK<2>::v); lanes(4, KsHashLaneK<4>::v); lanes(8, KsHashLaneK<8>::v); lanes(16, KsHashLaneK<16>::v); lanes(32, KsHashLaneK<32>::v);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum += (unsigned)__shfl_xor((int)sum, m, 64);
    __shared__ unsigned part[4][2];
    if (lane == 0) { part[wave][0] = crc; part[wave][1] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned v = part[0][0];
        for (int k = 1; k < 4; ++k) v = gf16_mul(v, kr) ^ part[k][0];
        unsigned f = 1, q = kr4;
        for (int e = nblocks - 1 - b; e; e >>= 1) { if (e & 1) f = gf16_mul(f, q); q = gf16_mul(q, q); }
        v = gf16_mul(v, f);
        const unsigned s = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (v) atomicXor(acc + pl, v);
        if (s) atomicAdd(acc + 3 + pl, s);
        __threadfence();
        // the last work-group to finish adds the preset's term, hands the values out and leaves the accumulators zeroed for the next call (no memset launch per picture)
        if (atomicAdd(acc + 6, 1u) == gridDim.x - 1u) {
            __threadfence();
            for (int i = 0; i < 3; ++i) {
                out[i] = atomicExch(acc + i, 0u) ^ (i ? kc.init : ky.init);
                out[3 + i] = atomicExch(acc + 3 + i, 0u);
            }
            atomicExch(acc + 6, 0u);
        }
    }
}

static KsHashPlane hash_plane_setup(int w, int h, int max_wg)
{
    KsHashPlane k{};
    const int items = (w + KS_HASH_WAVE_BYTES - 1) / KS_HASH_WAVE_BYTES;
    const int nwg = (h + 3) / 4 < max_wg ? (h + 3) / 4 : max_wg;                         // never more work-groups than the plane has rows for four waves
    k.rows = (h + 4 * nwg - 1) / (4 * nwg);
    k.nwaves = (h + k.rows - 1) / k.rows;
    k.nblocks = (k.nwaves + 3) / 4;
    k.ka = gf16_xpow8(KS_HASH_WAVE_BYTES);
    k.kb = gf16_xpow8((unsigned long long)(w - (items - 1) * KS_HASH_WAVE_BYTES));
    k.kr = gf16_xpow8((unsigned long long)w * k.rows);
    k.kr4 = gf16_xpow8((unsigned long long)w * k.rows * 4);
    k.init = gf16_mul(0xFFFFu, gf16_xpow8((unsigned long long)w * h + 2));
    return k;
}

extern "C" int ks265_picture_hash_on(ks265_ctx *cx, ks265_frame *f, ks265_pic p, uint32_t *dev_hash6)
{
    KS_FRAME_CHECK(f);
    if (!dev_hash6 || !cx || !p.y || !p.u || !p.v) return KS265_POINTER;
    ks_use_device(cx);
    const KsHashPlane ky = hash_plane_setup(f->g.W, f->g.H, KS_HASH_MAX_WG_Y), kc = hash_plane_setup(f->g.W / 2, f->g.H / 2, KS_HASH_MAX_WG_Y / 4);
    hipLaunchKernelGGL(picture_hash_kernel, dim3(ky.nblocks + 2 * kc.nblocks), dim3(256), 0, cx->stream, f->g, p.y, p.u, p.v, ky, kc, f->hash_acc, (unsigned *)dev_hash6);
    return ks265_check_launch(cx);
}
extern "C" int ks265_picture_hash(ks265_frame *f, ks265_pic p, uint32_t *dev_hash6) { return f ? ks265_picture_hash_on(f->ctx, f, p, dev_hash6) : KS265_POINTER; }
