// input_denoise.hip — `vpp_denoise` / `vpp_recur_filter`: the motion-compensated temporal filter on the way in (tests/denoise_ref.py is the specification of every
// byte).  One launch per picture, luma and both chroma planes: the current packed I420 picture C of W x H (multiples of 8) is filtered IN PLACE against the previous filtered
// picture P (the history) and the result is also written to the next history.
//
// A work-group of four waves owns a 64x16 luma tile, a wave one 16x16 block of it (an edge block is the 8-wide / 8-tall remainder):
//   staging   the tile of C (64x16) and the history window around it ((64 + 16 + 4) x (16 + 16) bytes, pitch 84 = 21 dwords: odd, so the rows of neighbouring candidates spread
//             over the banks) go to LDS as whole dwords.  The window hangs over the picture at its edges: THE GLOBAL ADDRESS OF EVERY STAGED DWORD IS CLAMPED INTO THE PICTURE
//             (column to [0, W - 4], row to [0, H - 1]).  A dword lies wholly inside or wholly outside (x, W multiples of 4); what a clamped one holds is never used: a
//             candidate whose displaced block leaves the picture is masked, not read.
//   search    the 17 x 17 = 289 candidates of a block over the 64 lanes (5 rounds), a lane sums one candidate's whole block: C's rows in registers (64 dwords, read once from
//             LDS), the window's rows as dwords + v_alignbyte for the column's byte offset, v_sad_u8 on the packed bytes.  cost = SAD + 16 (|dx| + |dy|) < 2^17; the argmin is ONE
//             32-bit key cost << 15 | l1 << 10 | dy + 8 << 5 | dx + 8, whose order is the reference's tie rule (cost, l1, dy, dx); the wave's minimum by DPP / ds_swizzle.
//   blend     the winner is wave-uniform.  Luma: a lane owns one dword (4 samples) of the block, C from the LDS tile, P from the window.  Chroma: a lane owns one sample of the
//             8x8 block of each plane; its prediction is the rounded mean of the 2x2 history samples at (dx >> 1, dy >> 1) + (0 .. dx & 1, 0 .. dy & 1), read from global memory
//             (L2: the luma window's rows were just fetched next to them) - inside the plane for every valid vector (tests/denoise_ref.py).  The weight per |c - p| comes from
//             two 64-entry tables in LDS (luma: T, chroma: (T + 1) >> 1), built once per work-group with the reference's integer division.
//   in place  a wave reads its block of C (LDS tile, and its own chroma samples) before it writes it, blocks are disjoint, and nothing else reads C; P is read across blocks
//             and is never written: the entry refuses a history-out or a picture that overlaps the history-in.
// No scratch, no atomics.
#include "frame_common.h"

using namespace ks265;

namespace {

constexpr int DN_RANGE = 8, DN_LAMBDA = 16, DN_TW = 64, DN_TH = 16;
constexpr int DN_WIN_P = DN_TW + 2 * DN_RANGE + 4, DN_WIN_ROWS = DN_TH + 2 * DN_RANGE;      // 84 x 32 bytes

struct DnArgs {
    uint8_t *cur;                 // in and out
    const uint8_t *hist;          // NULL: no history
    uint8_t *hist_out;
    int32_t *blocks;              // NULL: not wanted
    int W, H, thr, weight;
};

struct DnLds {
    uint8_t win[DN_WIN_ROWS * DN_WIN_P];
    uint8_t cur[DN_TH * DN_TW];
    uint8_t wt[2][64];            // the blend weight per |c - p| (0 from the threshold on): luma, chroma
};

__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    v = min(v, (unsigned)dpp_mov<KS265_DPP_QUAD_XOR1>((int)v));
    v = min(v, (unsigned)dpp_mov<KS265_DPP_QUAD_XOR2>((int)v));
    v = min(v, (unsigned)dpp_mov<KS265_DPP_ROW_HALF_MIRROR>((int)v));
    v = min(v, (unsigned)dpp_mov<KS265_DPP_ROW_MIRROR>((int)v));
    v = min(v, (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (16 << 10)));
    v = min(v, (unsigned)__shfl_xor((int)v, 32, 64));
    return v;
}

// the lane's candidates of a block of 4 BW4 x BH samples at (bx, by); win: the window's byte at the block's column, row 0 (= picture row by - 8, column bx - 8)
template <int BW4, int BH> __device__ __forceinline__ unsigned block_search(const uint8_t *win, const uint8_t *cur, int bx, int by, int W, int H, int lane)
{
    unsigned c[BH * BW4];
#pragma unroll
    for (int r = 0; r < BH; ++r)
#pragma unroll
        for (int q = 0; q < BW4; ++q) c[r * BW4 + q] = *(const unsigned *)(cur + r * DN_TW + 4 * q);
    unsigned best = ~0u;
#pragma unroll 1
    for (int k = lane; k < 320; k += 64) {
        const int dy = k / 17 - DN_RANGE, dx = k - (k / 17) * 17 - DN_RANGE;
        const bool ok = k < 289 && bx + dx >= 0 && bx + dx + 4 * BW4 <= W && by + dy >= 0 && by + dy + BH <= H;
        const int col = DN_RANGE + (ok ? dx : 0), row = DN_RANGE + (ok ? dy : 0);       // a masked candidate reads (and discards) the centre
        const uint8_t *p = win + row * DN_WIN_P + (col & ~3);
        const unsigned sh = col & 3;
        unsigned sd = 0;
#pragma unroll
        for (int r = 0; r < BH; ++r) {
            unsigned w[BW4 + 1];
#pragma unroll
            for (int q = 0; q <= BW4; ++q) w[q] = *(const unsigned *)(p + r * DN_WIN_P + 4 * q);
#pragma unroll
            for (int q = 0; q < BW4; ++q) sd = sad_u8x4(c[r * BW4 + q], align_bytes(w[q + 1], w[q], sh), sd);
        }
        const unsigned l1 = (unsigned)(abs(dx) + abs(dy));
        const unsigned key = (sd + DN_LAMBDA * l1) << 15 | l1 << 10 | (unsigned)(dy + DN_RANGE) << 5 | (unsigned)(dx + DN_RANGE);
        best = min(best, ok ? key : ~0u);
    }
    return wave_min_u32(best);
}

__device__ __forceinline__ unsigned blend1(unsigned c, unsigned p, const uint8_t *wt)
{
    const unsigned d = c > p ? c - p : p - c;
    const unsigned w = wt[d < 63 ? d : 63];                              // the weight is 0 from d = thr <= 64 on, and at d = 63 too: 2 * 30 * (64 - 63) / 64 = 0
    return (c * (32 - w) + p * w + 16) >> 5;
}
__device__ __forceinline__ unsigned blend4(unsigned c, unsigned p, const uint8_t *wt)
{
    unsigned o = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) o |= blend1(c >> 8 * k & 255u, p >> 8 * k & 255u, wt) << 8 * k;
    return o;
}

__global__ __launch_bounds__(256) void input_denoise_kernel(DnArgs a)
{
    __shared__ __attribute__((aligned(16))) DnLds L;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int W = a.W, H = a.H, tx = blockIdx.x * DN_TW, ty = blockIdx.y * DN_TH;
    const size_t npx = (size_t)W * H;
    // ---- staging: whole dwords, every global address clamped into the picture
    for (int i = t; i < DN_TH * DN_TW / 4; i += 256) {
        const int r = i / (DN_TW / 4), q = i - r * (DN_TW / 4);
        const int x = min(tx + 4 * q, W - 4), y = min(ty + r, H - 1);
        *(unsigned *)(L.cur + r * DN_TW + 4 * q) = *(const unsigned *)(a.cur + (size_t)y * W + x);
    }
    if (a.hist)
        for (int i = t; i < DN_WIN_ROWS * (DN_WIN_P / 4); i += 256) {
            const int r = i / (DN_WIN_P / 4), q = i - r * (DN_WIN_P / 4);
            const int x = min(max(tx - DN_RANGE + 4 * q, 0), W - 4), y = min(max(ty - DN_RANGE + r, 0), H - 1);
            *(unsigned *)(L.win + r * DN_WIN_P + 4 * q) = *(const unsigned *)(a.hist + (size_t)y * W + x);
        }
    if (t < 128) {
        const int thr = t < 64 ? a.thr : (a.thr + 1) >> 1, d = t & 63;
        const int w = (2 * a.weight * max(0, thr - d)) / thr;
        L.wt[t >> 6][d] = (uint8_t)min(a.weight, w);
    }
    __syncthreads();
    // ---- a wave, a block
    const int bx = tx + 16 * wv, by = ty;
    if (bx >= W) return;                                                // (no barrier below)
    const int bw4 = min(16, W - bx) / 4, bh = min(16, H - by);         // 2 or 4 dwords, 8 or 16 rows
    const uint8_t *win = L.win + 16 * wv, *cur = L.cur + 16 * wv;
    int dx = 0, dy = 0, gated = 1;
    unsigned sad = 0;
    if (a.hist) {
        unsigned key;
        if (bw4 == 4) key = bh == 16 ? block_search<4, 16>(win, cur, bx, by, W, H, lane) : block_search<4, 8>(win, cur, bx, by, W, H, lane);
        else key = bh == 16 ? block_search<2, 16>(win, cur, bx, by, W, H, lane) : block_search<2, 8>(win, cur, bx, by, W, H, lane);
        dx = (int)(key & 31u) - DN_RANGE; dy = (int)(key >> 5 & 31u) - DN_RANGE;
        sad = (key >> 15) - DN_LAMBDA * (key >> 10 & 31u);
        gated = sad >= (unsigned)(a.thr * 4 * bw4 * bh);
    }
    if (a.blocks && lane == 0) {
        int32_t *b = a.blocks + 2 * ((size_t)blockIdx.y * ((W + 15) / 16) + (bx >> 4));
        b[0] = (dx + DN_RANGE) | (dy + DN_RANGE) << 8 | gated << 16;
        b[1] = (int32_t)sad;
    }
    // ---- luma: a lane, a dword
    {
        const int r = lane >> 2, q = lane & 3;
        if (r < bh && q < bw4) {
            unsigned o = *(const unsigned *)(cur + r * DN_TW + 4 * q);
            if (!gated) {
                const int col = DN_RANGE + dx + 4 * q;
                const uint8_t *p = win + (DN_RANGE + dy + r) * DN_WIN_P + (col & ~3);
                o = blend4(o, align_bytes(*(const unsigned *)(p + 4), *(const unsigned *)p, (unsigned)(col & 3)), L.wt[0]);
            }
            const size_t at = (size_t)(by + r) * W + bx + 4 * q;
            if (!gated) *(unsigned *)(a.cur + at) = o;
            *(unsigned *)(a.hist_out + at) = o;
        }
    }
    // ---- chroma: a lane, a sample of each plane
    {
        const int y = lane >> 3, x = lane & 7, cw = W >> 1;
        if (y < bh / 2 && x < 2 * bw4) {
            const size_t at = (size_t)((by >> 1) + y) * cw + (bx >> 1) + x;
            const int fx = dx & 1, fy = dy & 1;
            const size_t h0 = (size_t)((by >> 1) + (dy >> 1) + y) * cw + (bx >> 1) + (dx >> 1) + x;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const size_t off = npx + (pl ? npx / 4 : 0);
                unsigned o = a.cur[off + at];
                if (!gated) {
                    const uint8_t *h = a.hist + off + h0;
                    const unsigned p = ((unsigned)h[0] + h[fx] + h[(size_t)fy * cw] + h[(size_t)fy * cw + fx] + 2) >> 2;
                    o = blend1(o, p, L.wt[1]);
                    a.cur[off + at] = (uint8_t)o;
                }
                a.hist_out[off + at] = (uint8_t)o;
            }
        }
    }
}

int dn_check(ks265_ctx *c, const ks265_denoise_cfg *cfg, int w, int h)
{
    if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || w > 8192 || h > 8192) { c->last_error = "denoise: width and height positive multiples of 8, at most 8192"; return KS265_NOTSUPPORTED; }
    if (cfg->thr < 1 || cfg->thr > 64 || cfg->weight < 1 || cfg->weight > 30) { c->last_error = "denoise: thr 1 .. 64, weight 1 .. 30"; return KS265_NOTSUPPORTED; }
    return KS265_OK;
}

bool dn_overlap(const uint8_t *a, const uint8_t *b, long long n) { return a < b + n && b < a + n; }

}  // namespace

extern "C" {

int ks265_input_denoise_validate(ks265_ctx *c, const ks265_denoise_cfg *cfg, int width, int height)
{
    if (!c || !cfg) return KS265_POINTER;
    return dn_check(c, cfg, width, height);
}

int ks265_input_denoise(ks265_ctx *c, const ks265_denoise_cfg *cfg, int width, int height, uint8_t *dev_i420, const uint8_t *dev_hist_in, uint8_t *dev_hist_out, int32_t *dev_blocks)
{
    if (!c || !cfg) return KS265_POINTER;
    ks_use_device(c);
    int r = dn_check(c, cfg, width, height);
    if (r) return r;
    const long long bytes = (long long)width * height * 3 / 2, nblk = (long long)((width + 15) / 16) * ((height + 15) / 16);
    if (((uintptr_t)dev_i420 | (uintptr_t)dev_hist_in | (uintptr_t)dev_hist_out | (uintptr_t)dev_blocks) & 3) { c->last_error = "denoise: a picture or the block words not 4-byte aligned"; return KS265_NOTSUPPORTED; }
    if ((r = ks265_check_extent(c, dev_i420, bytes, 1, bytes, "picture"))) return r;
    if ((r = ks265_check_extent(c, dev_hist_out, bytes, 1, bytes, "history out"))) return r;
    if (dev_hist_in && (r = ks265_check_extent(c, dev_hist_in, bytes, 1, bytes, "history in"))) return r;
    if (dev_blocks && (r = ks265_check_extent(c, dev_blocks, nblk * 8, 1, nblk * 8, "block words"))) return r;
    if (dn_overlap(dev_i420, dev_hist_out, bytes) || (dev_hist_in && (dn_overlap(dev_hist_in, dev_hist_out, bytes) || dn_overlap(dev_hist_in, dev_i420, bytes)))) {
        c->last_error = "denoise: the picture, the history in and the history out overlap"; return KS265_POINTER;
    }
    const DnArgs a = {dev_i420, dev_hist_in, dev_hist_out, dev_blocks, width, height, cfg->thr, cfg->weight};
    const dim3 grid((unsigned)((width + DN_TW - 1) / DN_TW), (unsigned)((height + DN_TH - 1) / DN_TH));
    hipLaunchKernelGGL(input_denoise_kernel, grid, dim3(256), 0, c->stream, a);
    return ks265_check_launch(c);
}

}  // extern "C"
