// input_enhance.hip — `vpp_edge` / `vpp_color`: edge and colour enhancement on the way in (tests/enhance_ref.py is the specification of every byte).  One launch
// per picture, luma and both chroma planes, no state: the luma of the packed I420 picture of W x H (multiples of 8) is WRITTEN from a copy that does not overlap it (the
// stencil reads neighbours across work-groups), the chroma planes are mapped pointwise IN PLACE.
//
// A work-group of 256 threads owns a 64x16 luma tile and the tile's chroma (32x8 of each plane):
//   staging   the tile with a halo of 2 - rows ty - 2 .. ty + 17, columns tx - 4 .. tx + 67 - goes to LDS as whole dwords, 18 a row at a pitch of 19 (odd: the rows of a wave's
//             lanes spread over the banks).  THE GLOBAL ADDRESS OF EVERY STAGED DWORD IS CLAMPED INTO THE PLANE (column to [0, W - 4], row to [0, H - 1]); a dword lies wholly
//             inside or wholly outside it (tx, W multiples of 4), and one that lies outside does not keep what the clamped load holds: it becomes four copies of the row's
//             first or last sample - the reference's edge replication.  Rows are replicated by the clamp itself.
//   h pass    h = S(x - 2) + 4 S(x - 1) + 6 S(x) + 4 S(x + 1) + S(x + 2) <= 4080 for the 20 x 64 samples, 4 adjacent ones a thread, into an int16 tile: the taps (1 4 6 4) on
//             the packed bytes x - 2 .. x + 1 are one v_dot4_u32_u8 on a v_alignbyte of two staged dwords, the fifth sample one byte extract.
//   v pass    a thread owns 4 adjacent samples of one row: five 8-byte reads of the int16 tile (pitch 32 dwords: the two rows of a 32-lane group fill the 64 banks), the blur
//             in 1/256 of a code, coring, gain, limit; the 3x3 minimum / maximum from the three rows' column minima / maxima; one aligned dword store.
//   chroma    the last wave: a lane loads one dword of U and the co-located dword of V in front of the staging (the latency hides behind it), maps the 4 pairs and stores
//             both where they came from.
// edge_gain == 0: no luma is read or written (dev_luma_src may be NULL); color_gain == 0: no chroma.  No scratch, no atomics.
#include "frame_common.h"

using namespace ks265;

namespace {

constexpr int EN_TW = 64, EN_TH = 16, EN_ROWS = EN_TH + 4, EN_SRC_DW = EN_TW / 4 + 2, EN_SRC_P = EN_SRC_DW + 1;      // 20 rows of 18 dwords at pitch 19

struct EnArgs {
    const uint8_t *src;           // luma in (NULL when edge_gain == 0)
    uint8_t *pic;                 // the picture: luma out, chroma in and out
    int W, H, gain, core, limit, over, cgain;
};

struct EnLds {
    unsigned src[EN_ROWS * EN_SRC_P];
    short h[EN_ROWS * EN_TW];
};

__device__ __forceinline__ unsigned byte_of(unsigned v, int k) { return v >> 8 * k & 255u; }

// one chroma component of a pair: c = the sample, K = the pair's gain in 1/8192
__device__ __forceinline__ unsigned color1(unsigned s, int K)
{
    const int c = (int)s - 128, m = (abs(c) * K + 4096) >> 13, o = c < 0 ? 128 - m : 128 + m;
    return (unsigned)min(255, max(0, o));
}
__device__ __forceinline__ void color4(unsigned &u, unsigned &v, int gain)
{
    unsigned ou = 0, ov = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned su = byte_of(u, k), sv = byte_of(v, k);
        const int K = 8192 + gain * (128 - max(abs((int)su - 128), abs((int)sv - 128)));
        ou |= color1(su, K) << 8 * k; ov |= color1(sv, K) << 8 * k;
    }
    u = ou; v = ov;
}

__global__ __launch_bounds__(256) void input_enhance_kernel(EnArgs a)
{
    __shared__ __attribute__((aligned(16))) EnLds L;
    const int t = threadIdx.x;
    const int W = a.W, H = a.H, tx = blockIdx.x * EN_TW, ty = blockIdx.y * EN_TH;
    const size_t npx = (size_t)W * H;
    // ---- chroma: the loads first
    const int cl = t - 192, ccx = (tx >> 1) + 4 * (cl & 7), ccy = (ty >> 1) + (cl >> 3);
    const bool chroma = a.cgain > 0 && cl >= 0 && ccx < (W >> 1) && ccy < (H >> 1);
    unsigned cu = 0, cv = 0;
    unsigned *pu = nullptr, *pv = nullptr;
    if (chroma) {
        pu = (unsigned *)(a.pic + npx + (size_t)ccy * (W >> 1) + ccx); pv = (unsigned *)((uint8_t *)pu + npx / 4);
        cu = *pu; cv = *pv;
    }
    if (a.gain > 0) {                                                   // (the same in every thread of the grid: the barriers below are met by all)
        // ---- staging
        for (int i = t; i < EN_ROWS * EN_SRC_DW; i += 256) {
            const int r = i / EN_SRC_DW, q = i - r * EN_SRC_DW;
            const int x = tx - 4 + 4 * q, y = min(max(ty - 2 + r, 0), H - 1);
            unsigned v = *(const unsigned *)(a.src + (size_t)y * W + min(max(x, 0), W - 4));
            if (x < 0) v = (v & 255u) * 0x01010101u;
            else if (x >= W) v = (v >> 24) * 0x01010101u;
            L.src[r * EN_SRC_P + q] = v;
        }
        __syncthreads();
        // ---- horizontal pass: 20 rows x 16 quads
        for (int i = t; i < EN_ROWS * (EN_TW / 4); i += 256) {
            const int r = i >> 4, q = i & 15;
            const unsigned *s = L.src + r * EN_SRC_P + q;
            const unsigned l = s[0], m = s[1], n = s[2];                 // samples x - 4 .. x - 1, x .. x + 3, x + 4 .. x + 7
            const unsigned taps = 0x04060401u;                           // (1 4 6 4) on bytes x + i - 2 .. x + i + 1
            const unsigned h0 = __builtin_amdgcn_udot4(align_bytes(m, l, 2), taps, byte_of(m, 2), false);
            const unsigned h1 = __builtin_amdgcn_udot4(align_bytes(m, l, 3), taps, byte_of(m, 3), false);
            const unsigned h2 = __builtin_amdgcn_udot4(m, taps, byte_of(n, 0), false);
            const unsigned h3 = __builtin_amdgcn_udot4(align_bytes(n, m, 1), taps, byte_of(n, 1), false);
            *(uint2 *)(L.h + r * EN_TW + 4 * q) = make_uint2(h0 | h1 << 16, h2 | h3 << 16);
        }
        __syncthreads();
        // ---- vertical pass, detail, limits: a thread, a dword
        const int r = t >> 4, q = t & 15, x = tx + 4 * q, y = ty + r;
        if (x < W && y < H) {
            int v[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const uint2 hh = *(const uint2 *)(L.h + (r + j) * EN_TW + 4 * q);
                const int k = j == 0 || j == 4 ? 1 : j == 2 ? 6 : 4;
                v[0] += k * (int)(hh.x & 0xffffu); v[1] += k * (int)(hh.x >> 16); v[2] += k * (int)(hh.y & 0xffffu); v[3] += k * (int)(hh.y >> 16);
            }
            // columns x - 1 .. x + 4 of rows y - 1 .. y + 1: the column minima and maxima
            unsigned cmn[6], cmx[6], ctr = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned *s = L.src + (r + 1 + j) * EN_SRC_P + q;
                const unsigned l = s[0], m = s[1], n = s[2];
                const unsigned c[6] = {l >> 24, byte_of(m, 0), byte_of(m, 1), byte_of(m, 2), m >> 24, byte_of(n, 0)};
                if (j == 1) ctr = m;
#pragma unroll
                for (int k = 0; k < 6; ++k) { cmn[k] = j ? min(cmn[k], c[k]) : c[k]; cmx[k] = j ? max(cmx[k], c[k]) : c[k]; }
            }
            unsigned o = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int S = (int)byte_of(ctr, k), d = 256 * S - v[k];
                const int aa = max(0, abs(d) - 256 * a.core), e = min(a.limit, (a.gain * aa + 2048) >> 12);
                const int lo = max(0, (int)min(min(cmn[k], cmn[k + 1]), cmn[k + 2]) - a.over), hi = min(255, (int)max(max(cmx[k], cmx[k + 1]), cmx[k + 2]) + a.over);
                o |= (unsigned)min(hi, max(lo, d < 0 ? S - e : S + e)) << 8 * k;
            }
            *(unsigned *)(a.pic + (size_t)y * W + x) = o;
        }
    }
    if (chroma) {
        color4(cu, cv, a.cgain);
        *pu = cu; *pv = cv;
    }
}

int en_check(ks265_ctx *c, const ks265_enhance_cfg *cfg, int w, int h)
{
    if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || w > 8192 || h > 8192) { c->last_error = "enhance: width and height positive multiples of 8, at most 8192"; return KS265_NOTSUPPORTED; }
    if (cfg->edge_gain < 0 || cfg->edge_gain > 64 || cfg->edge_core < 0 || cfg->edge_core > 16 || cfg->edge_over < 0 || cfg->edge_over > 32 || cfg->color_gain < 0 || cfg->color_gain > 32 ||
        (cfg->edge_gain > 0 && (cfg->edge_limit < 1 || cfg->edge_limit > 64))) {
        c->last_error = "enhance: edge_gain 0 .. 64, edge_core 0 .. 16, edge_limit 1 .. 64, edge_over 0 .. 32, color_gain 0 .. 32"; return KS265_NOTSUPPORTED;
    }
    if (!cfg->edge_gain && !cfg->color_gain) { c->last_error = "enhance: both gains 0"; return KS265_NOTSUPPORTED; }
    return KS265_OK;
}

}  // namespace

extern "C" {

int ks265_input_enhance_validate(ks265_ctx *c, const ks265_enhance_cfg *cfg, int width, int height)
{
    if (!c || !cfg) return KS265_POINTER;
    return en_check(c, cfg, width, height);
}

int ks265_input_enhance(ks265_ctx *c, const ks265_enhance_cfg *cfg, int width, int height, const uint8_t *dev_luma_src, uint8_t *dev_i420)
{
    if (!c || !cfg) return KS265_POINTER;
    ks_use_device(c);
    int r = en_check(c, cfg, width, height);
    if (r) return r;
    const long long npx = (long long)width * height, bytes = npx * 3 / 2;
    if (!cfg->edge_gain) dev_luma_src = nullptr;                        // (not read)
    if (((uintptr_t)dev_i420 | (uintptr_t)dev_luma_src) & 3) { c->last_error = "enhance: the picture or the luma source not 4-byte aligned"; return KS265_NOTSUPPORTED; }
    if ((r = ks265_check_extent(c, dev_i420, bytes, 1, bytes, "picture"))) return r;
    if (cfg->edge_gain) {
        if ((r = ks265_check_extent(c, dev_luma_src, npx, 1, npx, "luma source"))) return r;
        if (dev_luma_src < dev_i420 + bytes && dev_i420 < dev_luma_src + npx) { c->last_error = "enhance: the luma source overlaps the picture"; return KS265_POINTER; }
    }
    const EnArgs a = {dev_luma_src, dev_i420, width, height, cfg->edge_gain, cfg->edge_core, cfg->edge_limit, cfg->edge_over, cfg->color_gain};
    const dim3 grid((unsigned)((width + EN_TW - 1) / EN_TW), (unsigned)((height + EN_TH - 1) / EN_TH));
    hipLaunchKernelGGL(input_enhance_kernel, grid, dim3(256), 0, c->stream, a);
    return ks265_check_launch(c);
}

}  // extern "C"
