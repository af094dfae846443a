// input_scale.hip — pictures in device memory of ANOTHER size into the packed I420 layout of the encoder's input slots (include/ks265_hip.h ks265_input_scale):
// a separable triangle / Catmull-Rom resampler in exact integer arithmetic, tests/yuv_scale_ref.py is the specification and host/ks265_scale.h builds the tables.
// One launch makes all three planes.  A work-group owns a tile of 64 destination columns x up to 16 destination rows of one plane: it reads the tile's coefficients once into
// LDS, brings the tile's span of source rows in chunk by chunk (whole 16-byte words along the row where the row's own extent allows, narrower at its ends), filters every
// source row of the span horizontally into an int16 picture in LDS, then filters that vertically and stores one aligned word per thread.  No scratch memory, no atomics.
#include "convert_dev.h"
#include "../host/ks265_scale.h"
#include <algorithm>
#include <cstring>
#include <vector>

struct ks265_scale_plan {
    int device, sw, sh, dw, dh, filter, identity;
    int T[4];                                   // luma x, luma y, chroma x, chroma y
    void *blob;                                 // the four tables in one device block
    const int32_t *first[4];
    const int16_t *coef[4];
    int tile_rows, chunk_rows, lstr, lstr_planar, span_rows, tx_max, ty_max;   // the launch's shape, the same for every work-group (chosen in ks265_scale_plan_create);
    unsigned lds_bytes;                                                        // lstr: staged row bytes with NV12's two-byte chroma samples, lstr_planar: without; lds_bytes: with lstr
};

namespace {

constexpr int TILE_W = 64, TILE_H = 16, CHUNK = 16, NT = 256, LDS_LIMIT = 65536;

struct ScalePlane {
    const uint8_t *row0;                        // first byte of source row 0; nothing outside [row0 + y pitch, + row_bytes) is read
    long long pitch;
    int off, step, row_bytes;                   // sample k of a row is its byte off + k step (NV12 chroma: step 2, off 0 / 1)
    int sw, sh, dw, dh;
    uint8_t *dst;
};
struct ScaleArgs {
    ScalePlane pl[3];
    const int32_t *fx[2], *fy[2];               // [0] luma, [1] chroma
    const int16_t *cx[2], *cy[2];
    int Tx[2], Ty[2], nbx[2], nby[2];
    int tile_rows, chunk_rows, lstr, span_rows, tx_max, ty_max;
};

// the 16 bytes at the 16-byte aligned address a, of which only those inside [lo, hi) are read (the others count 0): one 16-byte load, else 8-byte, 4-byte, single bytes
__device__ inline uint4 load16_inside(uintptr_t a, uintptr_t lo, uintptr_t hi)
{
    if (a >= lo && a + 16 <= hi) return *(const uint4 *)a;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uintptr_t a8 = a + 8 * h;
        if (a8 >= lo && a8 + 8 <= hi) { const uint2 v = *(const uint2 *)a8; w[2 * h] = v.x; w[2 * h + 1] = v.y; continue; }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uintptr_t a4 = a8 + 4 * q;
            if (a4 >= lo && a4 + 4 <= hi) { w[2 * h + q] = *(const uint32_t *)a4; continue; }
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) if (a4 + b >= lo && a4 + b < hi) x |= (uint32_t)*(const uint8_t *)(a4 + b) << 8 * b;
            w[2 * h + q] = x;
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(NT) void scale_i420_kernel(ScaleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x;
    // which plane, which tile (uniform per work-group)
    const int nl = a.nbx[0] * a.nby[0], nc = a.nbx[1] * a.nby[1];
    int b = blockIdx.x;
    const int plane = b < nl ? 0 : b < nl + nc ? 1 : 2, cls = plane ? 1 : 0;
    b -= plane == 0 ? 0 : plane == 1 ? nl : nl + nc;
    const int bx = b % a.nbx[cls], by = b / a.nbx[cls];
    const ScalePlane &P = a.pl[plane];
    const int Tx = a.Tx[cls], Ty = a.Ty[cls], tr = a.tile_rows;
    const int x0 = bx * TILE_W, y0 = by * tr;

    int32_t *s_fx = (int32_t *)lds;                                            // [64]
    int32_t *s_fy = s_fx + TILE_W;                                              // [16]
    int16_t *s_cx = (int16_t *)(s_fy + TILE_H);                                 // [tx_max][64]: tap i of column t
    int16_t *s_cy = s_cx + a.tx_max * TILE_W;                                   // [ty_max][16]
    int16_t *s_h = s_cy + a.ty_max * TILE_H;                                    // [span_rows][64]: the horizontal pass of the tile's source rows
    uint8_t *s_src = (uint8_t *)(s_h + a.span_rows * TILE_W);                   // [chunk_rows][lstr]: source rows as they lie in memory, from a 16-byte boundary on

    // the tile's tables, once (columns and rows past the plane's edge repeat its last one: they are computed and not stored)
    if (tid < TILE_W) s_fx[tid] = a.fx[cls][min(x0 + tid, P.dw - 1)];
    if (tid < TILE_H) s_fy[tid] = a.fy[cls][min(y0 + min(tid, tr - 1), P.dh - 1)];
    for (int idx = tid; idx < Tx * TILE_W; idx += NT) { const int t = idx / Tx, i = idx - t * Tx; s_cx[i * TILE_W + t] = a.cx[cls][(size_t)min(x0 + t, P.dw - 1) * Tx + i]; }
    for (int idx = tid; idx < Ty * TILE_H; idx += NT) { const int t = idx / Ty, i = idx - t * Ty; s_cy[i * TILE_H + t] = a.cy[cls][(size_t)min(y0 + min(t, tr - 1), P.dh - 1) * Ty + i]; }
    __syncthreads();
    // the tile's span of source columns and rows: every wave reduces the 64 + 16 entries over its own lanes (one LDS read each, then lane exchanges)
    int c0 = s_fx[tid & 63], c1 = c0, r0 = s_fy[tid & 15], r1 = r0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c0 = min(c0, __shfl_xor(c0, d)); c1 = max(c1, __shfl_xor(c1, d));
        if (d < TILE_H) { r0 = min(r0, __shfl_xor(r0, d)); r1 = max(r1, __shfl_xor(r1, d)); }
    }
    c1 = min(c1 + Tx - 1, P.sw - 1);
    r1 = min(min(r1 + Ty - 1, P.sh - 1), r0 + a.span_rows - 1);                 // (the host sized span_rows by the same walk: the last term never binds)

    const int byte0 = P.off + c0 * P.step, byte1 = P.off + c1 * P.step;        // the first and the last byte of a row the tile needs
    const int nseg = a.lstr >> 4;
    const int j = tid & (TILE_W - 1), lane = tid >> 6;
    const int fxj = s_fx[j];
    for (int rs = r0; rs <= r1; rs += a.chunk_rows) {
        const int nr = min(a.chunk_rows, r1 - rs + 1);
        for (int idx = tid; idx < nr * nseg; idx += NT) {
            const int rr = idx / nseg, seg = idx - rr * nseg;
            const uintptr_t row = (uintptr_t)(P.row0 + (long long)(rs + rr) * P.pitch);
            const uintptr_t at = ((row + byte0) & ~(uintptr_t)15) + 16 * (uintptr_t)seg;
            if (at > row + byte1) continue;
            *(uint4 *)(s_src + rr * a.lstr + 16 * seg) = load16_inside(at, row, row + P.row_bytes);
        }
        __syncthreads();
        int acc[CHUNK / 4] = {0, 0, 0, 0};
        int base[CHUNK / 4];
#pragma unroll
        for (int m = 0; m < CHUNK / 4; ++m) {
            const int rr = min(lane + 4 * m, nr - 1);
            const uintptr_t row = (uintptr_t)(P.row0 + (long long)(rs + rr) * P.pitch);
            base[m] = rr * a.lstr + (int)((row + byte0) & 15) - c0 * P.step;
        }
        for (int i = 0; i < Tx; ++i) {
            const int c = s_cx[i * TILE_W + j], k = min(fxj + i, c1) * P.step;
#pragma unroll
            for (int m = 0; m < CHUNK / 4; ++m) acc[m] += c * (int)s_src[base[m] + k];
        }
#pragma unroll
        for (int m = 0; m < CHUNK / 4; ++m) {
            const int rr = lane + 4 * m;
            if (rr < nr) s_h[(rs - r0 + rr) * TILE_W + j] = (int16_t)((acc[m] + 128) >> 8);
        }
        __syncthreads();
    }

    // vertical: thread = 4 adjacent columns of one row
    const int cg = tid & 15, t = tid >> 4;
    const int x = x0 + 4 * cg, y = y0 + t;
    if (t >= tr || y >= P.dh || x >= P.dw) return;
    int v[4] = {0, 0, 0, 0};
    const int fyt = s_fy[t];
    for (int i = 0; i < Ty; ++i) {
        const int c = s_cy[i * TILE_H + t], k = min(fyt + i, r1) - r0;
        const uint2 h = *(const uint2 *)(s_h + k * TILE_W + 4 * cg);
        v[0] += c * (int)(int16_t)(h.x & 0xffff); v[1] += c * ((int)h.x >> 16);
        v[2] += c * (int)(int16_t)(h.y & 0xffff); v[3] += c * ((int)h.y >> 16);
    }
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w |= shr_clip255(v[e] + (1 << 19), 20) << 8 * e;   // (convert_dev.h: the clamp in front of the shift)
    *(uint32_t *)(P.dst + (size_t)y * P.dw + x) = w;
}

// over the tiles of `tile` outputs of an axis: the longest span of source samples one tile touches
int max_span(const std::vector<int32_t> &first, int T, int S, int tile)
{
    int best = 0;
    const int D = (int)first.size();
    for (int t0 = 0; t0 < D; t0 += tile) {
        int lo = first[t0], hi = first[t0];
        for (int t = t0; t < D && t < t0 + tile; ++t) { lo = std::min(lo, first[t]); hi = std::max(hi, first[t]); }
        best = std::max(best, std::min(hi + T - 1, S - 1) - lo + 1);
    }
    return best;
}

int plan_matches(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s)
{
    if (p->device != c->device) { c->last_error = "scale: a plan of another device"; return KS265_NOTSUPPORTED; }
    if (s->width != p->sw || s->height != p->sh) { c->last_error = "scale: the source is not of the plan's size"; return KS265_NOTSUPPORTED; }
    return KS265_OK;
}

}  // namespace

extern "C" {

int ks265_scale_plan_create(ks265_ctx *c, int src_w, int src_h, int dst_w, int dst_h, int filter, ks265_scale_plan **out)
{
    if (!c || !out) return KS265_POINTER;
    *out = nullptr;
    ks_use_device(c);
    if (!ks265_scale_size_ok(src_w, src_h, dst_w, dst_h)) { c->last_error = "scale: source width a multiple of 8 and height even, destination multiples of 8, at most 8192, ratios at most 8"; return KS265_NOTSUPPORTED; }
    if (filter != KS_SCALE_TRIANGLE && filter != KS_SCALE_CATMULL_ROM) { c->last_error = "scale: filter 0 (triangle) or 1 (Catmull-Rom)"; return KS265_NOTSUPPORTED; }
    ks265_scale_plan *p = new ks265_scale_plan();
    p->device = c->device; p->sw = src_w; p->sh = src_h; p->dw = dst_w; p->dh = dst_h; p->filter = filter;
    p->identity = src_w == dst_w && src_h == dst_h;
    if (p->identity) { *out = p; return KS265_OK; }                    // ks265_input_convert alone: no tables
    int S[4], D[4], cos[4];
    ks265_scale_axes(src_w, src_h, dst_w, dst_h, S, D, cos);
    std::vector<int32_t> first[4];
    std::vector<int16_t> coef[4];
    size_t off_first[4], off_coef[4], total = 0;
    for (int k = 0; k < 4; ++k) {
        p->T[k] = ks265_scale_axis_taps(S[k], D[k], filter, cos[k]);
        first[k].resize((size_t)D[k]); coef[k].resize((size_t)D[k] * (size_t)std::max(p->T[k], 1));
        if (!p->T[k] || ks265_scale_axis_fill(S[k], D[k], filter, cos[k], p->T[k], first[k].data(), coef[k].data())) { delete p; c->last_error = "scale: no table for this pair of sizes"; return KS265_NOTSUPPORTED; }
        off_first[k] = total; total += ((size_t)D[k] * 4 + 15) & ~(size_t)15;
        off_coef[k] = total; total += ((size_t)D[k] * p->T[k] * 2 + 15) & ~(size_t)15;
    }
    // the launch's shape: LDS for the tables, the span of source rows of a tile (int16 x 64 columns) and a chunk of source rows as they lie in memory; tiles of fewer rows
    // where the span of a 16-row tile would not fit into 64 KB
    p->tx_max = std::max(p->T[0], p->T[2]); p->ty_max = std::max(p->T[1], p->T[3]);
    const int span_l = max_span(first[0], p->T[0], S[0], TILE_W), span_c = max_span(first[2], p->T[2], S[2], TILE_W);   // samples; NV12 chroma: two bytes per sample
    p->lstr = ((15 + std::max(span_l, 2 * span_c) + 15) & ~15) + 16;
    p->lstr_planar = ((15 + std::max(span_l, span_c) + 15) & ~15) + 16;
    p->lds_bytes = 0;
    for (int tr = TILE_H; tr >= 1 && !p->lds_bytes; tr >>= 1)
        for (int ch = CHUNK; ch >= 4 && !p->lds_bytes; ch >>= 1) {
            const int span = std::max(max_span(first[1], p->T[1], S[1], tr), max_span(first[3], p->T[3], S[3], tr));
            const size_t need = (size_t)(TILE_W + TILE_H) * 4 + (size_t)p->tx_max * TILE_W * 2 + (size_t)p->ty_max * TILE_H * 2 + (size_t)span * TILE_W * 2 + (size_t)ch * p->lstr;
            if (need <= LDS_LIMIT) { p->tile_rows = tr; p->chunk_rows = ch; p->span_rows = span; p->lds_bytes = (unsigned)need; }
        }
    if (!p->lds_bytes) { delete p; c->last_error = "scale: the tile does not fit into LDS"; return KS265_NOTSUPPORTED; }
    int r = ks265_dev_malloc(c, &p->blob, total);
    if (r) { delete p; return r; }
    std::vector<uint8_t> host(total, 0);
    for (int k = 0; k < 4; ++k) {
        memcpy(host.data() + off_first[k], first[k].data(), first[k].size() * 4);
        memcpy(host.data() + off_coef[k], coef[k].data(), coef[k].size() * 2);
        p->first[k] = (const int32_t *)((uint8_t *)p->blob + off_first[k]);
        p->coef[k] = (const int16_t *)((uint8_t *)p->blob + off_coef[k]);
    }
    r = ks265_hip(c, hipMemcpy(p->blob, host.data(), total, hipMemcpyHostToDevice));   // (returns when the tables are there: the per-picture call copies nothing)
    if (r) { (void)ks265_dev_free(c, p->blob); delete p; return r; }
    *out = p;
    return KS265_OK;
}

int ks265_scale_plan_destroy(ks265_ctx *c, ks265_scale_plan *p)
{
    if (!c) return KS265_POINTER;
    if (!p) return KS265_OK;
    ks_use_device(c);
    const int r = p->blob ? ks265_dev_free(c, p->blob) : KS265_OK;
    delete p;
    return r;
}

int ks265_input_scale_validate(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s)
{
    if (!c || !p || !s) return KS265_POINTER;
    ks_use_device(c);
    const int r = plan_matches(c, p, s);
    return r ? r : ks265_input_validate(c, s);
}

int ks265_input_scale(ks265_ctx *c, const ks265_scale_plan *p, const ks265_in_desc *s, uint8_t *scratch, uint8_t *dst)
{
    int r = ks265_input_scale_validate(c, p, s);
    if (r) return r;
    if (p->identity) return ks265_input_convert(c, s, dst);
    const long long sn = (long long)p->sw * p->sh, dn = (long long)p->dw * p->dh;
    if ((r = ks_check_slot(c, dst, dn * 3 / 2, "scale", "destination"))) return r;
    ScaleArgs a = {};
    ks265_yuv_fmt yf;
    const int fam = ks265_yuv_decode(s->format, &yf);                  // (validated above: a valid code of the YUV family, or none of it)
    const bool nv12 = s->format == KS265_IN_NV12 || (fam > 0 && yf.alias && yf.layout == 1);
    if (ks265_rgb_elem_size(s->format) || (fam > 0 && !yf.alias)) {    // RGB of any sample type, YUV of more bits or more chroma: converted at the source's size first
        if (!scratch) { c->last_error = "scale: an RGB or KS265_IN_YUV source needs the scratch picture"; return KS265_POINTER; }
        if ((r = ks_check_slot(c, scratch, sn * 3 / 2, "scale", "scratch"))) return r;
        if ((r = ks265_input_convert(c, s, scratch))) return r;        // the conversion at the source's size, then the scaler on the same stream
        a.pl[0] = {scratch, p->sw, 0, 1, p->sw, 0, 0, 0, 0, nullptr};
        a.pl[1] = {scratch + sn, p->sw / 2, 0, 1, p->sw / 2, 0, 0, 0, 0, nullptr};
        a.pl[2] = {scratch + sn + sn / 4, p->sw / 2, 0, 1, p->sw / 2, 0, 0, 0, 0, nullptr};
    } else if (nv12) {
        a.pl[0] = {(const uint8_t *)s->plane[0], s->pitch[0], 0, 1, p->sw, 0, 0, 0, 0, nullptr};
        a.pl[1] = {(const uint8_t *)s->plane[1], s->pitch[1], 0, 2, p->sw, 0, 0, 0, 0, nullptr};
        a.pl[2] = {(const uint8_t *)s->plane[1], s->pitch[1], 1, 2, p->sw, 0, 0, 0, 0, nullptr};
    } else {
        for (int k = 0; k < 3; ++k) a.pl[k] = {(const uint8_t *)s->plane[k], s->pitch[k], 0, 1, k ? p->sw / 2 : p->sw, 0, 0, 0, 0, nullptr};
    }
    for (int k = 0; k < 3; ++k) {
        ScalePlane &P = a.pl[k];
        P.sw = k ? p->sw / 2 : p->sw; P.sh = k ? p->sh / 2 : p->sh; P.dw = k ? p->dw / 2 : p->dw; P.dh = k ? p->dh / 2 : p->dh;
        P.dst = dst + (k == 0 ? 0 : k == 1 ? dn : dn + dn / 4);
    }
    for (int k = 0; k < 2; ++k) {
        a.fx[k] = p->first[2 * k]; a.cx[k] = p->coef[2 * k]; a.Tx[k] = p->T[2 * k];
        a.fy[k] = p->first[2 * k + 1]; a.cy[k] = p->coef[2 * k + 1]; a.Ty[k] = p->T[2 * k + 1];
        a.nbx[k] = (a.pl[k].dw + TILE_W - 1) / TILE_W; a.nby[k] = (a.pl[k].dh + p->tile_rows - 1) / p->tile_rows;
    }
    a.tile_rows = p->tile_rows; a.chunk_rows = p->chunk_rows; a.lstr = nv12 ? p->lstr : p->lstr_planar; a.span_rows = p->span_rows; a.tx_max = p->tx_max; a.ty_max = p->ty_max;
    const unsigned blocks = (unsigned)(a.nbx[0] * a.nby[0] + 2 * a.nbx[1] * a.nby[1]);
    hipLaunchKernelGGL(scale_i420_kernel, dim3(blocks), dim3(NT), p->lds_bytes - (unsigned)(p->chunk_rows * (p->lstr - a.lstr)), c->stream, a);
    return ks265_check_launch(c);
}

}  // extern "C"
