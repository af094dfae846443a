// input_tonemap.hip — tone mapping on the way in (include/ks265_hip.h ks265_input_tonemap): an HDR10 picture - PQ, BT.2020, 4:2:0 of 10 to 16 bits, planar or
// semi-planar - into the packed 8-bit I420 of the encoder's input slots as BT.709 in limited range, by ONE kernel that reads the source once where it lies.
// tests/tonemap_ref.py is the specification of every byte and host/ks265_tonemap.h builds the tables (E: PQ code -> linear light, G: gain by the largest code, O: linear ->
// q with interpolation).  The kernel belongs to convert_dev.h's family: a thread owns 8 luma columns across the two rows of one chroma row, loads runs as exactly their own
// bytes (load_run: no load leaves [row start, row start + row bytes)), keeps every register array indexed by unrolled constants (no scratch) and ends in the float RGB path's
// luma and chroma pieces (rgb_store_luma / rgb_store_chroma with 64-bit sums: aligned word stores).  The chroma filter's left neighbour, column x0 - 1, is RECOMPUTED (9
// columns per 8): no lane depends on another, so the 512-column boundary between waves is no case of its own.  Ten table gathers per pixel; where the tables live was
// decided by measurement (profiles/tonemap.txt): `tm_global_kernel` gathers from global memory through the caches, `tm_lds_kernel` stages the 32 KB into LDS once per
// work-group and walks many cells with a grid sized to the CUs.
#include "convert_dev.h"
#include "../host/ks265_tonemap.h"

struct ks265_tonemap_plan {
    int device = 0, full_range = 0, cus = 0, where = 1;                // where: 0 global gathers, 1 LDS (the faster: profiles/tonemap.txt)
    ks265_tm_tables host;
    void *blob = nullptr;                                              // E | G | O as ks265_tm_tables lays them out
};

namespace {

constexpr int TAB_BYTES = 4096 * 4 + 4096 * 2 + KS_TM_O_LEN * 2;       // a multiple of 16
static_assert(TAB_BYTES % 16 == 0 && offsetof(ks265_tm_tables, G) == 16384 && offsetof(ks265_tm_tables, O) == 24576 && offsetof(ks265_tm_tables, M) == TAB_BYTES, "the blob is the struct's front");
constexpr int LDS_GROUPS_PER_CU = 4;                                   // 4 x 32 KB of the CU's 160 KB, 16 waves

struct TmArgs {
    const uint8_t *p[3];          // planar: Y, U, V; semi-planar: Y, UV
    long long pitch[3];
    int W, H;
    int nsh, mask;                // the sample of a stored element w: (w >> nsh) & mask
    int yoff, coff, ky, krv, kgu, kgv, kbu;
    int m[3][3];
    int cy[3], cb[3], cr[3], oy;  // BT.709, limited range, Q16
    const uint8_t *tab;           // the blob
    uint8_t *dst;
    int tiles_x, tiles;           // the LDS kernel's walk: 64 x 4 cells per tile
};

__device__ inline int tm_norm(const TmArgs &a, uint32_t w) { return (int)((w >> a.nsh) & (uint32_t)a.mask); }
__device__ inline int tm_elem(const TmArgs &a, const uint8_t *p) { return tm_norm(a, *(const uint16_t *)p); }
__device__ inline int tm_clamp(int v, int hi) { v = v < 0 ? 0 : v; return v > hi ? hi : v; }

// one pixel: samples -> q of R, G, B (host/ks265_tonemap.h ks265_tm_pixel, step for step)
__device__ inline void tm_pixel(const TmArgs &a, const uint32_t *E, const uint16_t *G, const uint16_t *O, int Y, int Cb, int Cr, int &qr, int &qg, int &qb)
{
    const int ly = a.ky * (Y - a.yoff) + (1 << (KS_TM_SH_CODE - 1)), cb = Cb - a.coff, cr = Cr - a.coff;
    const int r12 = tm_clamp((ly + a.krv * cr) >> KS_TM_SH_CODE, 4095), g12 = tm_clamp((ly - a.kgu * cb - a.kgv * cr) >> KS_TM_SH_CODE, 4095), b12 = tm_clamp((ly + a.kbu * cb) >> KS_TM_SH_CODE, 4095);
    const unsigned long long g = G[max(max(r12, g12), b12)];
    const unsigned long long vr = ((unsigned long long)E[r12] * g + (1u << 18)) >> 19, vg = ((unsigned long long)E[g12] * g + (1u << 18)) >> 19, vb = ((unsigned long long)E[b12] * g + (1u << 18)) >> 19;
    const int tr = vr > 65536 ? 65536 : (int)vr, tg = vg > 65536 ? 65536 : (int)vg, tb = vb > 65536 ? 65536 : (int)vb;
    int q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int v = tm_clamp((a.m[r][0] * tr + a.m[r][1] * tg + a.m[r][2] * tb + (1 << 9)) >> 10, 1 << 20);
        const int i = v >> 8, f = v & 255;
        q[r] = ((int)O[i] * (256 - f) + (int)O[i + 1] * f + 128) >> 8;
    }
    qr = q[0]; qg = q[1]; qb = q[2];
}

// the cell: 8 luma columns (and column x0 - 1, clamped to 0) x the two rows of chroma row i -> 16 Y, 4 Cb, 4 Cr
template <bool SEMI> __device__ inline void tm_cell(const TmArgs &a, const uint32_t *E, const uint16_t *G, const uint16_t *O, int x0, int i)
{
    // chroma samples x0 / 2 - 1 (clamped to 0) .. x0 / 2 + 4 (clamped to the last) as cu / cv[0 .. 5]
    const int k0 = x0 / 2, cw = a.W / 2, kl = k0 > 0 ? k0 - 1 : 0, kr = k0 + 4 < cw ? k0 + 4 : cw - 1;
    int cu[6], cv[6];
    if constexpr (SEMI) {
        const uint8_t *row = a.p[1] + (long long)i * a.pitch[1];
        uint32_t w[4];
        load_run<16, 2>(row + (long long)x0 * 2, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) { cu[k + 1] = tm_norm(a, run_elem<2>(w, 2 * k)); cv[k + 1] = tm_norm(a, run_elem<2>(w, 2 * k + 1)); }
        cu[0] = tm_elem(a, row + (long long)kl * 4); cv[0] = tm_elem(a, row + (long long)kl * 4 + 2);
        cu[5] = tm_elem(a, row + (long long)kr * 4); cv[5] = tm_elem(a, row + (long long)kr * 4 + 2);
    } else {
        const uint8_t *ru = a.p[1] + (long long)i * a.pitch[1], *rv = a.p[2] + (long long)i * a.pitch[2];
        uint32_t wu[2], wv[2];
        load_run<8, 2>(ru + (long long)k0 * 2, wu);
        load_run<8, 2>(rv + (long long)k0 * 2, wv);
#pragma unroll
        for (int k = 0; k < 4; ++k) { cu[k + 1] = tm_norm(a, run_elem<2>(wu, k)); cv[k + 1] = tm_norm(a, run_elem<2>(wv, k)); }
        cu[0] = tm_elem(a, ru + (long long)kl * 2); cv[0] = tm_elem(a, rv + (long long)kl * 2);
        cu[5] = tm_elem(a, ru + (long long)kr * 2); cv[5] = tm_elem(a, rv + (long long)kr * 2);
    }
    // at luma resolution, entries 0 .. 8 = columns x0 - 1 .. x0 + 7: an even column takes its sample, an odd one the rounded mean of its neighbours
    int eu[9], ev[9];
    eu[0] = x0 > 0 ? (cu[0] + cu[1] + 1) >> 1 : cu[1]; ev[0] = x0 > 0 ? (cv[0] + cv[1] + 1) >> 1 : cv[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        eu[2 * k + 1] = cu[k + 1]; ev[2 * k + 1] = cv[k + 1];
        eu[2 * k + 2] = (cu[k + 1] + cu[k + 2] + 1) >> 1; ev[2 * k + 2] = (cv[k + 1] + cv[k + 2] + 1) >> 1;
    }
    const int xl = x0 > 0 ? x0 - 1 : 0;
    int s[3][4] = {};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const uint8_t *row = a.p[0] + (long long)(2 * i + dy) * a.pitch[0];
        uint32_t w[4];
        load_run<16, 2>(row + (long long)x0 * 2, w);
        int c[3][9];
        tm_pixel(a, E, G, O, tm_elem(a, row + (long long)xl * 2), eu[0], ev[0], c[0][0], c[1][0], c[2][0]);
#pragma unroll
        for (int k = 0; k < 8; ++k) tm_pixel(a, E, G, O, tm_norm(a, run_elem<2>(w, k)), eu[k + 1], ev[k + 1], c[0][k + 1], c[1][k + 1], c[2][k + 1]);
        rgb_store_luma<long long, 24>(a, 2 * i + dy, x0, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s[ch][k] += rgb_sum121(c[ch], k);
        }
    }
    rgb_store_chroma<long long, 24>(a, i, x0, s);
}

// the tables where they lie in global memory: 32 KB that every CU keeps in its caches
template <bool SEMI> __global__ __launch_bounds__(256) void tm_global_kernel(TmArgs a)
{
    int x0, i;
    if (!ks_cell<8>(a.W, a.H, x0, i)) return;
    tm_cell<SEMI>(a, (const uint32_t *)a.tab, (const uint16_t *)(a.tab + 16384), (const uint16_t *)(a.tab + 24576), x0, i);
}

// the tables staged into LDS once per work-group, which then walks tiles of 64 x 4 cells (512 x 8 pixels) with the grid's stride
template <bool SEMI> __global__ __launch_bounds__(256) void tm_lds_kernel(TmArgs a)
{
    __shared__ uint4 tab[TAB_BYTES / 16];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int k = tid; k < TAB_BYTES / 16; k += 256) tab[k] = ((const uint4 *)a.tab)[k];
    __syncthreads();
    const uint8_t *t = (const uint8_t *)tab;
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int x0 = ((tile % a.tiles_x) * 64 + threadIdx.x) * 8, i = (tile / a.tiles_x) * 4 + threadIdx.y;
        if (x0 < a.W && 2 * i < a.H) tm_cell<SEMI>(a, (const uint32_t *)t, (const uint16_t *)(t + 16384), (const uint16_t *)(t + 24576), x0, i);
    }
}

int tm_check(ks265_ctx *c, const ks265_tonemap_plan *p, const ks265_in_desc *d, ks265_yuv_fmt *f)
{
    if (p->device != c->device) { c->last_error = "tonemap: the plan belongs to another device"; return KS265_NOTSUPPORTED; }
    if (ks265_yuv_decode(d->format, f) <= 0 || !ks265_tm_format_ok(f->layout, f->sub, f->depth)) { c->last_error = "tonemap: 4:2:0 of 10 to 16 bits, planar or semi-planar"; return KS265_NOTSUPPORTED; }
    return ks265_yuv_check_desc(c, d, *f);
}

}  // namespace

extern "C" {

int ks265_tonemap_plan_create(ks265_ctx *c, const ks265_tonemap_cfg *cfg, ks265_tonemap_plan **out)
{
    if (!c || !cfg || !out) return KS265_POINTER;
    *out = nullptr;
    ks_use_device(c);
    if (!ks265_tm_cfg_ok(cfg->transfer, cfg->curve, cfg->peak_nits, cfg->white_nits) || (cfg->full_range != 0 && cfg->full_range != 1)) {
        c->last_error = "tonemap: transfer 16 (PQ), curve 0 .. 2, full_range 0 / 1, peak 100 .. 10000, white 80 .. 1000 and at most the peak"; return KS265_NOTSUPPORTED;
    }
    ks265_tonemap_plan *p = new ks265_tonemap_plan();
    p->device = c->device; p->full_range = cfg->full_range;
    int r = ks265_hip(c, hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, c->device));
    ks265_tm_tables_fill(cfg->curve, cfg->peak_nits, cfg->white_nits, &p->host);
    if (!r) r = ks265_dev_malloc(c, &p->blob, TAB_BYTES);
    if (!r) r = ks265_hip(c, hipMemcpy(p->blob, &p->host, TAB_BYTES, hipMemcpyHostToDevice));   // (returns when the tables are there: the per-picture call copies nothing)
    if (r) { if (p->blob) (void)ks265_dev_free(c, p->blob); delete p; return r; }
    *out = p;
    return KS265_OK;
}

int ks265_tonemap_plan_destroy(ks265_ctx *c, ks265_tonemap_plan *p)
{
    if (!c) return KS265_POINTER;
    if (!p) return KS265_OK;
    ks_use_device(c);
    const int r = p->blob ? ks265_dev_free(c, p->blob) : KS265_OK;
    delete p;
    return r;
}

int ks265_tonemap_plan_tables(ks265_tonemap_plan *p, int where)
{
    if (!p) return KS265_POINTER;
    if (where != 0 && where != 1) return KS265_NOTSUPPORTED;
    p->where = where;
    return KS265_OK;
}

int ks265_input_tonemap_validate(ks265_ctx *c, const ks265_tonemap_plan *p, const ks265_in_desc *d)
{
    if (!c || !p || !d) return KS265_POINTER;
    ks_use_device(c);
    ks265_yuv_fmt f;
    return tm_check(c, p, d, &f);
}

int ks265_input_tonemap(ks265_ctx *c, const ks265_tonemap_plan *p, const ks265_in_desc *d, uint8_t *dst)
{
    if (!c || !p || !d) return KS265_POINTER;
    ks_use_device(c);
    ks265_yuv_fmt f;
    int r = tm_check(c, p, d, &f);
    if (r) return r;
    const long long W = d->width, H = d->height;
    if ((r = ks_check_slot(c, dst, W * H * 3 / 2, "tonemap", "destination"))) return r;
    TmArgs a = {};
    for (int k = 0; k < 3; ++k) { a.p[k] = (const uint8_t *)d->plane[k]; a.pitch[k] = d->pitch[k]; }
    a.W = (int)W; a.H = (int)H; a.dst = dst; a.tab = (const uint8_t *)p->blob;
    a.nsh = f.msb ? 16 - f.depth : 0; a.mask = (1 << f.depth) - 1;
    ks265_tm_norm n;
    ks265_tm_norm_fill(f.depth, p->full_range, &n);
    a.yoff = n.yoff; a.coff = n.coff; a.ky = n.ky; a.krv = n.krv; a.kgu = n.kgu; a.kgv = n.kgv; a.kbu = n.kbu;
    for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) a.m[j][k] = p->host.M[j][k];
    const KsRgbCoef k = ks_rgb_coef(KS265_MATRIX_BT709, 0);
    for (int j = 0; j < 3; ++j) { a.cy[j] = k.cy[j]; a.cb[j] = k.cb[j]; a.cr[j] = k.cr[j]; }
    a.oy = k.oy;
    const KsCellLaunch l = ks_cell_launch(W, H, 8);
    if (p->where == 1) {
        a.tiles_x = (int)l.grid.x; a.tiles = (int)(l.grid.x * l.grid.y);
        const dim3 grid((unsigned)std::min(a.tiles, std::max(p->cus, 1) * LDS_GROUPS_PER_CU));
        if (f.layout == 1) hipLaunchKernelGGL(tm_lds_kernel<true>, grid, l.blk, 0, c->stream, a);
        else hipLaunchKernelGGL(tm_lds_kernel<false>, grid, l.blk, 0, c->stream, a);
    } else {
        if (f.layout == 1) hipLaunchKernelGGL(tm_global_kernel<true>, l.grid, l.blk, 0, c->stream, a);
        else hipLaunchKernelGGL(tm_global_kernel<false>, l.grid, l.blk, 0, c->stream, a);
    }
    return ks265_check_launch(c);
}

}  // extern "C"
