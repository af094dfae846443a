// frame_loop.hip — in-loop filters.
//   Stage E  ks265_deblock : boundary strength (CalcBsInterP enc@0x402960, single reference) fused with the normative edge
//            filters (EdgeFilterLuma{Ver,Hor}_c enc@0x403630/0x4038c0, PixelFilterChroma{Ver,Hor}_c enc@0x403c50/0x403d10);
//            all vertical edges of the picture in one launch, then all horizontal ones, in place: one thread per 4-line
//            segment, neighbouring threads touch neighbouring 8-byte (ver) / 4-byte (hor) columns -> coalesced rows.
//   Stage F  ks265_sao     : per CTU statistics (register accumulators + DPP reductions for the 16 EO bins, LDS atomics for
//            the 32 bands; s8 difference truncation of statSaoBoEo01_c enc@0x4ae9c0), decision, and out-of-place apply.
#include "frame_common.h"

using namespace ks265;

__device__ __forceinline__ int edge_bs(const ks265_cu8 p, const ks265_cu8 q, int pos8)
{
    const int part = q.log2_cu >> 4, cu8n = 1 << ((q.log2_cu & 15) - 3), tu8n = min(part ? cu8n >> 1 : cu8n, 4);   // a CU in two partitions (cfg.part) holds four transform units
    const bool tu_edge = (pos8 % tu8n) == 0, cu_edge = (pos8 % cu8n) == 0;
    if (!tu_edge && !cu_edge) return 0;
    if (p.pred_mode != 0 || q.pred_mode != 0) return 2;
    if (tu_edge && ((p.cbf | q.cbf) & 1)) return 1;
    if (cu_edge || part) {                                   // a prediction-block edge: the CU's border, or the TU edges inside a CU in two partitions (equal vectors: nothing fires)
        // CalcBsInterP enc@0x402960 / CalcBsInterB enc@0x4029d0 with one picture per list
        if (p.inter_dir != q.inter_dir) return 1;
        if ((p.inter_dir & 1) && (abs((int)p.mvx - (int)q.mvx) >= 4 || abs((int)p.mvy - (int)q.mvy) >= 4)) return 1;
        if ((p.inter_dir & 2) && (abs((int)p.mv1x - (int)q.mv1x) >= 4 || abs((int)p.mv1y - (int)q.mv1y) >= 4)) return 1;
    }
    return 0;
}

// DIR 0: vertical edges (filter across x), DIR 1: horizontal edges.
// thread = (edge block bx/by, 4-line segment); luma first, then the two chroma planes (bS == 2 only)
// eff (null = the slice QP everywhere): QpY of every 8x8 block as the decoder derives it (qp_eff_kernel); an edge filters at QpL = (QpP + QpQ + 1) >> 1 (8.7.2.5.3)
template <int DIR>
__global__ __launch_bounds__(256) void deblock_kernel(KsGeom g, int qp, int beta, int beta_off2, int tc_off2, const ks265_cu8 *cu8, uint8_t *ry, uint8_t *ru, uint8_t *rv, const uint8_t *eff)
{
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int nseg_l = DIR == 0 ? g.w8 * (g.H / 4) : (g.W / 4) * g.h8;       // luma segments (incl. the skipped picture-edge column/row)
    if (gid < nseg_l) {
        int bx, by, seg;                                                      // 8x8 block of Q, 4-line segment inside it (0/1)
        if (DIR == 0) { bx = gid % g.w8; int y4 = gid / g.w8; by = y4 >> 1; seg = y4 & 1; }
        else { int x4 = gid % (g.W / 4); by = gid / (g.W / 4); bx = x4 >> 1; seg = x4 & 1; }
        if ((DIR == 0 ? bx : by) == 0) return;
        const ks265_cu8 q = cu8[(long)by * g.w8 + bx], p = DIR == 0 ? cu8[(long)by * g.w8 + bx - 1] : cu8[(long)(by - 1) * g.w8 + bx];
        const int bs = edge_bs(p, q, DIR == 0 ? bx : by);
        if (!bs) return;
        if (eff) { qp = (eff[(long)by * g.w8 + bx] + eff[(long)by * g.w8 + bx - (DIR == 0 ? 1 : g.w8)] + 1) >> 1; beta = kBetaTable[clip3(0, 51, qp + beta_off2)]; }
        const int tc = kTcTable[clip3(0, 53, qp + 2 * (bs - 1) + tc_off2)];
        uint8_t *Y = ks_org_y(g, ry);
        int px[4][8];
        if (DIR == 0) {
            uint8_t *p0 = Y + (long)(by * 8 + seg * 4) * g.sy + bx * 8 - 4;
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const unsigned a = *(const unsigned *)(p0 + (long)l * g.sy), b = *(const unsigned *)(p0 + (long)l * g.sy + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) { px[l][i] = (a >> (8 * i)) & 255; px[l][4 + i] = (b >> (8 * i)) & 255; }
            }
            deblock_luma_segment(px, beta, tc, true, true);
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                unsigned a = 0, b = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) { a |= (unsigned)px[l][i] << (8 * i); b |= (unsigned)px[l][4 + i] << (8 * i); }
                *(unsigned *)(p0 + (long)l * g.sy) = a; *(unsigned *)(p0 + (long)l * g.sy + 4) = b;
            }
        } else {
            uint8_t *p0 = Y + (long)(by * 8 - 4) * g.sy + bx * 8 + seg * 4;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned a = *(const unsigned *)(p0 + (long)i * g.sy);
#pragma unroll
                for (int l = 0; l < 4; ++l) px[l][i] = (a >> (8 * l)) & 255;
            }
            deblock_luma_segment(px, beta, tc, true, true);
#pragma unroll
            for (int i = 1; i < 7; ++i) {
                unsigned a = 0;
#pragma unroll
                for (int l = 0; l < 4; ++l) a |= (unsigned)px[l][i] << (8 * l);
                *(unsigned *)(p0 + (long)i * g.sy) = a;
            }
        }
        return;
    }
    // chroma: one thread per (comp, 8x8 luma block on the 16-sample grid) = 4 chroma lines
    int cid = gid - nseg_l;
    const int nblk = g.w8 * g.h8;
    if (cid >= 2 * nblk) return;
    const int comp = cid / nblk; cid -= comp * nblk;
    const int bx = cid % g.w8, by = cid / g.w8;
    if (DIR == 0 ? (bx == 0 || (bx & 1)) : (by == 0 || (by & 1))) return;
    const ks265_cu8 q = cu8[(long)by * g.w8 + bx], p = DIR == 0 ? cu8[(long)by * g.w8 + bx - 1] : cu8[(long)(by - 1) * g.w8 + bx];
    if (edge_bs(p, q, DIR == 0 ? bx : by) != 2) return;
    if (eff) qp = (eff[(long)by * g.w8 + bx] + eff[(long)by * g.w8 + bx - (DIR == 0 ? 1 : g.w8)] + 1) >> 1;
    const int tc = kTcTable[clip3(0, 53, chroma_qp(qp) + 2 + tc_off2)];
    uint8_t *C = ks_org_c(g, comp ? rv : ru) + (long)by * 4 * g.sc + bx * 4;
    const long xs = DIR == 0 ? 1 : g.sc, ys = DIR == 0 ? g.sc : 1;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        uint8_t *pp = C + l * ys;
        int p1 = pp[-2 * xs], p0 = pp[-xs], q0 = pp[0], q1 = pp[xs];
        deblock_chroma_line(p1, p0, q0, q1, tc, true, true);
        pp[-xs] = (uint8_t)p0; pp[0] = (uint8_t)q0;
    }
}

// QpY per 8x8 block with a QP per CTU (H.265 8.6.1, Log2MinCuQpDeltaSize = CtbLog2SizeY, entropy_coding_sync): cu_qp_delta arrives with the first coded residual of a
// CTU, so the CUs in front of it (z-order) keep the predicted QP = the QpY of the previous CTU's last CU, the slice QP at the start of a CTU row.  Two launches, one wave
// per CTU, lane = 8x8 block in z-order: (1) the z index of the CTU's first CU that carries residual (64: none) - a CU's blocks are adjacent lanes, "any cbf" is a masked
// ballot; (2) the predictor = the map entry of the nearest CTU to the left in the row that codes residual (one ballot over the row's first-z words), then the blocks.
// (The first version walked a CTU row per thread: 3 840 dependent loads, 1.9 ms at 2160p.)
__global__ __launch_bounds__(64) void qp_first_kernel(KsGeom g, const ks265_cu8 *cu8, unsigned char *firstz)
{
    const int ctu = blockIdx.x, cx = ctu % g.ctu_cols, cy = ctu / g.ctu_cols, z = threadIdx.x;
    const int lx = (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4), ly = ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4);
    const int bx = cx * 8 + lx, by = cy * 8 + ly;
    const bool in = bx < g.w8 && by < g.h8;
    ks265_cu8 c; c.log2_cu = 3; c.cbf = 0;
    if (in) c = cu8[(long)by * g.w8 + bx];
    const unsigned long long coded = __ballot(in && c.cbf != 0);
    const int nb = 1 << (2 * (((c.log2_cu & 15) < 3 ? 3 : (c.log2_cu & 15)) - 3));          // blocks of this lane's CU (1, 4, 16, 64)
    const unsigned long long gm = (nb == 64 ? ~0ull : ((1ull << nb) - 1ull)) << (z & ~(nb - 1));
    const unsigned long long cu_coded = __ballot(in && (coded & gm) != 0ull);                // lanes whose CU carries residual
    if (z == 0) firstz[ctu] = (unsigned char)(cu_coded ? __ffsll((long long)cu_coded) - 1 : 64);
}
__global__ __launch_bounds__(64) void qp_eff_kernel(KsGeom g, int slice_qp, const int8_t *qp_map, const unsigned char *firstz, uint8_t *eff)
{
    const int ctu = blockIdx.x, cx = ctu % g.ctu_cols, cy = ctu / g.ctu_cols, z = threadIdx.x;
    int prev = slice_qp;
    for (int hi = cx; hi > 0; hi -= 64) {                                                   // the row's CTUs left of this one, 64 at a time from the right
        const int c = hi - 64 + z;                                                          // lane 63 = CTU hi - 1
        const unsigned long long has = __ballot(c >= 0 && firstz[cy * g.ctu_cols + (c < 0 ? 0 : c)] < 64);
        if (has) { prev = qp_map[cy * g.ctu_cols + hi - 64 + (63 - __clzll((long long)has))]; break; }
    }
    const int lx = (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4), ly = ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4);
    const int bx = cx * 8 + lx, by = cy * 8 + ly;
    if (bx < g.w8 && by < g.h8) eff[(long)by * g.w8 + bx] = (uint8_t)(z < (int)firstz[ctu] ? prev : qp_map[ctu]);
}

extern "C" int ks265_deblock(ks265_frame *f, const ks265_cu8 *cu8, ks265_pic recon)
{
    KS_FRAME_CHECK(f);
    if (!cu8 || !recon.y) return KS265_POINTER;
    const KsGeom &g = f->g;
    const int qp = f->cfg.qp;
    const int b = qp + 2 * f->cfg.beta_offset_div2, beta_idx = b < 0 ? 0 : (b > 51 ? 51 : b);
    static const unsigned char beta_tab[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24,
                                               26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64};
    const int beta = beta_tab[beta_idx];
    const uint8_t *eff = nullptr;
    if (f->qp_map) {
        const int nctu = g.ctu_cols * g.ctu_rows;
        if (!f->qp_eff && hipMalloc((void **)&f->qp_eff, (size_t)g.w8 * g.h8 + (size_t)nctu) != hipSuccess) return KS265_OUTOFMEMORY;   // + one first-z byte per CTU
        unsigned char *firstz = f->qp_eff + (size_t)g.w8 * g.h8;
        hipLaunchKernelGGL(qp_first_kernel, dim3(nctu), dim3(64), 0, f->ctx->stream, g, cu8, firstz);
        hipLaunchKernelGGL(qp_eff_kernel, dim3(nctu), dim3(64), 0, f->ctx->stream, g, qp, f->qp_map, (const unsigned char *)firstz, f->qp_eff);
        eff = f->qp_eff;
    }
    const int n0 = g.w8 * (g.H / 4) + 2 * g.w8 * g.h8, n1 = (g.W / 4) * g.h8 + 2 * g.w8 * g.h8;
    hipLaunchKernelGGL(deblock_kernel<0>, dim3((n0 + 255) / 256), dim3(256), 0, f->ctx->stream, g, qp, beta, 2 * f->cfg.beta_offset_div2, 2 * f->cfg.tc_offset_div2, cu8, recon.y, recon.u, recon.v, eff);
    hipLaunchKernelGGL(deblock_kernel<1>, dim3((n1 + 255) / 256), dim3(256), 0, f->ctx->stream, g, qp, beta, 2 * f->cfg.beta_offset_div2, 2 * f->cfg.tc_offset_div2, cu8, recon.y, recon.u, recon.v, eff);
    return ks265_check_launch(f->ctx);
}

// ------------------------------------------------------------------ Stage F: SAO
struct SaoStats { int cnt[5][32]; int sum[5][32]; };      // [0] BO bands, [1..4] EO class 0..3 (4 categories used)

__device__ __forceinline__ int sao_offset(int sum, int cnt, int lo, int hi)
{
    if (!cnt) return 0;
    int o = sum >= 0 ? (sum + cnt / 2) / cnt : -((-sum + cnt / 2) / cnt);
    return clip3(lo, hi, o);
}

// per-band offset and distortion change, computed once per band (one integer division each) by 32 threads per component
struct SaoBand { signed char off[32]; long long dd[32]; };
__device__ __forceinline__ void sao_band_prepare(const SaoStats *s, SaoBand *b, int band)
{
    const int of = sao_offset(s->sum[0][band], s->cnt[0][band], -7, 7);
    b->off[band] = (signed char)of;
    b->dd[band] = (long long)s->cnt[0][band] * of * of - 2LL * of * s->sum[0][band];
}

__device__ long long sao_eval(const SaoStats *s, const SaoBand *bnd, int type, int lam, ks265_sao_param *out)
{
    const long long lam2 = (long long)lam * lam;
    ks265_sao_param o;
    o.type = (int8_t)type; o.band = 0; o.offset[0] = o.offset[1] = o.offset[2] = o.offset[3] = 0; o.rsv[0] = o.rsv[1] = 0;
    long long res;
    if (type == 0) {
        int best = 0; long long bd = 0;
        for (int p = 0; p <= 28; ++p) {
            const long long d = bnd->dd[p] + bnd->dd[p + 1] + bnd->dd[p + 2] + bnd->dd[p + 3];
            if (p == 0 || d < bd) { bd = d; best = p; }
        }
        int bits = 7;
        for (int k = 0; k < 4; ++k) { o.offset[k] = bnd->off[best + k]; bits += abs((int)bnd->off[best + k]) + 2; }
        o.band = (int8_t)best;
        res = bd * 256 + lam2 * bits;
    } else {
        long long d = 0; int bits = 4;
        for (int c = 0; c < 4; ++c) {
            const int of = sao_offset(s->sum[type][c], s->cnt[type][c], c < 2 ? 0 : -7, c < 2 ? 7 : 0);
            o.offset[c] = (int8_t)of;
            d += (long long)s->cnt[type][c] * of * of - 2LL * of * s->sum[type][c];
            bits += abs(of) + 1;
        }
        res = d * 256 + lam2 * bits;
    }
    *out = o;
    return res;
}

// ---- cfg.sao == 2 (round 6): the decision of CEncSao::modeDecisionCtu enc@0x4af690 on its -sao 4 path (modeDecisionBoEo01 enc@0x4af300: EO class 0, EO class 1, band offset per
// component group, strictly cheaper wins against "off" = one bin), priced by the reference's own functions - estIterOffset enc@0x4adbe0, BoTypeDistEstimation enc@0x4adc70,
// EoTypeDistEstimation enc@0x4adf60 (the oracle's restatements are pinned on the reference's outputs: sao_iter.npz, sao_type.npz) - with its rates (calcRDcostEoY / BoY / EoUV / BoUV:
// 4 / 7 / 4 / 12 lambda) and its lambda table g_lambdaOptforSAO enc@0x4df240.  32-bit arithmetic as in the binary.  Whole-CTU statistics and no merge candidates: see the oracle.
__constant__ int kLambdaSaoQ8[52] = {9, 12, 15, 19, 24, 31, 39, 50, 63, 79, 100, 127, 161, 203, 257, 325, 411, 519, 656, 829, 1048, 1324, 1674, 2115, 2673, 3377, 4268, 5393, 6815, 8612, 10883,
                                     13752, 17378, 21960, 27750, 35066, 44311, 55994, 70757, 89411, 112984, 142772, 180413, 227978, 288084, 364036, 460012, 581291, 734546, 928205, 1172921, 1482155};
__device__ __forceinline__ void sao_ref_iter_offset(int lam, int rate_base, int &offset, int count, int diff_sum, int &best_cost)
{
    int off = offset;
    const int step = off <= 0 ? 1 : -1;
    offset = 0;
    for (; off != 0; off += step) {
        const int dist = (int)((unsigned)off * ((unsigned)count * (unsigned)off - 2u * (unsigned)diff_sum));
        const int rate = (int)(((unsigned)lam * (unsigned)(rate_base + abs(off) + 1) + 128u)) >> 8;
        const int cost = (int)((unsigned)dist + (unsigned)rate);
        if (cost < best_cost) { offset = off; best_cost = cost; }
    }
}
__device__ __forceinline__ int sao_ref_start_offset(int d, int count, int sign_half)
{
    const int v = (d + ((sign_half * count) >> 1)) / count;
    return v > 3 ? 3 : (v < -3 ? -3 : v);
}
// one band of one component: its offset and cost (the per-band half of BoTypeDistEstimation)
__device__ __forceinline__ void sao_ref_band(int lam, int count, int sum, int &off, int &cost)
{
    const int zero = (lam + 128) >> 8;
    off = 0; cost = zero;
    if (!count) return;
    off = sao_ref_start_offset(sum, count, (sum > 0) - (sum < 0));
    sao_ref_iter_offset(lam, 1, off, count, sum, cost);
}
// one EO class of one component (EoTypeDistEstimation): the four offsets, returns the categories' cost sum
__device__ __forceinline__ int sao_ref_eo(int lam, const int *count, const int *sum, int8_t (&offs)[4])
{
    const int zero = (lam + 128) >> 8;
    int total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        offs[k] = 0;
        const bool positive = k < 2;
        if (!count[k] || (positive ? sum[k] <= 0 : sum[k] >= 0)) { total += zero; continue; }
        int off = sao_ref_start_offset(sum[k], count[k], positive ? 1 : -1), best = zero;
        sao_ref_iter_offset(lam, 0, off, count[k], sum[k], best);
        offs[k] = (int8_t)off; total += best;
    }
    return total;
}

// the candidates of modeDecisionBoEo01 in the reference's order, on the priced bands and edge classes of the three components: sel[3] = the CTU's own records, by / buv = the
// costs of its luma and chroma choice (what the merge candidates of cfg.sao == 3 are compared with)
__device__ __forceinline__ void sao_ref_decide(const int (*rb_off)[32], const int (*rb_cost)[32], const int (*re_cost)[2], const int8_t (*re_off)[2][4], int lamY, int lamC,
                                               ks265_sao_param *sel, int &by, int &buv)
{
    ks265_sao_param off;
    off.type = -1; off.band = 0; off.offset[0] = off.offset[1] = off.offset[2] = off.offset[3] = 0; off.rsv[0] = off.rsv[1] = 0;
    sel[0] = sel[1] = sel[2] = off;
    int bandc[3], bcost[3];
    for (int c = 0; c < 3; ++c) {                                  // the first of the 28 windows of four bands with the smallest cost sum
        int bc = 0xffff000, bb = 0;
        for (int k = 0; k < 28; ++k) { const int cc = rb_cost[c][k] + rb_cost[c][k + 1] + rb_cost[c][k + 2] + rb_cost[c][k + 3]; if (cc < bc) { bc = cc; bb = k; } }
        bandc[c] = bb; bcost[c] = bc;
    }
    int best = (lamY + 128) >> 8;
    for (int cls = 0; cls < 2; ++cls) {
        const int cost = re_cost[0][cls] + ((4 * lamY + 128) >> 8);
        if (cost < best) { best = cost; sel[0].type = (int8_t)(1 + cls); sel[0].band = 0; for (int k = 0; k < 4; ++k) sel[0].offset[k] = re_off[0][cls][k]; }
    }
    if (bcost[0] + ((7 * lamY + 128) >> 8) < best) { best = bcost[0] + ((7 * lamY + 128) >> 8); sel[0].type = 0; sel[0].band = (int8_t)bandc[0]; for (int k = 0; k < 4; ++k) sel[0].offset[k] = (int8_t)rb_off[0][bandc[0] + k]; }
    by = best;
    best = (lamC + 128) >> 8;
    for (int cls = 0; cls < 2; ++cls) {
        const int cost = re_cost[1][cls] + re_cost[2][cls] + ((4 * lamC + 128) >> 8);
        if (cost < best) {
            best = cost;
            for (int c = 1; c < 3; ++c) { sel[c].type = (int8_t)(1 + cls); sel[c].band = 0; for (int k = 0; k < 4; ++k) sel[c].offset[k] = re_off[c][cls][k]; }
        }
    }
    if (bcost[1] + bcost[2] + ((12 * lamC + 128) >> 8) < best) {
        best = bcost[1] + bcost[2] + ((12 * lamC + 128) >> 8);
        for (int c = 1; c < 3; ++c) { sel[c].type = 0; sel[c].band = (int8_t)bandc[c]; for (int k = 0; k < 4; ++k) sel[c].offset[k] = (int8_t)rb_off[c][bandc[c] + k]; }
    }
    buv = best;
}

// ---- LDS-staged CTU tiles: deblocked samples with a 1-sample halo (row pitch TP, sample (0,0) at [1][4]) + source samples.
// One thread owns a 4x4 block: 6 rows x 3 dwords of the deblocked tile feed all four EO classes of its 16 samples.
// Per-thread EO statistics are PACKED: per class one register of four 8-bit counts and two registers of two 16-bit sums
// of the biased difference (d + 128, d = the reference's s8-truncated org - rec, statSaoBoEo01_c enc@0x4ae9c0); 16 samples
// per thread cannot overflow the fields.  Band statistics go to LDS with one 64-bit atomic per sample (sum << 32 | count).
template <int TS>
struct SaoTile {
    static constexpr int TP = TS + 8;                      // row pitch (bytes): columns -4 .. TS+3
    uint8_t rec[(TS + 2) * TP];
    uint8_t org[TS * TS];
};
struct SaoAcc { unsigned long long bo[32]; int ecnt[4][4]; int esum[4][4]; };

template <int TS>
__device__ __forceinline__ void sao_load_tile(SaoTile<TS> &t, const uint8_t *org, const uint8_t *rec, long stride, int x0, int y0, int lt, int nt)
{
    constexpr int TP = SaoTile<TS>::TP;
    for (int i = lt; i < (TS + 2) * (TP / 4); i += nt) {
        const int r = i / (TP / 4), c = i - r * (TP / 4);
        *(unsigned *)&t.rec[r * TP + c * 4] = *(const unsigned *)(rec + (long)(y0 - 1 + r) * stride + x0 - 4 + c * 4);
    }
    for (int i = lt; i < TS * (TS / 4); i += nt) {
        const int r = i / (TS / 4), c = i - r * (TS / 4);
        *(unsigned *)&t.org[r * TS + c * 4] = *(const unsigned *)(org + (long)(y0 + r) * stride + x0 + c * 4);
    }
}

__device__ __forceinline__ int eo_index(int c, int a, int b) { return 2 + sgn(c - a) + sgn(c - b); }

// statistics of this thread's 4x4 block (bx4, by4 in units of 4 samples); w, h = valid tile size; (gx, gy) = picture coords of the tile
template <int TS>
__device__ __forceinline__ void sao_stats_block(const SaoTile<TS> &t, int bx4, int by4, int w, int h, int gx, int gy, int picW, int picH,
                                                SaoAcc *acc, bool active, int lane)
{
    constexpr int TP = SaoTile<TS>::TP;
    unsigned cntp[4] = {0, 0, 0, 0}, sumlo[4] = {0, 0, 0, 0}, sumhi[4] = {0, 0, 0, 0};
    int run_band = -1;                                      // band statistics are run-length merged: neighbouring samples mostly
    unsigned long long run_acc = 0;                         // share a band, so a 4x4 block flushes 1-3 LDS atomics instead of 16
    if (active) {
        const int x4 = bx4 * 4, y4 = by4 * 4;
        unsigned rows[6][3];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const unsigned *p = (const unsigned *)&t.rec[(y4 + r) * TP + x4];     // tile row y4-1+r, columns x4-4 .. x4+7
            rows[r][0] = p[0]; rows[r][1] = p[1]; rows[r][2] = p[2];
        }
        auto px = [&](int r, int x) -> int {                    // sample at block-relative (x, r-1), x in -1..4
            const int bi = x + 4;
            return (int)((rows[r][bi >> 2] >> (8 * (bi & 3))) & 255);
        };
#pragma unroll
        for (int yy = 0; yy < 4; ++yy) {
            const unsigned ov = *(const unsigned *)&t.org[(y4 + yy) * TS + x4];
#pragma unroll
            for (int xx = 0; xx < 4; ++xx) {
                const int lx = x4 + xx, ly = y4 + yy;
                if (lx >= w || ly >= h) continue;
                const int c = px(yy + 1, xx);
                const int d = (int)(int8_t)(uint8_t)(((ov >> (8 * xx)) & 255) - c);
                const unsigned ud = (unsigned)(d + 128);
                if ((c >> 3) != run_band) {
                    if (run_band >= 0) atomicAdd(&acc->bo[run_band], run_acc);
                    run_band = c >> 3; run_acc = 0;
                }
                run_acc += ((unsigned long long)ud << 32) | 1ull;
                const int X = gx + lx, Y = gy + ly;
                const bool okL = X > 0, okR = X < picW - 1, okU = Y > 0, okD = Y < picH - 1;
                const int e[4] = {eo_index(c, px(yy + 1, xx - 1), px(yy + 1, xx + 1)), eo_index(c, px(yy, xx), px(yy + 2, xx)),
                                  eo_index(c, px(yy, xx - 1), px(yy + 2, xx + 1)), eo_index(c, px(yy, xx + 1), px(yy + 2, xx - 1))};
                const bool ok[4] = {okL && okR, okU && okD, okL && okR && okU && okD, okL && okR && okU && okD};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!ok[k] || e[k] == 2) continue;
                    const int cat = e[k] < 2 ? e[k] : e[k] - 1;
                    cntp[k] += 1u << (8 * cat);
                    if (cat < 2) sumlo[k] += ud << (16 * cat); else sumhi[k] += ud << (16 * (cat - 2));
                }
            }
        }
    }
    if (run_band >= 0) atomicAdd(&acc->bo[run_band], run_acc);
    if (!__any(active)) return;                             // a wave without blocks (chroma: waves 2, 3) has nothing to reduce
    // unpack, reduce over the wave - count (<= 64 x 16 = 1024: 11 bits) and biased sum (<= 64 x 16 x 255 < 2^18) share one word,
    // so one DPP reduction per (class, category) - un-bias, one LDS atomic pair per (class, category) per wave
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int cat = 0; cat < 4; ++cat) {
            const unsigned cn = (cntp[k] >> (8 * cat)) & 255u;
            const unsigned sb = ((cat < 2 ? sumlo[k] : sumhi[k]) >> (16 * (cat & 1))) & 0xFFFFu;
            const unsigned tot = wave_sum((sb << 11) | cn);
            const int cs = (int)(tot & 2047u), ss = (int)(tot >> 11) - 128 * cs;
            if (lane == 0 && cs) { atomicAdd(&acc->ecnt[k][cat], cs); atomicAdd(&acc->esum[k][cat], ss); }
        }
}

__device__ __forceinline__ void sao_acc_to_stats(const SaoAcc *a, SaoStats *st, int lt, int nt)
{
    for (int i = lt; i < 32; i += nt) {
        const unsigned long long v = a->bo[i];
        const int cn = (int)(v & 0xFFFFFFFFull);
        st->cnt[0][i] = cn; st->sum[0][i] = (int)(v >> 32) - 128 * cn;
    }
    for (int i = lt; i < 16; i += nt) { st->cnt[1 + (i >> 2)][i & 3] = a->ecnt[i >> 2][i & 3]; st->sum[1 + (i >> 2)][i & 3] = a->esum[i >> 2][i & 3]; }
}

// apply to this thread's 4x4 block, from the LDS tile to the destination picture (one dword per row)
template <int TS>
__device__ __forceinline__ void sao_apply_block(const SaoTile<TS> &t, int bx4, int by4, int w, int h, int gx, int gy, int picW, int picH,
                                                const ks265_sao_param p, uint8_t *dst, long stride)
{
    constexpr int TP = SaoTile<TS>::TP;
    const int x4 = bx4 * 4, y4 = by4 * 4;
    if (x4 >= w || y4 >= h) return;
    // (no run-time indexed arrays: the record's four offsets as one word, the class's direction by arithmetic - indexing put 12 bytes per lane into scratch memory)
    const int k = p.type > 0 ? p.type - 1 : 0, dx = k == 1 ? 0 : k == 3 ? -1 : 1, dy = k == 0 ? 0 : 1;
    const unsigned offs = (unsigned)(uint8_t)p.offset[0] | ((unsigned)(uint8_t)p.offset[1] << 8) | ((unsigned)(uint8_t)p.offset[2] << 16) | ((unsigned)(uint8_t)p.offset[3] << 24);
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) {
        if (y4 + yy >= h) break;
        unsigned o = 0;
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) {
            const int lx = x4 + xx, ly = y4 + yy;
            const uint8_t *r = &t.rec[(ly + 1) * TP + lx + 4];
            const int c = r[0];
            int off = 0;
            if (p.type == 0) {
                const int kk = (c >> 3) - p.band;
                if (kk >= 0 && kk < 4) off = (int)(int8_t)(offs >> (8 * kk));
            } else if (p.type > 0) {
                const int X = gx + lx, Y = gy + ly;
                const int ax = X - dx, ay = Y - dy, bx = X + dx, by = Y + dy;
                if (!(ax < 0 || bx < 0 || ax >= picW || bx >= picW || ay < 0 || by >= picH)) {
                    const int e = eo_index(c, (int)r[-dy * TP - dx], (int)r[dy * TP + dx]);
                    if (e != 2) off = (int)(int8_t)(offs >> (8 * (e < 2 ? e : e - 1)));
                }
            }
            o |= (unsigned)clip8(c + off) << (8 * xx);
        }
        *(unsigned *)(dst + (long)(gy + y4 + yy) * stride + gx + x4) = o;       // widths are multiples of 4 (W % 8 == 0)
    }
}

template <bool REF>                                      // REF: cfg.sao == 2, the reference's decision (a kernel of its own: the default rule keeps its registers)
__global__ __launch_bounds__(256) void sao_ctu_kernel(KsGeom g, int lam, int enable, const uint8_t *sy, const uint8_t *su, const uint8_t *sv,
                                                      const uint8_t *dy, const uint8_t *du, const uint8_t *dv, ks265_sao_param *sao, uint8_t *oy,
                                                      uint8_t *ou, uint8_t *ov, int qp, const int8_t *qp_map)
{
    __shared__ int rb_off[3][32], rb_cost[3][32], re_cost[3][2];            // cfg.sao == 2: per band offset / cost, per component and EO class the categories' cost
    __shared__ int8_t re_off[3][2][4];
    __shared__ __attribute__((aligned(16))) SaoTile<64> tl;
    __shared__ __attribute__((aligned(16))) SaoTile<32> tc[2];
    __shared__ __attribute__((aligned(16))) SaoAcc acc[3];
    __shared__ SaoStats st[3];
    __shared__ SaoBand bnd[3];
    __shared__ ks265_sao_param sel[3];
    __shared__ long long jl[5], jc[5];
    __shared__ ks265_sao_param cand[3][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctu = ks_xcd_swizzle(blockIdx.x, g.ctu_cols * g.ctu_rows), cx = ctu % g.ctu_cols, cy = ctu / g.ctu_cols;
    const int x0 = cx * 64, y0 = cy * 64, w = min(64, g.W - x0), h = min(64, g.H - y0);
    for (int i = tid; i < (int)(sizeof(acc) / 4); i += 256) ((int *)acc)[i] = 0;
    sao_load_tile<64>(tl, ks_org_y(g, sy), ks_org_y(g, dy), g.sy, x0, y0, tid, 256);
    {
        const int cc = tid >> 7;                          // threads 0..127 stage Cb, 128..255 stage Cr
        sao_load_tile<32>(tc[cc], ks_org_c(g, cc ? sv : su), ks_org_c(g, cc ? dv : du), g.sc, x0 / 2, y0 / 2, tid & 127, 128);
    }
    __syncthreads();
    // luma: 16 x 16 blocks of 4x4 = 256 threads; chroma: 8 x 8 blocks per component, wave 0 = Cb, wave 1 = Cr
    sao_stats_block<64>(tl, tid & 15, tid >> 4, w, h, x0, y0, g.W, g.H, &acc[0], true, lane);
    sao_stats_block<32>(tc[wave & 1], lane & 7, lane >> 3, w / 2, h / 2, x0 / 2, y0 / 2, g.W / 2, g.H / 2, &acc[1 + (wave & 1)], wave < 2, lane);
    __syncthreads();
    sao_acc_to_stats(&acc[0], &st[0], tid, 256);
    sao_acc_to_stats(&acc[1], &st[1], tid, 256);
    sao_acc_to_stats(&acc[2], &st[2], tid, 256);
    __syncthreads();
    if (REF) {
        // the reference's decision: bands and EO classes priced in parallel, then one thread walks the candidates in the reference's order
        const int q = qp_map ? qp_map[ctu] : qp, lamY = kLambdaSaoQ8[q], lamC = kLambdaSaoQ8[chroma_qp(q)];
        if (tid < 96) { const int c = tid >> 5, b = tid & 31; sao_ref_band(c ? lamC : lamY, st[c].cnt[0][b], st[c].sum[0][b], rb_off[c][b], rb_cost[c][b]); }
        else if (tid < 102) { const int c = (tid - 96) >> 1, cls = (tid - 96) & 1; re_cost[c][cls] = sao_ref_eo(c ? lamC : lamY, st[c].cnt[1 + cls], st[c].sum[1 + cls], re_off[c][cls]); }
        __syncthreads();
        if (tid == 0) {
            int by, buv;
            sao_ref_decide(rb_off, rb_cost, re_cost, re_off, lamY, lamC, sel, by, buv);
            sao[(long)ctu * 3 + 0] = sel[0]; sao[(long)ctu * 3 + 1] = sel[1]; sao[(long)ctu * 3 + 2] = sel[2];
        }
    } else {
    if (tid < 96) sao_band_prepare(&st[tid >> 5], &bnd[tid >> 5], tid & 31);
    __syncthreads();
    if (tid < 15) {                                    // 3 components x 5 types evaluated in parallel
        const int comp = tid / 5, t = tid % 5;
        long long j = sao_eval(&st[comp], &bnd[comp], t, lam, &cand[comp][t]);
        if (comp == 0) jl[t] = j;
        else if (comp == 1) jc[t] = j;
    }
    __syncthreads();
    if (tid >= 10 && tid < 15) {                       // chroma cost is the sum over Cb and Cr
        ks265_sao_param tmp;
        jc[tid - 10] += sao_eval(&st[2], &bnd[2], tid - 10, lam, &tmp);
    }
    __syncthreads();
    if (tid == 0) {
        ks265_sao_param off;
        off.type = -1; off.band = 0; off.offset[0] = off.offset[1] = off.offset[2] = off.offset[3] = 0; off.rsv[0] = off.rsv[1] = 0;
        sel[0] = sel[1] = sel[2] = off;
        long long bj = 0, bjc = 0;
        if (enable)
            for (int t = 0; t < 5; ++t) {
                if (jl[t] < bj) { bj = jl[t]; sel[0] = cand[0][t]; }
                if (jc[t] < bjc) { bjc = jc[t]; sel[1] = cand[1][t]; sel[2] = cand[2][t]; }
            }
        sao[(long)ctu * 3 + 0] = sel[0]; sao[(long)ctu * 3 + 1] = sel[1]; sao[(long)ctu * 3 + 2] = sel[2];
    }
    }
    __syncthreads();
    sao_apply_block<64>(tl, tid & 15, tid >> 4, w, h, x0, y0, g.W, g.H, sel[0], ks_org_y(g, oy), g.sy);
    if (wave < 2) sao_apply_block<32>(tc[wave], lane & 7, lane >> 3, w / 2, h / 2, x0 / 2, y0 / 2, g.W / 2, g.H / 2, sel[1 + wave], ks_org_c(g, wave ? ov : ou), g.sc);
}

// ---- cfg.sao == 3: cfg.sao == 2 plus the merge candidates of CEncSao::modeDecisionCtu enc@0x4af690 (checkMerge enc@0x4ae7f0; the oracle's pinned restatement of it with both
// neighbours, masks 0x13).  After its own choice a CTU prices the FINAL records of its left and upper CTU on its own statistics; strictly cheaper copies them and sets
// sao_merge_left_flag / sao_merge_up_flag (rsv[0] / rsv[1] of the luma record).  The final record of a CTU depends on those of (cx - 1, cy) and (cx, cy - 1): a chain in coding
// order, run along the anti-diagonals cx + cy.  Three launches:
//   sao_merge_stats_kernel  one work-group per CTU: statistics + own decision (the front of sao_ctu_kernel<true>) into the workspace, KS_SAO_WS_WORDS words per CTU:
//                           [0..312) the statistics in the reference's 312-word layout (bands Y / U / V, edge classes at 96 + 20 component + 5 class; sums 156 words on), [312..318) the own three records, [318] the own cost by + buv,
//                           [319] (lambda_avg + 128) >> 8, what an upper CTU adds to the own cost and to the upper candidate;
//   sao_merge_chain_kernel  ONE work-group: wave 0 decides a diagonal, a lane per CTU, from LDS only; the other waves meanwhile stage the next diagonal's words;
//   sao_merge_apply_kernel  one work-group per CTU: the final records applied out of place.
// No work-group waits for another one.
__global__ __launch_bounds__(256) void sao_merge_stats_kernel(KsGeom g, const uint8_t *sy, const uint8_t *su, const uint8_t *sv, const uint8_t *dy, const uint8_t *du,
                                                              const uint8_t *dv, int *ws, int qp, const int8_t *qp_map)
{
    __shared__ int rb_off[3][32], rb_cost[3][32], re_cost[3][2];
    __shared__ int8_t re_off[3][2][4];
    __shared__ __attribute__((aligned(16))) SaoTile<64> tl;
    __shared__ __attribute__((aligned(16))) SaoTile<32> tc[2];
    __shared__ __attribute__((aligned(16))) SaoAcc acc[3];
    __shared__ SaoStats st[3];
    __shared__ __attribute__((aligned(8))) ks265_sao_param sel[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctu = ks_xcd_swizzle(blockIdx.x, g.ctu_cols * g.ctu_rows), cx = ctu % g.ctu_cols, cy = ctu / g.ctu_cols;
    const int x0 = cx * 64, y0 = cy * 64, w = min(64, g.W - x0), h = min(64, g.H - y0);
    for (int i = tid; i < (int)(sizeof(acc) / 4); i += 256) ((int *)acc)[i] = 0;
    sao_load_tile<64>(tl, ks_org_y(g, sy), ks_org_y(g, dy), g.sy, x0, y0, tid, 256);
    {
        const int cc = tid >> 7;
        sao_load_tile<32>(tc[cc], ks_org_c(g, cc ? sv : su), ks_org_c(g, cc ? dv : du), g.sc, x0 / 2, y0 / 2, tid & 127, 128);
    }
    __syncthreads();
    sao_stats_block<64>(tl, tid & 15, tid >> 4, w, h, x0, y0, g.W, g.H, &acc[0], true, lane);
    sao_stats_block<32>(tc[wave & 1], lane & 7, lane >> 3, w / 2, h / 2, x0 / 2, y0 / 2, g.W / 2, g.H / 2, &acc[1 + (wave & 1)], wave < 2, lane);
    __syncthreads();
    sao_acc_to_stats(&acc[0], &st[0], tid, 256);
    sao_acc_to_stats(&acc[1], &st[1], tid, 256);
    sao_acc_to_stats(&acc[2], &st[2], tid, 256);
    __syncthreads();
    const int q = qp_map ? qp_map[ctu] : qp, lamY = kLambdaSaoQ8[q], lamC = kLambdaSaoQ8[chroma_qp(q)];
    if (tid < 96) { const int c = tid >> 5, b = tid & 31; sao_ref_band(c ? lamC : lamY, st[c].cnt[0][b], st[c].sum[0][b], rb_off[c][b], rb_cost[c][b]); }
    else if (tid < 102) { const int c = (tid - 96) >> 1, cls = (tid - 96) & 1; re_cost[c][cls] = sao_ref_eo(c ? lamC : lamY, st[c].cnt[1 + cls], st[c].sum[1 + cls], re_off[c][cls]); }
    int *out = ws + (long)ctu * KS_SAO_WS_WORDS;
    for (int i = tid; i < 156; i += 256) {               // counts, then the sums 156 words on: bands of Y, U, V; per component 4 classes x 5 words, classes 0 and 1 x 4 categories used
        int cn = 0, sm = 0;
        if (i < 96) { cn = st[i >> 5].cnt[0][i & 31]; sm = st[i >> 5].sum[0][i & 31]; }
        else {
            const int j = i - 96, c = j / 20, r = j - 20 * c, cls = r / 5, k = r - 5 * cls;
            if (cls < 2 && k < 4) { cn = st[c].cnt[1 + cls][k]; sm = st[c].sum[1 + cls][k]; }
        }
        out[i] = cn; out[156 + i] = sm;
    }
    __syncthreads();
    if (tid == 0) {
        int by, buv;
        sao_ref_decide(rb_off, rb_cost, re_cost, re_off, lamY, lamC, sel, by, buv);
        const int *sw = (const int *)sel;
        for (int i = 0; i < 6; ++i) out[312 + i] = sw[i];
        out[318] = (int)((unsigned)by + (unsigned)buv);
        out[319] = (((lamY + lamC + 1) >> 1) + 128) >> 8;
    }
}

// the words of a CTU's workspace that the chain can ask for, compacted for LDS: [0..96) band counts of Y, U, V, [96..120) edge counts [component][class 0, 1][category],
// [120..240) the sums likewise, [240..248) the own records, own cost and the upper CTU's lambda term
#define KS_SAO_CHAIN_WORDS 248
__device__ __forceinline__ int sao_chain_src_word(int w)
{
    if (w >= 240) return 312 + (w - 240);
    const int half = w >= 120, v = w - 120 * half, e = v - 96;
    return 156 * half + (v < 96 ? v : 96 + 20 * (e >> 3) + 5 * ((e >> 2) & 1) + (e & 3));
}
// the distortion change the three records p[] give on the statistics m[] of another CTU (sao_merge_dist of the oracle in this build's record codes; 32-bit wrap-around)
__device__ __forceinline__ int sao_chain_merge_dist(const int *m, const ks265_sao_param *p)
{
    unsigned d = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const ks265_sao_param r = p[c];
        if (r.type < 0) continue;
        const int at = r.type == 0 ? 32 * c + r.band : 96 + 8 * c + 4 * (r.type - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const unsigned o = (unsigned)(int)r.offset[i]; d += ((unsigned)m[at + i] * o - 2u * (unsigned)m[120 + at + i]) * o; }
    }
    return (int)d;
}
// the diagonal d holds the CTUs (d - cy, cy), cy in [lo, hi]; a step = up to 64 of them from cy0 on
struct SaoChainStep { int d, cy0, n; };
__device__ __forceinline__ SaoChainStep sao_chain_step(int d, int cy0, int cols, int rows)
{
    const int hi = min(rows - 1, d);
    SaoChainStep s = {d, cy0, min(64, hi - cy0 + 1)};
    return s;
}
__device__ __forceinline__ SaoChainStep sao_chain_next(SaoChainStep s, int cols, int rows)
{
    if (s.cy0 + 64 <= min(rows - 1, s.d)) return sao_chain_step(s.d, s.cy0 + 64, cols, rows);
    return sao_chain_step(s.d + 1, max(0, s.d + 1 - (cols - 1)), cols, rows);
}
__device__ __forceinline__ void sao_chain_stage(int (*dst)[KS_SAO_CHAIN_WORDS], const int *ws, SaoChainStep s, int cols, int lt, int nt)
{
    for (int i = lt; i < s.n * KS_SAO_CHAIN_WORDS; i += nt) {
        const int l = i / KS_SAO_CHAIN_WORDS, w = i - l * KS_SAO_CHAIN_WORDS, cy = s.cy0 + l;
        dst[l][w] = ws[(long)(cy * cols + s.d - cy) * KS_SAO_WS_WORDS + sao_chain_src_word(w)];
    }
}
__global__ __launch_bounds__(256) void sao_merge_chain_kernel(int cols, int rows, const int *ws, ks265_sao_param *sao)
{
    __shared__ int ms[2][64][KS_SAO_CHAIN_WORDS];                                            // the step being decided and the next one
    __shared__ __attribute__((aligned(8))) ks265_sao_param fin[2][KS_SAO_CHAIN_ROWS][3];     // final records of the diagonal being decided and of the one before, by CTU row
    const int tid = threadIdx.x, last = cols + rows - 2;
    SaoChainStep s = sao_chain_step(0, 0, cols, rows);
    sao_chain_stage(ms[0], ws, s, cols, tid, 256);
    __syncthreads();
    for (int b = 0; s.d <= last; b ^= 1) {
        const SaoChainStep nx = sao_chain_next(s, cols, rows);
        if (tid >= 64) { if (nx.d <= last) sao_chain_stage(ms[b ^ 1], ws, nx, cols, tid - 64, 192); }
        else if (tid < s.n) {
            const int cy = s.cy0 + tid, cx = s.d - cy, *m = ms[b][tid];
            const ks265_sao_param *prev = &fin[(s.d & 1) ^ 1][0][0];
            ks265_sao_param r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = ((const ks265_sao_param *)(m + 240))[c];
            int tot = (int)((unsigned)m[246] + (cy > 0 ? (unsigned)m[247] : 0u)), ml = 0, mu = 0;
            if (cx > 0) {
                const int c = sao_chain_merge_dist(m, prev + 3 * cy);
                if (tot > c) { tot = c; ml = 1; }
            }
            if (cy > 0) {
                const int c = (int)((unsigned)sao_chain_merge_dist(m, prev + 3 * (cy - 1)) + (unsigned)m[247]);
                if (tot > c) { ml = 0; mu = 1; }
            }
            if (ml | mu) {
                const ks265_sao_param *n = prev + 3 * (cy - mu);
#pragma unroll
                for (int c = 0; c < 3; ++c) { r[c] = n[c]; r[c].rsv[0] = r[c].rsv[1] = 0; }
                r[0].rsv[0] = (int8_t)ml; r[0].rsv[1] = (int8_t)mu;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { fin[s.d & 1][cy][c] = r[c]; sao[(long)(cy * cols + cx) * 3 + c] = r[c]; }
        }
        __syncthreads();
        s = nx;
    }
}

__global__ __launch_bounds__(256) void sao_merge_apply_kernel(KsGeom g, const uint8_t *sy, const uint8_t *su, const uint8_t *sv, const uint8_t *dy, const uint8_t *du,
                                                              const uint8_t *dv, const ks265_sao_param *sao, uint8_t *oy, uint8_t *ou, uint8_t *ov)
{
    __shared__ __attribute__((aligned(16))) SaoTile<64> tl;
    __shared__ __attribute__((aligned(16))) SaoTile<32> tc[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctu = ks_xcd_swizzle(blockIdx.x, g.ctu_cols * g.ctu_rows), cx = ctu % g.ctu_cols, cy = ctu / g.ctu_cols;
    const int x0 = cx * 64, y0 = cy * 64, w = min(64, g.W - x0), h = min(64, g.H - y0);
    sao_load_tile<64>(tl, ks_org_y(g, sy), ks_org_y(g, dy), g.sy, x0, y0, tid, 256);
    {
        const int cc = tid >> 7;
        sao_load_tile<32>(tc[cc], ks_org_c(g, cc ? sv : su), ks_org_c(g, cc ? dv : du), g.sc, x0 / 2, y0 / 2, tid & 127, 128);
    }
    __syncthreads();
    sao_apply_block<64>(tl, tid & 15, tid >> 4, w, h, x0, y0, g.W, g.H, sao[(long)ctu * 3], ks_org_y(g, oy), g.sy);
    if (wave < 2) sao_apply_block<32>(tc[wave], lane & 7, lane >> 3, w / 2, h / 2, x0 / 2, y0 / 2, g.W / 2, g.H / 2, sao[(long)ctu * 3 + 1 + wave], ks_org_c(g, wave ? ov : ou), g.sc);
}

// a picture without SAO (cfg.sao = 0 per picture, ks265_frame_set_picture_tools): every record "off" - what sao_ctu_kernel writes with enable = 0
__global__ void sao_off_kernel(int n, ks265_sao_param *sao)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ks265_sao_param off;
    off.type = -1; off.band = 0; off.offset[0] = off.offset[1] = off.offset[2] = off.offset[3] = 0; off.rsv[0] = off.rsv[1] = 0;
    sao[i] = off;
}
// the tail of a picture that was reconstructed and deblocked in dst itself: records off, borders padded
int ks265_sao_off(ks265_frame *f, ks265_sao_param *sao, ks265_pic dst)
{
    KS_FRAME_CHECK(f);
    if (!sao || !dst.y) return KS265_POINTER;
    const int n = f->g.ctu_cols * f->g.ctu_rows * 3;
    hipLaunchKernelGGL(sao_off_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, f->ctx->stream, n, sao);
    int r = ks265_check_launch(f->ctx);
    if (r) return r;
    return ks265_pad_picture(f, dst);
}

extern "C" int ks265_sao(ks265_frame *f, ks265_pic src, ks265_pic deb, ks265_sao_param *sao, ks265_pic dst)
{
    KS_FRAME_CHECK(f);
    if (!src.y || !deb.y || !sao || !dst.y) return KS265_POINTER;
    if (f->cfg.sao == 3) {
        if (!f->sao_ws) return KS265_NOTSUPPORTED;
        const int n = f->g.ctu_cols * f->g.ctu_rows;
        hipLaunchKernelGGL(sao_merge_stats_kernel, dim3(n), dim3(256), 0, f->ctx->stream, f->g, src.y, src.u, src.v, deb.y, deb.u, deb.v, f->sao_ws, f->cfg.qp, f->qp_map);
        hipLaunchKernelGGL(sao_merge_chain_kernel, dim3(1), dim3(256), 0, f->ctx->stream, f->g.ctu_cols, f->g.ctu_rows, (const int *)f->sao_ws, sao);
        hipLaunchKernelGGL(sao_merge_apply_kernel, dim3(n), dim3(256), 0, f->ctx->stream, f->g, src.y, src.u, src.v, deb.y, deb.u, deb.v, (const ks265_sao_param *)sao, dst.y, dst.u, dst.v);
    } else if (f->cfg.sao == 2) hipLaunchKernelGGL(sao_ctu_kernel<true>, dim3(f->g.ctu_cols * f->g.ctu_rows), dim3(256), 0, f->ctx->stream, f->g, f->cfg.lambda_q4, f->cfg.sao, src.y, src.u,
                                            src.v, deb.y, deb.u, deb.v, sao, dst.y, dst.u, dst.v, f->cfg.qp, f->qp_map);
    else hipLaunchKernelGGL(sao_ctu_kernel<false>, dim3(f->g.ctu_cols * f->g.ctu_rows), dim3(256), 0, f->ctx->stream, f->g, f->cfg.lambda_q4, f->cfg.sao, src.y, src.u,
                            src.v, deb.y, deb.u, deb.v, sao, dst.y, dst.u, dst.v, f->cfg.qp, f->qp_map);
    int r = ks265_check_launch(f->ctx);
    if (r) return r;
    return ks265_pad_picture(f, dst);
}
