// analysis.hip — what the encoder decided about a picture, as arrays (include/ks265_hip.h ks265_analysis_*; tests/analysis_ref.py is the specification):
//   ks265_analysis_pack    the CU map (one ks265_cu8 per 8x8 luma block), the per-CTU QP map and the squared error between the padded source and reconstruction ->
//                          ONE packed block in HBM: motion vectors and reference POC deltas per list, the CU tree / mode / coded-block planes, the QP of every CTU, the SSE
//                          of every 8x8 luma and 4x4 chroma block.  Bandwidth-shaped (two pictures read once: 2 x 1.5 W H bytes): a lane owns two horizontally adjacent
//                          blocks, i.e. 16 bytes of each of 8 luma rows and 8 bytes of each of 4 rows of either chroma plane, per picture - all 64 loads issued before
//                          the first use; v_dot4 sums; no LDS, no atomics, no cross-lane traffic: every output word has one writer, so work-group order cannot matter.
//   ks265_analysis_export  the packed block -> the caller's five arrays with their own pitches, one launch; a thread moves one dword of a packed row and writes only
//                          the bytes of it that lie inside the destination row.
//
// The packed block (ks265_analysis_layout): five segments, each starting on a multiple of 256 bytes, rows of P = round_up(W / 8, 4) entries (so that a lane's pair of entries
// is one aligned store and an export thread's dword never straddles two rows); entries w8 .. P - 1 of a row are never read:
//   off[0] mv   int16 [2][h8][P][2]      off[1] ref  int8 [2][h8][P]      off[2] cu   uint8 [5][h8][P]      off[3] sse  int32 [3][h8][P]
//   off[4] qp   int8 [cr][round_up(cc, 4)]                                off[5] = size of the block
#include "frame_common.h"

namespace {

struct AnLayout { size_t off[6]; int w8, h8, P, cc, cr, Pq; };

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

AnLayout an_layout(int W, int H)
{
    AnLayout L{};
    L.w8 = W / 8; L.h8 = H / 8; L.P = (L.w8 + 3) & ~3; L.cc = (W + 63) / 64; L.cr = (H + 63) / 64; L.Pq = (L.cc + 3) & ~3;
    const size_t n = (size_t)L.P * L.h8;
    L.off[0] = 0;
    L.off[1] = up256(L.off[0] + n * 8);
    L.off[2] = up256(L.off[1] + n * 2);
    L.off[3] = up256(L.off[2] + n * 5);
    L.off[4] = up256(L.off[3] + n * 12);
    L.off[5] = up256(L.off[4] + (size_t)L.Pq * L.cr);
    return L;
}

struct AnPackArgs {
    const uint8_t *sy, *su, *sv, *ry, *ru, *rv;   // sample (0, 0) of the six planes
    const unsigned *cu8;                          // ks265_cu8 records as three dwords each
    const int8_t *qp_map;
    int picture_qp;
    unsigned delta[2];                            // list L's four POC deltas, byte i = index i
    int stride_y, stride_c;
    int w8, h8, P, ppr, nctu, cc, Pq;             // ppr = pairs of blocks per row = ceil(w8 / 2)
    int wide_y, wide_c;                           // luma rows 16-byte aligned / chroma rows 8-byte aligned (else dword loads)
    uint8_t *blk; unsigned long long off_ref, off_cu, off_sse, off_qp;
};

__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_udot4(a, b, acc, false); }
// sum (a - b)^2 over the four bytes of a dword pair, added to acc: a.a + b.b - 2 a.b, every partial sum below 2^23 for a block's 64 samples
__device__ __forceinline__ unsigned sq4(unsigned a, unsigned b, unsigned acc) { return dot4(a, a, dot4(b, b, acc)) - 2u * dot4(a, b, 0u); }

struct AnRec { int mv0, mv1; int ref0, ref1; unsigned kind, lg, part, cbf, mode; };

// one ks265_cu8 record (w0 = mvx | mvy << 16, w1 = mv1x | mv1y << 16, w2 = log2_cu | cbf << 8 | pred_mode << 16 | inter_dir << 24) -> the fields of tests/analysis_ref.py
__device__ __forceinline__ AnRec an_decode(unsigned w0, unsigned w1, unsigned w2, unsigned d0, unsigned d1)
{
    AnRec r;
    const unsigned lc = w2 & 255u, pm = w2 >> 16 & 255u, id = w2 >> 24;
    const unsigned dir = pm ? 0u : (id & 3u);
    r.mv0 = (dir & 1u) ? (int)w0 : 0;
    r.mv1 = (dir & 2u) ? (int)w1 : 0;
    r.ref0 = (dir & 1u) ? (int)(int8_t)(d0 >> (8u * (id >> 4 & 3u))) : 0;
    r.ref1 = (dir & 2u) ? (int)(int8_t)(d1 >> (8u * (id >> 6 & 3u))) : 0;
    r.kind = dir; r.lg = lc & 15u; r.part = lc >> 4 & 3u; r.cbf = w2 >> 8 & 255u;
    r.mode = pm == 2u ? (w0 & 255u) : 255u;
    return r;
}

// A lane owns the blocks (by, 2 px) and (by, 2 px + 1); the second does not exist in the last pair of a row with an odd block count - its samples are then the first
// 8 (4) columns of the right border, which are read (they lie inside the padding of 80 / 40 samples) and whose sums are dropped.  Lanes below nctu also write one CTU's QP.
__global__ __launch_bounds__(256) void analysis_pack_kernel(AnPackArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.nctu) ((int8_t *)(a.blk + a.off_qp))[(i / a.cc) * a.Pq + i % a.cc] = a.qp_map ? a.qp_map[i] : (int8_t)a.picture_qp;
    if (i >= a.ppr * a.h8) return;
    const int by = i / a.ppr, px = i - by * a.ppr;
    const bool two = 2 * px + 1 < a.w8;
    const long oy = (long)(by * 8) * a.stride_y + px * 16, oc = (long)(by * 4) * a.stride_c + px * 8;
    const uint8_t *psy = a.sy + oy, *pry = a.ry + oy;
    const uint8_t *pc[4] = {a.su + oc, a.ru + oc, a.sv + oc, a.rv + oc};
    uint4 vs[8], vr[8];
    uint2 c[4][4];
    if (a.wide_y) {
#pragma unroll
        for (int r = 0; r < 8; ++r) { vs[r] = *(const uint4 *)(psy + (long)r * a.stride_y); vr[r] = *(const uint4 *)(pry + (long)r * a.stride_y); }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned *p = (const unsigned *)(psy + (long)r * a.stride_y), *q = (const unsigned *)(pry + (long)r * a.stride_y);
            vs[r] = make_uint4(p[0], p[1], p[2], p[3]); vr[r] = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
    if (a.wide_c) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) c[k][r] = *(const uint2 *)(pc[k] + (long)r * a.stride_c);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const unsigned *p = (const unsigned *)(pc[k] + (long)r * a.stride_c); c[k][r] = make_uint2(p[0], p[1]); }
    }
    // the two records: six dwords (a record is 12 bytes, so a pair is only 4-byte aligned in general); the missing second block reads the first one's again
    const unsigned *rec0 = a.cu8 + 3l * ((long)by * a.w8 + 2 * px), *rec1 = two ? rec0 + 3 : rec0;
    const unsigned q0 = rec0[0], q1 = rec0[1], q2 = rec0[2], q3 = rec1[0], q4 = rec1[1], q5 = rec1[2];

    unsigned y0 = 0, y1 = 0, u0 = 0, u1 = 0, v0 = 0, v1 = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        y0 = sq4(vs[r].y, vr[r].y, sq4(vs[r].x, vr[r].x, y0));
        y1 = sq4(vs[r].w, vr[r].w, sq4(vs[r].z, vr[r].z, y1));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        u0 = sq4(c[0][r].x, c[1][r].x, u0); u1 = sq4(c[0][r].y, c[1][r].y, u1);
        v0 = sq4(c[2][r].x, c[3][r].x, v0); v1 = sq4(c[2][r].y, c[3][r].y, v1);
    }
    const AnRec A = an_decode(q0, q1, q2, a.delta[0], a.delta[1]);
    AnRec B = an_decode(q3, q4, q5, a.delta[0], a.delta[1]);
    if (!two) { B = AnRec{0, 0, 0, 0, 0u, 0u, 0u, 0u, 0u}; y1 = u1 = v1 = 0; }

    const long n = (long)a.P * a.h8, e = (long)by * a.P + 2 * px;       // entries per plane; this pair's first entry (even: P is a multiple of 4)
    uint2 *mv = (uint2 *)a.blk;
    mv[(e) >> 1] = make_uint2((unsigned)A.mv0, (unsigned)B.mv0);
    mv[(n + e) >> 1] = make_uint2((unsigned)A.mv1, (unsigned)B.mv1);
    unsigned short *rf = (unsigned short *)(a.blk + a.off_ref);
    rf[(e) >> 1] = (unsigned short)((A.ref0 & 255) | (B.ref0 & 255) << 8);
    rf[(n + e) >> 1] = (unsigned short)((A.ref1 & 255) | (B.ref1 & 255) << 8);
    unsigned short *cu = (unsigned short *)(a.blk + a.off_cu);
    cu[(e) >> 1] = (unsigned short)(A.kind | B.kind << 8);
    cu[(n + e) >> 1] = (unsigned short)(A.lg | B.lg << 8);
    cu[(2 * n + e) >> 1] = (unsigned short)(A.part | B.part << 8);
    cu[(3 * n + e) >> 1] = (unsigned short)(A.cbf | B.cbf << 8);
    cu[(4 * n + e) >> 1] = (unsigned short)(A.mode | B.mode << 8);
    uint2 *ss = (uint2 *)(a.blk + a.off_sse);
    ss[(e) >> 1] = make_uint2(y0, y1);
    ss[(n + e) >> 1] = make_uint2(u0, u1);
    ss[(2 * n + e) >> 1] = make_uint2(v0, v1);
}

// one field of the export: nplanes x rows rows of row_bytes, read at src (pitch src_pitch, planes rows x src_pitch apart), written at dst (pitch, plane)
struct AnField { const uint8_t *src; uint8_t *dst; long long pitch, plane; int src_pitch, rows, row_bytes, rdw /* dwords per row, the last one possibly cut */, es, al4; unsigned first, end; };
struct AnExportArgs { AnField f[5]; };

// A thread per dword of a packed row (packed rows start on multiples of 4 and are padded to them).  A whole dword goes out as one store where the destination's address,
// pitch and plane step are multiples of 4, else - and the row's last, cut dword always - as elements; never a byte outside [row start, row start + row_bytes).
__global__ __launch_bounds__(256) void analysis_export_kernel(AnExportArgs a)
{
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    // the field by a chain of selects (an indexed read of the argument array would cost scratch)
    int k = -1;
#pragma unroll
    for (int q = 0; q < 5; ++q) if (j >= a.f[q].first && j < a.f[q].end) k = q;
    if (k < 0) return;
#define AN_SEL(m) (k == 0 ? a.f[0].m : k == 1 ? a.f[1].m : k == 2 ? a.f[2].m : k == 3 ? a.f[3].m : a.f[4].m)
    const uint8_t *src = AN_SEL(src); uint8_t *dst = AN_SEL(dst);
    const long long pitch = AN_SEL(pitch), plane = AN_SEL(plane);
    const int src_pitch = AN_SEL(src_pitch), rows = AN_SEL(rows), row_bytes = AN_SEL(row_bytes), rdw = AN_SEL(rdw), es = AN_SEL(es), al4 = AN_SEL(al4);
    const unsigned t = j - AN_SEL(first);
#undef AN_SEL
    const unsigned row = t / (unsigned)rdw, cdw = t - row * (unsigned)rdw;
    const unsigned p = row / (unsigned)rows, r = row - p * (unsigned)rows;
    const unsigned v = *(const unsigned *)(src + (long long)row * src_pitch + 4ll * cdw);
    uint8_t *d = dst + (long long)p * plane + (long long)r * pitch + 4ll * cdw;
    const int nb = min(4, row_bytes - 4 * (int)cdw);                    // bytes of this dword inside the row: 4, or 1 .. 3 at the end of a row of bytes, or 2 (int16 elements)
    if (nb == 4 && al4) { *(unsigned *)d = v; return; }
    if (es == 2) {
        *(unsigned short *)d = (unsigned short)v;
        if (nb == 4) *(unsigned short *)(d + 2) = (unsigned short)(v >> 16);
    } else if (es == 1) {
        d[0] = (uint8_t)v;
        if (nb > 1) d[1] = (uint8_t)(v >> 8);
        if (nb > 2) d[2] = (uint8_t)(v >> 16);
        if (nb > 3) d[3] = (uint8_t)(v >> 24);
    }                                                                   // (es == 4: address, pitch and plane are multiples of 4 - al4 holds)
}

struct AnShape { int es, nplanes, rows; long long row_bytes; const char *name; };

// the five fields of a descriptor in the block's order, with their shapes
void an_shapes(const AnLayout &L, AnShape s[5])
{
    s[0] = {2, 2, L.h8, (long long)L.w8 * 4, "analysis mv"};
    s[1] = {1, 2, L.h8, (long long)L.w8, "analysis ref"};
    s[2] = {1, 5, L.h8, (long long)L.w8, "analysis cu"};
    s[3] = {4, 3, L.h8, (long long)L.w8 * 4, "analysis sse"};
    s[4] = {1, 1, L.cr, (long long)L.cc, "analysis qp"};
}

int check_analysis(ks265_ctx *c, const ks265_analysis_desc *d, AnLayout *out)
{
    if (d->width <= 0 || d->height <= 0 || (d->width & 7) || (d->height & 7) || d->width > 16384 || d->height > 16384) {
        c->last_error = "analysis: width and height multiples of 8, at most 16384"; return KS265_NOTSUPPORTED;
    }
    const AnLayout L = an_layout(d->width, d->height);
    AnShape s[5];
    an_shapes(L, s);
    const ks265_an_field *fl[5] = {&d->mv, &d->ref, &d->cu, &d->qp, &d->sse};
    const int shape_of[5] = {0, 1, 2, 4, 3};
    int wanted = 0;
    for (int i = 0; i < 5; ++i) {
        const ks265_an_field *f = fl[i];
        if (!f->data) continue;
        ++wanted;
        const AnShape &sh = s[shape_of[i]];
        if (f->pitch < sh.row_bytes) { c->last_error = std::string(sh.name) + ": pitch below the row's bytes"; return KS265_NOTSUPPORTED; }
        if (f->pitch % sh.es || (uintptr_t)f->data % (uintptr_t)sh.es) { c->last_error = std::string(sh.name) + ": pitch and address must be multiples of the element size"; return KS265_NOTSUPPORTED; }
        const long long plane_bytes = (long long)f->pitch * (sh.rows - 1) + sh.row_bytes;
        if (sh.nplanes > 1 && (f->plane < plane_bytes || f->plane % sh.es)) {
            c->last_error = std::string(sh.name) + ": plane step below a plane's bytes or no multiple of the element size"; return KS265_NOTSUPPORTED;
        }
    }
    if (!wanted) { c->last_error = "analysis: no field wanted"; return KS265_NOTSUPPORTED; }
    for (int i = 0; i < 5; ++i) {
        const ks265_an_field *f = fl[i];
        if (!f->data) continue;
        const AnShape &sh = s[shape_of[i]];
        const long long ext = (sh.nplanes > 1 ? (long long)f->plane * (sh.nplanes - 1) : 0) + (long long)f->pitch * (sh.rows - 1) + sh.row_bytes;
        const int r = ks265_check_extent(c, f->data, ext, 1, ext, sh.name);
        if (r) return r;
    }
    if (out) *out = L;
    return KS265_OK;
}

}  // namespace

extern "C" {

int ks265_analysis_layout(int width, int height, size_t off[6])
{
    if (!off) return KS265_POINTER;
    if (width <= 0 || height <= 0 || (width & 7) || (height & 7)) return KS265_NOTSUPPORTED;
    const AnLayout L = an_layout(width, height);
    for (int i = 0; i < 6; ++i) off[i] = L.off[i];
    return KS265_OK;
}

size_t ks265_analysis_bytes(ks265_frame *f) { return f ? an_layout(f->g.W, f->g.H).off[5] : 0; }

int ks265_analysis_pack_on(ks265_ctx *cx, ks265_frame *f, ks265_pic src, ks265_pic recon, const ks265_cu8 *dev_cu8, const int8_t *dev_qp_map, int picture_qp,
                           const int8_t delta[2][4], void *dev_block)
{
    KS_FRAME_CHECK(f);
    if (!cx || !dev_block || !delta || !src.y || !src.u || !src.v || !recon.y || !recon.u || !recon.v) return KS265_POINTER;
    if (((uintptr_t)dev_block & 255) || (((uintptr_t)src.y | (uintptr_t)src.u | (uintptr_t)src.v | (uintptr_t)recon.y | (uintptr_t)recon.u | (uintptr_t)recon.v | (uintptr_t)dev_cu8) & 3)) {
        cx->last_error = "analysis: block not 256-byte aligned, or a plane or the CU map not 4-byte aligned"; return KS265_NOTSUPPORTED;
    }
    if (picture_qp < -128 || picture_qp > 127) return KS265_NOTSUPPORTED;
    ks_use_device(cx);
    const KsGeom &g = f->g;
    const AnLayout L = an_layout(g.W, g.H);
    AnPackArgs a{};
    a.sy = src.y + g.org_y; a.su = src.u + g.org_c; a.sv = src.v + g.org_c;
    a.ry = recon.y + g.org_y; a.ru = recon.u + g.org_c; a.rv = recon.v + g.org_c;
    a.cu8 = (const unsigned *)(dev_cu8 ? dev_cu8 : f->cu8);
    a.qp_map = dev_qp_map; a.picture_qp = picture_qp;
    for (int l = 0; l < 2; ++l) {
        a.delta[l] = 0;
        for (int i = 0; i < 4; ++i) a.delta[l] |= (unsigned)(uint8_t)delta[l][i] << (8 * i);
    }
    a.stride_y = g.sy; a.stride_c = g.sc;
    a.w8 = L.w8; a.h8 = L.h8; a.P = L.P; a.ppr = (L.w8 + 1) / 2; a.nctu = L.cc * L.cr; a.cc = L.cc; a.Pq = L.Pq;
    a.wide_y = ((((uintptr_t)a.sy | (uintptr_t)a.ry) & 15) == 0 && g.sy % 16 == 0) ? 1 : 0;
    a.wide_c = ((((uintptr_t)a.su | (uintptr_t)a.sv | (uintptr_t)a.ru | (uintptr_t)a.rv) & 7) == 0 && g.sc % 8 == 0) ? 1 : 0;
    a.blk = (uint8_t *)dev_block; a.off_ref = L.off[1]; a.off_cu = L.off[2]; a.off_sse = L.off[3]; a.off_qp = L.off[4];
    const int lanes = a.ppr * a.h8 > a.nctu ? a.ppr * a.h8 : a.nctu;
    hipLaunchKernelGGL(analysis_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, cx->stream, a);
    return ks265_check_launch(cx);
}

int ks265_analysis_pack(ks265_frame *f, ks265_pic src, ks265_pic recon, const ks265_cu8 *dev_cu8, const int8_t *dev_qp_map, int picture_qp, const int8_t delta[2][4], void *dev_block)
{
    return f ? ks265_analysis_pack_on(f->ctx, f, src, recon, dev_cu8, dev_qp_map, picture_qp, delta, dev_block) : KS265_POINTER;
}

int ks265_analysis_validate(ks265_ctx *c, const ks265_analysis_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    ks_use_device(c);
    return check_analysis(c, d, nullptr);
}

int ks265_analysis_export(ks265_ctx *c, const void *dev_block, const ks265_analysis_desc *d)
{
    if (!c || !d || !dev_block) return KS265_POINTER;
    ks_use_device(c);
    AnLayout L;
    int r = check_analysis(c, d, &L);
    if (r) return r;
    if ((uintptr_t)dev_block & 255) { c->last_error = "analysis: block not 256-byte aligned"; return KS265_NOTSUPPORTED; }
    if ((r = ks265_check_extent(c, dev_block, (long long)L.off[5], 1, (long long)L.off[5], "analysis block"))) return r;
    AnShape s[5];
    an_shapes(L, s);
    const ks265_an_field *fl[5] = {&d->mv, &d->ref, &d->cu, &d->sse, &d->qp};      // the block's order
    AnExportArgs a{};
    unsigned total = 0;
    for (int i = 0; i < 5; ++i) {
        AnField &o = a.f[i];
        o.first = o.end = total;
        if (!fl[i]->data) continue;
        o.src = (const uint8_t *)dev_block + L.off[i];
        o.dst = (uint8_t *)fl[i]->data; o.pitch = fl[i]->pitch; o.plane = s[i].nplanes > 1 ? fl[i]->plane : 0;
        o.src_pitch = i == 4 ? L.Pq : L.P * (i == 0 || i == 3 ? 4 : 1);
        o.rows = s[i].rows; o.row_bytes = (int)s[i].row_bytes; o.rdw = (o.row_bytes + 3) / 4; o.es = s[i].es;
        o.al4 = (((uintptr_t)o.dst | (uintptr_t)o.pitch | (uintptr_t)o.plane) & 3) == 0 ? 1 : 0;
        total += (unsigned)(s[i].nplanes * o.rows * o.rdw);
        o.end = total;
    }
    hipLaunchKernelGGL(analysis_export_kernel, dim3((total + 255) / 256), dim3(256), 0, c->stream, a);
    return ks265_check_launch(c);
}

}  // extern "C"
