/* TEST INFRASTRUCTURE: the device library's CPU stand-in with the way back (hip_stub_recon.c, included as it is) plus what `analysis` (include/ks265_enc.h) asks of a device
 * library: ks265_analysis_bytes / _pack / _pack_on / _validate / _export as plain C.  The stand-in analyses nothing: the pack records what the HOST handed it - the picture's QP,
 * whether a QP map came with it (and its first entry), the two lists' POC deltas, the first eight luma samples of the source picture (a stamp that tells pictures apart) - and
 * the export lays those out in the caller's arrays, so that the host's bookkeeping (which block belongs to which picture, what was passed for it, which slot was read when) is
 * what the tests of tests/test_analysis_host_cpu.py look at.  The kernels are held to tests/analysis_ref.py on the GPU. */
#include "hip_stub_recon.c"

#define STUB_AN_MAGIC 0x414E4C59
typedef struct { int32_t magic, width, height, picture_qp, has_map, map0; int8_t delta[2][4]; uint8_t stamp[8]; } StubAnalysis;

size_t ks265_analysis_bytes(ks265_frame *f) { return f ? 256 : 0; }

int ks265_analysis_pack_on(ks265_ctx *c, ks265_frame *f, ks265_pic src, ks265_pic recon, const ks265_cu8 *cu8, const int8_t *qp_map, int picture_qp, const int8_t delta[2][4], void *blk)
{
    LOGF(c, f, picture_qp);
    (void)cu8;
    if (!c || !f || !blk || !delta || !src.y || !recon.y) return KS265_POINTER;
    StubAnalysis a;
    memset(&a, 0, sizeof a);
    a.magic = STUB_AN_MAGIC; a.width = f->cfg.width; a.height = f->cfg.height; a.picture_qp = picture_qp; a.has_map = qp_map != NULL; a.map0 = qp_map ? qp_map[0] : 0;
    memcpy(a.delta, delta, 8);
    memcpy(a.stamp, luma0(f, src), 8);
    memset(blk, 0, 256);
    memcpy(blk, &a, sizeof a);
    return KS265_OK;
}
int ks265_analysis_pack(ks265_frame *f, ks265_pic src, ks265_pic recon, const ks265_cu8 *cu8, const int8_t *qp_map, int picture_qp, const int8_t delta[2][4], void *blk)
{
    return f ? ks265_analysis_pack_on(f->ctx, f, src, recon, cu8, qp_map, picture_qp, delta, blk) : KS265_POINTER;
}

/* the stand-in knows no allocations: what it can judge is the pitch, the alignment and whether anything is wanted */
int ks265_analysis_validate(ks265_ctx *c, const ks265_analysis_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    if (d->width <= 0 || d->height <= 0 || (d->width & 7) || (d->height & 7)) return KS265_NOTSUPPORTED;
    const int w8 = d->width / 8, cc = (d->width + 63) / 64;
    const ks265_an_field *f[5] = {&d->mv, &d->ref, &d->cu, &d->qp, &d->sse};
    const int es[5] = {2, 1, 1, 1, 4}, row[5] = {w8 * 4, w8, w8, cc, w8 * 4};
    int wanted = 0;
    for (int i = 0; i < 5; ++i) {
        if (!f[i]->data) continue;
        ++wanted;
        if (f[i]->pitch < row[i] || f[i]->pitch % es[i] || (uintptr_t)f[i]->data % (uintptr_t)es[i]) return KS265_NOTSUPPORTED;
    }
    return wanted ? KS265_OK : KS265_NOTSUPPORTED;
}

/* qp: the picture's QP everywhere (entry [0][0]: the map's first entry if a map came); ref[L][0][0..3]: list L's deltas; mv[0][0][0..1]: the stamp's first eight bytes as four
 * int16; sse[0][0][0]: the magic, [0][0][1]: has_map; everything else zero */
int ks265_analysis_export(ks265_ctx *c, const void *blk, const ks265_analysis_desc *d)
{
    LOGC(c);
    const int r = blk ? ks265_analysis_validate(c, d) : KS265_POINTER;
    if (r) return r;
    StubAnalysis a;
    memcpy(&a, blk, sizeof a);
    if (a.magic != STUB_AN_MAGIC || a.width != d->width || a.height != d->height) return KS265_FAIL;     /* a block nothing was packed into */
    const int w8 = d->width / 8, h8 = d->height / 8, cc = (d->width + 63) / 64, cr = (d->height + 63) / 64;
    const ks265_an_field *f[5] = {&d->mv, &d->ref, &d->cu, &d->qp, &d->sse};
    const int np[5] = {2, 2, 5, 1, 3}, rows[5] = {h8, h8, h8, cr, h8}, row[5] = {w8 * 4, w8, w8, cc, w8 * 4};
    for (int i = 0; i < 5; ++i)
        for (int p = 0; f[i]->data && p < np[i]; ++p)
            for (int y = 0; y < rows[i]; ++y) memset((uint8_t *)f[i]->data + (size_t)p * (size_t)f[i]->plane + (size_t)y * (size_t)f[i]->pitch, i == 3 ? a.picture_qp : 0, (size_t)row[i]);
    if (d->qp.data && a.has_map) *(int8_t *)d->qp.data = (int8_t)a.map0;
    if (d->ref.data) for (int l = 0; l < 2; ++l) memcpy((uint8_t *)d->ref.data + (size_t)l * (size_t)d->ref.plane, a.delta[l], (size_t)(w8 < 4 ? w8 : 4));
    if (d->mv.data) memcpy(d->mv.data, a.stamp, (size_t)(w8 * 4 < 8 ? w8 * 4 : 8));
    if (d->sse.data) { int32_t v[2] = {a.magic, a.has_map}; memcpy(d->sse.data, v, (size_t)(w8 < 2 ? 4 : 8)); }
    return KS265_OK;
}
