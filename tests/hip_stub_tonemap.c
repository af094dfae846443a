/* TEST INFRASTRUCTURE: the device library's CPU stand-in with everything hip_stub_overlay.c has (included as it is) plus the entries of tone mapping on the way in
 * (include/ks265_hip.h: ks265_tonemap_plan_create / _destroy, ks265_input_tonemap[_validate]), in plain C after tests/tonemap_ref.py with the tables and the arithmetic of
 * ../ks265codec_amd/host/ks265_tonemap.h.  "Device memory" is the process's own, so no extent can be judged: pointers are refused for NULL and a pitch below the row alone.
 * A plan counts as device memory alive (ks265_stub_live), its creation is a creating call; every ks265_input_tonemap call shows in the call log (arg: the format's code) and
 * a refused one does not.  The routine, stub_tonemap_to_i420, takes nothing but pointers and numbers: -DKS265_STUB_TONEMAP_ROUTINES_ONLY leaves it alone in the
 * translation unit, for a program of its own (tests/tonemap_main.c). */
#ifndef KS265_STUB_TONEMAP_ROUTINES_ONLY
#include "hip_stub_overlay.c"
#else
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "ks265_hip.h"
#endif
#include "../ks265codec_amd/host/ks265_tonemap.h"

/* a picture of the listed formats -> packed I420 (tests/tonemap_ref.py to_i420): reads the elements of the rows and nothing else.  0, or -1 without memory */
static int stub_tonemap_to_i420(const ks265_tm_tables *t, int layout, int depth, int msb, int full_range, const uint8_t *const plane[3], const long long pitch[3], int W, int H, uint8_t *dst)
{
    int32_t *q = (int32_t *)malloc((size_t)W * 6 * sizeof(int32_t));
    if (!q) return -1;
    ks265_tm_picture_host(t, layout, depth, msb, full_range, plane, pitch, W, H, dst, q);
    free(q);
    return 0;
}

#ifndef KS265_STUB_TONEMAP_ROUTINES_ONLY
struct ks265_tonemap_plan { int full_range; ks265_tm_tables t; };

int ks265_tonemap_plan_destroy(ks265_ctx *c, ks265_tonemap_plan *p)
{
    if (!c) return KS265_POINTER;
    if (!p) return KS265_OK;
    free(p); live(LIVE_DEV, -1);
    return KS265_OK;
}

int ks265_tonemap_plan_create(ks265_ctx *c, const ks265_tonemap_cfg *cfg, ks265_tonemap_plan **out)
{
    if (!c || !cfg || !out) return KS265_POINTER;
    *out = NULL;
    if (!ks265_tm_cfg_ok(cfg->transfer, cfg->curve, cfg->peak_nits, cfg->white_nits) || (cfg->full_range != 0 && cfg->full_range != 1)) return KS265_NOTSUPPORTED;
    if (creating_fails("tonemap_plan c%d curve %d peak %g white %g", ctx_ordinal(c), cfg->curve, cfg->peak_nits, cfg->white_nits)) return KS265_OUTOFMEMORY;
    ks265_tonemap_plan *p = (ks265_tonemap_plan *)calloc(1, sizeof *p);
    if (!p) return KS265_OUTOFMEMORY;
    live(LIVE_DEV, 1);
    p->full_range = cfg->full_range;
    ks265_tm_tables_fill(cfg->curve, cfg->peak_nits, cfg->white_nits, &p->t);
    *out = p;
    return KS265_OK;
}

/* the plan's tables, for the tests that hold them against the specification's: E, G, O (4097 entries) and M */
int ks265_stub_tonemap_tables(const ks265_tonemap_plan *p, uint32_t *E, uint16_t *G, uint16_t *O, int32_t *M)
{
    if (!p) return KS265_POINTER;
    memcpy(E, p->t.E, sizeof p->t.E); memcpy(G, p->t.G, sizeof p->t.G); memcpy(O, p->t.O, 4097 * sizeof(uint16_t)); memcpy(M, p->t.M, sizeof p->t.M);
    return KS265_OK;
}

static int stub_tm_check(const ks265_in_desc *d, int f[4])
{
    if (y_decode(d->format, &f[0], &f[1], &f[2], &f[3]) <= 0 || !ks265_tm_format_ok(f[0], f[1], f[2])) return KS265_NOTSUPPORTED;
    return stub_yuv_in_check(d, f[0], f[1], f[2]);
}

int ks265_input_tonemap_validate(ks265_ctx *c, const ks265_tonemap_plan *p, const ks265_in_desc *d)
{
    if (!c || !p || !d) return KS265_POINTER;
    int f[4];
    return stub_tm_check(d, f);
}

int ks265_input_tonemap(ks265_ctx *c, const ks265_tonemap_plan *p, const ks265_in_desc *d, uint8_t *dst)
{
    if (!c || !p || !d) return KS265_POINTER;
    int f[4];
    const int r = stub_tm_check(d, f);
    if (r) return r;
    if (!dst) return KS265_POINTER;
    if ((uintptr_t)dst & 15) return KS265_NOTSUPPORTED;
    if (call_log(__func__, c, NULL, NULL, d->format)) return KS265_FAIL;
    const uint8_t *pl[3] = {(const uint8_t *)d->plane[0], (const uint8_t *)d->plane[1], (const uint8_t *)d->plane[2]};
    const long long pitch[3] = {d->pitch[0], d->pitch[1], d->pitch[2]};
    return stub_tonemap_to_i420(&p->t, f[0], f[2], f[3], p->full_range, pl, pitch, d->width, d->height, dst) ? KS265_OUTOFMEMORY : KS265_OK;
}
#endif
