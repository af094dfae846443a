/* TEST INFRASTRUCTURE: the device library's CPU stand-in (hip_stub.c, included as it is) plus what `roi` (include/ks265_enc.h) asks of a device library: ks265_roi_validate,
 * ks265_roi_reduce and ks265_roi_ctu_map in plain C after tests/roi_map_ref.py, and the two entries that order a stream of the application against a context's (the stand-in
 * runs everything inside the call: they log and return).  "Device memory" is the process's own here, so a "device map" is any readable pointer.  The host tests of the switch
 * link this file instead of hip_stub.c. */
#include "hip_stub.c"
#include <math.h>
#include "../ks265codec_amd/host/ks265_roi.h"

int ks265_wait_external(ks265_ctx *c, void *s) { if (LOGC(c)) return KS265_FAIL; (void)s; return c ? KS265_OK : KS265_POINTER; }
int ks265_external_wait_event(ks265_ctx *c, void *s, void *ev) { if (LOGE(c, ev)) return KS265_FAIL; (void)s; return c && ev ? KS265_OK : KS265_POINTER; }

/* the stand-in knows no allocations: NULL is a KS265_POINTER, what the description itself shows wrong a KS265_NOTSUPPORTED, as on the device */
int ks265_roi_validate(ks265_ctx *c, const ks265_roi_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    const int es = ks265_roi_elem_size(d->type);
    if (!es || d->log2_block < 0 || d->log2_block > 6 || d->cols <= 0 || d->rows <= 0) return KS265_NOTSUPPORTED;
    if (d->pitch < d->cols * es || d->pitch % es) return KS265_NOTSUPPORTED;
    return d->data ? KS265_OK : KS265_POINTER;
}

int ks265_roi_reduce(ks265_ctx *c, const ks265_roi_desc *d, int width, int height, int32_t *rec)
{
    if (LOGC(c)) return KS265_FAIL;
    if (!rec) return KS265_POINTER;
    const int r = ks265_roi_validate(c, d);
    if (r) return r;
    if (d->cols != ks265_roi_map_cols(width, d->log2_block) || d->rows != ks265_roi_map_rows(height, d->log2_block)) return KS265_NOTSUPPORTED;
    return ks265_roi_reduce_host(d->type, d->log2_block, d->data, d->pitch, width, height, rec) ? KS265_NOTSUPPORTED : KS265_OK;
}

int ks265_roi_ctu_map(ks265_ctx *c, const int32_t *rec, const double *off, int nx, int ny, int bpc, int cols, int rows, int base, int lo, int hi, int8_t *map)
{
    call_log(__func__, c, NULL, NULL, base);
    if (!c || !map) return KS265_POINTER;
    for (int cy = 0; cy < rows; ++cy)
        for (int cx = 0; cx < cols; ++cx) {
            double sum = 0.0; int cnt = 0;
            if (off)
                for (int by = cy * bpc; by < (cy * bpc + bpc < ny ? cy * bpc + bpc : ny); ++by)
                    for (int bx = cx * bpc; bx < (cx * bpc + bpc < nx ? cx * bpc + bpc : nx); ++bx) { sum += off[by * nx + bx]; ++cnt; }
            const double mean = cnt ? sum / (double)cnt : 0.0;
            int d = rec ? (int)floor(mean + (double)rec[cy * cols + cx] / 256.0 + 0.5) : (int)floor(mean + 0.5);
            d = d < -12 ? -12 : d > 12 ? 12 : d;
            const int q = base + d;
            map[cy * cols + cx] = (int8_t)(q < lo ? lo : q > hi ? hi : q);
        }
    return KS265_OK;
}
