/* TEST INFRASTRUCTURE: the device library's CPU stand-in (hip_stub.c, included as it is) plus what `devrecon` (include/ks265_enc.h) asks of a device library: the way back -
 * ks265_output_validate / ks265_output_convert, as plain-C copies for KS265_IN_I420 and KS265_IN_NV12 (the host's bookkeeping is what the tests of this file look at; the
 * conversion itself is held to tests/yuv_output_ref.py on the GPU) - and ks265_set_stream, by which a context adopts a stream of the application (the stand-in runs everything
 * inside the call: it logs and returns).  The host tests of the switch link this file instead of hip_stub.c. */
#include "hip_stub.c"

int ks265_set_stream(ks265_ctx *c, void *hip_stream) { LOGC(c); (void)hip_stream; return c ? KS265_OK : KS265_POINTER; }

/* the stand-in knows no allocations: a plane that is NULL or whose pitch is below its row is a KS265_POINTER, as on the device */
int ks265_output_validate(ks265_ctx *c, const ks265_in_desc *d)
{
    if (!c || !d) return KS265_POINTER;
    if (d->width <= 0 || d->height <= 0 || (d->width & 1) || (d->height & 1)) return KS265_NOTSUPPORTED;
    if (d->format != KS265_IN_I420 && d->format != KS265_IN_NV12) return KS265_NOTSUPPORTED;
    const int nplanes = d->format == KS265_IN_I420 ? 3 : 2;
    for (int k = 0; k < nplanes; ++k) {
        const int row = k == 0 || d->format == KS265_IN_NV12 ? d->width : d->width / 2;
        if (!d->plane[k] || d->pitch[k] < row) return KS265_POINTER;
    }
    return KS265_OK;
}

int ks265_output_convert(ks265_ctx *c, const uint8_t *src, const ks265_in_desc *d)
{
    LOGC(c);
    const int r = src ? ks265_output_validate(c, d) : KS265_POINTER;
    if (r) return r;
    const int W = d->width, H = d->height;
    const uint8_t *u = src + (size_t)W * H, *v = u + (size_t)W * H / 4;
    for (int y = 0; y < H; ++y) memcpy((uint8_t *)d->plane[0] + (size_t)y * d->pitch[0], src + (size_t)y * W, (size_t)W);
    for (int y = 0; y < H / 2; ++y) {
        if (d->format == KS265_IN_I420) {
            memcpy((uint8_t *)d->plane[1] + (size_t)y * d->pitch[1], u + (size_t)y * (W / 2), (size_t)W / 2);
            memcpy((uint8_t *)d->plane[2] + (size_t)y * d->pitch[2], v + (size_t)y * (W / 2), (size_t)W / 2);
        } else {
            uint8_t *uv = (uint8_t *)d->plane[1] + (size_t)y * d->pitch[1];
            for (int x = 0; x < W / 2; ++x) { uv[2 * x] = u[(size_t)y * (W / 2) + x]; uv[2 * x + 1] = v[(size_t)y * (W / 2) + x]; }
        }
    }
    return KS265_OK;
}
