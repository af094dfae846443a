// ks265_internal.h — host-side context shared by the .hip translation units (not part of the C ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/ks265_hip.h"
#include "ks265_dev.h"

struct ks265_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_ext = nullptr;                 // ks265_wait_external: recorded on the application's stream, waited for by this one
    std::string last_error;
    // device-side error word: pinned, device-mapped host memory that kernels OR error bits into (KS_DEVERR_*); ks265_synchronize
    // reads and clears it after the stream has drained and turns a set bit into KS265_FAIL
    unsigned *err_host = nullptr, *err_dev = nullptr;
    bool capturing = false;                      // between ks265_capture_begin and ks265_capture_end on this context
    int wavefront_spin_limit = 1 << 22;          // ks265_debug_set(KS265_DBG_WAVEFRONT_SPINS): test hook for the timeout path
};
#define KS_DEVERR_WAVEFRONT_TIMEOUT 1u           // intra wavefront: the CTU row above did not make progress in time

// make the context's device the calling thread's current device (the runtime keeps it per thread; setting the device that is already current costs a
// thread-local compare inside the runtime - no caching here: several translation units and direct hipSetDevice calls would defeat it)
static inline void ks_use_device(const ks265_ctx *ctx) { (void)hipSetDevice(ctx->device); }
// record a HIP error (if any) from the launch just issued; kernels are asynchronous, so this only
// catches launch-configuration errors — execution errors surface at ks265_synchronize()
static inline int ks265_check_launch(ks265_ctx *ctx)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return KS265_OK;
    ctx->last_error = hipGetErrorString(e);
    return KS265_FAIL;
}
// [p, p + pitch (rows - 1) + row_bytes) lies inside one device allocation on the context's device, else KS265_POINTER and last_error (input_convert.hip)
int ks265_check_extent(ks265_ctx *c, const void *p, long long pitch, int rows, long long row_bytes, const char *what);
// bytes per sample of an RGB format of ks265_in_desc (KS265_IN_RGB 1; _F16 and _BF16 2; _F32 4); 0 for I420, NV12 and every unknown code
static inline int ks265_rgb_elem_size(int format)
{
    return format == KS265_IN_RGB ? 1 : format == KS265_IN_RGB_F16 || format == KS265_IN_RGB_BF16 ? 2 : format == KS265_IN_RGB_F32 ? 4 : 0;
}
// the YUV family KS265_IN_YUV(layout, sub, depth, msb) of ks265_in_desc: 0 for a code outside it, 1 for one of its valid codes (the fields then in f), -1 for any other code
// with a bit at or above 0x1000 (refused everywhere).  f->alias: the code is KS265_IN_I420 / KS265_IN_NV12 under its other name and goes the way of that format
struct ks265_yuv_fmt { int layout, sub, depth, msb, es, alias; };
static inline int ks265_yuv_decode(int format, ks265_yuv_fmt *f)
{
    if (!(format & ~0xFFF)) return 0;
    if ((format & ~0x3FF) != 0x1000) return -1;
    f->layout = format >> 8 & 3; f->sub = format >> 6 & 3; f->msb = format >> 5 & 1; f->depth = format & 31;
    if (f->depth < 8 || f->depth > 16 || f->sub > 2 || (f->depth == 8 && f->msb) || (f->layout >= 2 && f->sub != 1)) return -1;
    f->es = f->depth == 8 ? 1 : 2;
    f->alias = f->depth == 8 && f->sub == 0 && f->layout < 2;
    return 1;
}
// input_yuv.hip: the family's side of ks265_input_validate / ks265_input_convert (d->format a valid code that is no alias; the destination already judged)
int ks265_yuv_check_desc(ks265_ctx *c, const ks265_in_desc *d, const ks265_yuv_fmt &f);
int ks265_yuv_launch(ks265_ctx *c, const ks265_in_desc *d, const ks265_yuv_fmt &f, uint8_t *dst);
static inline int ks265_hip(ks265_ctx *ctx, hipError_t e)
{
    if (e == hipSuccess) return KS265_OK;
    if (ctx) ctx->last_error = hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? KS265_OUTOFMEMORY : KS265_FAIL;
}
