"""Device reconstruction (`devrecon`, include/ks265_enc.h) at 3840x2160: what the way back costs.

  --kernel N   ks265_output_convert alone, by HIP events around N back-to-back launches on one stream (after a warm-up of the same launches): microseconds per launch and the
               bytes it moves, for I420, NV12 and RGBA - beside ks265_input_convert of the same three formats, timed the same way in the same run.
  (default)    through the API: -preset slow -rc 0 -qp 27 -iper 128, the SDK's default GOP, host I420 input, for every lane count of --lanes three cases, alternated, median
               of --runs: the switch off, on with nothing fetched, on with every picture fetched as RGBA (into one tensor, torch's current stream).  Pictures per second, the
               scheduler's waiting time per picture (ring space and pool slots: ks265_enc_stats.submit_wait_ms), and whether the three streams are the same bytes.

    python tools/device_recon_bench.py [--kernel 200] [--pictures 256] [--runs 5] [--lanes 1,2] [--cases off,on,fetch] [--size 3840x2160] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")        # two lanes want more than four hardware queues (include/ks265_enc.h); set before the runtime starts
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Stats(C.Structure):
    _fields_ = [("frames", C.c_long), ("bytes", C.c_longlong), ("sse", C.c_double * 3), ("gpu_ms", C.c_double), ("host_write_ms", C.c_double),
                ("in_copy_ms", C.c_double), ("submit_ms", C.c_double), ("output_ms", C.c_double), ("lat_gpu_ms", C.c_double), ("lat_queue_ms", C.c_double),
                ("key_wall_ms", C.c_double), ("key_cpu_ms", C.c_double), ("keys", C.c_long), ("occ_samples", C.c_long), ("occ_ring", C.c_long),
                ("occ_gpu", C.c_long), ("occ_ready", C.c_long), ("submit_wait_ms", C.c_double)]


class YUV(C.Structure):
    _fields_ = [("iWidth", C.c_int), ("iHeight", C.c_int), ("pData", C.POINTER(C.c_ubyte) * 3), ("iStride", C.c_int * 3)]


class HostPicture(C.Structure):
    _fields_ = [("iSliceType", C.c_int), ("poc", C.c_int), ("pts", C.c_longlong), ("dts", C.c_longlong), ("yuv", C.POINTER(YUV))]


class InDesc(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


def kernel_times(W, H, reps):
    from ks265codec_amd.lib import load_library
    lib = load_library()
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    pic = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda")          # the caller's picture: RGBA, or its first bytes as I420 / NV12
    i420 = torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")  # the encoder's packed picture
    base = pic.data_ptr()
    descs = {}
    d = InDesc(); d.format, d.width, d.height = 0, W, H
    d.plane[0], d.plane[1], d.plane[2], d.pitch[0], d.pitch[1], d.pitch[2] = base, base + W * H, base + W * H * 5 // 4, W, W // 2, W // 2
    descs["i420"] = (d, 1.5)
    d = InDesc(); d.format, d.width, d.height = 1, W, H
    d.plane[0], d.plane[1], d.pitch[0], d.pitch[1] = base, base + W * H, W, W
    descs["nv12"] = (d, 1.5)
    d = InDesc(); d.format, d.width, d.height, d.pixel_step = 2, W, H, 4
    d.plane[0], d.plane[1], d.plane[2], d.pitch[0] = base, base + 1, base + 2, W * 4
    descs["rgba"] = (d, 4.0)
    torch.cuda.synchronize()
    rows = []
    for name, (d, bpp) in descs.items():
        res = {}
        for way, call in (("output", lambda: lib.ks265_output_convert(h, C.c_void_p(i420.data_ptr()), C.byref(d))),
                          ("input", lambda: lib.ks265_input_convert(h, C.byref(d), C.c_void_p(i420.data_ptr())))):
            for _ in range(10):
                assert call() == 0
            assert lib.ks265_synchronize(h) == 0
            ms = C.c_float(0)
            assert lib.ks265_timer_start(h) == 0
            for _ in range(reps):
                assert call() == 0
            assert lib.ks265_timer_stop_ms(h, C.byref(ms)) == 0
            res[way] = ms.value * 1000.0 / reps
        mb = W * H * (1.5 + bpp) / 1e6
        rows.append({"format": name, "MB_moved": mb, "output_us": res["output"], "input_us": res["input"], "output_GBps": mb / res["output"] * 1e3, "input_GBps": mb / res["input"] * 1e3})
    lib.ks265_destroy(h)
    return rows


def run(case, lanes, W, H, n, frames, rgba):
    from ks265codec_amd.encoder import Nal, Picture, describe, library
    lib = library()
    os.environ["KS265_GOP_LANES"] = str(lanes)
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 27), ("iper", 128), ("psnr", 0)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    if case != "off":                                   # ("off" also runs on a library that has no such switch: --cases off measures an older build with this script)
        assert lib.ks265_enc_set_default(b"devrecon", C.c_int(1)) == 0
    err = C.c_int(0)
    h = lib.QY265EncoderOpen(cfg, C.byref(err))
    lib.ks265_enc_set_default(b"devrecon", C.c_int(0))
    assert h, hex(err.value & 0xFFFFFFFF)
    nal, nn, pic, outp, yuv, info = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV(), Picture()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    md, fetched = hashlib.md5(), 0
    dst = describe(rgba, "rgba")

    def take():
        nonlocal fetched
        for i in range(nn.value):
            md.update(C.string_at(nal[i].pPayload, nal[i].iSize))
        if case == "fetch":
            while lib.ks265_enc_device_recon_pending(h) > 0:
                assert lib.ks265_enc_get_device_recon(h, C.byref(dst), C.addressof(info)) == 0
                fetched += 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(n):
        f = frames[t % len(frames)]
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(f.ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        rc = lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.addressof(pic), C.addressof(outp), 0)
        assert rc == 0, hex(rc & 0xFFFFFFFF)
        take()
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == 0
        take()
    torch.cuda.synchronize()                            # the last conversions are part of the work
    dt = time.perf_counter() - t0
    st = Stats()
    lib.ks265_enc_get_stats(C.c_void_p(h), C.byref(st))
    lanes_got = lib.ks265_enc_lanes(C.c_void_p(h))
    lib.QY265EncoderClose(h)
    assert case != "fetch" or fetched == n
    return {"pictures_per_s": n / dt, "submit_wait_ms_per_picture": st.submit_wait_ms / max(1, st.frames), "lanes": lanes_got, "md5": md.hexdigest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", type=int, default=0, metavar="N", help="time N launches of each conversion alone and exit")
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lanes", default="1,2")
    ap.add_argument("--cases", default="off,on,fetch", help="off: the switch off; on: on, nothing fetched; fetch: on, every picture fetched as RGBA")
    ap.add_argument("--distinct", type=int, default=16, help="distinct pictures, cycled (all pre-generated)")
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    lines, raw = [], {}
    if a.kernel:
        raw["kernel"] = kernel_times(W, H, a.kernel)
        lines.append(f"{W}x{H}, HIP events around {a.kernel} back-to-back launches: microseconds per launch, MB moved (read + written), GB/s")
        for r in raw["kernel"]:
            lines.append(f"{r['format']:5s} {r['MB_moved']:6.1f} MB   ks265_output_convert {r['output_us']:7.2f} us {r['output_GBps']:7.0f} GB/s   "
                         f"ks265_input_convert {r['input_us']:7.2f} us {r['input_GBps']:7.0f} GB/s")
    else:
        from ks265codec_amd.synth import make_clip
        frames = [np.ascontiguousarray(f) for f in make_clip(W, H, a.distinct, seed=1234, abc=(37, 53, 19), pan=(5, 3))]
        rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        lines.append(f"{W}x{H}, {a.pictures} pictures, -preset slow -rc 0 -qp 27 -iper 128, default GOP, host I420 input, GPU_MAX_HW_QUEUES={os.environ['GPU_MAX_HW_QUEUES']}, "
                     f"median of {a.runs} alternating runs")
        for lanes in (int(x) for x in a.lanes.split(",")):
            res = {c: [] for c in a.cases.split(",")}
            for _ in range(a.runs):
                for c in res:
                    res[c].append(run(c, lanes, W, H, a.pictures, frames, rgba))
            raw[f"lanes{lanes}"] = res
            for c, rs in res.items():
                lines.append(f"lanes {rs[0]['lanes']}  {c:5s}  {statistics.median(r['pictures_per_s'] for r in rs):7.1f} pictures/s (runs: {', '.join('%.1f' % r['pictures_per_s'] for r in rs)})   "
                             f"scheduler waits {statistics.median(r['submit_wait_ms_per_picture'] for r in rs):.3f} ms/picture   md5 {rs[0]['md5']}")
            lines.append(f"lanes {lanes}: one stream in all cases: {len({r['md5'] for rs in res.values() for r in rs}) == 1}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
