"""Host input against device input at 3840x2160: 256 pictures, -preset slow -rc 0 -qp 27 -iper 128, the SDK's default GOP on two GOP lanes (KS265_GOP_LANES=2).
Three variants, alternated, median of three runs each: host I420 (QY265EncoderEncodeFrame from numpy pictures), device I420 and device RGBA (ks265_enc_encode_device_frame
from tensors made on the GPU before the timed window).  Prints pictures/s and the calling thread's input milliseconds per picture (ks265_enc_get_stats in_copy_ms), and
checks that device I420 writes the host-input stream.

    python tools/device_input_rate.py [--pictures 256] [--runs 3] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

os.environ["KS265_GOP_LANES"] = "2"
os.environ["GPU_MAX_HW_QUEUES"] = "8"                 # two lanes want more than four hardware queues (include/ks265_enc.h); set before the runtime starts
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


def run(variant, W, H, n, host_frames, dev_frames):
    from ks265codec_amd.encoder import Nal, describe, library
    lib = library()
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 27), ("iper", 128), ("psnr", 0)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    err = C.c_int(0)
    h = lib.QY265EncoderOpen(cfg, C.byref(err))
    assert h, hex(err.value & 0xFFFFFFFF)
    if variant != "host_i420":
        assert lib.ks265_enc_enable_device_input(h) == 0
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    md, nbytes = hashlib.md5(), 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(n):
        if variant == "host_i420":
            f = host_frames[t % len(host_frames)]
            for k, off in enumerate((0, W * H, W * H * 5 // 4)):
                yuv.pData[k] = C.cast(f.ctypes.data + off, C.POINTER(C.c_ubyte))
            pic.pts = t
            rc = lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.addressof(pic), C.addressof(outp), 0)
        else:
            fmt = "i420" if variant == "device_i420" else "rgba"
            dp = describe(dev_frames[fmt][t % len(dev_frames[fmt])], fmt)
            dp.pts = t
            rc = lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(dp), C.addressof(outp))
        assert rc == 0, hex(rc & 0xFFFFFFFF)
        for i in range(nn.value):
            b = C.string_at(nal[i].pPayload, nal[i].iSize); md.update(b); nbytes += len(b)
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == 0
        for i in range(nn.value):
            b = C.string_at(nal[i].pPayload, nal[i].iSize); md.update(b); nbytes += len(b)
    dt = time.perf_counter() - t0
    st = Stats()
    lib.ks265_enc_get_stats(C.c_void_p(h), C.byref(st))
    lib.QY265EncoderClose(h)
    return {"pictures_per_s": n / dt, "in_ms_per_picture": st.in_copy_ms / max(1, st.frames), "frames": st.frames, "bytes": nbytes, "md5": md.hexdigest()}


def convert_only(W, H, reps):
    """the conversion kernel alone (nothing else on the device): `reps` conversions per source format into one destination, for a kernel trace"""
    from ks265codec_amd.encoder import IN_I420, IN_NV12, IN_RGB
    from ks265codec_amd.lib import load_library

    class InDesc(C.Structure):
        _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                    ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]
    lib = load_library()
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    src = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda")
    dst = torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda")
    base = src.data_ptr()
    descs = {}
    d = InDesc(); d.format, d.width, d.height, d.pixel_step = IN_RGB, W, H, 4
    d.plane[0], d.plane[1], d.plane[2], d.pitch[0] = base, base + 1, base + 2, W * 4
    descs["rgba"] = d
    d = InDesc(); d.format, d.width, d.height = IN_NV12, W, H
    d.plane[0], d.plane[1], d.pitch[0], d.pitch[1] = base, base + W * H, W, W
    descs["nv12"] = d
    d = InDesc(); d.format, d.width, d.height = IN_I420, W, H
    d.plane[0], d.plane[1], d.plane[2], d.pitch[0], d.pitch[1], d.pitch[2] = base, base + W * H, base + W * H * 5 // 4, W, W // 2, W // 2
    descs["i420"] = d
    torch.cuda.synchronize()
    for name, d in descs.items():
        for _ in range(reps):
            assert lib.ks265_input_convert(h, C.byref(d), C.c_void_p(dst.data_ptr())) == 0
        assert lib.ks265_synchronize(h) == 0
        print(f"{name}: {reps} conversions {W}x{H} (read {W * H * (4 if name == 'rgba' else 1.5) / 1e6:.1f} MB, write {W * H * 1.5 / 1e6:.1f} MB each)")
    lib.ks265_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--convert-only", type=int, default=0, metavar="N", help="run N conversions of each format alone (for rocprofv3 --kernel-trace --stats) and exit")
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16, help="distinct pictures, cycled (all pre-generated)")
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    if a.convert_only:
        convert_only(W, H, a.convert_only)
        return
    from ks265codec_amd.synth import make_clip
    clip = make_clip(W, H, a.distinct, seed=1234, abc=(37, 53, 19), pan=(5, 3))
    rgb = []
    for f in clip:                                     # RGB pictures whose reference conversion is the host variant's input
        y = f[:W * H].reshape(H, W).astype(np.int16)
        rgb.append((np.clip(y + 10, 0, 255).astype(np.uint8), (255 - y).astype(np.uint8), np.clip(y // 2 + 40, 0, 255).astype(np.uint8)))
    host_frames = [np.ascontiguousarray(f) for f in clip]
    dev = {"i420": [torch.from_numpy(f).cuda().view(H * 3 // 2, W) for f in clip],
           "rgba": [torch.from_numpy(np.stack([*c, np.full_like(c[0], 255)], axis=2)).cuda() for c in rgb]}
    torch.cuda.synchronize()
    res = {v: [] for v in ("host_i420", "device_i420", "device_rgba")}
    for _ in range(a.runs):
        for v in res:
            res[v].append(run(v, W, H, a.pictures, host_frames, dev))
    lines = []
    for v, rs in res.items():
        med = statistics.median(r["pictures_per_s"] for r in rs)
        inp = statistics.median(r["in_ms_per_picture"] for r in rs)
        runs = ", ".join("%.1f" % r["pictures_per_s"] for r in rs)
        lines.append(f"{v:12s}  {med:7.1f} pictures/s (runs: {runs})   calling thread input {inp:.3f} ms/picture   "
                     f"{rs[0]['bytes']} bytes  md5 {rs[0]['md5']}")
    same = res["host_i420"][0]["md5"] == res["device_i420"][0]["md5"]
    lines.append(f"device I420 stream == host I420 stream: {same}")
    lines.append("(device RGBA codes different pixels - the RGB pictures above - so its stream is its own)")
    hdr = f"{W}x{H}, {a.pictures} pictures, -preset slow -rc 0 -qp 27 -iper 128, default GOP, KS265_GOP_LANES=2, GPU_MAX_HW_QUEUES=8, median of {a.runs} alternating runs"
    text = "\n".join([hdr] + lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
