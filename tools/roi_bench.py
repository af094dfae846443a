"""ROI maps (`roi`, include/ks265_enc.h) at 3840x2160 through the API: what the switch costs, and that a map does what it says.

  (default)    -preset slow -rc 0 -qp 27 -iper 128 -psnr 1, the SDK's default GOP, host I420 input; one case per invocation of --runs runs (a job alternates invocations, so
               that another build of the library - `--lib DIR`, e.g. the parent commit's - is measured by the same script in the same job):
                 off   the switch off (runs on a library without the switch too)
                 on    the switch on, no map ever set: cu_qp_delta in the stream, one ks265_roi_ctu_map per picture
                 map   on, a per-pixel float32 device map (33.2 MB, constant 0.0) with every picture: + one ks265_roi_reduce per picture
               pictures per second, the stream's bytes and MD5, PSNR-Y.
  --rect DQP   Encoder(roi=True, recon="i420"), device I420 input, 64 pictures: a centre rectangle (half the width x half the height) at DQP against no map - bytes, and the
               luma SSE inside and outside the rectangle from the reconstructions the encoder hands out.

    python tools/roi_bench.py [--case off|on|map] [--lib DIR] [--pictures 256] [--runs 5] [--lanes 1] [--rect -6] [--size 3840x2160] [--out FILE]"""
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


class Nal(C.Structure):
    _fields_ = [("naltype", C.c_int), ("tid", C.c_int), ("iSize", C.c_int), ("pts", C.c_longlong), ("pPayload", C.POINTER(C.c_ubyte))]


class Roi(C.Structure):
    _fields_ = [("type", C.c_int), ("log2_block", C.c_int), ("device", C.c_int), ("data", C.c_void_p), ("pitch", C.c_int), ("stream", C.c_void_p)]


def load(lib_dir):
    if lib_dir is None:
        from ks265codec_amd import stream
        path = stream.build()
    else:
        path = os.path.join(lib_dir, "libks265enc.so")
    lib = C.CDLL(path)
    lib.QY265EncoderOpen.restype = C.c_void_p
    return lib


def run(lib, case, lanes, W, H, n, frames, fmap):
    os.environ["KS265_GOP_LANES"] = str(lanes)
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 27), ("iper", 128), ("psnr", 1), ("log", 3)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    if case != "off":
        assert lib.ks265_enc_set_default(b"roi", C.c_int(1)) == 0
    err = C.c_int(0)
    h = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err)))
    if case != "off":
        lib.ks265_enc_set_default(b"roi", C.c_int(0))
    assert h.value, hex(err.value & 0xFFFFFFFF)
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    md, nbytes = hashlib.md5(), 0
    roi = Roi()
    if case == "map":
        roi.type, roi.log2_block, roi.device, roi.data, roi.pitch = 1, 0, fmap.device.index or 0, fmap.data_ptr(), fmap.stride(0) * 4
        roi.stream = torch.cuda.current_stream().cuda_stream

    def take():
        nonlocal nbytes
        for i in range(nn.value):
            b = C.string_at(nal[i].pPayload, nal[i].iSize); md.update(b); nbytes += len(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(n):
        f = frames[t % len(frames)]
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(f.ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        if case == "map":
            assert lib.ks265_enc_set_next_roi(h, C.byref(roi)) == 0
        rc = lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0)
        assert rc == 0, hex(rc & 0xFFFFFFFF)
        take()
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
        take()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = Stats()
    lib.ks265_enc_get_stats(h, C.byref(st))
    lanes_got = lib.ks265_enc_lanes(h)
    lib.QY265EncoderClose(h)
    mse = st.sse[0] / max(1, st.frames) / (W * H)
    return {"pictures_per_s": n / dt, "bytes": nbytes, "md5": md.hexdigest(), "psnr_y": 10 * np.log10(255.0 ** 2 / mse) if mse > 0 else 99.0, "lanes": lanes_got}


def rect_case(W, H, n, dqp):
    """a centre rectangle at dqp against no map: bytes and the luma SSE inside / outside, from the encoder's own reconstructions"""
    from ks265codec_amd.encoder import Encoder
    from ks265codec_amd.synth import make_clip
    clip = make_clip(W, H, 16, seed=1234, abc=(37, 53, 19), pan=(5, 3))
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda().view(H * 3 // 2, W) for f in clip]
    x0, x1, y0, y1 = W // 4 // 64 * 64, W * 3 // 4 // 64 * 64, H // 4 // 64 * 64, H * 3 // 4 // 64 * 64          # on the CTU grid: what the map says is what every CTU inside gets
    m = np.zeros(((H + 15) // 16, (W + 15) // 16), np.int8)
    m[y0 // 16:y1 // 16, x0 // 16:x1 // 16] = dqp
    out = {}
    os.environ["KS265_GOP_LANES"] = "1"
    for name, roi in (("none", None), ("rect", m)):
        sse_in = sse_out = 0.0
        nbytes = 0

        def account(pics):
            nonlocal sse_in, sse_out
            for poc, t in pics:
                d = (t[:H].to(torch.int32) - dev[poc % len(dev)][:H].to(torch.int32)) ** 2
                inside = float(d[y0:y1, x0:x1].sum())
                sse_in += inside; sse_out += float(d.sum()) - inside
        with Encoder(W, H, "slow", rc=0, qp=27, iper=128, fr=50, psnr=1, roi=True, recon="i420") as enc:
            for t in range(n):
                nbytes += len(enc.encode(dev[t % len(dev)], "i420", roi=roi, roi_block=16))
                account(enc.recon())
            nbytes += len(enc.flush())
            account(enc.recon())
        n_in, n_out = (y1 - y0) * (x1 - x0) * n, (W * H - (y1 - y0) * (x1 - x0)) * n
        out[name] = {"bytes": nbytes, "sse_inside": sse_in, "sse_outside": sse_out,
                     "psnr_y_inside": 10 * np.log10(255.0 ** 2 * n_in / sse_in), "psnr_y_outside": 10 * np.log10(255.0 ** 2 * n_out / sse_out)}
    return (x0, y0, x1 - x0, y1 - y0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="off", choices=["off", "on", "map"])
    ap.add_argument("--lib", default=None, metavar="DIR", help="a directory with another build's libks265enc.so + libks265hip.so (default: this tree's)")
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=1)
    ap.add_argument("--rect", type=int, default=None, metavar="DQP")
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    if a.rect is not None:
        n = min(a.pictures, 64)
        (x, y, w, h), res = rect_case(W, H, n, a.rect)
        lines = [f"{W}x{H}, {n} pictures, -preset slow -rc 0 -qp 27 -iper 128, default GOP, one lane: the rectangle {x}:{y}:{w}:{h} at {a.rect:+d} against no map (the switch on in both)"]
        for name, r in res.items():
            lines.append(f"{name:5s} {r['bytes']:10d} bytes   luma SSE inside {r['sse_inside']:.4e} (PSNR-Y {r['psnr_y_inside']:.2f} dB)   outside {r['sse_outside']:.4e} (PSNR-Y {r['psnr_y_outside']:.2f} dB)")
        raw = res
    else:
        from ks265codec_amd.synth import make_clip
        lib = load(a.lib)
        frames = [np.ascontiguousarray(f) for f in make_clip(W, H, a.distinct, seed=1234, abc=(37, 53, 19), pan=(5, 3))]
        fmap = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        rs = [run(lib, a.case, a.lanes, W, H, a.pictures, frames, fmap) for _ in range(a.runs)]
        tag = a.tag or (("other build " if a.lib else "") + a.case)
        lines = [f"{tag:18s} lanes {rs[0]['lanes']}  {statistics.median(r['pictures_per_s'] for r in rs):7.1f} pictures/s (runs: {', '.join('%.1f' % r['pictures_per_s'] for r in rs)})   "
                 f"{rs[0]['bytes']} bytes  md5 {rs[0]['md5']}  PSNR-Y {rs[0]['psnr_y']:.3f} dB   one stream in all runs: {len({r['md5'] for r in rs}) == 1}"]
        raw = rs
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
