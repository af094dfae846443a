"""Analysis out (`analysis`, include/ks265_enc.h) at 3840x2160: what the pack, the export and the switch cost.

  --kernel N   ks265_analysis_pack, ks265_ssim_picture on the same two pictures (the yardstick: the fused SSIM + SSE pass reads the same bytes and does more arithmetic) and
               ks265_analysis_export with all five fields, each by HIP events around N back-to-back launches on one stream after a warm-up of the same launches: microseconds
               per launch, the bytes it moves (computed from the shapes) and bytes per second.
  (default)    through the API: -preset slow -rc 0 -qp 27 -iper 128, the SDK's default GOP, host I420 input, for every lane count of --lanes the cases of --cases, alternated,
               median of --runs: `parent` (the encoder library of --parent-lib, e.g. a build of the commit before the switch existed; skipped without it), `off` (this
               library, the switch off), `on` (on, nothing fetched), `fetch` (on, every picture's five fields fetched into one set of tensors on torch's current stream).
               Pictures per second with the runs' spread, the scheduler's waiting time per picture, the pool's log line, and whether all streams are the same bytes.

    python tools/analysis_bench.py [--kernel 200] [--pictures 256] [--runs 5] [--lanes 1,2] [--cases parent,off,on,fetch] [--parent-lib FILE] [--size 3840x2160] [--out FILE]"""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from device_recon_bench import HostPicture, Stats, YUV  # noqa: E402  (tools/ is the script's directory)


def kernel_times(W, H, reps):
    from ks265codec_amd.lib import KsContext, KsFrame, analysis_shapes
    from ks265codec_amd.synth import lambda_q4
    ks = KsContext(0)
    f = KsFrame(ks, W, H, 27, lambda_q4(27))
    rng = np.random.default_rng(1)
    a, b = f.new_pic(), f.new_pic()
    for p in (a, b):
        f.load_i420(ks.dev(rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)), p)
    n8, nctu = (W // 8) * (H // 8), ((W + 63) // 64) * ((H + 63) // 64)
    rec = rng.integers(0, 256, 12 * n8, dtype=np.uint8)
    rec[10::12] = 0                                      # pred_mode 0: every block inter, both vectors and both references are resolved
    cu8 = ks.dev(rec)
    qmap = torch.randint(20, 40, (nctu,), dtype=torch.int8, device=ks.device)
    blk = torch.empty(f.analysis_bytes(), dtype=torch.uint8, device=ks.device)
    out = {n: torch.empty(shape, dtype=getattr(torch, dt), device=ks.device) for n, (dt, shape) in analysis_shapes(W, H).items()}
    desc = ks.analysis_desc(W, H, **out)
    sse, ssim = ks.zeros(24), ks.zeros(24)
    out_bytes = sum(t.numel() * t.element_size() for t in out.values())
    pics = 2 * (W * H * 3 // 2)
    cases = [("ks265_analysis_pack", lambda: f.analysis_pack(a, b, 27, ((-1, -2, -3, -4), (1, 2, 3, 4)), qp_map=qmap, cu8=cu8, block=blk), pics + 12 * n8 + nctu + out_bytes),
             ("ks265_ssim_picture", lambda: ks._chk(ks.lib.ks265_ssim_picture(f.h, a.c(), b.c(), C.c_void_p(sse.data_ptr()), C.c_void_p(ssim.data_ptr()))), pics),
             ("ks265_analysis_export", lambda: ks.analysis_export(blk, desc), 2 * out_bytes)]
    rows = []
    for name, call, nbytes in cases:
        for _ in range(20):
            call()
        ks.sync()
        ms = C.c_float(0)
        ks._chk(ks.lib.ks265_timer_start(ks.h))
        for _ in range(reps):
            call()
        ks._chk(ks.lib.ks265_timer_stop_ms(ks.h, C.byref(ms)))
        us = ms.value * 1000.0 / reps
        rows.append({"entry": name, "us": us, "MB_moved": nbytes / 1e6, "GBps": nbytes / us / 1e3})
    f.close(); ks.close()
    return rows, f"packed block {blk.numel()} bytes, the five fields {out_bytes} bytes"


class AnField(C.Structure):
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_int), ("plane", C.c_longlong)]


class DevAnalysis(C.Structure):
    _fields_ = [("device", C.c_int), ("stream", C.c_void_p), ("mv", AnField), ("ref", AnField), ("cu", AnField), ("qp", AnField), ("sse", AnField)]


_libs = {}


def host_library(path):
    from ks265codec_amd.encoder import Nal
    if path not in _libs:
        lib = C.CDLL(path)
        lib.QY265EncoderOpen.restype = C.c_void_p
        lib.QY265EncoderOpen.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        for n in ("QY265EncoderClose", "QY265EncoderDelayedFrames", "ks265_enc_lanes"):
            getattr(lib, n).argtypes = [C.c_void_p]
        lib.QY265EncoderEncodeFrame.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Nal)), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int]
        lib.ks265_enc_get_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(lib, "ks265_enc_get_device_analysis"):
            lib.ks265_enc_device_analysis_pending.argtypes = [C.c_void_p]
            lib.ks265_enc_get_device_analysis.argtypes = [C.c_void_p, C.POINTER(DevAnalysis), C.c_void_p]
        _libs[path] = lib
    return _libs[path]


LOG_CB = C.CFUNCTYPE(None, C.c_char_p)


def run(case, lib, lanes, W, H, n, frames, dst):
    from ks265codec_amd.encoder import Nal, Picture
    os.environ["KS265_GOP_LANES"] = str(lanes)
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 27), ("iper", 128), ("psnr", 0), ("log", 1)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    if case in ("on", "fetch"):
        assert lib.ks265_enc_set_default(b"analysis", C.c_int(1)) == 0
    log = []
    cb = LOG_CB(lambda m: log.append(m.decode()))
    lib.QY265SetLogPrintf(cb)
    err = C.c_int(0)
    h = lib.QY265EncoderOpen(cfg, C.byref(err))
    if case in ("on", "fetch"):
        lib.ks265_enc_set_default(b"analysis", C.c_int(0))
    assert h, hex(err.value & 0xFFFFFFFF)
    nal, nn, pic, outp, yuv, info = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV(), Picture()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    md, fetched = hashlib.md5(), 0

    def take():
        nonlocal fetched
        for i in range(nn.value):
            md.update(C.string_at(nal[i].pPayload, nal[i].iSize))
        if case == "fetch":
            while lib.ks265_enc_device_analysis_pending(h) > 0:
                assert lib.ks265_enc_get_device_analysis(h, C.byref(dst), C.addressof(info)) == 0
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
    torch.cuda.synchronize()                            # the last exports are part of the work
    dt = time.perf_counter() - t0
    st = Stats()
    lib.ks265_enc_get_stats(C.c_void_p(h), C.byref(st))
    lanes_got = lib.ks265_enc_lanes(C.c_void_p(h))
    lib.QY265EncoderClose(h)
    lib.QY265SetLogPrintf(None)
    assert case != "fetch" or fetched == n
    pool = [ln.strip() for ln in "".join(log).splitlines() if "analysis: a pool of" in ln]
    return {"pictures_per_s": n / dt, "submit_wait_ms_per_picture": st.submit_wait_ms / max(1, st.frames), "lanes": lanes_got, "md5": md.hexdigest(), "pool": pool[0] if pool else ""}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", type=int, default=0, metavar="N", help="time N launches of the pack, the SSIM + SSE pass and the export alone and exit")
    ap.add_argument("--pictures", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lanes", default="1,2")
    ap.add_argument("--cases", default="parent,off,on,fetch")
    ap.add_argument("--parent-lib", default=None, help="an encoder library (libks265enc.so) of another build, for the `parent` case")
    ap.add_argument("--distinct", type=int, default=16, help="distinct pictures, cycled (all pre-generated)")
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    lines, raw = [], {}
    if a.kernel:
        raw["kernel"], note = kernel_times(W, H, a.kernel)
        lines.append(f"{W}x{H}, HIP events around {a.kernel} back-to-back launches: microseconds per launch, MB moved (read + written), GB/s; {note}")
        for r in raw["kernel"]:
            lines.append(f"{r['entry']:24s} {r['us']:8.2f} us  {r['MB_moved']:6.1f} MB  {r['GBps']:7.0f} GB/s")
    else:
        from ks265codec_amd import stream
        from ks265codec_amd.lib import analysis_shapes
        from ks265codec_amd.synth import make_clip
        frames = [np.ascontiguousarray(f) for f in make_clip(W, H, a.distinct, seed=1234, abc=(37, 53, 19), pan=(5, 3))]
        out = {n: torch.empty(shape, dtype=getattr(torch, dt), device="cuda") for n, (dt, shape) in analysis_shapes(W, H).items()}
        dst = DevAnalysis()
        dst.device, dst.stream = torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream
        for n, t in out.items():
            es = t.element_size()
            setattr(dst, n, AnField(t.data_ptr(), t.stride(0) * es, 0) if n == "qp" else AnField(t.data_ptr(), t.stride(1) * es, t.stride(0) * es))
        here = host_library(stream.build())
        cases = [c for c in a.cases.split(",") if c != "parent" or a.parent_lib]
        libs = {c: host_library(a.parent_lib) if c == "parent" else here for c in cases}
        lines.append(f"{W}x{H}, {a.pictures} pictures, -preset slow -rc 0 -qp 27 -iper 128, default GOP, host I420 input, GPU_MAX_HW_QUEUES={os.environ['GPU_MAX_HW_QUEUES']}, "
                     f"median of {a.runs} alternating runs")
        for lanes in (int(x) for x in a.lanes.split(",")):
            res = {c: [] for c in cases}
            for _ in range(a.runs):
                for c in res:
                    res[c].append(run(c, libs[c], lanes, W, H, a.pictures, frames, dst))
            raw[f"lanes{lanes}"] = res
            for c, rs in res.items():
                pps = [r["pictures_per_s"] for r in rs]
                lines.append(f"lanes {rs[0]['lanes']}  {c:6s}  {statistics.median(pps):7.1f} pictures/s (runs: {', '.join('%.1f' % p for p in pps)}; spread {max(pps) - min(pps):.1f})   "
                             f"scheduler waits {statistics.median(r['submit_wait_ms_per_picture'] for r in rs):.3f} ms/picture   md5 {rs[0]['md5']}")
            pool = next((r["pool"] for rs in res.values() for r in rs if r["pool"]), "")
            if pool:
                lines.append(f"lanes {lanes}: {pool}")
            lines.append(f"lanes {lanes}: one stream in all cases: {len({r['md5'] for rs in res.values() for r in rs}) == 1}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
