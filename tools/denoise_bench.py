"""The temporal denoiser on the way in (include/ks265_hip.h ks265_input_denoise; ks265codec_amd/csrc/input_denoise.hip): what the kernel costs, what a handle
with `denoise` on costs beside the same handle with it off, and what the levels do to the bytes of a noisy clip.  Nothing here is a pass mark.

Kernel: as tools/window_bench.py measures - everything on ONE stream (torch's current one, which the context adopts), events around --reps warm launches that queue up behind a
few milliseconds of other work and so run back to back, --rounds times; the figure is the median round's microseconds per launch, at 1920x1080 and 3840x2160.  Every launch
filters the next picture of a ring (--ring-mb in all) against the next history of a second ring into one of eight history-out pictures.  Reported against the 6 W H bytes the
filter has to move (picture in and out, history in and out: 1.5 W H each) and the 289 W H absolute differences of the exhaustive luma search; a device-to-device copy of the
same 6 W H bytes (two copies of 1.5 W H) in the same run is the yardstick for the traffic.

Encoder: a 1920x1080 handle fed --pictures host pictures through the C API, -rc 0 -qp 27, default GOP, `denoise` 0 against 2 on the same clip: wall time from the first picture
to the end of the flush, median of --runs, alternating.  Bytes: the same clip with Gaussian noise of sigma 3 added, levels 0 .. 3.

    python tools/denoise_bench.py [--reps 32] [--rounds 7] [--ring-mb 300] [--pictures 64] [--runs 5] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ks265codec_amd import lib as kl  # noqa: E402

SIZES = [(1920, 1080), (3840, 2160)]


def kernels(W, H, reps, rounds, ring_mb, thr=10, weight=20):
    ks = kl.KsContext(0)                                                # torch's current stream
    n = W * H * 3 // 2
    nring = max(2, -(-ring_mb * 1000000 // (2 * n)))
    base = torch.randint(0, 256, (H + 16, W + 16), dtype=torch.uint8, device="cuda").float()
    base = torch.nn.functional.avg_pool2d(base[None, None], 3, 1, 1)[0, 0]                           # a smooth-ish field: blocks that find their vector

    def shot(ox, oy):
        y = base[8 + oy:8 + oy + H, 8 + ox:8 + ox + W]
        u = y[0::2, 0::2] / 2 + 60
        return torch.cat([(q + 2 * torch.randn_like(q)).clamp(0, 255).round().to(torch.uint8).reshape(-1) for q in (y, u, 250 - u)])

    cur = [shot(3 * (k % 3), k % 2) for k in range(nring)]
    hist = [shot(0, 0) for _ in range(nring)]
    out = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(8)]
    blocks = torch.empty(2 * ((W + 15) // 16) * ((H + 15) // 16), dtype=torch.int32, device="cuda")
    ks.input_denoise(thr, weight, W, H, cur[1].clone(), hist[1], out[0], blocks)                      # (picture 1 of the ring: panned by (3, 1))
    ks.sync()
    word = blocks.view(-1, 2)[:, 0]
    moved = float(((word & 0xFFFF) != (8 | 8 << 8)).float().mean()), float((word >> 16 & 1).float().mean())
    turn = [0]

    def filt():
        ks.input_denoise(thr, weight, W, H, cur[turn[0] % nring], hist[turn[0] % nring], out[turn[0] % 8])

    def copy():
        for k in range(2):
            rc = ks.lib.ks265_memcpy_d2d_async(ks.h, C.c_void_p(out[(turn[0] + k) % 8].data_ptr()), C.c_void_p(hist[turn[0] % nring].data_ptr()), C.c_size_t(n))
            assert rc == 0

    busy, busy_out = torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda")
    rows = []
    for name, fn in (("copy 2 x 1.5 W H", copy), ("denoise", filt), ("copy (again)", copy)):
        for _ in range(nring + 5):                                      # warm: the code object, every buffer touched once
            fn(); turn[0] += 1
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):                                          # a few milliseconds of other work in front: the launches queue up behind it and run back to back
                torch.mm(busy, busy, out=busy_out)
            e0.record()
            for _ in range(reps):
                fn(); turn[0] += 1
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / reps)
        m = statistics.median(us)
        rows.append({"size": f"{W}x{H}", "what": name, "us": m, "us_min": min(us), "us_max": max(us), "MB": 6 * W * H / 1e6, "GBps": 6 * W * H / m / 1e3,
                     "Gabsdiff_per_s": 289 * W * H / m / 1e3 if fn is filt else None, "blocks_moved": moved[0], "blocks_gated": moved[1]})
    ks.close()
    return rows


class YUV(C.Structure):
    _fields_ = [("iWidth", C.c_int), ("iHeight", C.c_int), ("pData", C.POINTER(C.c_ubyte) * 3), ("iStride", C.c_int * 3)]


class HostPicture(C.Structure):
    _fields_ = [("iSliceType", C.c_int), ("poc", C.c_int), ("pts", C.c_longlong), ("dts", C.c_longlong), ("yuv", C.POINTER(YUV))]


def session(W, H, pictures, denoise):
    """(seconds from the first picture to the end of the flush, bytes of the stream) of one handle fed host pictures"""
    from ks265codec_amd.encoder import Nal, library
    lib = library()
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("threads", 16), ("rc", 0), ("qp", 27), ("iper", 128), ("log", 0), ("denoise", denoise)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0, k
    err = C.c_int(0)
    h = lib.QY265EncoderOpen(cfg, C.byref(err))
    assert h, hex(err.value & 0xFFFFFFFF)
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    size = 0
    t0 = time.perf_counter()
    for t, p in enumerate(pictures):
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(p.ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.addressof(pic), C.addressof(outp), 0) == 0
        size += sum(nal[i].iSize for i in range(nn.value) if nal[i].iSize > 0)
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == 0
        size += sum(nal[i].iSize for i in range(nn.value) if nal[i].iSize > 0)
    dt = time.perf_counter() - t0
    lib.QY265EncoderClose(h)
    return dt, size


def clips(W, H, n):
    """(a moving clip with a little noise, the same with Gaussian noise of sigma 3 added)"""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    src, noisy = [], []
    for t in range(n):
        pl = [128 + 80 * np.sin(0.05 * (xx + 3 * t)) * np.cos(0.04 * (yy + 2 * t)), 128 + 60 * np.sin(0.02 * (xx[::2, ::2] + 2 * t)), 128 + 60 * np.cos(0.03 * (yy[::2, ::2] - t))]
        src.append(np.concatenate([np.clip(q + rng.integers(0, 6, q.shape), 0, 255).astype(np.uint8).ravel() for q in pl]))
        noisy.append(np.concatenate([np.clip(np.rint(q + rng.normal(0, 3, q.shape)), 0, 255).astype(np.uint8).ravel() for q in pl]))
    return src, noisy


def encoder(n, runs):
    W, H = 1920, 1080
    src, noisy = clips(W, H, n)
    session(W, H, src[:16], 2)                                          # warm: code objects, the allocator
    off, on = [], []
    for _ in range(runs):
        off.append(session(W, H, src, 0)[0])
        on.append(session(W, H, src, 2)[0])
    mo, mn = statistics.median(off), statistics.median(on)
    sizes = [session(W, H, noisy, lvl)[1] for lvl in range(4)]
    return {"pictures": n, "size": f"{W}x{H}", "off_pps": n / mo, "on_pps": n / mn, "off_s": off, "on_s": on, "us_per_picture_more": (mn - mo) / n * 1e6,
            "noisy_bytes_per_level": sizes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring-mb", type=int, default=300)
    ap.add_argument("--pictures", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    rows = []
    for W, H in SIZES:
        rows += kernels(W, H, a.reps, a.rounds, a.ring_mb)
    lines = [f"events around {a.reps} back-to-back warm launches on one stream over rings of {a.ring_mb} MB, median of {a.rounds} rounds: microseconds per launch (min .. max), "
             "the 6 W H bytes over that time, the 289 W H absolute differences over that time"]
    for r in rows:
        tail = f"  {r['Gabsdiff_per_s']:7.0f} G absolute differences/s  (level 2 on a noisy pan: {100 * r['blocks_moved']:.0f} % of the blocks moved, {100 * r['blocks_gated']:.0f} % gated)" if r["Gabsdiff_per_s"] else ""
        lines.append(f"{r['size']:10s} {r['what']:17s} {r['us']:8.2f} us ({r['us_min']:7.2f} .. {r['us_max']:7.2f})  {r['MB']:6.1f} MB  {r['GBps']:6.0f} GB/s{tail}")
    enc = encoder(a.pictures, a.runs) if a.pictures > 0 else None
    if enc:
        lines.append(f"encoder {enc['size']}, -qp 27, default GOP, {enc['pictures']} host pictures, median of {a.runs} runs: denoise 0 {enc['off_pps']:.1f} pictures/s, denoise 2 {enc['on_pps']:.1f} pictures/s: "
                     f"{enc['us_per_picture_more']:+.1f} us per picture")
        b = enc["noisy_bytes_per_level"]
        lines.append("the clip with Gaussian noise of sigma 3, bytes of the stream at levels 0 / 1 / 2 / 3: " + " / ".join(str(x) for x in b) + "  (" + " / ".join(f"{x / b[0]:.3f}" for x in b) + ")")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps({"rows": rows, "encoder": enc}) + "\n")


if __name__ == "__main__":
    main()
