"""Edge and colour enhancement on the way in (include/ks265_hip.h ks265_input_enhance; ks265codec_amd/csrc/input_enhance.hip): what the kernel costs beside a
copy of the same bytes, and what a handle with `edge` on costs beside the same handle with it off.  Nothing here is a pass mark.

Kernel: as tools/denoise_bench.py measures - everything on ONE stream (torch's current one, which the context adopts), events around --reps warm launches that queue up behind a
few milliseconds of other work and so run back to back, --rounds times; the figure is the median round's microseconds per launch, at 1920x1080 and 3840x2160.  Every launch
enhances the next picture of a ring from the next luma copy of a second ring (--ring-mb in all: larger than the caches).  Reported against the 3 W H bytes the filter has to
move (W H luma and W H / 2 chroma in, 1.5 W H out); a ks265_memcpy_d2d_async pair that moves the same 3 W H bytes (the luma plane, then the chroma planes, ring to ring) in
the same run is the yardstick.  Edge-only and colour-only launches are timed beside the full one.

Encoder: a 1920x1080 handle fed --pictures host pictures through the C API, -rc 0 -qp 27, default GOP, `edge` 0 against 2 (and 2 with `color` 2) on the same clip: wall time
from the first picture to the end of the flush, median of --runs, alternating.

    python tools/enhance_bench.py [--reps 32] [--rounds 7] [--ring-mb 300] [--pictures 64] [--runs 5] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from denoise_bench import HostPicture, YUV, clips  # noqa: E402
from ks265codec_amd import lib as kl  # noqa: E402

SIZES = [(1920, 1080), (3840, 2160)]
LEVEL2 = (16, 2, 16, 4, 16)                                             # vpp_edge 2, vpp_color 2 (tests/enhance_ref.py)


def kernels(W, H, reps, rounds, ring_mb):
    ks = kl.KsContext(0)                                                # torch's current stream
    npx = W * H
    n = npx * 3 // 2
    nring = max(2, -(-ring_mb * 1000000 // (n + npx)))
    base = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda").float()
    base = torch.nn.functional.avg_pool2d(base[None, None], 3, 1, 1)[0, 0]
    pic = [torch.cat([(base + 2 * k).clamp(0, 255).to(torch.uint8).reshape(-1), torch.randint(0, 256, (npx // 2,), dtype=torch.uint8, device="cuda")]) for k in range(nring)]
    luma = [p[:npx].clone() for p in pic]
    turn = [0]

    def enhance(cfg):
        def fn():
            k = turn[0] % nring
            ks.input_enhance(cfg, W, H, luma[k] if cfg[0] else None, pic[(k + 1) % nring])
        return fn

    def copy():
        k = turn[0] % nring
        dst, src = pic[(k + 1) % nring], pic[k]
        for off, cnt in ((0, npx), (npx, npx // 2)):
            rc = ks.lib.ks265_memcpy_d2d_async(ks.h, C.c_void_p(dst.data_ptr() + off), C.c_void_p(src.data_ptr() + off), C.c_size_t(cnt))
            assert rc == 0

    busy, busy_out = torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda")
    rows = []
    for name, fn, moved in (("copy W H + W H / 2", copy, 3.0), ("edge 2 + colour 2", enhance(LEVEL2), 3.0), ("edge 2 alone", enhance(LEVEL2[:4] + (0,)), 2.0),
                            ("colour 2 alone", enhance((0, 0, 0, 0, 16)), 1.0), ("copy (again)", copy, 3.0)):
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
        rows.append({"size": f"{W}x{H}", "what": name, "us": m, "us_min": min(us), "us_max": max(us), "MB": moved * npx / 1e6, "GBps": moved * npx / m / 1e3})
    for r in rows:
        r["ratio_to_copy"] = r["us"] / rows[0]["us"]
    ks.close()
    return rows


def session(W, H, pictures, **params):
    """(seconds from the first picture to the end of the flush, bytes of the stream) of one handle fed host pictures"""
    from ks265codec_amd.encoder import Nal, library
    lib = library()
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("threads", 16), ("rc", 0), ("qp", 27), ("iper", 128), ("log", 0), *params.items()):
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


def encoder(n, runs):
    W, H = 1920, 1080
    src, _ = clips(W, H, n)
    session(W, H, src[:16], edge=2, color=2)                            # warm: code objects, the allocator
    legs = {"off": {}, "edge 2": dict(edge=2), "edge 2 color 2": dict(edge=2, color=2)}
    secs, size = {k: [] for k in legs}, {}
    for _ in range(runs):
        for k, p in legs.items():
            dt, size[k] = session(W, H, src, **p)
            secs[k].append(dt)
    med = {k: statistics.median(v) for k, v in secs.items()}
    return {"pictures": n, "size": f"{W}x{H}", "pps": {k: n / v for k, v in med.items()}, "seconds": secs, "bytes": size,
            "us_per_picture_more": {k: (med[k] - med["off"]) / n * 1e6 for k in legs if k != "off"}}


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
             "the bytes it has to move over that time, the time over the copy pair's"]
    for r in rows:
        lines.append(f"{r['size']:10s} {r['what']:19s} {r['us']:8.2f} us ({r['us_min']:7.2f} .. {r['us_max']:7.2f})  {r['MB']:6.1f} MB  {r['GBps']:6.0f} GB/s  x {r['ratio_to_copy']:.2f}")
    enc = encoder(a.pictures, a.runs) if a.pictures > 0 else None
    if enc:
        lines.append(f"encoder {enc['size']}, -qp 27, default GOP, {enc['pictures']} host pictures, median of {a.runs} runs, alternating: " +
                     ", ".join(f"{k} {v:.1f} pictures/s" for k, v in enc["pps"].items()) + "; " + ", ".join(f"{k}: {v:+.1f} us per picture" for k, v in enc["us_per_picture_more"].items()))
        lines.append("bytes of the stream: " + ", ".join(f"{k} {v}" for k, v in enc["bytes"].items()))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps({"rows": rows, "encoder": enc}) + "\n")


if __name__ == "__main__":
    main()
