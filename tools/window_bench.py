"""Picture sizes that are no multiple of 8 (include/ks265_hip.h ks265_input_pad / ks265_output_crop; ks265codec_amd/csrc/picture_window.hip): what the two
kernels cost beside a device-to-device copy of the coded picture's bytes IN THE SAME RUN - the yardstick: all three stream a picture through once - and what a ragged encoder
handle costs beside the coded-size handle over the same pictures.

Kernels: as tools/yuv_in_bench.py measures - everything on ONE stream (torch's current one, which the context adopts), events around --reps warm launches that queue up behind
a few milliseconds of other work and so run back to back, --rounds times; the figure is the median round's microseconds per launch.  Every launch reads the next source of a
ring (--ring-mb in all, so that a picture is not still in a cache when its turn comes again) and writes the next of eight destinations.  The copy is measured first and once
more at the end: the two figures show the run's own spread.  Bytes moved: source picture + destination picture (the copy: twice the coded picture).

Encoder: a 1366x768 handle fed --pictures host pictures against a 1368x768 handle fed the same pictures padded (tests/picture_window_ref.py), through the C API, -rc 0, default
GOP: wall time from the first picture to the end of the flush, median of --runs, alternating; every NAL unit but the SPS must be equal.

    python tools/window_bench.py [--reps 48] [--rounds 7] [--ring-mb 300] [--pictures 96] [--runs 5] [--out FILE]"""
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

import picture_window_ref as pw  # noqa: E402
from ks265codec_amd import lib as kl  # noqa: E402

SIZES = [(1366, 768), (3838, 2158)]


def kernels(W, H, reps, rounds, ring_mb):
    lib = kl.load_library()
    lib.ks265_last_error.restype = C.c_char_p
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    assert lib.ks265_set_stream(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0   # one stream for the library's kernels and torch's events
    cw, ch = pw.coded_size(W, H)
    nsrc, ncod = W * H * 3 // 2, cw * ch * 3 // 2
    nring = max(2, -(-ring_mb * 1000000 // ncod))
    raw = [torch.randint(0, 256, (nsrc,), dtype=torch.uint8, device="cuda") for _ in range(nring)]
    cod = [torch.randint(0, 256, (ncod,), dtype=torch.uint8, device="cuda") for _ in range(nring)]
    out_c = [torch.empty(ncod, dtype=torch.uint8, device="cuda") for _ in range(8)]
    out_r = [torch.empty(nsrc, dtype=torch.uint8, device="cuda") for _ in range(8)]
    descs = []
    for t in raw:
        d = kl.InDesc()
        d.format, d.width, d.height = kl.IN_I420, W, H
        p = t.data_ptr()
        d.plane[0], d.plane[1], d.plane[2] = p, p + W * H, p + W * H * 5 // 4
        d.pitch[0], d.pitch[1], d.pitch[2] = W, W // 2, W // 2
        descs.append(d)
    turn = [0]

    def pad():
        rc = lib.ks265_input_pad(h, C.byref(descs[turn[0] % nring]), cw, ch, C.c_void_p(out_c[turn[0] % 8].data_ptr()))
        assert rc == 0, (rc, lib.ks265_last_error(h))

    def crop():
        rc = lib.ks265_output_crop(h, C.c_void_p(cod[turn[0] % nring].data_ptr()), cw, ch, W, H, C.c_void_p(out_r[turn[0] % 8].data_ptr()))
        assert rc == 0, (rc, lib.ks265_last_error(h))

    def copy():
        assert lib.ks265_memcpy_d2d_async(h, C.c_void_p(out_c[turn[0] % 8].data_ptr()), C.c_void_p(cod[turn[0] % nring].data_ptr()), C.c_size_t(ncod)) == 0

    busy, busy_out = torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda")
    rows = []
    for name, fn, mb in (("copy", copy, 2 * ncod / 1e6), ("pad", pad, (nsrc + ncod) / 1e6), ("crop", crop, (nsrc + ncod) / 1e6), ("copy (again)", copy, 2 * ncod / 1e6)):
        for _ in range(nring + 5):                                      # warm: the code object, every buffer touched once
            fn(); turn[0] += 1
        torch.cuda.synchronize()
        us, host = [], []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):                                          # a few milliseconds of other work in front: the launches queue up behind it and run back to back
                torch.mm(busy, busy, out=busy_out)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn(); turn[0] += 1
            host.append((time.perf_counter() - t0) * 1e6 / reps)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / reps)
        m = statistics.median(us)
        rows.append({"size": f"{W}x{H}", "what": name, "us": m, "us_min": min(us), "us_max": max(us), "host_us": statistics.median(host), "MB": mb, "GBps": mb / m * 1e3})
    lib.ks265_destroy(h)
    return rows


class YUV(C.Structure):
    _fields_ = [("iWidth", C.c_int), ("iHeight", C.c_int), ("pData", C.POINTER(C.c_ubyte) * 3), ("iStride", C.c_int * 3)]


class HostPicture(C.Structure):
    _fields_ = [("iSliceType", C.c_int), ("poc", C.c_int), ("pts", C.c_longlong), ("dts", C.c_longlong), ("yuv", C.POINTER(YUV))]


def session(W, H, pictures):
    """(seconds from the first picture to the end of the flush, the stream) of one handle fed host pictures"""
    from ks265codec_amd.encoder import Nal, library
    lib = library()
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("threads", 8), ("rc", 0), ("qp", 30), ("iper", 128), ("log", 0)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0, k
    err = C.c_int(0)
    h = lib.QY265EncoderOpen(cfg, C.byref(err))
    assert h, hex(err.value & 0xFFFFFFFF)
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    bs = bytearray()

    def take():
        for i in range(nn.value):
            if nal[i].iSize > 0:
                bs.extend(C.string_at(nal[i].pPayload, nal[i].iSize))
    t0 = time.perf_counter()
    for t, p in enumerate(pictures):
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(p.ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.addressof(pic), C.addressof(outp), 0) == 0
        take()
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == 0
        take()
    dt = time.perf_counter() - t0
    lib.QY265EncoderClose(h)
    return dt, bytes(bs)


def nals(stream):
    parts = stream.split(b"\x00\x00\x01")[1:]
    return [((p[0] >> 1) & 63, p.rstrip(b"\x00") if i + 1 < len(parts) else p) for i, p in enumerate(parts)]


def encoder(n, runs):
    W, H = 1366, 768
    cw, ch = pw.coded_size(W, H)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    src = []
    for t in range(n):
        y = np.clip(128 + 80 * np.sin(0.05 * (xx + 3 * t)) * np.cos(0.04 * (yy + 2 * t)) + rng.integers(0, 6, (H, W)), 0, 255).astype(np.uint8)
        u = np.clip(128 + 60 * np.sin(0.02 * (xx[::2, ::2] + 2 * t)), 0, 255).astype(np.uint8)
        v = np.clip(128 + 60 * np.cos(0.03 * (yy[::2, ::2] - t)), 0, 255).astype(np.uint8)
        src.append(pw.pack([y, u, v]))
    padded = [pw.pad_i420(p, W, H) for p in src]
    session(cw, ch, padded[:16])                                       # warm: code objects, the allocator
    tr, tc, equal = [], [], True
    for _ in range(runs):
        dr, sr = session(W, H, src)
        dc, sc = session(cw, ch, padded)
        tr.append(dr); tc.append(dc)
        a, b = nals(sr), nals(sc)
        equal = equal and len(a) == len(b) and all((x == y) == (t != 33) for (t, x), (_, y) in zip(a, b))
    mr, mc = statistics.median(tr), statistics.median(tc)
    return {"pictures": n, "ragged": f"{W}x{H}", "coded": f"{cw}x{ch}", "ragged_pps": n / mr, "coded_pps": n / mc, "ragged_s": tr, "coded_s": tc,
            "us_per_picture_more": (mr - mc) / n * 1e6, "streams_equal_but_sps": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring-mb", type=int, default=300)
    ap.add_argument("--pictures", type=int, default=96)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    rows = []
    for W, H in SIZES:
        rows += kernels(W, H, a.reps, a.rounds, a.ring_mb)
    lines = [f"events around {a.reps} back-to-back warm launches on one stream over a ring of {a.ring_mb} MB of sources, median of {a.rounds} rounds: microseconds per launch "
             "(min .. max), MB moved, GB/s"]
    for r in rows:
        lines.append(f"{r['size']:10s} {r['what']:13s} {r['us']:8.2f} us ({r['us_min']:7.2f} .. {r['us_max']:7.2f})  {r['MB']:6.1f} MB  {r['GBps']:6.0f} GB/s   (the host's call: {r['host_us']:6.1f} us)")
    enc = encoder(a.pictures, a.runs) if a.pictures > 0 else None
    if enc:
        lines.append(f"encoder, {enc['pictures']} pictures, median of {a.runs} runs: {enc['ragged']} {enc['ragged_pps']:.1f} pictures/s, {enc['coded']} {enc['coded_pps']:.1f} pictures/s: "
                     f"{enc['us_per_picture_more']:+.1f} us per picture; every NAL unit but the SPS equal: {enc['streams_equal_but_sps']}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps({"rows": rows, "encoder": enc}) + "\n")


if __name__ == "__main__":
    main()
