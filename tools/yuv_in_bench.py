"""The YUV family of the device input (KS265_IN_YUV, include/ks265_hip.h; ks265codec_amd/csrc/input_yuv.hip) at 3840x2160: what each format's conversion costs beside the
NV12 kernel of input_convert.hip IN THE SAME RUN - the yardstick: both are streaming kernels with the same store pattern, so a format should not move fewer bytes per second
than NV12 does.

Everything runs on ONE stream (torch's current one, which the context adopts), timed by events around --reps warm launches that queue up behind a few milliseconds of other
work and so run back to back, --rounds times; the figure is the median round's microseconds per launch.  NV12 is measured first and once more behind every other format: the
two figures show the run's own spread.  Every launch reads the next source of a ring of sources (--ring-mb in all, so that a picture is not still in a cache when its turn
comes again) and writes the next of eight destinations.  Bytes moved are what the conversion has to touch: every stored element of the source
once and the packed I420 picture, 1.5 bytes per pixel.

    python tools/yuv_in_bench.py [--reps 48] [--rounds 7] [--size 3840x2160] [--ring-mb 600] [--out FILE]"""
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

import torch  # noqa: E402

from ks265codec_amd import lib as kl  # noqa: E402

# name -> (code, layout, subsampling, depth)
FORMATS = {"NV12": (kl.IN_NV12, 1, 0, 8), "I420": (kl.IN_I420, 0, 0, 8),
           "P010": (kl.IN_P010, 1, 0, 10), "P016": (kl.IN_P016, 1, 0, 16), "I010": (kl.IN_I010, 0, 0, 10),
           "NV16": (kl.IN_NV16, 1, 1, 8), "I422": (kl.IN_I422, 0, 1, 8), "YUYV": (kl.IN_YUYV, 2, 1, 8), "UYVY": (kl.IN_UYVY, 3, 1, 8),
           "P210": (kl.IN_P210, 1, 1, 10), "I210": (kl.IN_I210, 0, 1, 10), "Y210": (kl.IN_Y210, 2, 1, 10),
           "NV24": (kl.IN_NV24, 1, 2, 8), "I444": (kl.IN_I444, 0, 2, 8), "P410": (kl.IN_P410, 1, 2, 10), "I410": (kl.IN_I410, 0, 2, 10)}


def plane_shapes(layout, sub, W, H):
    cw, ch = (W if sub == 2 else W // 2), (H // 2 if sub == 0 else H)
    return [(H, W), (ch, cw), (ch, cw)] if layout == 0 else [(H, W), (ch, 2 * cw)] if layout == 1 else [(H, 2 * W)]


def source_bytes(layout, sub, depth, W, H):
    return sum(r * n for r, n in plane_shapes(layout, sub, W, H)) * (1 if depth == 8 else 2)


def make_source(code, layout, sub, depth, W, H):
    """(descriptor, the tensors it points into): random words - every bit pattern is a legal element"""
    planes = [torch.randint(0, 256, (r, n * (1 if depth == 8 else 2)), dtype=torch.uint8, device="cuda") for r, n in plane_shapes(layout, sub, W, H)]
    d = kl.InDesc()
    d.format, d.width, d.height = code, W, H
    for k, p in enumerate(planes):
        d.plane[k], d.pitch[k] = p.data_ptr(), p.shape[1]
    return d, planes


def measure(W, H, reps, rounds, ring_mb, names):
    lib = kl.load_library()
    lib.ks265_last_error.restype = C.c_char_p
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    assert lib.ks265_set_stream(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0   # one stream for the library's kernels and torch's events
    dsts = [torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda") for _ in range(8)]
    busy, busy_out = torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda")
    us, host = {n: [] for n in names}, {n: [] for n in names}
    mb = {}
    for n in names:                                                     # one format's ring at a time: the rings do not have to fit into memory together
        code, layout, sub, depth = FORMATS[n]
        nbytes = source_bytes(layout, sub, depth, W, H)
        mb[n] = (nbytes + W * H * 1.5) / 1e6
        ring = [make_source(code, layout, sub, depth, W, H) for _ in range(max(2, -(-ring_mb * 1000000 // nbytes)))]
        turn = [0]

        def launch():
            d = ring[turn[0] % len(ring)][0]
            rc = lib.ks265_input_convert(h, C.byref(d), C.c_void_p(dsts[turn[0] % len(dsts)].data_ptr()))
            assert rc == 0, (rc, lib.ks265_last_error(h))
            turn[0] += 1
        for _ in range(len(ring) + 5):                                  # warm: the code object, every buffer touched once
            launch()
        torch.cuda.synchronize()
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):                                          # a few milliseconds of other work in front: the launches queue up behind it and run back to back,
                torch.mm(busy, busy, out=busy_out)                      # so the events time the kernels, not the host's calls (host_us beside it shows what those cost)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(reps):
                launch()
            host[n].append((time.perf_counter() - t0) * 1e6 / reps)
            e1.record()
            e1.synchronize()
            us[n].append(e0.elapsed_time(e1) * 1000.0 / reps)
        del ring
        torch.cuda.empty_cache()
    lib.ks265_destroy(h)
    return [{"format": n, "us": statistics.median(v), "us_min": min(v), "us_max": max(v), "host_us": statistics.median(host[n]), "MB": mb[n], "GBps": mb[n] / statistics.median(v) * 1e3}
            for n, v in us.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--ring-mb", type=int, default=600)
    ap.add_argument("--formats", default=",".join(FORMATS), help="comma-separated names; NV12 (the yardstick) is always measured, first and again last")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    names = ["NV12"] + [n for n in a.formats.split(",") if n != "NV12"]
    rows = measure(W, H, a.reps, a.rounds, a.ring_mb, names)
    again = measure(W, H, a.reps, a.rounds, a.ring_mb, ["NV12"])[0]    # the yardstick once more behind everything else: its own spread over the run
    again["format"] = "NV12 (again)"
    rows.append(again)
    ref = rows[0]["GBps"]
    lines = [f"{W}x{H}, events around {a.reps} back-to-back warm launches on one stream over a ring of {a.ring_mb} MB of sources, median of {a.rounds} rounds: microseconds per launch "
             "(min .. max), MB the conversion has to move, GB/s, GB/s relative to NV12's"]
    for r in rows:
        lines.append(f"{r['format']:13s} {r['us']:8.2f} us ({r['us_min']:7.2f} .. {r['us_max']:7.2f})  {r['MB']:6.1f} MB  {r['GBps']:6.0f} GB/s  {100.0 * r['GBps'] / ref:5.1f} %"
                     f"   (the host's call: {r['host_us']:6.1f} us)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps({"rows": rows}) + "\n")


if __name__ == "__main__":
    main()
