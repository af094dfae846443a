"""Tone mapping on the way in (include/ks265_hip.h ks265_input_tonemap; ks265codec_amd/csrc/input_tonemap.hip): what the one launch costs with its tables in
global memory and in LDS, beside the plain conversion of the same P010 picture (ks265_input_convert: the memory-bound kernel this one adds arithmetic to) and beside a
copy of the bytes moved.  Nothing here is a pass mark.

As tools/overlay_bench.py measures: everything on ONE stream (torch's current one, which the context adopts), events around --reps warm calls that queue up behind a few
milliseconds of other work and so run back to back, --rounds times; the figure is the median round's microseconds per call (= per picture), at 1920x1080 and 3840x2160.
Every call reads the next P010 picture of a ring and writes the next packed I420 picture of another (--ring-mb: larger than the caches).  A launch moves 3 bytes a pixel in
and 1.5 out; the ks265_memcpy_d2d_async yardstick moves as many (half read, half written) through two rings of its own.  The content is random words: every table gather
goes somewhere else, which is the worst case for both placements (a real picture's neighbouring pixels share table lines and LDS words).  --content ramp measures smooth
content instead.

    python tools/tonemap_bench.py [--reps 16] [--rounds 7] [--ring-mb 300] [--content random|ramp] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ks265codec_amd import lib as kl  # noqa: E402

SIZES = [(1920, 1080), (3840, 2160)]


def kernels(W, H, reps, rounds, ring_mb, content):
    ks = kl.KsContext(0)                                                # torch's current stream
    nsrc, ndst = W * H * 3, W * H * 3 // 2
    nring = max(2, -(-ring_mb * 1000000 // nsrc))
    if content == "ramp":
        yy, xx = torch.meshgrid(torch.arange(H * 3 // 2, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        one = (((xx * 800 // W + yy // 8) % 1024) << 6).to(torch.int16)
        one[H:] = (512 + ((xx[H:] // 2) % 64)) << 6
        src = [one.clone() for _ in range(nring)]
    else:
        src = [torch.randint(-32768, 32768, (H * 3 // 2, W), dtype=torch.int16, device="cuda") for _ in range(nring)]
    dst = [torch.empty(ndst, dtype=torch.uint8, device="cuda") for _ in range(nring)]
    plan = ks.tonemap_plan_create(0, 1000.0, 203.0, False)
    moved = nsrc + ndst
    span = ring_mb * 1000000
    big = [torch.empty(span + moved // 2 + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    turn = [0]

    def desc(t):
        d = kl.InDesc()
        d.format, d.width, d.height = kl.IN_P010, W, H
        d.plane[0], d.plane[1], d.pitch[0], d.pitch[1] = t.data_ptr(), t.data_ptr() + 2 * W * H, 2 * W, 2 * W
        return d
    descs = [desc(t) for t in src]

    def tonemap(where):
        def fn():
            ks.input_tonemap(plan, descs[turn[0] % nring], dst[turn[0] % nring])
        return fn

    def convert():
        assert ks.lib.ks265_input_convert(ks.h, C.byref(descs[turn[0] % nring]), C.c_void_p(dst[turn[0] % nring].data_ptr())) == 0

    def copy():
        at = (turn[0] * (moved // 2 + 4095) // 4096 * 4096) % span      # (the next stretch of both rings)
        assert ks.lib.ks265_memcpy_d2d_async(ks.h, C.c_void_p(big[0].data_ptr() + at), C.c_void_p(big[1].data_ptr() + at), C.c_size_t(moved // 2)) == 0

    busy, busy_out = torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda")
    rows = []
    for name, fn, where in (("copy", copy, None), ("convert", convert, None), ("tonemap global", tonemap(0), 0), ("tonemap lds", tonemap(1), 1)):
        if where is not None:
            ks.tonemap_plan_tables(plan, where)
        for _ in range(6):                                              # warm: the code object, the buffers touched
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
        rows.append({"size": f"{W}x{H}", "content": content, "what": name, "us": m, "us_min": min(us), "us_max": max(us), "MB": moved / 1e6, "GBps": moved / m / 1e3})
    for r in rows:
        r["ratio_to_copy"] = r["us"] / rows[0]["us"]
        r["ratio_to_convert"] = r["us"] / rows[1]["us"]
    torch.cuda.synchronize()
    ks.tonemap_plan_destroy(plan)
    ks.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring-mb", type=int, default=300)
    ap.add_argument("--content", choices=("random", "ramp"), default="random")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    rows = []
    for W, H in SIZES:
        rows += kernels(W, H, a.reps, a.rounds, a.ring_mb, a.content)
    lines = [f"P010 of {a.content} content, bt2390 / 1000 / 203: events around {a.reps} back-to-back warm calls (one launch each) on one stream over rings of {a.ring_mb} MB, median of "
             f"{a.rounds} rounds: microseconds per picture (min .. max), the bytes the launch moves over that time, the time over the copy's and over the plain conversion's"]
    for r in rows:
        lines.append(f"{r['size']:10s} {r['what']:16s} {r['us']:9.2f} us ({r['us_min']:8.2f} .. {r['us_max']:8.2f})  {r['MB']:7.2f} MB  {r['GBps']:6.0f} GB/s  x {r['ratio_to_copy']:.2f} copy  x {r['ratio_to_convert']:.2f} convert")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps({"rows": rows}) + "\n")


if __name__ == "__main__":
    main()
