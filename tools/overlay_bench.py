"""Overlays on the way in (include/ks265_hip.h ks265_input_overlay; ks265codec_amd/csrc/input_overlay.hip): what the one launch costs beside a copy of the
bytes it moves.  Nothing here is a pass mark.

As tools/hdr_bench.py measures: everything on ONE stream (torch's current one, which the context adopts), events around --reps warm calls that queue up behind a few
milliseconds of other work and so run back to back, --rounds times; the figure is the median round's microseconds per call (= per picture), at 1920x1080 and 3840x2160, for
  logo      one 256x128 RGBA overlay of bytes near the top right corner, at an x that is no multiple of 8;
  8 logos   eight of them, each over half of the one before;
  full f16  one float16 RGBA overlay of the picture's size.
Every call blends onto the next picture of a ring (--ring-mb: larger than the caches).  The bytes a launch moves: the overlay's samples once (4 elements a pixel; its chroma
filter's left neighbours come from the cache) and the picture's bytes under the rectangles read and written (2 x 1.5 a pixel).  A ks265_memcpy_d2d_async that moves as many
bytes (half read, half written) in the same run is the yardstick; like the blend it walks a ring larger than the caches - source and destination advance through two buffers
of --ring-mb each - so neither side is helped by the Infinity Cache.  For the logos it is a copy of a few hundred kilobytes, which measures a launch.

Host side: the kernel figures are device time.  Every call also validates every overlay on the calling thread (up to four extent queries of the runtime per overlay and one
for the picture, as ks265_input_convert validates its source); `host us` is the wall time of the calling thread per call, the stream not waited for, median of the rounds.

    python tools/overlay_bench.py [--reps 16] [--rounds 7] [--ring-mb 300] [--out FILE]"""
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

SIZES = [(1920, 1080), (3840, 2160)]
LW, LH = 256, 128


def desc(t, x, y, opacity=256):
    """the descriptor tuple of KsContext.overlay_descs for an (h, w, 4) RGBA tensor"""
    es = t.element_size()
    fmt = {torch.uint8: kl.IN_RGB, torch.float16: kl.IN_RGB_F16}[t.dtype]
    return (fmt, t.shape[1], t.shape[0], [t.data_ptr() + k * es for k in range(3)], t.data_ptr() + 3 * es, t.stride(0) * es, t.stride(1) * es, x, y, opacity, 0, False)


def kernels(W, H, reps, rounds, ring_mb):
    ks = kl.KsContext(0)                                                # torch's current stream
    n = W * H * 3 // 2
    nring = max(2, -(-ring_mb * 1000000 // n))
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    pic = [src.clone() for _ in range(nring)]
    logos = [torch.randint(0, 256, (LH, LW, 4), dtype=torch.uint8, device="cuda") for _ in range(8)]
    full = torch.rand((H, W, 4), device="cuda").to(torch.float16)
    cases = {"logo": [desc(logos[0], W - LW - 58, 32)],
             "8 logos": [desc(logos[k], W - LW - 58 - (LW // 2) * k, 32 + 16 * k, 256 - 16 * k) for k in range(8)],
             "full f16": [desc(full, 0, 0, 200)]}
    covered = {"logo": LW * LH, "8 logos": 8 * LW * LH, "full f16": W * H}                   # overlay pixels (what overlaps is blended once per overlay, in registers)
    touched = {"logo": LW * LH, "8 logos": (LW + 7 * LW // 2) * (LH + 7 * 16) // 2 + LW * LH, "full f16": W * H}    # picture pixels under the rectangles, an estimate for the staircase
    moved = {k: covered[k] * 4 * (2 if k == "full f16" else 1) + 3 * touched[k] for k in cases}
    span = ring_mb * 1000000
    big = [torch.empty(span + max(moved.values()) // 2 + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    turn = [0]

    def blend(ovs):
        def fn():
            ks.input_overlay(ovs, W, H, pic[turn[0] % nring])
        return fn

    def copy(nbytes):
        def fn():
            at = (turn[0] * (nbytes // 2 + 4095) // 4096 * 4096) % span     # (the next stretch of both rings)
            assert ks.lib.ks265_memcpy_d2d_async(ks.h, C.c_void_p(big[0].data_ptr() + at), C.c_void_p(big[1].data_ptr() + at), C.c_size_t(nbytes // 2)) == 0
        return fn

    busy, busy_out = torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda")
    rows = []
    legs = []
    for k in cases:
        legs += [(f"copy for {k}", copy(moved[k]), k, True), (k, blend(cases[k]), k, False)]
    for name, fn, case, is_copy in legs:
        for _ in range(6):                                              # warm: the code object, the buffers touched
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
        rows.append({"size": f"{W}x{H}", "what": name, "case": case, "copy": is_copy, "us": m, "us_min": min(us), "us_max": max(us), "host_us": statistics.median(host), "MB": moved[case] / 1e6, "GBps": moved[case] / m / 1e3})
    for r in rows:
        r["ratio_to_copy"] = r["us"] / next(q["us"] for q in rows if q["copy"] and q["case"] == r["case"])
    ks.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring-mb", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    rows = []
    for W, H in SIZES:
        rows += kernels(W, H, a.reps, a.rounds, a.ring_mb)
    lines = [f"events around {a.reps} back-to-back warm calls (one launch each) on one stream over a ring of {a.ring_mb} MB, median of {a.rounds} rounds: microseconds per picture "
             "(min .. max), the bytes the launch moves over that time, the time over that of a copy moving as many bytes, the calling thread's microseconds per call"]
    for r in rows:
        lines.append(f"{r['size']:10s} {r['what']:18s} {r['us']:9.2f} us ({r['us_min']:8.2f} .. {r['us_max']:8.2f})  {r['MB']:7.2f} MB  {r['GBps']:6.0f} GB/s  x {r['ratio_to_copy']:.2f}  host {r['host_us']:6.2f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps({"rows": rows}) + "\n")


if __name__ == "__main__":
    main()
