"""Local contrast on the way in (include/ks265_hip.h ks265_input_hdr; ks265codec_amd/csrc/input_hdr.hip): what the 2 x iters passes cost beside a copy of the
bytes they move, and what a handle with `hdr` on costs beside the same handle with it off.  Nothing here is a pass mark.

Kernel: as tools/enhance_bench.py measures - everything on ONE stream (torch's current one, which the context adopts), events around --reps warm calls that queue up behind a
few milliseconds of other work and so run back to back, --rounds times; the figure is the median round's microseconds per call (= per picture: all passes), at 1920x1080 and
3840x2160, for iter 2 and 3 at sigma_s 20 and 100 (strength and sigma_r at their defaults).  Every call filters the next picture of a ring (--ring-mb: larger than the
caches) with one work buffer, as a lane does.  The bytes the passes move: every pass reads the guidance (W H) and, but for the first, a 16-bit plane (2 W H) and writes one
(the first also the guidance copy, the last the luma instead) - 18 W H at 2 iterations, 28 W H at 3.  A ks265_memcpy_d2d_async that moves as many bytes (half of them read,
half written, between two buffers) in the same run is the yardstick.

Encoder: a 1920x1080 handle fed --pictures host pictures through the C API, -rc 0 -qp 27, default GOP, `hdr` 0 against 1 (defaults, and iter 2 at sigma_s 100) on the same
clip: wall time from the first picture to the end of the flush, median of --runs, alternating.

    python tools/hdr_bench.py [--reps 16] [--rounds 7] [--ring-mb 300] [--pictures 64] [--runs 5] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import hdr_ref as hr  # noqa: E402
from denoise_bench import clips  # noqa: E402
from enhance_bench import session  # noqa: E402
from ks265codec_amd import lib as kl  # noqa: E402

SIZES = [(1920, 1080), (3840, 2160)]
POINTS = [(2, 20), (3, 20), (2, 100), (3, 100)]                         # (iter, sigma_s)


def moved_wh(iters):
    """the bytes all passes of one call read and write, in units of W H"""
    return 4 + 5 * (2 * iters - 2) + 4


def kernels(W, H, reps, rounds, ring_mb):
    ks = kl.KsContext(0)                                                # torch's current stream
    npx = W * H
    n = npx * 3 // 2
    nring = max(2, -(-ring_mb * 1000000 // n))
    base = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda").float()
    base = torch.nn.functional.avg_pool2d(base[None, None], 5, 1, 2)[0, 0]
    src = torch.cat([base.clamp(0, 255).to(torch.uint8).reshape(-1), torch.full((npx // 2,), 128, dtype=torch.uint8, device="cuda")])
    pic = [src.clone() for _ in range(nring)]
    nb = ks.input_hdr_work_bytes(W, H)
    work = torch.empty(nb, dtype=torch.uint8, device="cuda")
    big = [torch.empty(14 * npx, dtype=torch.uint8, device="cuda") for _ in range(2)]
    turn = [0]

    def hdr(cfg):
        def fn():
            ks.input_hdr(cfg, W, H, pic[turn[0] % nring], work)
        return fn

    def copy(iters):
        def fn():
            k = turn[0] & 1
            assert ks.lib.ks265_memcpy_d2d_async(ks.h, C.c_void_p(big[k].data_ptr()), C.c_void_p(big[k ^ 1].data_ptr()), C.c_size_t(moved_wh(iters) * npx // 2)) == 0
        return fn

    busy, busy_out = torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda")
    rows = []
    legs = [(f"copy of {moved_wh(i)} W H", copy(i), i, None) for i in (2, 3)]
    legs += [(f"iter {i} sigma_s {s}", hdr(hr.params(0, i, s, 0)), i, hr.params(0, i, s, 0)) for i, s in POINTS]
    for name, fn, iters, cfg in legs:
        for _ in range(6):                                              # warm: the code object, the buffers touched
            fn(); turn[0] += 1
        torch.cuda.synchronize()
        for p in pic:                                                   # (a filtered picture is another picture: every leg starts from the same ring)
            p.copy_(src)
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
        mb = moved_wh(iters) * npx / 1e6
        rows.append({"size": f"{W}x{H}", "what": name, "iters": iters, "cfg": cfg, "us": m, "us_min": min(us), "us_max": max(us), "MB": mb, "GBps": mb / m * 1e3, "work_bytes": nb})
    for r in rows:
        r["ratio_to_copy"] = r["us"] / rows[0 if r["iters"] == 2 else 1]["us"]
    ks.close()
    return rows


def encoder(n, runs):
    W, H = 1920, 1080
    src, _ = clips(W, H, n)
    session(W, H, src[:16], hdr=1)                                      # warm: code objects, the allocator
    legs = {"off": {}, "hdr (3, 20)": dict(hdr=1), "hdr (2, 100)": {"hdr": 1, "hdr-iter": 2, "hdr-sigma-s": 100}}
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
    ap.add_argument("--reps", type=int, default=16)
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
    lines = [f"events around {a.reps} back-to-back warm calls (2 x iter launches each) on one stream over a ring of {a.ring_mb} MB, median of {a.rounds} rounds: microseconds per "
             "picture (min .. max), the bytes the passes move over that time, the time over that of a copy moving as many bytes"]
    for r in rows:
        lines.append(f"{r['size']:10s} {r['what']:19s} {r['us']:9.2f} us ({r['us_min']:8.2f} .. {r['us_max']:8.2f})  {r['MB']:6.1f} MB  {r['GBps']:6.0f} GB/s  x {r['ratio_to_copy']:.2f}")
    lines.append("work buffer per lane: " + ", ".join(f"{W}x{H} {hr.work_bytes(W, H)} bytes" for W, H in SIZES))
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
