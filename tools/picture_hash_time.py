#!/usr/bin/env python3
"""Times the decoded picture hash pass (picture_hash_kernel, one picture read) against its yardstick, the fused SSIM + SSE pass (ssim_picture_kernel, two pictures read), on
random pictures at 2160p and 1080p: alternating launches, warm, device events around each launch, the median of --iters (at least 20) launches.  Also checks the six values
against tests/picture_hash_ref.py once per size.  The lines go to stdout; profiles/picture_hash.txt keeps them."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from ks265codec_amd.lib import KsContext, KsFrame  # noqa: E402
from ks265codec_amd.synth import lambda_q4  # noqa: E402
import picture_hash_ref as ph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="3840x2160,1920x1080"); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
assert a.iters >= 20
ks = KsContext(0)
for size in a.sizes.split(","):
    W, H = (int(x) for x in size.split("x"))
    fr = KsFrame(ks, W, H, 27, lambda_q4(27))
    pa, pb = fr.new_pic(), fr.new_pic()
    for p in (pa, pb):
        for t in (p.y, p.u, p.v):
            t.copy_(torch.randint(0, 256, t.shape, dtype=torch.uint8, device=t.device))
    sse, ssim, h6 = ks.zeros(24), ks.zeros(24), ks.zeros(24)
    calls = {"ssim_picture (+ sse), 2 pictures": lambda: fr.lib.ks265_ssim_picture(fr.h, pa.c(), pb.c(), C.c_void_p(sse.data_ptr()), C.c_void_p(ssim.data_ptr())),
             "picture_hash, 1 picture": lambda: fr.lib.ks265_picture_hash(fr.h, pa.c(), C.c_void_p(h6.data_ptr()))}
    ms = {k: [] for k in calls}
    for it in range(a.warmup + a.iters):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); rc = f(); e1.record()
            assert rc == 0
            if it >= a.warmup:
                ms[k].append((e0, e1))
    torch.cuda.synchronize()
    i420 = fr.store_i420(pa).cpu().numpy()
    ok = ks.host(h6, np.uint32).tolist() == ph.picture_hashes(*ph.i420_planes(i420, W, H))
    for k, ev in ms.items():
        t = np.median([x.elapsed_time(y) for x, y in ev])
        nbytes = W * H * 3 // 2 * (2 if "ssim" in k else 1)
        print(f"{W}x{H} {k}: median of {len(ev)} launches {t * 1000:.1f} us between events, {nbytes / t / 1e9:.2f} TB/s of {nbytes / 1e6:.1f} MB read")
    print(f"{W}x{H} values equal the specification: {ok}")
    fr.close()
    if not ok:
        sys.exit(1)
