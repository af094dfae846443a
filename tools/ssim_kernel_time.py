#!/usr/bin/env python3
"""Times the fused SSIM + SSE pass (ssim_picture_kernel) against the SSE pass (sse_picture_kernel) on two random pictures, alternating, with device events; run it under
`rocprofv3 --kernel-trace --stats -- python tools/ssim_kernel_time.py` for the kernels' own durations.  Both read the same bytes: 2 x W x H x 3 / 2."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ks265codec_amd.lib import KsContext, KsFrame  # noqa: E402
from ks265codec_amd.synth import lambda_q4  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=3840); ap.add_argument("--height", type=int, default=2160); ap.add_argument("--iters", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
ks = KsContext(0)
fr = KsFrame(ks, a.width, a.height, 27, lambda_q4(27))
pa, pb = fr.new_pic(), fr.new_pic()
for p in (pa, pb):
    for t in (p.y, p.u, p.v):
        t.copy_(torch.randint(0, 256, t.shape, dtype=torch.uint8, device=t.device))
sse, sse2, ssim = ks.zeros(24), ks.zeros(24), ks.zeros(24)
calls = {"sse_picture": lambda: fr.lib.ks265_sse_picture(fr.h, pa.c(), pb.c(), C.c_void_p(sse.data_ptr())),
         "ssim_picture (+ sse)": lambda: fr.lib.ks265_ssim_picture(fr.h, pa.c(), pb.c(), C.c_void_p(sse2.data_ptr()), C.c_void_p(ssim.data_ptr()))}
ms = {k: [] for k in calls}
for it in range(a.warmup + a.iters):
    for k, f in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); rc = f(); e1.record()
        assert rc == 0
        if it >= a.warmup:
            ms[k].append((e0, e1))
torch.cuda.synchronize()
assert sse.cpu().numpy().tobytes() == sse2.cpu().numpy().tobytes(), "the fused pass's SSE is the SSE pass's"
nbytes = 2 * a.width * a.height * 3 // 2
for k, ev in ms.items():
    t = np.median([x.elapsed_time(y) for x, y in ev])
    print(f"{k}: median of {len(ev)} launches {t * 1000:.1f} us between events, {nbytes / t / 1e9:.2f} TB/s of {nbytes / 1e6:.1f} MB read")
print("ssim sums", ssim.cpu().numpy().view(np.int64).tolist(), "sse", sse.cpu().numpy().view(np.uint64).tolist())
