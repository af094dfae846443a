"""ks265_roi_reduce alone at 3840x2160: device events around 200 back-to-back warm launches, the median of several such windows, for a per-pixel float32 map
(33.2 MB), a per-pixel int8 map (8.3 MB) and an int8 map of 16 x 16 blocks - each on ONE buffer (33 MB stay in the 256 MiB Infinity Cache between launches) and, for the
per-pixel maps, cycling through enough distinct buffers that every launch reads from HBM.  Beside them ks265_input_convert RGBA (33.2 MB read + 12.4 MB written) timed the
same way in the same run, as the yardstick, and each kernel's bandwidth as a share of it.  Every result is checked against tests/roi_map_ref.py once.

    python tools/roi_map_rate.py [--launches 200] [--windows 7] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class InDesc(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


def timed(ks, launch, launches, windows):
    """median over `windows` of (ms per launch over `launches` back-to-back launches); launch(i) enqueues launch i"""
    for i in range(launches):                                              # warm: code object, every buffer touched
        launch(i)
    ks.sync()
    per = []
    for _ in range(windows):
        ks._chk(ks.lib.ks265_timer_start(ks.h))
        for i in range(launches):
            launch(i)
        ms = C.c_float(0)
        ks._chk(ks.lib.ks265_timer_stop_ms(ks.h, C.byref(ms)))
        per.append(ms.value / launches)
    return statistics.median(per), min(per), max(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    import roi_map_ref as R
    from ks265codec_amd.lib import KsContext
    ks = KsContext(0)
    dev = ks.device
    n = ((W + 63) // 64) * ((H + 63) // 64)
    rec = torch.empty(n, dtype=torch.int32, device=dev)
    lines = [f"{W}x{H}, {a.launches} back-to-back launches per window, median (min .. max) of {a.windows} windows, device events"]

    src = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device=dev)
    dst = torch.empty(W * H * 3 // 2, dtype=torch.uint8, device=dev)
    d = InDesc(); d.format, d.width, d.height, d.pixel_step = 2, W, H, 4
    d.plane[0], d.plane[1], d.plane[2], d.pitch[0] = src.data_ptr(), src.data_ptr() + 1, src.data_ptr() + 2, W * 4
    med, lo, hi = timed(ks, lambda i: ks._chk(ks.lib.ks265_input_convert(ks.h, C.byref(d), C.c_void_p(dst.data_ptr()))), a.launches, a.windows)
    yard_bytes = W * H * 4 + W * H * 3 // 2
    yard = yard_bytes / (med * 1e-3)
    lines.append(f"ks265_input_convert RGBA (yardstick)      {yard_bytes / 1e6:6.1f} MB  {med * 1e3:8.2f} us ({lo * 1e3:.2f} .. {hi * 1e3:.2f})  {yard / 1e12:5.2f} TB/s")

    rng = np.random.default_rng(1)
    cases = [("float32 per pixel", np.float32, 0), ("int8 per pixel", np.int8, 0), ("int8 16 x 16 blocks", np.int8, 4)]
    for name, dtype, lb in cases:
        rows, cols = R.map_shape(W, H, lb)
        nbytes = rows * cols * np.dtype(dtype).itemsize
        nbuf = 1 if lb else max(2, int(300e6 // nbytes) + 1)               # more than 256 MiB of distinct maps: no launch finds its map in the Infinity Cache
        host = [(rng.standard_normal((rows, cols)) * 8).astype(np.float32) if dtype == np.float32 else rng.integers(-60, 61, (rows, cols)).astype(np.int8) for _ in range(min(nbuf, 2))]
        bufs = [torch.from_numpy(host[i % len(host)]).to(dev) for i in range(nbuf)]
        for i in (0, nbuf - 1):
            ks.roi_reduce(bufs[i], lb, W, H, out=rec); ks.sync()
            assert (rec.cpu().numpy() == R.reduce(host[i % len(host)], W, H, lb)).all(), name
        descs = [ks.roi_desc(b, lb) for b in bufs]
        for label, k in [("one buffer", 1)] + ([(f"{nbuf} buffers in turn", nbuf)] if nbuf > 1 else []):
            med, lo, hi = timed(ks, lambda i: ks._chk(ks.lib.ks265_roi_reduce(ks.h, C.byref(descs[i % k]), W, H, C.c_void_p(rec.data_ptr()))), a.launches, a.windows)
            bw = nbytes / (med * 1e-3)
            lines.append(f"ks265_roi_reduce {name:20s} {label:22s} {nbytes / 1e6:6.2f} MB  {med * 1e3:8.2f} us ({lo * 1e3:.2f} .. {hi * 1e3:.2f})  {bw / 1e12:6.3f} TB/s  = {100 * bw / yard:5.1f} % of the yardstick")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ks.close()


if __name__ == "__main__":
    main()
