"""TEST INFRASTRUCTURE: the shapes, parameters and picture contents on which ks265_input_hdr (tests/test_gpu_hdr.py) and its CPU stand-in (tests/test_hdr_host_cpu.py) are
held to tests/hdr_ref.py.
SIZES: 8x8 (every window is cut by the picture), 72x24 and 136x40 (the enhancement's sizes: a 16-line group plus an 8-line remainder both ways), 1288x16 and 16x1288, 8192x8
and 8x8192 (the longest lines the running sums can meet).  The kernel's tile is 16 lines by 240 samples along the pass with a halo of radius / 16 <= 155 samples a side: 1288
= 5 tiles + 88, so a line has interior tiles whose both halos lie in neighbours (3 x 240 + 2 x 155 = 1030 <= 1288), tiles cut by either end of the line and a ragged last
tile; 16 lines across is one full group, 8 is the half-filled one.  The radii of CFGS fall on both sides of the kernel's two builds (halo <= 38 and above).
CFGS: the defaults, the corners of every range (gain 1 / 80, slope 0 / 4096, radius 16 / 2480, iters 2 / 3) and the three parameter sets of the specification, through params.
contents(): flat; a ramp; a noisy step at a tile seam (239 | 240 both ways, in the middle of a smaller picture); uniform noise; columns and rows alternating 0 / 255 (the
largest ct); noise with saturated blocks."""
from __future__ import annotations

import numpy as np

import hdr_ref as hr

SIZES = [(8, 8), (72, 24), (136, 40), (1288, 16), (16, 1288), (8192, 8), (8, 8192)]
CFGS = [hr.params(0, 0, 0, 0), hr.params(1.0, 3, 20, 15), hr.params(5, 2, 100, 100), hr.params(0.5, 3, 100, 0.01),
        (1, 2, 0, (16, 16)), (80, 3, 4096, (2480, 2480, 2480)), (80, 2, 0, (2480, 16)), (1, 3, 4096, (16, 2480, 16)), (80, 3, 0, (2480, 2480, 2480)), (37, 3, 1, (2480, 1000, 77))]


def _pack(y, w, h, rng):
    return np.concatenate([np.asarray(y, np.uint8).ravel(), rng.integers(0, 256, w * h // 2, dtype=np.uint8)])


def contents(w, h, seed):
    """name -> packed picture (the chroma is noise: it must come back as it went in)"""
    rng = np.random.default_rng(seed)
    sx, sy = (240 if w > 240 else w // 2), (240 if h > 240 else h // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"flat": _pack(np.full((h, w), 93), w, h, rng)}
    out["ramp"] = _pack((xx * 255) // max(1, w - 1) // 2 + (yy * 255) // max(1, h - 1) // 2, w, h, rng)
    out["step"] = _pack(np.clip(np.where((xx >= sx) ^ (yy >= sy), 200, 40) + rng.integers(-3, 4, (h, w)), 0, 255), w, h, rng)
    out["noise"] = _pack(rng.integers(0, 256, (h, w)), w, h, rng)
    out["stripes_v"] = _pack(255 * (xx & 1), w, h, rng)
    out["stripes_h"] = _pack(255 * (yy & 1), w, h, rng)
    y = rng.integers(0, 256, (h, w))
    y[(xx // 5 + yy // 3) % 4 == 0] = 255
    y[(xx // 7 + yy // 5) % 5 == 0] = 0
    out["blocks"] = _pack(y, w, h, rng)
    return out
