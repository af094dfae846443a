"""TEST INFRASTRUCTURE: the shapes, parameters and picture contents on which ks265_input_enhance (tests/test_gpu_enhance.py) and its CPU stand-in
(tests/test_enhance_host_cpu.py) are held to tests/enhance_ref.py.
SIZES: 8x8 (a partial tile where every neighbourhood clamps), 72x24 (one 64x16 work-group tile of the kernel plus 8-column and 8-row remainders, chroma rows of 36 bytes),
136x40 (interior tile seams both ways).
CFGS: every pair of levels (edge 0 .. 3 x colour 0 .. 3 without 0 / 0: edge-only and colour-only among them) and the corners of the parameter ranges.
contents(): uniform noise; flats of 0 / 77 / 255; steps 0 | 255 - vertical, horizontal, diagonal - on the tile seams (x = 63 | 64, y = 15 | 16; at a smaller size in the
middle); single-sample impulses at the four corners and at the seams, white on black and black on white; a checkerboard.  The chroma planes: noise, the extremes 0 / 128 / 255
in every pairing, and ramps."""
from __future__ import annotations

import numpy as np

import enhance_ref as er

SIZES = [(8, 8), (72, 24), (136, 40)]
CFGS = [er.level_params(e, c) for e in range(4) for c in range(4) if e or c] + [
    (64, 0, 64, 0, 32), (64, 0, 64, 32, 1), (1, 0, 1, 0, 0), (64, 16, 64, 32, 0), (37, 1, 5, 3, 29)]


def _pack(y, u, v):
    return np.concatenate([np.asarray(q, np.uint8).ravel() for q in (y, u, v)])


def contents(w, h, seed):
    """name -> packed picture"""
    rng = np.random.default_rng(seed)
    cw, ch = w // 2, h // 2
    sx, sy = (64 if w > 64 else w // 2), (16 if h > 16 else h // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ch, 0:cw]
    noise_c = lambda: rng.integers(0, 256, (ch, cw))
    ext = np.array([0, 128, 255, 1, 127, 129, 254])
    ext_u, ext_v = ext[(cx + cy) % 7], ext[(cx // 7 + 3 * cy) % 7]
    ramp_u, ramp_v = (cx * 255) // max(1, cw - 1), 255 - (cy * 255) // max(1, ch - 1)
    out = {"noise": _pack(rng.integers(0, 256, (h, w)), noise_c(), noise_c())}
    for v in (0, 77, 255):
        out[f"flat{v}"] = _pack(np.full((h, w), v), np.full((ch, cw), v), np.full((ch, cw), 255 - v))
    out["step_v"] = _pack(255 * (xx >= sx), ext_u, ext_v)
    out["step_h"] = _pack(255 * (yy >= sy), ramp_u, ramp_v)
    out["step_d"] = _pack(255 * (xx - sx >= yy - sy), noise_c(), ext_v)
    out["step_d_inv"] = _pack(255 * (xx - sx + yy - sy < 0), ext_u, noise_c())
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (sx - 1, sy - 1), (sx, sy), (sx - 1, min(h - 1, sy + 3)), (min(w - 1, sx + 3), sy - 1), (sx, 0), (0, sy), (w - 1, sy - 1), (sx - 1, h - 1)]
    for name, bg in (("impulses", 0), ("impulses_inv", 255)):
        y = np.full((h, w), bg)
        for x0, y0 in spots:
            y[y0, x0] = 255 - bg
        out[name] = _pack(y, ramp_v, ramp_u)
    out["checker"] = _pack(255 * ((xx + yy) & 1), 255 * ((cx + cy) & 1), 255 * (cx & 1))
    out["soft"] = _pack(np.clip(128 + 60 * np.sin(0.21 * xx) * np.cos(0.17 * yy) + rng.normal(0, 2, (h, w)), 0, 255), np.clip(128 + rng.normal(0, 30, (ch, cw)), 0, 255), np.clip(128 + rng.normal(0, 30, (ch, cw)), 0, 255))
    return out
