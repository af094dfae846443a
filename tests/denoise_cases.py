"""TEST INFRASTRUCTURE: the shapes, parameters and picture contents on which ks265_input_denoise (tests/test_gpu_denoise.py) and its CPU stand-in
(tests/test_denoise_host_cpu.py) are held to tests/denoise_ref.py.
SIZES: 16x16 (one candidate), 24x40 (every block partial), 104x72, 152x40 (two whole 64x16 work-group tiles of the kernel and a partial one in each direction).
PARAMS: (thr, weight) - the three levels, weight 1 and 30, thr 1 and 64."""
from __future__ import annotations

import numpy as np

import denoise_ref as dr

SIZES = [(16, 16), (24, 40), (104, 72), (152, 40)]
PARAMS = [dr.LEVELS[1], dr.LEVELS[2], dr.LEVELS[3], (10, 1), (10, 30), (1, 20), (64, 30)]


def _pack(y, u, v):
    return np.concatenate([np.asarray(q, np.uint8).ravel() for q in (y, u, v)])


def contents(w, h, seed):
    """name -> (current, history)"""
    rng = np.random.default_rng(seed)
    n = w * h * 3 // 2
    base = rng.integers(0, 256, (h + 32, w + 32)).astype(np.float64)
    k = np.ones(3) / 3
    base = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, base)
    yy, xx = np.mgrid[0:h, 0:w]

    def shot(ox, oy, sigma):
        y = base[16 + oy:16 + oy + h, 16 + ox:16 + ox + w]
        u = y[0::2, 0::2] / 2 + 60
        pl = [y, u, 250 - u]
        return _pack(*[np.clip(np.rint(q + rng.normal(0, sigma, q.shape)), 0, 255) for q in pl])

    out = {
        "displaced": (shot(5, -3, 2.0), shot(0, 0, 2.0)),
        "displaced_odd_far": (shot(-8, 7, 1.0), shot(0, 0, 1.0)),
        "noise": (rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)),
        "flat": (np.full(n, 77, np.uint8), np.full(n, 80, np.uint8)),
        "ramp_x": (_pack((2 * xx) % 256, (xx[::2, ::2]) % 256, 255 - xx[::2, ::2] % 256), _pack((2 * xx + 2) % 256, (xx[::2, ::2] + 1) % 256, 255 - xx[::2, ::2] % 256)),
        "ramp_y": (_pack((3 * yy) % 256, yy[::2, ::2] % 256, yy[::2, ::2] % 256), _pack((3 * yy) % 256, yy[::2, ::2] % 256, yy[::2, ::2] % 256)),
        "extremes": (np.repeat(rng.integers(0, 2, (n + 3) // 4), 4)[:n].astype(np.uint8) * 255, np.repeat(rng.integers(0, 2, (n + 5) // 6), 6)[:n].astype(np.uint8) * 255),
    }
    out["extremes_same"] = (out["extremes"][0], out["extremes"][0].copy())
    return out
