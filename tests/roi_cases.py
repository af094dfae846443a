"""Maps for the ROI tests: random offsets salted with the values at which an implementation of tests/roi_map_ref.py can go wrong - ties of the element's rounding
(x.5 / 256), the clip at +-51, non-finite and huge values, -0.0, denormals."""
from __future__ import annotations

import numpy as np

import roi_map_ref as R

F32_SPECIALS = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, -0.0, 0.0, 0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256, -1.5 / 256, -2.5 / 256, 1027.5 / 256, -1027.5 / 256,
                         51.0, -51.0, 51.001, -51.001, 50.998046875, 63.9, 64.0, 1e-40, -1e-40, 2.0 ** -9, 2.0 ** -9 * 1.0000001, 3.4e38, 0.001953125 * 3], np.float32)
I8_SPECIALS = np.array([-128, -52, -51, -50, 0, 50, 51, 52, 127], np.int8)


def special_map(seed: int, width: int, height: int, log2_block: int, dtype) -> np.ndarray:
    """a map of the picture's shape: random values, about one in five a special one"""
    rng = np.random.default_rng(seed)
    rows, cols = R.map_shape(width, height, log2_block)
    if np.dtype(dtype) == np.int8:
        m = rng.integers(-60, 61, (rows, cols)).astype(np.int8)
        sp = I8_SPECIALS
    else:
        m = (rng.integers(-15000, 15001, (rows, cols)) / np.float32(256)).astype(np.float32)          # includes many exact x.0 and, through the / 512 below, x.5 ties
        m[rng.random((rows, cols)) < 0.3] += np.float32(1 / 512)
        sp = F32_SPECIALS
    pick = rng.random((rows, cols)) < 0.2
    m[pick] = sp[rng.integers(0, len(sp), int(pick.sum()))]
    return m


def half_mean_map(width: int, height: int, log2_block: int, k: int) -> np.ndarray:
    """float32 map of log2_block <= 5 whose every whole CTU has a mean of exactly k + 0.5 (in 1/256 QP): all k / 256 except every other element of each row, (k + 1) / 256"""
    rows, cols = R.map_shape(width, height, log2_block)
    m = np.full((rows, cols), k / 256.0, np.float32)
    m[:, 1::2] = (k + 1) / 256.0
    return m
