"""Specification of the device-output conversion (ks265codec_amd/csrc/output_convert.hip): packed 8-bit I420 -> RGB in exact integer arithmetic, the counterpart of
tests/yuv_convert_ref.py (its matrices, its ranges, its q).

  matrix   (Kr, Kb) of yuv_convert_ref; Kg = 1 - Kr - Kb
  range    limited: sy = 219/255, sc = 224/255, oy = 16; full: sy = sc = 1, oy = 0
  Q16      q(x) = floor(x * 65536 + 0.5) of  ky = 1 / sy;  rv = 2 (1 - Kr) / sc;  gu = -2 Kb (1 - Kb) / (Kg sc);  gv = -2 Kr (1 - Kr) / (Kg sc);  bu = 2 (1 - Kb) / sc
  chroma   to the luma grid bilinearly at HEVC's default siting (type 0: co-sited horizontally, midway vertically), kept at weight 8 and never rounded on its own.
           For chroma row i of plane C (h x w, indices clamped into the plane):
               v(2i, j) = 3 C(i, j) + C(i - 1, j)        v(2i + 1, j) = 3 C(i, j) + C(i + 1, j)
               C8(r, 2j) = 2 v(r, j)                     C8(r, 2j + 1) = v(r, j) + v(r, j + 1)
  pixel    Y8 = (Y - oy) 8 ky + (1 << 18);  U' = U8 - 1024;  V' = V8 - 1024
           R = clip255((Y8 + rv V') >> 19)   G = clip255((Y8 + gu U' + gv V') >> 19)   B = clip255((Y8 + bu U') >> 19)
  int32 throughout, arithmetic (floor) shifts.
"""
from __future__ import annotations

import numpy as np

from yuv_convert_ref import _K, MATRIX_BT601, MATRIX_BT709  # noqa: F401  (the constants are the input conversion's)


def coefficients(matrix: int = MATRIX_BT709, full_range: bool = False) -> dict:
    """the Q16 coefficients and the luma offset (what the kernel receives as arguments)"""
    Kr, Kb = _K[matrix]
    Kg = 1 - Kr - Kb
    if full_range:
        sy = sc = 1.0
        oy = 0
    else:
        sy, sc, oy = 219 / 255, 224 / 255, 16

    def q(x: float) -> int:
        return int(np.floor(x * 65536 + 0.5))
    return {"ky": q(1 / sy), "rv": q(2 * (1 - Kr) / sc), "gu": q(-2 * Kb * (1 - Kb) / (Kg * sc)), "gv": q(-2 * Kr * (1 - Kr) / (Kg * sc)), "bu": q(2 * (1 - Kb) / sc), "oy": oy}


def planes(i420: np.ndarray, W: int, H: int):
    """Y (H, W), U and V (H/2, W/2) of a packed I420 picture"""
    i420 = np.asarray(i420, np.uint8).ravel()
    n = W * H
    return i420[:n].reshape(H, W), i420[n:n + n // 4].reshape(H // 2, W // 2), i420[n + n // 4:n + n // 2].reshape(H // 2, W // 2)


def chroma8(C: np.ndarray) -> np.ndarray:
    """(h, w) chroma plane -> (2h, 2w) int32 at weight 8"""
    C = np.asarray(C, np.int32)
    up = np.concatenate([C[:1], C[:-1]])                               # row clamp(i - 1)
    down = np.concatenate([C[1:], C[-1:]])                             # row clamp(i + 1)
    v = np.empty((2 * C.shape[0], C.shape[1]), np.int32)
    v[0::2] = 3 * C + up
    v[1::2] = 3 * C + down
    right = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)              # column clamp(j + 1)
    out = np.empty((v.shape[0], 2 * v.shape[1]), np.int32)
    out[:, 0::2] = 2 * v
    out[:, 1::2] = v + right
    return out


def terms(i420: np.ndarray, W: int, H: int, matrix: int = MATRIX_BT709, full_range: bool = False):
    """the three sums in front of the shift (int64, so that a test can hold them to the int32 bound)"""
    k = coefficients(matrix, full_range)
    y, u, v = planes(i420, W, H)
    y8 = (y.astype(np.int64) - k["oy"]) * 8 * k["ky"] + (1 << 18)
    us, vs = chroma8(u).astype(np.int64) - 1024, chroma8(v).astype(np.int64) - 1024
    return y8 + k["rv"] * vs, y8 + k["gu"] * us + k["gv"] * vs, y8 + k["bu"] * us


def i420_to_rgb(i420: np.ndarray, W: int, H: int, matrix: int = MATRIX_BT709, full_range: bool = False):
    """packed I420 -> three (H, W) uint8 planes R, G, B; W and H even"""
    assert W % 2 == 0 and H % 2 == 0
    k = coefficients(matrix, full_range)
    y, u, v = planes(i420, W, H)
    y8 = (y.astype(np.int32) - np.int32(k["oy"])) * np.int32(8 * k["ky"]) + np.int32(1 << 18)
    us, vs = chroma8(u) - np.int32(1024), chroma8(v) - np.int32(1024)
    clip = lambda a: np.clip(a >> 19, 0, 255).astype(np.uint8)
    return clip(y8 + np.int32(k["rv"]) * vs), clip(y8 + np.int32(k["gu"]) * us + np.int32(k["gv"]) * vs), clip(y8 + np.int32(k["bu"]) * us)


def i420_to_nv12(i420: np.ndarray, W: int, H: int) -> np.ndarray:
    """packed I420 -> (H * 3 / 2, W): the luma rows, then H / 2 rows of interleaved U V"""
    y, u, v = planes(i420, W, H)
    uv = np.empty((H // 2, W), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return np.concatenate([y, uv])
