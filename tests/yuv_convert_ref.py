"""Specification of the device-input conversion (ks265codec_amd/csrc/input_convert.hip): 8-bit RGB -> packed I420 in exact integer arithmetic.

  matrix   BT.709 (Kr, Kb) = (0.2126, 0.0722), BT.601 (0.299, 0.114); Kg = 1 - Kr - Kb
  range    limited: sy = 219/255, sc = 224/255, oy = 16; full: sy = sc = 1, oy = 0
  Q16      floor(x * 65536 + 0.5) of  cy* = sy (Kr, Kg, Kb);  cb* = (-sc Kr / (2 (1 - Kb)), -sc Kg / (2 (1 - Kb)), sc / 2);
                                      cr* = (sc / 2, -sc Kg / (2 (1 - Kr)), -sc Kb / (2 (1 - Kr)))
  luma     Y = clip255((cyr R + cyg G + cyb B + (oy << 16) + 32768) >> 16)
  chroma   HEVC's default chroma siting (type 0: co-sited horizontally, midway vertically): for sample (i, j)
           S = sum over dy in {0, 1}, dx in {-1, 0, 1} of (1, 2, 1)[dx] * C(2i + dy, clamp(2j + dx, 0, W - 1))   (weight 8, per component)
           Cb = clip255((cbr SR + cbg SG + cbb SB + (128 << 19) + (1 << 18)) >> 19), Cr the same with cr*
  int32 throughout, arithmetic (floor) shifts.
"""
from __future__ import annotations

import numpy as np

MATRIX_BT709, MATRIX_BT601 = 0, 1
_K = {MATRIX_BT709: (0.2126, 0.0722), MATRIX_BT601: (0.299, 0.114)}


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
    return {"cy": (q(sy * Kr), q(sy * Kg), q(sy * Kb)),
            "cb": (q(-sc * Kr / (2 * (1 - Kb))), q(-sc * Kg / (2 * (1 - Kb))), q(sc / 2)),
            "cr": (q(sc / 2), q(-sc * Kg / (2 * (1 - Kr))), q(-sc * Kb / (2 * (1 - Kr)))),
            "oy": oy}


def _clip255(v: np.ndarray) -> np.ndarray:
    return np.clip(v, 0, 255).astype(np.uint8)


def rgb_to_i420(r: np.ndarray, g: np.ndarray, b: np.ndarray, matrix: int = MATRIX_BT709, full_range: bool = False) -> np.ndarray:
    """three (H, W) uint8 planes -> packed I420 (Y W x H, then U and V W/2 x H/2), one flat uint8 array; W and H even"""
    H, W = r.shape
    assert W % 2 == 0 and H % 2 == 0 and g.shape == r.shape == b.shape
    k = coefficients(matrix, full_range)
    R, G, B = (np.asarray(c, np.int32) for c in (r, g, b))
    cyr, cyg, cyb = (np.int32(c) for c in k["cy"])
    y = _clip255((cyr * R + cyg * G + cyb * B + np.int32(k["oy"] << 16) + np.int32(32768)) >> 16)

    def chroma_sum(C: np.ndarray) -> np.ndarray:
        left = np.concatenate([C[:, :1], C[:, :-1]], axis=1)          # column clamp(x - 1, 0, W - 1)
        right = np.concatenate([C[:, 1:], C[:, -1:]], axis=1)         # column clamp(x + 1, 0, W - 1)
        h = left + 2 * C + right                                       # horizontal (1, 2, 1) at every column
        h = h[:, 0::2]                                                 # at the co-sited columns 2j
        return h[0::2] + h[1::2]                                       # rows 2i and 2i + 1
    SR, SG, SB = chroma_sum(R), chroma_sum(G), chroma_sum(B)
    off = np.int32((128 << 19) + (1 << 18))
    cb = _clip255((np.int32(k["cb"][0]) * SR + np.int32(k["cb"][1]) * SG + np.int32(k["cb"][2]) * SB + off) >> 19)
    cr = _clip255((np.int32(k["cr"][0]) * SR + np.int32(k["cr"][1]) * SG + np.int32(k["cr"][2]) * SB + off) >> 19)
    return np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])


def nv12_to_i420(y: np.ndarray, uv: np.ndarray) -> np.ndarray:
    """(H, W) luma + (H/2, W) interleaved chroma -> packed I420"""
    return np.concatenate([y.ravel(), uv[:, 0::2].ravel(), uv[:, 1::2].ravel()])
