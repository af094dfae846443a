"""Specification of the float sample formats of the pixel API (KS265_IN_RGB_F16 / _BF16 / _F32 of include/ks265_hip.h; ks265codec_amd/csrc/input_convert.hip and
output_convert.hip): RGB as float16, bfloat16 or float32 with [0, 1] the full 8-bit range, next to tests/yuv_convert_ref.py (its matrices, its ranges, its Q16 coefficients)
and tests/yuv_output_ref.py.

  input    sample v -> float32 (exact for float16 / bfloat16).  NaN counts 0.
           t = v * 65280.0f (ONE IEEE float32 multiply, round to nearest even); t clamped to [0, 65280]; q = rint(t), ties to even.
           q is the sample in 1 / 256 of an 8-bit code.
           luma     Y  = clip255((cyr qR + cyg qG + cyb qB + (oy << 24) + (1 << 23)) >> 24)
           chroma   S  = the (1, 2, 1) x (1, 1) sum of q at HEVC's default siting, as yuv_convert_ref sums bytes (weight 8)
                    Cb = clip255((cbr SR + cbg SG + cbb SB + (128 << 27) + (1 << 26)) >> 27),  Cr the same with cr*
           int64 throughout (the sums need 36 bits), arithmetic (floor) shifts.
  output   with k the byte tests/yuv_output_ref.py defines for a channel and pixel: the sample is the correctly rounded float32 of k / 255; for float16 and bfloat16 that
           float32 rounded to nearest even.  The fourth element of a four-element pixel is 1.0.

bfloat16 has no NumPy type: such samples travel as their uint16 bit patterns (bf16_to_f32 / f32_to_bf16)."""
from __future__ import annotations

import numpy as np

from yuv_convert_ref import MATRIX_BT601, MATRIX_BT709, coefficients  # noqa: F401
import yuv_output_ref as yo

IN_RGB_F16, IN_RGB_BF16, IN_RGB_F32 = 16, 17, 18
ELEM_SIZE = {IN_RGB_F16: 2, IN_RGB_BF16: 2, IN_RGB_F32: 4}
QMAX = 65280                                                            # 255 * 256


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    """uint16 bit patterns of bfloat16 -> float32 (exact)"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x: np.ndarray) -> np.ndarray:
    """float32 (no NaN) -> the uint16 bit patterns of bfloat16, round to nearest even"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def to_f32(samples: np.ndarray, fmt: int) -> np.ndarray:
    """the samples of a format as float32: float16 / float32 arrays, or uint16 bit patterns for IN_RGB_BF16"""
    if fmt == IN_RGB_BF16:
        return bf16_to_f32(samples)
    assert np.asarray(samples).dtype == (np.float16 if fmt == IN_RGB_F16 else np.float32)
    return np.asarray(samples).astype(np.float32)


def q(v: np.ndarray) -> np.ndarray:
    """float32 samples -> q (int64, 0 .. 65280)"""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        t = v * np.float32(QMAX)                                       # float32 x float32: one IEEE multiply
        t = np.where(t > np.float32(0), t, np.float32(0))              # NaN, -0.0 and everything negative: 0
        t = np.where(t < np.float32(QMAX), t, np.float32(QMAX))
        return np.rint(t).astype(np.int64)                             # ties to even


def _clip255(v: np.ndarray) -> np.ndarray:
    return np.clip(v, 0, 255).astype(np.uint8)


def _chroma_sum(C: np.ndarray) -> np.ndarray:
    left = np.concatenate([C[:, :1], C[:, :-1]], axis=1)
    right = np.concatenate([C[:, 1:], C[:, -1:]], axis=1)
    h = (left + 2 * C + right)[:, 0::2]
    return h[0::2] + h[1::2]


def q_to_i420(qr: np.ndarray, qg: np.ndarray, qb: np.ndarray, matrix: int = MATRIX_BT709, full_range: bool = False) -> np.ndarray:
    """three (H, W) planes of q -> packed I420, one flat uint8 array; W and H even"""
    H, W = qr.shape
    assert W % 2 == 0 and H % 2 == 0 and qg.shape == qr.shape == qb.shape
    k = coefficients(matrix, full_range)
    R, G, B = (np.asarray(c, np.int64) for c in (qr, qg, qb))
    y = _clip255((k["cy"][0] * R + k["cy"][1] * G + k["cy"][2] * B + (k["oy"] << 24) + (1 << 23)) >> 24)
    SR, SG, SB = _chroma_sum(R), _chroma_sum(G), _chroma_sum(B)
    off = (128 << 27) + (1 << 26)
    cb = _clip255((k["cb"][0] * SR + k["cb"][1] * SG + k["cb"][2] * SB + off) >> 27)
    cr = _clip255((k["cr"][0] * SR + k["cr"][1] * SG + k["cr"][2] * SB + off) >> 27)
    return np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])


def rgbf_to_i420(r: np.ndarray, g: np.ndarray, b: np.ndarray, matrix: int = MATRIX_BT709, full_range: bool = False) -> np.ndarray:
    """three (H, W) float32 planes (to_f32 of the samples) -> packed I420"""
    return q_to_i420(q(r), q(g), q(b), matrix, full_range)


def code_to_f32(k: np.ndarray) -> np.ndarray:
    """bytes -> the correctly rounded float32 of k / 255 (the float64 quotient is within 2^-53 relative of k / 255 and no k / 255 lies that close to a float32 tie:
    tests/test_yuv_float_ref.py checks all 256 against exact rational arithmetic)"""
    return (np.asarray(k, np.float64) / 255.0).astype(np.float32)


def code_to_sample(k: np.ndarray, fmt: int) -> np.ndarray:
    """bytes -> the output samples of a format: float32, float16, or uint16 bit patterns of bfloat16"""
    f = code_to_f32(k)
    return f if fmt == IN_RGB_F32 else f.astype(np.float16) if fmt == IN_RGB_F16 else f32_to_bf16(f)


def i420_to_rgbf(i420: np.ndarray, W: int, H: int, fmt: int, matrix: int = MATRIX_BT709, full_range: bool = False):
    """packed I420 -> three (H, W) planes R, G, B of output samples (code_to_sample of tests/yuv_output_ref.py's bytes)"""
    return tuple(code_to_sample(c, fmt) for c in yo.i420_to_rgb(i420, W, H, matrix, full_range))
