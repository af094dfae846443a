"""CPU: the specification of the float sample formats (tests/yuv_float_ref.py) itself - the properties the kernels and the stand-in are then held to:
  * float32 is exact: q(float32(k) / 255) = 256 k, so a picture u8 / 255 converts to the bytes of u8, both matrices and both ranges;
  * ties go to even, NaN / infinities / -0.0 / negatives / values above 1 / denormals land where the definition says;
  * the float16 and bfloat16 images of k / 255 stay within one code of the uint8 result;
  * the float route is closer to real-valued arithmetic than the route by way of uint8;
  * the way back is byte / 255 correctly rounded, for all 256 codes."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import yuv_convert_ref as cref
import yuv_float_ref as fref
import yuv_output_ref as oref

CASES = [(m, f) for m in (cref.MATRIX_BT709, cref.MATRIX_BT601) for f in (False, True)]


def _u8_picture(W, H, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    for k, (r, g, b) in enumerate([(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]):   # saturated corners
        y, x = (k // 4) * (H - 4), (k % 4) * (W // 4)
        p[0, y:y + 4, x:x + 4], p[1, y:y + 4, x:x + 4], p[2, y:y + 4, x:x + 4] = r, g, b
    return p


def _div255(u8):
    return u8.astype(np.float32) / np.float32(255)


def test_float32_codes_are_exact():
    k = np.arange(256, dtype=np.uint8)
    assert (fref.q(_div255(k)) == 256 * np.arange(256)).all()


@pytest.mark.parametrize("matrix,full", CASES)
def test_float32_picture_of_u8_gives_the_u8_bytes(matrix, full):
    p = _u8_picture(64, 48, 5 + matrix)
    assert (fref.rgbf_to_i420(*_div255(p), matrix, full) == cref.rgb_to_i420(*p, matrix, full)).all()


def test_ties_round_to_even():
    assert fref.q(np.float32([1 / 512, 3 / 512])).tolist() == [128, 382]              # 127.5 -> 128, 382.5 -> 382
    assert fref.q(np.float32([5 / 512, 7 / 512])).tolist() == [638, 892]              # 637.5 -> 638, 892.5 -> 892


def test_special_values():
    f16_den = np.array([1, 0x3FF], np.uint16).view(np.float16).astype(np.float32)      # the smallest and the largest float16 denormal: normal float32 values
    v = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -1e-30, 1.0, 1.0000001, 2.0, 3e38, 1e-45, 1.1754942e-38])
    assert fref.q(v).tolist() == [0, 65280, 0, 0, 0, 0, 0, 65280, 65280, 65280, 65280, 0, 0]
    assert fref.q(f16_den).tolist() == [0, 4]                                          # 2^-24 x 65280 = 0.0039; 1023 x 2^-24 x 65280 = 3.98
    nan_bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert fref.q(nan_bits).tolist() == [0, 0, 0, 0]
    # a picture of NaN is a picture of black
    z = np.full((4, 8), np.nan, np.float32)
    assert (fref.rgbf_to_i420(z, z, z) == cref.rgb_to_i420(*(np.zeros((3, 4, 8), np.uint8)))).all()


def test_sums_need_more_than_32_bits():
    k = cref.coefficients(cref.MATRIX_BT709, True)
    assert sum(k["cy"]) * fref.QMAX + (1 << 23) > 2 ** 31
    assert k["cb"][2] * 8 * fref.QMAX + (128 << 27) > 2 ** 32


@pytest.mark.parametrize("matrix,full", CASES)
def test_sixteen_bit_types_within_one_code(matrix, full):
    p = _u8_picture(64, 48, 9 + matrix)
    exp = cref.rgb_to_i420(*p, matrix, full).astype(np.int32)
    f = _div255(p)
    h = f.astype(np.float16)
    b = fref.f32_to_bf16(f)
    assert np.abs(fref.q(fref.to_f32(h, fref.IN_RGB_F16)) - 256 * p.astype(np.int64)).max() <= 16
    assert np.abs(fref.q(fref.to_f32(b, fref.IN_RGB_BF16)) - 256 * p.astype(np.int64)).max() <= 127
    for fmt, s in ((fref.IN_RGB_F16, h), (fref.IN_RGB_BF16, b)):
        got = fref.rgbf_to_i420(*fref.to_f32(s, fmt), matrix, full).astype(np.int32)
        d = np.abs(got - exp)
        print(f"format {fmt} matrix {matrix} full {full}: {100.0 * (d != 0).mean():.2f} % of the bytes differ")
        assert d.max() <= 1


def test_float_route_is_closer_to_real_arithmetic_than_the_uint8_route():
    rng = np.random.default_rng(1)
    H, W = 64, 96
    x = rng.random((3, H, W), dtype=np.float32)
    Kr, Kb = 0.2126, 0.0722
    real = 16 + 219 * (Kr * x[0].astype(np.float64) + (1 - Kr - Kb) * x[1] + Kb * x[2])
    yf = fref.rgbf_to_i420(*x)[:W * H].reshape(H, W)
    u8 = np.clip(np.rint(x.astype(np.float64) * 255), 0, 255).astype(np.uint8)
    yu = cref.rgb_to_i420(*u8)[:W * H].reshape(H, W)
    ef, eu = np.abs(yf - real).mean(), np.abs(yu - real).mean()
    print(f"mean |luma error|: float route {ef:.4f}, uint8 route {eu:.4f}")
    assert ef < eu


def test_output_is_the_byte_over_255_correctly_rounded():
    k = np.arange(256)
    f = fref.code_to_f32(k)
    for i in k:                                                         # exact: the float32 neighbours are no closer to i / 255
        x, t = Fraction(float(f[i])), Fraction(int(i), 255)
        lo, hi = Fraction(float(np.nextafter(f[i], np.float32(-1)))), Fraction(float(np.nextafter(f[i], np.float32(2))))
        assert abs(x - t) < abs(lo - t) and abs(x - t) < abs(hi - t)
    assert (f * np.float32(255) == k).all()                             # recon * 255 gives the uint8 reconstruction back, exactly
    import torch
    assert (torch.arange(256, dtype=torch.uint8).float().div(255).numpy() == f).all()
    assert (fref.code_to_sample(k, fref.IN_RGB_F16) == f.astype(np.float16)).all()
    assert (fref.code_to_sample(k, fref.IN_RGB_BF16) == torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).all()
    assert np.abs(fref.code_to_sample(k, fref.IN_RGB_F16).astype(np.float32) * 255 - k).max() <= 255 * 2.0 ** -11
    assert np.abs(fref.bf16_to_f32(fref.code_to_sample(k, fref.IN_RGB_BF16)) * 255 - k).max() <= 255 * 2.0 ** -8


@pytest.mark.parametrize("matrix,full", CASES)
def test_output_definition_against_yuv_output_ref(matrix, full):
    W, H = 32, 16
    ramp = np.concatenate([np.arange(W * H, dtype=np.int64) % 256, np.full(W * H // 2, 128)]).astype(np.uint8)   # a grey ramp: every channel through many codes
    rnd = np.random.default_rng(3).integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    for pic in (ramp, rnd):
        u8 = oref.i420_to_rgb(pic, W, H, matrix, full)
        for fmt in (fref.IN_RGB_F16, fref.IN_RGB_BF16, fref.IN_RGB_F32):
            got = fref.i420_to_rgbf(pic, W, H, fmt, matrix, full)
            for c in range(3):
                f = fref.to_f32(got[c], fmt) if fmt != fref.IN_RGB_F32 else got[c]
                assert (np.rint(f * np.float32(255)).astype(np.uint8) == u8[c]).all()
                if fmt == fref.IN_RGB_F32:
                    assert (got[c] == u8[c].astype(np.float32) / np.float32(255)).all()
    if full:
        u8 = oref.i420_to_rgb(ramp, W, H, matrix, True)
        assert all(len(np.unique(c)) == 256 for c in u8), "the full-range grey ramp drives every channel through all 256 codes"
