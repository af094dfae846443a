"""CPU: the properties of the device-output conversion's specification (tests/yuv_output_ref.py), for both matrices and both ranges:
gray is exact, flat colours survive the way in (yuv_convert_ref.rgb_to_i420) and back within 1 level, and every intermediate value fits int32 with room to spare."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import yuv_convert_ref as cin
import yuv_output_ref as cout

MODES = [(m, f) for m in (cin.MATRIX_BT709, cin.MATRIX_BT601) for f in (False, True)]


def _i420(y, u, v):
    return np.concatenate([np.asarray(p, np.uint8).ravel() for p in (y, u, v)])


@pytest.mark.parametrize("matrix,full", MODES)
def test_gray_is_exact(matrix, full):
    """U = V = 128 gives R = G = B for every luma value (the chroma terms vanish: 8 x 128 - 1024 = 0), and they are the luma value scaled back to full range"""
    W, H = 32, 16
    y = (np.arange(W * H) % 256).astype(np.uint8).reshape(H, W)
    r, g, b = cout.i420_to_rgb(_i420(y, np.full((H // 2, W // 2), 128), np.full((H // 2, W // 2), 128)), W, H, matrix, full)
    assert (r == g).all() and (g == b).all()
    if full:
        assert (r == y).all()
    else:
        want = np.clip(np.floor((y.astype(np.float64) - 16) * 255 / 219 + 0.5), 0, 255)
        assert np.abs(r.astype(np.int32) - want).max() <= 1 and r.ravel()[16] == 0 and r.ravel()[235] == 255


def _round_trip_error(c, matrix, full):
    W, H = 8, 4
    planes = [np.full((H, W), v, np.uint8) for v in c]
    back = cout.i420_to_rgb(cin.rgb_to_i420(*planes, matrix, full), W, H, matrix, full)
    return max(int(np.abs(back[k].astype(np.int32) - c[k]).max()) for k in range(3))


@pytest.mark.parametrize("matrix,full", MODES)
def test_flat_primaries_come_back_within_one_level(matrix, full):
    """the eight corners of the RGB cube (the primaries, their complements, black, white) through rgb_to_i420 and back"""
    assert max(_round_trip_error(c, matrix, full) for c in itertools.product((0, 255), repeat=3)) <= 1


@pytest.mark.parametrize("matrix,full", MODES)
def test_flat_colours_come_back_within_the_quantisation_of_8_bit_ycbcr(matrix, full):
    """Any flat colour.  The way in rounds Y, Cb and Cr to 8 bits (half a level each), the way back multiplies those errors by its gains and rounds once more: at most
    0.5 ky + 0.5 max(rv, bu) + 0.5 levels.  Full range: 0.5 + 0.5 x 1.86 + 0.5 = 1.93 - an integer error of at most 1; limited range: 0.5 x 1.164 + 0.5 x 2.12 + 0.5 = 2.14 -
    at most 2 (BT.709's bu = 2.112 is the largest gain)."""
    k = cout.coefficients(matrix, full)
    bound = (0.5 * k["ky"] + 0.5 * max(k["rv"], k["bu"])) / 65536 + 0.5
    assert (bound < 2) == full and bound < 3
    worst = max(_round_trip_error(c, matrix, full) for c in itertools.product((0, 37, 64, 128, 191, 230, 255), repeat=3))
    assert worst <= int(bound)


@pytest.mark.parametrize("matrix,full", MODES)
def test_every_sum_fits_int32(matrix, full):
    """the extreme pictures (every plane flat at 0 or 255) and noise: the sums in front of the shift stay below 3e8 in magnitude, far inside int32"""
    W, H = 16, 8
    rng = np.random.default_rng(5)
    worst = 0
    pics = [_i420(np.full((H, W), a), np.full((H // 2, W // 2), b), np.full((H // 2, W // 2), c)) for a, b, c in itertools.product((0, 255), repeat=3)]
    pics += [rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8) for _ in range(8)]
    for p in pics:
        worst = max(worst, max(int(np.abs(t).max()) for t in cout.terms(p, W, H, matrix, full)))
        rgb64 = [np.clip(t >> 19, 0, 255) for t in cout.terms(p, W, H, matrix, full)]
        assert all((a == b).all() for a, b in zip(rgb64, cout.i420_to_rgb(p, W, H, matrix, full))), "the int32 arithmetic equals the int64 one"
    assert worst < 3e8


def test_chroma_interpolation_weights_and_clamps():
    """a single chroma sample of 1 among zeros spreads with weights (1, 3, 3, 1) / 4 vertically x (1, 2, 1) / 2 horizontally, total 8 per luma position summed = 32; at the
    plane's edges the clamped neighbour adds its weight to the edge sample"""
    C = np.zeros((4, 4), np.int32); C[1, 1] = 1
    up = cout.chroma8(C)
    assert up.sum() == 32 and up[2:4, 2].tolist() == [6, 6] and up[1, 2] == 2 and up[4, 2] == 2 and up[2, 1] == 3 and up[2, 3] == 3 and up[1, 1] == 1
    assert (cout.chroma8(np.full((3, 5), 77)) == 8 * 77).all()
    C = np.zeros((2, 2), np.int32); C[0, 0] = 1
    assert cout.chroma8(C)[0].tolist() == [8, 4, 0, 0] and cout.chroma8(C)[:, 0].tolist() == [8, 6, 2, 0]


def test_coefficients_are_the_documented_integers():
    k = cout.coefficients(cin.MATRIX_BT709, False)
    assert k == {"ky": 76309, "rv": 117489, "gu": -13975, "gv": -34925, "bu": 138438, "oy": 16}
    assert cout.coefficients(cin.MATRIX_BT601, True) == {"ky": 65536, "rv": 91881, "gu": -22553, "gv": -46802, "bu": 116130, "oy": 0}
