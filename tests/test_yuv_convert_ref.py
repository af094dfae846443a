"""CPU: the specification of the device-input conversion (tests/yuv_convert_ref.py) against the properties it must have and the floating-point BT.709 / BT.601 formulas."""
from __future__ import annotations

import numpy as np
import pytest

import yuv_convert_ref as ref

CASES = [(m, fr) for m in (ref.MATRIX_BT709, ref.MATRIX_BT601) for fr in (False, True)]


def _float(r, g, b, matrix, full_range):
    Kr, Kb = {ref.MATRIX_BT709: (0.2126, 0.0722), ref.MATRIX_BT601: (0.299, 0.114)}[matrix]
    Kg = 1 - Kr - Kb
    sy, sc, oy = (1.0, 1.0, 0) if full_range else (219 / 255, 224 / 255, 16)
    R, G, B = (np.asarray(c, np.float64) for c in (r, g, b))
    y = sy * (Kr * R + Kg * G + Kb * B) + oy
    cb = sc * (B - (Kr * R + Kg * G + Kb * B)) / (2 * (1 - Kb)) + 128
    cr = sc * (R - (Kr * R + Kg * G + Kb * B)) / (2 * (1 - Kr)) + 128
    return (np.clip(v, 0, 255) for v in (y, cb, cr))


@pytest.mark.parametrize("matrix,full_range", CASES)
def test_grey_is_neutral(matrix, full_range):
    v = np.arange(256, dtype=np.uint8)
    plane = np.repeat(v[None, :], 2, axis=0)                              # 256 greys side by side, two rows
    out = ref.rgb_to_i420(plane, plane, plane, matrix, full_range)
    n = plane.size
    assert (out[n:] == 128).all()
    # a uniform grey picture: chroma exactly 128 whatever the filter sees
    for g in (0, 1, 77, 128, 254, 255):
        p = np.full((4, 8), g, np.uint8)
        o = ref.rgb_to_i420(p, p, p, matrix, full_range)
        assert (o[32:] == 128).all()


@pytest.mark.parametrize("matrix,full_range", CASES)
def test_black_and_white(matrix, full_range):
    for val, lim, full in ((0, 16, 0), (255, 235, 255)):
        p = np.full((2, 2), val, np.uint8)
        o = ref.rgb_to_i420(p, p, p, matrix, full_range)
        assert (o[:4] == (full if full_range else lim)).all() and (o[4:] == 128).all()


@pytest.mark.parametrize("matrix,full_range", CASES)
def test_luma_coefficients_sum_to_the_scale(matrix, full_range):
    k = ref.coefficients(matrix, full_range)
    sy = 1.0 if full_range else 219 / 255
    assert abs(sum(k["cy"]) - round(sy * 65536)) <= 1
    assert abs(sum(k["cb"])) <= 1 and abs(sum(k["cr"])) <= 1


@pytest.mark.parametrize("matrix,full_range", CASES)
def test_luma_of_every_colour_within_one(matrix, full_range):
    c = np.arange(1 << 24, dtype=np.uint32)
    r, g, b = ((c >> s) & 255 for s in (16, 8, 0))
    r, g, b = (x.astype(np.uint8).reshape(4096, 4096) for x in (r, g, b))
    y = ref.rgb_to_i420(r, g, b, matrix, full_range)[: 1 << 24].astype(np.float64)
    yf, _, _ = _float(r.ravel(), g.ravel(), b.ravel(), matrix, full_range)
    assert np.abs(y - yf).max() <= 1.0


@pytest.mark.parametrize("matrix,full_range", CASES)
def test_chroma_of_uniform_blocks_within_one(matrix, full_range):
    rng = np.random.default_rng(matrix * 2 + int(full_range))
    H, W = 256, 512
    blk = rng.integers(0, 256, (3, H // 2, W // 2), dtype=np.uint8)
    blk[:, 0, :8] = [[255], [0], [0]]                                     # saturated primaries and their complements
    blk[:, 1, :8] = [[0], [255], [0]]
    blk[:, 2, :8] = [[0], [0], [255]]
    blk[:, 3, :8] = [[0], [255], [255]]
    blk[:, 4, :8] = [[255], [0], [255]]
    blk[:, 5, :8] = [[255], [255], [0]]
    r, g, b = (np.repeat(np.repeat(x, 2, axis=0), 2, axis=1) for x in blk)   # uniform 2 x 2 blocks
    out = ref.rgb_to_i420(r, g, b, matrix, full_range)
    n = H * W
    cb = out[n:n + n // 4].reshape(H // 2, W // 2).astype(np.float64)
    cr = out[n + n // 4:].reshape(H // 2, W // 2).astype(np.float64)
    # the filter spans the neighbouring blocks horizontally: compare where both neighbours equal the block (here: interior of runs) - and, for every block, against the
    # filtered float value, which is what the integer arithmetic rounds
    _, cbf, crf = _float(*(x.astype(np.float64) for x in _filtered(r, g, b)), matrix, full_range)
    assert np.abs(cb - cbf).max() <= 1.0 and np.abs(cr - crf).max() <= 1.0
    _, cbu, cru = _float(*blk, matrix, full_range)
    same = np.ones_like(cb, bool)
    for x in blk:
        same[:, 1:] &= x[:, 1:] == x[:, :-1]
        same[:, :-1] &= x[:, :-1] == x[:, 1:]
    assert same[:6, 1:7].all()
    assert np.abs(cb - cbu)[same].max() <= 1.0 and np.abs(cr - cru)[same].max() <= 1.0


def _filtered(r, g, b):
    """the chroma filter of the specification in floating point: (1, 2, 1) horizontally at the co-sited columns, the mean of the two rows"""
    def f(C):
        C = C.astype(np.float64)
        left = np.concatenate([C[:, :1], C[:, :-1]], axis=1)
        right = np.concatenate([C[:, 1:], C[:, -1:]], axis=1)
        h = ((left + 2 * C + right) / 4)[:, 0::2]
        return (h[0::2] + h[1::2]) / 2
    return f(r), f(g), f(b)


def test_nv12_deinterleave():
    rng = np.random.default_rng(1)
    y = rng.integers(0, 256, (4, 8), dtype=np.uint8)
    uv = rng.integers(0, 256, (2, 8), dtype=np.uint8)
    o = ref.nv12_to_i420(y, uv)
    assert (o[:32] == y.ravel()).all() and (o[32:40] == uv[:, 0::2].ravel()).all() and (o[40:] == uv[:, 1::2].ravel()).all()
