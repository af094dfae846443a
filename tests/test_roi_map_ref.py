"""CPU: properties of the ROI map specification itself (tests/roi_map_ref.py) - what every implementation is then compared with word for word."""
from __future__ import annotations

import numpy as np
import pytest

import roi_map_ref as R


def _rand_map(rng, w, h, lb, dtype):
    rows, cols = R.map_shape(w, h, lb)
    if dtype == np.int8:
        return rng.integers(-128, 128, (rows, cols)).astype(np.int8)
    return (rng.standard_normal((rows, cols)) * 20).astype(np.float32)


@pytest.mark.parametrize("lb", range(7))
@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_constant_map_gives_that_constant(lb, dtype):
    for w, h in ((64, 64), (200, 136), (72, 72)):
        for c in (-51, -7, 0, 3, 51):
            m = np.full(R.map_shape(w, h, lb), c, dtype)
            assert (R.reduce(m, w, h, lb) == c * 256).all()
    m = np.full(R.map_shape(200, 136, lb), 2.71875, np.float32)            # 696 / 256 exactly
    if dtype == np.float32:
        assert (R.reduce(m, 200, 136, lb) == 696).all()


@pytest.mark.parametrize("lb", range(1, 7))
@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_map_repeated_2x2_one_level_finer_gives_the_same_records(lb, dtype):
    rng = np.random.default_rng(lb)
    w, h = 256, 192                                                        # multiples of 64: every block of the coarse map splits into whole finer ones
    m = _rand_map(rng, w, h, lb, dtype)
    fine = np.repeat(np.repeat(m, 2, axis=0), 2, axis=1)
    assert fine.shape == R.map_shape(w, h, lb - 1)
    assert (R.reduce(fine, w, h, lb - 1) == R.reduce(m, w, h, lb)).all()


@pytest.mark.parametrize("lb", range(7))
def test_int8_and_the_same_integers_as_float32_agree(lb):
    rng = np.random.default_rng(100 + lb)
    for w, h in ((200, 136), (72, 72), (128, 64)):
        m = _rand_map(rng, w, h, lb, np.int8)                              # includes values beyond +-51: both types clip
        assert (R.reduce(m, w, h, lb) == R.reduce(m.astype(np.float32), w, h, lb)).all()


@pytest.mark.parametrize("w,h", [(200, 136), (72, 72)])
@pytest.mark.parametrize("lb", range(7))
def test_partial_ctus_average_only_what_the_map_holds(w, h, lb):
    rng = np.random.default_rng(7 * lb + w)
    m = _rand_map(rng, w, h, lb, np.int8)
    q = np.clip(m.astype(np.int64), -51, 51) * 256
    n = 64 >> lb
    cols, rows = (w + 63) // 64, (h + 63) // 64
    rec = R.reduce(m, w, h, lb)
    assert rec.shape == (rows * cols,) and rec.dtype == np.int32
    for cy in range(rows):
        for cx in range(cols):
            t = q[cy * n:cy * n + n, cx * n:cx * n + n]
            assert t.size > 0
            exact = t.sum() / t.size                                       # |S| < 2^53: exact enough to tell a wrong count from a right one
            assert abs(rec[cy * cols + cx] - exact) <= 0.5
    # 72 x 72 per pixel: the corner CTU holds 8 x 8 elements, the edge ones 64 x 8 and 8 x 64
    if (w, h, lb) == (72, 72, 0):
        m2 = np.zeros((72, 72), np.int8); m2[64:, 64:] = 5; m2[:64, 64:] = -3; m2[64:, :64] = 2
        assert R.reduce(m2, 72, 72, 0).tolist() == [0, -768, 512, 1280]


def test_ties():
    # elements: x.5 / 256 rounds half to even in the element's conversion
    m = np.array([[0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256, -1.5 / 256, -2.5 / 256]], np.float32)
    assert R.to_q8(m).tolist() == [[0, 2, 2, 0, -2, -2]]
    # a CTU of one element (log2_block 6) keeps the element's Q8 value
    assert R.reduce(np.array([[1.5 / 256]], np.float32), 64, 64, 6).tolist() == [2]
    # means of exactly k + 0.5 (in 1/256 QP) round up, towards +inf, for either sign: floor((2 S + cnt) / (2 cnt))
    for k in (-3, -1, 0, 4):
        m = np.full((2, 2), k / 256.0, np.float32); m[0, 0] = (k + 2) / 256.0            # S = 4 k + 2, cnt = 4: mean k + 0.5
        assert R.reduce(m, 64, 64, 5).tolist() == [k + 1]
    m = np.zeros((2, 2), np.int8); m[0, 0] = 1                             # S = 256, cnt 4: 64 exactly
    assert R.reduce(m, 64, 64, 5).tolist() == [64]
    # the combination: base mean + record / 256 of exactly k + 0.5 rounds up
    off = np.full((4, 4), 0.25)
    assert R.ctu_map(np.array([64], np.int32), off, 4, 4, 4, 1, 1, 30, 0, 51).tolist() == [31]       # 0.25 + 0.25 + 0.5 = 1.0
    assert R.ctu_map(np.array([-192], np.int32), off, 4, 4, 4, 1, 1, 30, 0, 51).tolist() == [30]     # 0.25 - 0.75 + 0.5 = 0.0
    assert R.ctu_map(np.array([-193], np.int32), off, 4, 4, 4, 1, 1, 30, 0, 51).tolist() == [29]
    assert R.ctu_map(None, np.full((4, 4), -0.5), 4, 4, 4, 1, 1, 30, 0, 51).tolist() == [30]


def test_non_finite_huge_and_negative_zero():
    m = np.array([[np.nan, np.inf, -np.inf, 1e9, -1e9, -0.0, 51.001, -51.001]], np.float32)
    assert R.to_q8(m).tolist() == [[0, 0, 0, 13056, -13056, 0, 13056, -13056]]
    m8 = np.array([[-128, -52, -51, 51, 52, 127]], np.int8)
    assert R.to_q8(m8).tolist() == [[-13056, -13056, -13056, 13056, 13056, 13056]]
    full = np.full((64, 64), 1e9, np.float32)
    assert R.reduce(full, 64, 64, 0).tolist() == [13056]                   # the largest |S|: 4096 * 13056 < 2^31 / 2
    assert 2 * 4096 * 13056 + 4096 < 2 ** 31


def test_combination_clips_and_matches_the_plain_rule_without_a_record():
    rng = np.random.default_rng(5)
    nx, ny = 13, 9                                                         # 200 x 136 in 16 x 16 blocks
    off = rng.standard_normal((ny, nx)) * 4
    plain = R.ctu_map(None, off, nx, ny, 4, 4, 3, 30, 10, 45)
    assert (R.ctu_map(np.zeros(12, np.int32), off, nx, ny, 4, 4, 3, 30, 10, 45) == plain).all()
    up = R.ctu_map(np.full(12, 20 * 256, np.int32), off, nx, ny, 4, 4, 3, 30, 10, 45)
    assert (up == 42).all()                                                # d clipped to +12
    assert (R.ctu_map(np.full(12, 20 * 256, np.int32), off, nx, ny, 4, 4, 3, 40, 10, 45) == 45).all()
    assert (R.ctu_map(np.full(12, -5 * 256, np.int32), None, 0, 0, 4, 4, 3, 30, 0, 51) == 25).all()


def test_rasteriser_later_rectangles_win():
    m = R.rasterise([(0, 0, 64, 64, -6), (64, 0, 136, 136, 4)], 200, 136)
    assert m.shape == (9, 13) and m.dtype == np.int8
    assert (m[:4, :4] == -6).all() and (m[:, 4:] == 4).all() and (m[4:, :4] == 0).all()
    m = R.rasterise([(0, 0, 200, 136, 3), (17, 17, 1, 1, -2), (500, 0, 10, 10, 9), (-8, -8, 9, 9, 7)], 200, 136)
    assert m[1, 1] == -2 and m[0, 0] == 7 and m[0, 1] == 3 and int((m == 3).sum()) == 9 * 13 - 2
    with pytest.raises(ValueError):
        R.rasterise([(0, 0, 1, 1, 1)] * 9, 64, 64)
