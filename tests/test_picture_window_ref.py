"""CPU: tests/picture_window_ref.py, the specification of ragged picture sizes, against cases written out by hand."""
from __future__ import annotations

import numpy as np

import picture_window_ref as pw


def test_coded_sizes_and_windows_of_the_reference():
    # what the reference's encoder wrote into its SPS for these sources
    assert pw.coded_size(854, 480) == (856, 480) and pw.conf_window(854, 480) == (0, 1, 0, 0)
    assert pw.coded_size(960, 540) == (960, 544) and pw.conf_window(960, 540) == (0, 0, 0, 2)
    assert pw.coded_size(250, 130) == (256, 136) and pw.conf_window(250, 130) == (0, 3, 0, 3)
    assert pw.coded_size(128, 72) == (128, 72) and pw.conf_window(128, 72) == (0, 0, 0, 0)
    assert pw.coded_size(2, 2) == (8, 8)


def test_pad_by_hand_6x2():
    y = np.array([[1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12]], np.uint8)
    u = np.array([[20, 21, 22]], np.uint8)
    v = np.array([[30, 31, 32]], np.uint8)
    got = pw.pad_i420(pw.pack([y, u, v]), 6, 2)
    gy, gu, gv = pw.planes(got, 8, 8)
    assert gy[0].tolist() == [1, 2, 3, 4, 5, 6, 6, 6]
    for r in range(1, 8):
        assert gy[r].tolist() == [7, 8, 9, 10, 11, 12, 12, 12]
    assert (gu == np.array([20, 21, 22, 22], np.uint8)).all() and gu.shape == (4, 4)
    assert (gv == np.array([30, 31, 32, 32], np.uint8)).all() and gv.shape == (4, 4)


def test_pad_2x2_fills_one_cu():
    got = pw.pad_i420(np.array([1, 2, 3, 4, 9, 17], np.uint8), 2, 2)
    gy, gu, gv = pw.planes(got, 8, 8)
    assert gy[0].tolist() == [1] + [2] * 7 and all(gy[r].tolist() == [3] + [4] * 7 for r in range(1, 8))
    assert (gu == 9).all() and (gv == 17).all()


def test_padded_250x130_is_256x136_and_crops_back():
    rng = np.random.default_rng(1)
    pic = rng.integers(0, 256, 250 * 130 * 3 // 2, dtype=np.uint8)
    pad = pw.pad_i420(pic, 250, 130)
    assert pad.size == 256 * 136 * 3 // 2
    py, pu, pv = pw.planes(pad, 256, 136)
    sy, su, sv = pw.planes(pic, 250, 130)
    assert (py[:130, :250] == sy).all() and (py[:130, 250:] == sy[:, -1:]).all() and (py[130:, :250] == sy[-1]).all() and (py[130:, 250:] == sy[-1, -1]).all()
    assert (pu[:65, :125] == su).all() and (pu[:65, 125:] == su[:, -1:]).all() and (pu[65:, :125] == su[-1]).all()
    assert (pv[65:, 125:] == sv[-1, -1]).all()
    assert (pw.crop_i420(pad, 256, 136, 250, 130) == pic).all()


def test_a_multiple_of_8_is_left_alone():
    pic = np.random.default_rng(2).integers(0, 256, 16 * 8 * 3 // 2, dtype=np.uint8)
    assert (pw.pad_i420(pic, 16, 8) == pic).all() and (pw.crop_i420(pic, 16, 8, 16, 8) == pic).all()


def test_nv12_is_deinterleaved():
    y = np.arange(16, dtype=np.uint8).reshape(2, 8)[:, :6]
    uv = np.array([[1, 101, 2, 102, 3, 103]], np.uint8)
    got = pw.pad_planes(pw.nv12_planes(y, uv), 6, 2)
    _, gu, gv = pw.planes(got, 8, 8)
    assert gu[0].tolist() == [1, 2, 3, 3] and gv[3].tolist() == [101, 102, 103, 103]


def test_window_sse_plus_strip_sse_is_the_coded_sse():
    rng = np.random.default_rng(3)
    for w, h in ((250, 130), (854, 480), (480, 270), (2, 2), (10, 2)):
        cw, ch = pw.coded_size(w, h)
        a, b = (rng.integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8) for _ in range(2))
        win, strips, whole = pw.sse_window(a, b, cw, ch, w, h), pw.sse_strips(a, b, cw, ch, w, h), pw.sse3(a, b, cw, ch)
        assert [x + y for x, y in zip(win, strips)] == whole
        assert all(s > 0 for s in strips)


def test_sse_by_hand():
    a = np.zeros(8 * 8 * 3 // 2, np.uint8)
    b = a.copy()
    pw.planes(b, 8, 8)[0][0, 0] = 3            # inside a 6 x 6 window
    pw.planes(b, 8, 8)[0][7, 0] = 2            # below it
    pw.planes(b, 8, 8)[0][0, 6] = 5            # right of it
    pw.planes(b, 8, 8)[1][3, 3] = 4            # chroma: outside the 3 x 3 window
    pw.planes(b, 8, 8)[2][2, 2] = 7            # chroma: inside
    assert pw.sse3(a, b, 8, 8) == [9 + 4 + 25, 16, 49]
    assert pw.sse_window(a, b, 8, 8, 6, 6) == [9, 0, 49]
    assert pw.sse_strips(a, b, 8, 8, 6, 6) == [29, 16, 0]
    assert pw.psnr(0, 10) == 99.0 and abs(pw.psnr(255 * 255, 1)) < 1e-12
