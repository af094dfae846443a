"""CPU: the specification of the overlay stage (tests/overlay_ref.py) against tests/yuv_convert_ref.py and against itself, at 72x40, both matrices and both ranges:
  a. A = 0 everywhere, or opacity 0: the picture is unchanged byte for byte;
  b. an opaque overlay over the whole picture IS rgb_to_i420 of that RGB; an opaque overlay at an even offset equals, inside its rectangle, rgb_to_i420 of the overlay as a
     picture of its own, and outside the rectangle no byte changes;
  c. a flat colour blended at random alpha over its own conversion changes nothing (the reference yields deviation 0: asserted as such);
  * slot order matters where two overlays overlap; a clipped overlay equals the cropped overlay; every luma result lies between Y and the overlay's luma;
  * a float32 overlay u8 / 255 is the u8 overlay, and the window clips inside the coded picture without touching the padding."""
from __future__ import annotations

import numpy as np
import pytest

import overlay_ref as ovr
import yuv_convert_ref as yc
import yuv_float_ref as yf

W, H = 72, 40
MODES = [(m, fr) for m in (yc.MATRIX_BT709, yc.MATRIX_BT601) for fr in (False, True)]


def _picture(seed: int, w: int = W, h: int = H) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, w * h * 3 // 2, dtype=np.uint8)


def _rgba(seed: int, w: int, h: int):
    return tuple(np.random.default_rng(seed).integers(0, 256, (4, h, w), dtype=np.uint8))


def _planes(i420: np.ndarray, w: int, h: int):
    n = w * h
    return i420[:n].reshape(h, w), i420[n:n + n // 4].reshape(h // 2, w // 2), i420[n + n // 4:].reshape(h // 2, w // 2)


@pytest.mark.parametrize("matrix,full", MODES)
def test_transparent_changes_nothing(matrix, full):
    pic = _picture(1)
    r, g, b, a = _rgba(2, 24, 16)
    zero = ovr.overlay(r, g, b, np.zeros_like(a), 10, 6, 256, matrix, full)
    off = ovr.overlay(r, g, b, a, 10, 6, 0, matrix, full)
    assert np.array_equal(ovr.blend(pic, W, H, [zero]), pic)
    assert np.array_equal(ovr.blend(pic, W, H, [off]), pic)


@pytest.mark.parametrize("matrix,full", MODES)
def test_opaque_is_the_conversion(matrix, full):
    pic = _picture(3)
    r, g, b, _ = _rgba(4, W, H)
    assert np.array_equal(ovr.blend(pic, W, H, [ovr.overlay(r, g, b, None, 0, 0, 256, matrix, full)]), yc.rgb_to_i420(r, g, b, matrix, full))
    w, h, x, y = 24, 16, 14, 6
    r, g, b, _ = _rgba(5, w, h)
    out = ovr.blend(pic, W, H, [ovr.overlay(r, g, b, np.full((h, w), 255, np.uint8), x, y, 256, matrix, full)])
    own = _planes(yc.rgb_to_i420(r, g, b, matrix, full), w, h)
    for P, Q, O, s in zip(_planes(out, W, H), _planes(pic, W, H), own, (1, 2, 2)):
        assert np.array_equal(P[y // s:(y + h) // s, x // s:(x + w) // s], O)
        mask = np.ones(P.shape, bool)
        mask[y // s:(y + h) // s, x // s:(x + w) // s] = False
        assert np.array_equal(P[mask], Q[mask])


@pytest.mark.parametrize("matrix,full", MODES)
def test_flat_colour_over_its_own_conversion(matrix, full):
    rng = np.random.default_rng(6)
    for _ in range(8):
        col = rng.integers(0, 256, 3)
        r, g, b = (np.full((H, W), c, np.uint8) for c in col)
        pic = yc.rgb_to_i420(r, g, b, matrix, full)
        a = rng.integers(0, 256, (H, W), dtype=np.uint8)
        out = ovr.blend(pic, W, H, [ovr.overlay(r, g, b, a, 0, 0, int(rng.integers(0, 257)), matrix, full)])
        assert int(np.abs(out.astype(int) - pic.astype(int)).max()) == 0


def test_slot_order_matters_on_an_overlap():
    pic = _picture(7)
    a = ovr.overlay(*_rgba(8, 24, 16), 8, 4, 200)
    b = ovr.overlay(*_rgba(9, 24, 16), 20, 12, 256)
    ab, ba = ovr.blend(pic, W, H, [a, b]), ovr.blend(pic, W, H, [b, a])
    assert not np.array_equal(ab, ba)
    assert np.array_equal(ab, ovr.blend_one(ovr.blend_one(pic, W, H, a), W, H, b))
    assert np.array_equal(ovr.blend(pic, W, H, [None, a, None, b]), ab)


@pytest.mark.parametrize("x,y", [(-10, -6), (60, 30), (-10, 30), (60, -6)])
def test_clipped_equals_cropped(x, y):
    """away from the overlay's own left edge (whose chroma column clamps) a clipped overlay is the overlay of its visible part; luma always is"""
    pic = _picture(10)
    w, h = 24, 16
    r, g, b, a = _rgba(11, w, h)
    out = ovr.blend(pic, W, H, [ovr.overlay(r, g, b, a, x, y, 230)])
    c0, c1, r0, r1 = max(0, -x), min(w, W - x), max(0, -y), min(h, H - y)
    crop = ovr.overlay(*(p[r0:r1, c0:c1] for p in (r, g, b, a)), x + c0, y + r0, 230)
    ref = ovr.blend(pic, W, H, [crop])
    n = W * H
    assert np.array_equal(out[:n], ref[:n])
    if c0 == 0:
        assert np.array_equal(out, ref)
    else:                                                                # the cropped overlay's first chroma column clamps where the whole one has a neighbour
        for P, Q in zip(_planes(out, W, H)[1:], _planes(ref, W, H)[1:]):
            assert np.array_equal(P[:, 1:], Q[:, 1:])
    # wholly outside: nothing
    assert np.array_equal(ovr.blend(pic, W, H, [ovr.overlay(r, g, b, a, W, 0), ovr.overlay(r, g, b, a, 0, -h), ovr.overlay(r, g, b, a, -w, H)]), pic)


@pytest.mark.parametrize("matrix,full", MODES)
def test_luma_lies_between_picture_and_overlay(matrix, full):
    pic = _picture(12)
    r, g, b, a = _rgba(13, W, H)
    ov = ovr.overlay(r, g, b, a, 0, 0, 190, matrix, full)
    y0, y1 = pic[:W * H].reshape(H, W).astype(int), ovr.blend(pic, W, H, [ov])[:W * H].reshape(H, W).astype(int)
    lum = ovr.overlay_luma(ov)
    assert np.all(y1 >= np.minimum(y0, lum)) and np.all(y1 <= np.maximum(y0, lum))


def test_float_codes_and_window():
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ovr.codes((u8 / 255).astype(np.float32), yf.IN_RGB_F32), u8)
    assert np.array_equal(ovr.codes(yf.code_to_sample(u8, yf.IN_RGB_F16), yf.IN_RGB_F16), u8)
    odd = np.array([np.nan, -1.0, 0.0, 0.5, 1.0, 7.0, np.inf, -np.inf], np.float32)
    assert list(ovr.codes(odd, yf.IN_RGB_F32)) == [0, 0, 0, 128, 255, 255, 255, 0]
    assert list(ovr.effective_alpha(np.array([0, 1, 128, 255]), 256)) == [0, 1, 128, 255] and int(ovr.effective_alpha(255, 128)) == 128
    # a coded picture of 72 x 40 with a window of 70 x 38: the padding keeps its bytes, the window's bytes are those of the unpadded blend
    pic = _picture(14)
    r, g, b, a = _rgba(15, 24, 16)
    ov = ovr.overlay(r, g, b, a, 56, 30, 256)
    out, full = ovr.blend(pic, W, H, [ov], 70, 38), ovr.blend(pic, W, H, [ov])
    for P, Q, F, s in zip(_planes(out, W, H), _planes(pic, W, H), _planes(full, W, H), (1, 2, 2)):
        assert np.array_equal(P[:38 // s, :70 // s], F[:38 // s, :70 // s])
        assert np.array_equal(P[38 // s:], Q[38 // s:]) and np.array_equal(P[:, 70 // s:], Q[:, 70 // s:])
    assert not np.array_equal(out, pic)
