"""CPU: tests/denoise_ref.py - the specification of the temporal denoiser (`vpp_denoise` / `vpp_recur_filter`) - held to its own rules:
  * no history is the identity; C == P gives O == C; every output sample lies between c and its prediction (so between 0 and 255);
  * a flat picture gives (0, 0) everywhere, a horizontal ramp dy = 0 everywhere (the tie rule: cost, then |dx| + |dy|, then dy, then dx);
  * a pan by (8, -8) is found in the blocks that can see it; a pan by 9 is out of range: those blocks are gated or take another vector;
  * at 16x16 the only candidate is (0, 0); edge blocks are the 8-wide / 8-tall remainder;
  * the chroma prediction's reads stay inside the plane for every valid vector of every block, by index;
  * the levels: vpp_denoise 1 / 2 / 3, vpp_recur_filter alone and on top;
  * the effect on the synthetic clip (104x72, 10 pictures panning (3, 1), Gaussian noise of sigma 4), last picture, PSNR against the clean clip.  Measured with this
    generator: luma 35.96 dB unfiltered -> 36.21 / 37.35 / 39.04 dB at levels 1 / 2 / 3 (gains 0.24 / 1.39 / 3.08 dB); chroma 35.88 dB -> 35.90 / 36.03 / 36.40 dB.  Asserted:
    more than 0.5 dB at level 2, more than 1.5 dB at level 3, chroma never more than 0.1 dB down."""
from __future__ import annotations

import numpy as np
import pytest

import denoise_ref as dr

W, H = 104, 72


def _pack(y, u, v):
    return np.concatenate([np.asarray(q, np.uint8).ravel() for q in (y, u, v)])


def _textured(w, h, seed, ox=0, oy=0):
    """a picture cut out of a larger smooth-ish random field at offset (ox, oy); chroma follows luma"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h + 64, w + 64)).astype(np.float64)
    k = np.ones(3) / 3
    f = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, f)
    y = np.rint(f[32 + oy:32 + oy + h, 32 + ox:32 + ox + w])
    u = np.rint(y[0::2, 0::2] / 2 + 60)
    return _pack(y, u, 250 - u)


def test_no_history_is_the_identity():
    c = _textured(W, H, 1)
    o, b = dr.filter_picture(c, None, W, H, 10, 20)
    assert (o == c).all() and o is not c
    dx, dy, gated = dr.vectors(b)
    assert len(b) == 7 * 5 and (dx == 0).all() and (dy == 0).all() and gated.all() and (b[:, 1] == 0).all()


@pytest.mark.parametrize("thr,wmax", [(6, 16), (16, 24), (1, 1), (64, 30)])
def test_equal_pictures_and_the_blend_s_bounds(thr, wmax):
    c = _textured(W, H, 2)
    o, b = dr.filter_picture(c, c.copy(), W, H, thr, wmax)
    assert (o == c).all() and (b[:, 1] == 0).all()
    # every sample between c and p, over all differences
    cc, pp = np.meshgrid(np.arange(256), np.arange(256))
    o = dr.blend(cc, pp, thr, wmax).astype(np.int32)
    assert (o >= np.minimum(cc, pp)).all() and (o <= np.maximum(cc, pp)).all()
    assert (o[np.abs(cc - pp) >= thr] == cc[np.abs(cc - pp) >= thr]).all(), "no weight from the threshold on"
    # and through the filter: the output lies between the picture and the displaced history, sample by sample
    p = _textured(W, H, 2, 2, 1).astype(np.int32)
    p = np.clip(p + np.random.default_rng(3).integers(-3, 4, p.shape), 0, 255).astype(np.uint8)
    o, b = dr.filter_picture(c, p, W, H, thr, wmax)
    dx, dy, gated = dr.vectors(b)
    oy, cy, py = (dr.planes(x, W, H)[0].astype(np.int32) for x in (o, c, p))
    for (bx, by, bw, bh), x, y, g in zip(dr.block_grid(W, H), dx, dy, gated):
        a, cb = oy[by:by + bh, bx:bx + bw], cy[by:by + bh, bx:bx + bw]
        if g:
            assert (a == cb).all()
        else:
            pb = py[by + y:by + y + bh, bx + x:bx + x + bw]
            assert (a >= np.minimum(cb, pb)).all() and (a <= np.maximum(cb, pb)).all()


def test_flat_and_ramp_ties():
    n = W * H * 3 // 2
    o, b = dr.filter_picture(np.full(n, 90, np.uint8), np.full(n, 93, np.uint8), W, H, 10, 20)
    dx, dy, gated = dr.vectors(b)
    assert (dx == 0).all() and (dy == 0).all() and not gated.any() and (b[:, 1] > 0).all()
    assert set(np.unique(o)) <= {91, 92}, "a flat picture moves towards its history"
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = _pack(2 * xx, xx[::2, ::2], 200 - xx[::2, ::2])
    for hist in (ramp, _pack(2 * xx + 2, xx[::2, ::2], 200 - xx[::2, ::2])):    # the same ramp; the ramp one column on: every dy ties, at equal cost the smaller |dy| wins
        _, b = dr.filter_picture(ramp, hist, W, H, 10, 20)
        dx, dy, _ = dr.vectors(b)
        assert (dy == 0).all()
    grid = dr.block_grid(W, H)
    inner = [i for i, (bx, by, bw, bh) in enumerate(grid) if bx > 0]
    assert (dx[inner] == -1).all(), "the ramp one column on is found one column to the left"
    # dx ties: a vertical ramp, every dx ties -> dx = 0
    vr = _pack(3 * yy, yy[::2, ::2], yy[::2, ::2])
    _, b = dr.filter_picture(vr, vr.copy(), W, H, 10, 20)
    dx, dy, _ = dr.vectors(b)
    assert (dx == 0).all() and (dy == 0).all()


def test_pan_inside_and_outside_the_range():
    grid = dr.block_grid(W, H)
    c = _textured(W, H, 5)
    # the current picture shows what the history shows at (+8, -8)
    p = _textured(W, H, 5, -8, 8)
    _, b = dr.filter_picture(c, p, W, H, 10, 20)
    dx, dy, gated = dr.vectors(b)
    can = [i for i, (bx, by, bw, bh) in enumerate(grid) if bx + 8 + bw <= W and by - 8 >= 0]
    assert len(can) >= 12
    assert (dx[can] == 8).all() and (dy[can] == -8).all() and not gated[can].any() and (b[can, 1] == 0).all()
    p = _textured(W, H, 5, -9, 0)                                       # nine columns: out of range
    _, b = dr.filter_picture(c, p, W, H, 10, 20)
    dx, dy, gated = dr.vectors(b)
    assert (np.abs(dx) <= 8).all() and (np.abs(dy) <= 8).all()
    assert ((b[:, 1] > 0) | (dx != 9)).all() and (gated | (b[:, 1] < 10 * 256)).all()
    assert gated.sum() > len(grid) // 2, "a pan out of range closes the gate in most blocks"


def test_single_block_and_edge_blocks():
    c, p = _textured(16, 16, 7), _textured(16, 16, 7, 1, 0)
    assert [len(x) for x in dr.candidates(0, 0, 16, 16, 16, 16)] == [1, 1]
    _, b = dr.filter_picture(c, p, 16, 16, 64, 30)
    assert tuple(x[0] for x in dr.vectors(b))[:2] == (0, 0)
    assert dr.block_grid(24, 40) == [(0, 0, 16, 16), (16, 0, 8, 16), (0, 16, 16, 16), (16, 16, 8, 16), (0, 32, 16, 8), (16, 32, 8, 8)]
    dx, dy = dr.candidates(16, 32, 8, 8, 24, 40)
    assert dx.max() == 0 and dy.max() == 0 and dx.min() == -8 and dy.min() == -8 and len(dx) == 81
    with pytest.raises(AssertionError):
        dr.filter_picture(np.zeros(20 * 16 * 3 // 2, np.uint8), None, 20, 16, 10, 20)


@pytest.mark.parametrize("w,h", [(16, 16), (24, 40), (104, 72), (8, 8), (40, 24)])
def test_chroma_reads_stay_inside_the_plane(w, h):
    n = 0
    for bx, by, bw, bh in dr.block_grid(w, h):
        dx, dy = dr.candidates(bx, by, bw, bh, w, h)
        assert ((dx == 0) & (dy == 0)).sum() == 1, "(0, 0) is always valid"
        for x, y in zip(dx.tolist(), dy.tolist()):
            x0, x1, y0, y1 = dr.chroma_reads(bx, by, bw, bh, x, y)
            assert 0 <= x0 <= x1 <= w // 2 - 1 and 0 <= y0 <= y1 <= h // 2 - 1, (bx, by, x, y)
            assert x1 - x0 == bw // 2 - 1 + (x & 1) and y1 - y0 == bh // 2 - 1 + (y & 1)
            n += 1
    assert n > 0


def test_levels():
    assert dr.level_params(0, 0) is None
    assert [dr.level_params(k) for k in (1, 2, 3)] == [(6, 16), (10, 20), (16, 24)]
    assert dr.level_params(0, 30) == (10, 30) and dr.level_params(0, 0.2) == (10, 1) and dr.level_params(3, 7.5) == (16, 8) and dr.level_params(1, 12.4) == (6, 12)


def test_effect_on_the_synthetic_clip():
    clean, noisy = dr.synthetic_clip()
    assert len(noisy) == 10 and noisy[0].size == W * H * 3 // 2
    ny = W * H
    base_y, base_c = dr.psnr(clean[-1][:ny], noisy[-1][:ny]), dr.psnr(clean[-1][ny:], noisy[-1][ny:])
    gains = {}
    for lvl in (1, 2, 3):
        out = dr.filter_clip(noisy, W, H, *dr.level_params(lvl))
        gains[lvl] = (dr.psnr(clean[-1][:ny], out[-1][:ny]) - base_y, dr.psnr(clean[-1][ny:], out[-1][ny:]) - base_c)
        print(f"level {lvl}: luma {base_y:.2f} -> {base_y + gains[lvl][0]:.2f} dB, chroma {base_c:.2f} -> {base_c + gains[lvl][1]:.2f} dB")
    assert gains[2][0] > 0.5 and gains[3][0] > 1.5
    assert all(g[1] > -0.1 for g in gains.values())
