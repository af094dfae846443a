"""CPU: tests/enhance_ref.py - the specification of the edge / colour enhancement (`vpp_edge` / `vpp_color`) - held to its own rules:
  * a flat picture is unchanged; a horizontal ramp of step 4 is unchanged away from its ends (the blur of a linear ramp is the ramp);
  * every output lies inside [mn - over, mx + over] of its 3x3 neighbourhood and |o - S| <= limit, on the shared case list (tests/enhance_cases.py) at every cfg;
  * a 64 | 192 step becomes 62 | 194, 60 | 196 and 56 | 200 at the three levels; the levels order by mean |o - S| on a moving step clip;
  * Gaussian noise of sigma 2 on grey changes 6 - 16 % of the samples (in whole per cent; with this generator 9.4 / 16.1 / 6.3 % at levels 1 / 2 / 3: level 3's wider coring
    lets less noise through than level 2's);
  * colour, over all 65 536 (u, v) pairs at gains 8, 16 and 32: monotone along either axis, never shrinks a component, the clip never binds, grey stays grey, the gain is 1
    at full saturation; at gain 64 the clip would bind (1984 pairs per component), and at 33 already - why the range ends at 32;
  * gain 0 of either half leaves its planes untouched; both 0 is no cfg at all;
  * the 5x5 blur equals the direct 25-tap sum with clamped coordinates."""
from __future__ import annotations

import numpy as np
import pytest

import enhance_ref as er
from enhance_cases import CFGS, SIZES, contents

LEVELS = [er.level_params(k, 0) for k in (1, 2, 3)]


def _pack(y, u, v):
    return np.concatenate([np.asarray(q, np.uint8).ravel() for q in (y, u, v)])


def test_levels_and_ranges():
    assert er.level_params(0, 0) is None
    assert [er.level_params(k, 0) for k in (1, 2, 3)] == [(8, 2, 8, 2, 0), (16, 2, 16, 4, 0), (24, 3, 24, 8, 0)]
    assert [er.level_params(0, k) for k in (1, 2, 3)] == [(0, 0, 0, 0, 8), (0, 0, 0, 0, 16), (0, 0, 0, 0, 32)]
    assert er.level_params(2, 1) == (16, 2, 16, 4, 8)
    assert all(er.check_cfg(c, 8, 8) for c in CFGS)
    for bad in ((0, 0, 0, 0, 0), (65, 0, 1, 0, 0), (-1, 0, 1, 0, 0), (8, 17, 8, 2, 0), (8, 2, 0, 2, 0), (8, 2, 65, 2, 0), (8, 2, 8, 33, 0), (0, 0, 0, 0, 33), (8, 2, 8, -1, 0)):
        assert not er.check_cfg(bad, 8, 8), bad
    for w, h in ((12, 8), (8, 0), (8200, 8), (8, 20)):
        assert not er.check_cfg(CFGS[0], w, h)


def test_flat_and_ramp_are_unchanged():
    w, h = 72, 24
    for cfg in CFGS:
        if not cfg[0]:
            continue
        for v in (0, 77, 255):
            assert (er.enhance_luma(np.full((h, w), v), *cfg[:4]) == v).all()
        ramp = np.tile(4 * np.arange(w)[None, :] % 256, (h, 1))[:, :60]       # 0 .. 236, no wrap
        o = er.enhance_luma(ramp, *cfg[:4])
        assert (o[:, 2:-2] == ramp[:, 2:-2]).all(), cfg


def test_blur_is_the_direct_sum():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 256, (9, 11))
    h, w = s.shape
    v = er.blur256(s)
    for y in range(h):
        for x in range(w):
            d = sum(er.K5[i] * er.K5[j] * int(s[min(max(y + j - 2, 0), h - 1), min(max(x + i - 2, 0), w - 1)]) for i in range(5) for j in range(5))
            assert v[y, x] == d
    assert er.blur256(np.full((8, 8), 255)).max() == 65280


@pytest.mark.parametrize("w,h", SIZES)
def test_halo_and_limit_bounds(w, h):
    changed = 0
    for name, pic in contents(w, h, seed=w + h).items():
        y, u, v = er.planes(pic, w, h)
        mn, mx = er.min_max3(y)
        for cfg in CFGS:
            o3 = er.planes(er.enhance_picture(pic, w, h, cfg), w, h)
            o = o3[0].astype(np.int32)
            if cfg[0]:
                assert (o >= np.maximum(0, mn - cfg[3])).all() and (o <= np.minimum(255, mx + cfg[3])).all(), (name, cfg)
                assert (np.abs(o - y.astype(np.int32)) <= cfg[2]).all(), (name, cfg)
                changed += int((o != y).sum())
            else:
                assert (o3[0] == y).all()
            if not cfg[4]:
                assert (o3[1] == u).all() and (o3[2] == v).all()
    assert changed > 0


def test_step_edge_rows():
    w, h = 32, 16
    y = np.where(np.arange(w)[None, :] >= 16, 192, 64) * np.ones((h, 1), np.int64)
    for cfg, (lo, hi) in zip(LEVELS, ((62, 194), (60, 196), (56, 200))):
        o = er.enhance_luma(y, *cfg[:4])
        assert (o[:, 15] == lo).all() and (o[:, 16] == hi).all(), (cfg, o[0, 12:20])
        assert (o[:, :13] == 64).all() and (o[:, 19:] == 192).all()


def test_levels_order_on_a_step_clip():
    w, h = 72, 40
    yy, xx = np.mgrid[0:h, 0:w]
    means = []
    for cfg in LEVELS:
        tot = 0.0
        for t in range(4):
            y = np.where(xx + yy // 3 >= 20 + 5 * t, 170, 90) + ((xx * 7 + yy * 3 + t) % 3)
            tot += np.abs(er.enhance_luma(y, *cfg[:4]).astype(np.int32) - y).mean()
        means.append(tot)
    assert 0 < means[0] < means[1] < means[2], means


def test_noise_on_grey():
    rng = np.random.default_rng(11)
    y = np.clip(np.rint(128 + rng.normal(0, 2, (136, 208))), 0, 255).astype(np.int32)
    share = [float((er.enhance_luma(y, *cfg[:4]) != y).mean()) for cfg in LEVELS]
    print("share of samples changed by noise of sigma 2 on grey:", share)
    assert all(6 <= round(100 * s) <= 16 for s in share), share             # the specification's figures are whole per cent


@pytest.mark.parametrize("gain", [8, 16, 32])
def test_colour_properties_over_all_pairs(gain):
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    ou, ov = er.color_map(u, v, gain)
    assert ou.min() >= 0 and ou.max() <= 255 and ov.min() >= 0 and ov.max() <= 255, "the clip binds"
    assert (np.diff(ou, axis=0) >= 0).all() and (np.diff(ov, axis=1) >= 0).all(), "not monotone along a component's own axis"
    assert (np.abs(ou - 128) >= np.abs(u - 128)).all() and (np.abs(ov - 128) >= np.abs(v - 128)).all(), "a component shrank"
    assert ou[128, 128] == 128 and ov[128, 128] == 128 and (ou[128, :] == 128).all() and (ov[:, 128] == 128).all(), "grey does not stay grey"
    assert ou[0, 0] == 0 and ou[255, 255] == 255 and ov[0, 255] == 255, "the gain at full saturation is not 1"
    assert (ou != u).any()
    eu, ev = er.enhance_chroma(u, v, gain)
    assert (eu == ou).all() and (ev == ov).all()


def test_colour_gain_64_would_clip():
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    ou, ov = er.color_map(u, v, 64)
    assert int(((ou < 0) | (ou > 255)).sum()) == 1984 == int(((ov < 0) | (ov > 255)).sum())       # per component
    ou, ov = er.color_map(u, v, 33)
    assert ou.max() == 256, "33 is the first gain at which a component leaves 0 .. 255"


def test_gain_zero_leaves_its_planes():
    w, h = 72, 24
    pic = contents(w, h, 5)["noise"]
    y, u, v = er.planes(pic, w, h)
    e = er.planes(er.enhance_picture(pic, w, h, er.level_params(3, 0)), w, h)
    assert (e[1] == u).all() and (e[2] == v).all() and (e[0] != y).any()
    c = er.planes(er.enhance_picture(pic, w, h, er.level_params(0, 3)), w, h)
    assert (c[0] == y).all() and ((c[1] != u).any() or (c[2] != v).any())
    both = er.enhance_picture(pic, w, h, er.level_params(3, 3))
    assert (both == _pack(e[0], c[1], c[2])).all(), "the two halves are independent"
    with pytest.raises(AssertionError):
        er.enhance_picture(pic, w, h, (0, 0, 0, 0, 0))
