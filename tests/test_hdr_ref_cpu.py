"""CPU: the specification of `vpp_hdr` (tests/hdr_ref.py) against itself:
  * params() over a grid - quarter steps of strength, integer sigmas, both iteration counts - stays inside the device ranges, gives the three quoted parameter sets, and a 0
    takes the default;
  * a flat picture is unchanged for every cfg of tests/hdr_cases.py; slope 4096 on noise is the identity (every |dY| >= 1 closes the window; equal neighbours average equals);
  * a pass equals the direct double loop over |ct[j] - ct[x]| <= r;
  * the result does not depend on where the running sums start: filtering a crop with a halo equals the crop of the filtered picture away from the cut - the property the
    kernel's tiling rests on - and holding d to 2481 (above every radius) changes no window;
  * a noisy 40 | 200 step keeps its edge at the defaults and no sample moves by more than 3; chroma is untouched."""
from __future__ import annotations

import numpy as np
import pytest

import hdr_ref as hr
from hdr_cases import CFGS, contents


def test_params_quoted_values_and_ranges():
    assert hr.params(1.0, 3, 20, 15) == (16, 3, 8, (484, 242, 121))
    assert hr.params(5, 2, 100, 100) == (80, 2, 6, (2479, 1239))
    assert hr.params(0.5, 3, 100, 0.01) == (8, 3, 4096, (2419, 1209, 605))
    assert hr.params(0, 0, 0, 0) == hr.params(*hr.DEFAULTS) == (16, 3, 8, (484, 242, 121))
    for q in range(1, 21):
        for iters in (2, 3):
            for ss in range(1, 101):
                for sr in (1, 2, 3, 7, 15, 50, 99, 100):
                    cfg = hr.params(q / 4, iters, ss, sr)
                    assert hr.check_cfg(cfg, 8, 8), (q, iters, ss, sr, cfg)
                    assert cfg[0] == 4 * q and len(cfg[3]) == iters and list(cfg[3]) == sorted(cfg[3], reverse=True)


def test_a_flat_picture_is_unchanged():
    for w, h in ((8, 8), (72, 24)):
        pic = contents(w, h, 3)["flat"]
        for cfg in CFGS:
            assert (hr.hdr_picture(pic, w, h, cfg) == pic).all(), cfg


def test_slope_4096_is_the_identity_on_noise():
    w, h = 136, 40
    pic = contents(w, h, 5)["noise"]
    for cfg in ((80, 3, 4096, (2480, 2480, 2480)), (16, 2, 4096, (484, 242))):
        assert (hr.hdr_picture(pic, w, h, cfg) == pic).all()


def _pass_direct(j, y, slope, r):
    out = np.zeros_like(j)
    for row in range(j.shape[0]):
        ct = [0]
        for x in range(1, j.shape[1]):
            ct.append(ct[-1] + 16 + slope * abs(int(y[row, x]) - int(y[row, x - 1])))
        for x in range(j.shape[1]):
            win = [int(j[row, k]) for k in range(j.shape[1]) if abs(ct[k] - ct[x]) <= r]
            out[row, x] = (2 * sum(win) + len(win)) // (2 * len(win))
    return out


@pytest.mark.parametrize("slope,r", [(0, 16), (8, 484), (6, 2479), (1, 77), (4096, 2480), (0, 2480)])
def test_a_pass_is_the_double_loop(slope, r):
    rng = np.random.default_rng(slope + r)
    y = rng.integers(0, 256, (5, 200))
    y[:, 60:90] = 128 + rng.integers(-2, 3, (5, 30))
    j = rng.integers(0, 4081, y.shape)
    assert (hr.pass_rows(j, hr.transform(y, slope), r) == _pass_direct(j, y, slope, r)).all()


def test_a_crop_with_halo_filters_like_the_picture():
    """one pass: r // 16 samples a side are enough; the sums may start anywhere"""
    rng = np.random.default_rng(11)
    y = (128 + 40 * np.sin(np.arange(900) / 37.0)[None, :] + rng.integers(-4, 5, (3, 900))).astype(np.int64)
    j = 16 * y
    for slope, r in ((8, 484), (0, 2480), (3, 1000)):
        full = hr.pass_rows(j, hr.transform(y, slope), r)
        halo = r // 16
        for x0, x1 in ((0, 256), (256, 512), (644, 900), (300, 301)):
            a, b = max(0, x0 - halo), min(900, x1 + halo)
            part = hr.pass_rows(j[:, a:b], hr.transform(y[:, a:b], slope), r)
            assert (part[:, x0 - a:x1 - a] == full[:, x0:x1]).all(), (slope, r, x0)


def test_holding_d_to_2481_changes_no_window():
    rng = np.random.default_rng(13)
    y = rng.integers(0, 256, (4, 300))
    j = 16 * y
    for slope, r in ((4096, 2480), (40, 2480), (40, 16), (300, 1000)):
        ct = hr.transform(y, slope)
        d = np.minimum(2481, np.diff(ct, axis=1))
        held = np.concatenate([np.zeros((4, 1), np.int64), np.cumsum(d, axis=1)], axis=1)
        assert (hr.pass_rows(j, ct, r) == hr.pass_rows(j, held, r)).all()


def test_a_noisy_step_keeps_its_edge_and_chroma_is_untouched():
    w, h = 136, 40
    rng = np.random.default_rng(17)
    y = np.where(np.arange(w)[None, :] >= 68, 200, 40) + rng.integers(-3, 4, (h, w))
    pic = np.concatenate([y.astype(np.uint8).ravel(), rng.integers(0, 256, w * h // 2, dtype=np.uint8)])
    out = hr.hdr_picture(pic, w, h, hr.params(0, 0, 0, 0))
    oy = out[:w * h].reshape(h, w).astype(int)
    assert np.abs(oy - y).max() <= 3
    assert oy[:, :68].max() < 60 and oy[:, 68:].min() > 180
    assert (out[w * h:] == pic[w * h:]).all()
    strong = hr.hdr_picture(pic, w, h, (80, 3, 8, (484, 242, 121)))
    assert (strong[:w * h] != pic[:w * h]).sum() > w * h // 4 and (strong[w * h:] == pic[w * h:]).all()
