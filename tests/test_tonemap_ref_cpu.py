"""CPU: the specification of tone mapping on the way in (tests/tonemap_ref.py) - properties of the integer form, the integer form against the float64 model, and the tables
the C host builds (ks265codec_amd/host/ks265_tonemap.h, through tests/tonemap_main.c) against the specification's, entry by entry."""
from __future__ import annotations

import math
import subprocess

import numpy as np
import pytest

import tonemap_ref as tm
import yuv_hibit_ref as yh
from host_harness import build_host_program

CONFIGS = [(c, fr) for c in tm.CURVES.values() for fr in (False, True)]


def planes_of(i420, W, H):
    n = W * H
    return i420[:n].reshape(H, W), i420[n:n + n // 4], i420[n + n // 4:]


def maxima(a, b, W, H):
    """the largest difference per plane, in 8-bit codes"""
    return tuple(int(np.abs(p.astype(np.int32) - q.astype(np.int32)).max()) for p, q in zip(planes_of(a, W, H), planes_of(b, W, H)))


@pytest.mark.parametrize("curve,full", CONFIGS)
@pytest.mark.parametrize("peak", [1000.0, 4000.0])
def test_grey_ramp(curve, full, peak):
    pl = tm.grey_ramp(10)
    H, W = pl[0].shape
    out = tm.to_i420(pl, yh.SEMI, 10, 1, curve, peak, 203.0, full)
    y, u, v = planes_of(out, W, H)
    assert (u == 128).all() and (v == 128).all()                        # neutral in, neutral out: the matrix rows sum to exactly one
    ramp = y.ravel().astype(np.int32)
    assert (np.diff(ramp) >= 0).all()
    assert ramp[0 if full else 64] == 16 and ramp.min() == 16
    # every luma at or above the peak is white
    e = tm.pq_inv(peak)
    first = math.ceil(e * 1023) if full else math.ceil(64 + 876 * e)
    assert (ramp[first:] == 235).all() and ramp.max() == 235
    # and the float64 model is nowhere more than one code away (measured: 1; more would mean fixed-point widths too narrow)
    assert maxima(out, tm.model(pl, yh.SEMI, 10, 1, curve, peak, 203.0, full), W, H) == (1, 0, 0)


def test_clip_with_peak_at_white_leaves_the_greys_below_white():
    pl = tm.grey_ramp(10)
    H, W = pl[0].shape
    out = tm.to_i420(pl, yh.SEMI, 10, 1, tm.CLIP, 203.0, 203.0, False)
    ref = tm.model(pl, yh.SEMI, 10, 1, tm.CLIP, 203.0, 203.0, False)
    white = math.floor(64 + 876 * tm.pq_inv(203.0))                     # the last code below white
    y, r = planes_of(out, W, H)[0].ravel().astype(np.int32), planes_of(ref, W, H)[0].ravel().astype(np.int32)
    assert np.abs(y[:white + 1] - r[:white + 1]).max() <= 1
    assert (y[white + 1:] == 235).all() and y[white // 2] < 235
    # a gain of one below white: the other curves at this setting change nothing either below the knee
    assert (np.asarray(tm.tables(tm.CLIP, 203.0, 203.0)[1]) == tm.G_ONE).all()


@pytest.mark.parametrize("curve,full", CONFIGS)
def test_saturated_primaries_stay_in_range(curve, full):
    W, H = 64, 4
    for depth, layout, msb in ((10, yh.SEMI, 1), (10, yh.PLANAR, 0), (16, yh.SEMI, 1)):
        y, u, v = planes_of(tm.to_i420(tm.primaries(depth, layout, msb, W, H, full), layout, depth, msb, curve, 1000.0, 203.0, full), W, H)
        assert 16 <= y.min() and y.max() <= 235 and 16 <= min(u.min(), v.min()) and max(u.max(), v.max()) <= 240
        assert y.max() == 235 and y.min() == 16                         # the white and the black bar


def test_tables_hold_their_invariants():
    for curve in tm.CURVES.values():
        for peak, white in ((1000.0, 203.0), (4000.0, 203.0), (10000.0, 80.0), (100.0, 100.0)):
            E, G, O, M = tm.tables(curve, peak, white)
            assert (M.sum(axis=1) == tm.M_ONE).all()
            assert (np.diff(E.astype(np.int64)) >= 0).all() and E[0] == 0 and int(E[-1]) == round(peak / white * tm.E_ONE) and int(E[-1]) < 1 << 27
            assert G.max() <= tm.G_ONE and G[0] == tm.G_ONE
            assert (np.diff(O.astype(np.int64)) >= 0).all() and O[0] == 0 and O[4096] == 65280
            # the curve never lifts: the light behind the gain is at most white, up to the rounding of the gain (half a unit of G: a relative 0.5 / G) and of the product;
            # the arithmetic clamps what is left
            assert ((E.astype(np.int64) * G.astype(np.int64) + (1 << 18)) >> 19).max() <= tm.T_ONE * (1 + 0.5 / int(G.min())) + 1


# the integer form against the float64 model on random words - out-of-nominal codes and stray bits included: the largest difference per plane (Y, U, V), as measured
# (CPU arithmetic: exact and repeatable).  DESIGN.md 4v carries the same figures
RANDOM = [(10, yh.SEMI, 1), (10, yh.PLANAR, 0), (12, yh.SEMI, 1), (16, yh.SEMI, 1)]


@pytest.mark.parametrize("depth,layout,msb", RANDOM)
def test_integer_form_against_the_model_on_random_pictures(depth, layout, msb):
    W, H = 64, 48
    rng = np.random.default_rng(1000 + depth + layout)
    worst = np.zeros(3, np.int64)
    for curve, full in CONFIGS:
        pl = yh.random_planes(rng, layout, yh.S420, depth, msb, W, H)
        a = tm.to_i420(pl, layout, depth, msb, curve, 1000.0, 203.0, full)
        b = tm.model(pl, layout, depth, msb, curve, 1000.0, 203.0, full)
        worst = np.maximum(worst, maxima(a, b, W, H))
    assert tuple(worst) == (1, 1, 1)                                    # over the three curves and both ranges


@pytest.fixture(scope="module")
def program():
    return build_host_program("tonemap_main.c")


@pytest.mark.parametrize("curve", sorted(tm.CURVES.values()))
@pytest.mark.parametrize("peak,white", [(1000.0, 203.0), (4000.0, 203.0), (10000.0, 80.0), (203.0, 203.0)])
def test_the_c_host_builds_the_specification_s_tables(program, tmp_path, curve, peak, white):
    pl = yh.random_planes(np.random.default_rng(3), yh.SEMI, yh.S420, 10, 1, 8, 2)
    src = tmp_path / "in"
    src.write_bytes(b"".join(p.tobytes() for p in pl))
    r = subprocess.run([program, "1", "10", "1", "0", str(curve), repr(peak), repr(white), "8", "2", "0", str(src), str(tmp_path / "out"), str(tmp_path / "tab")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = (tmp_path / "tab").read_bytes()
    E, G, O, M = tm.tables(curve, peak, white)
    assert len(raw) == 4096 * 4 + 4096 * 2 + 4097 * 2 + 36
    assert (np.frombuffer(raw, np.uint32, 4096) == E).all()
    assert (np.frombuffer(raw, np.uint16, 4096, 16384) == G).all()
    assert (np.frombuffer(raw, np.uint16, 4097, 24576) == O).all()
    assert (np.frombuffer(raw, np.int32, 9, 24576 + 8194).reshape(3, 3) == M).all()
