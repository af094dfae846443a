"""tests/ssim_ref.py against the reference's own printed ` ssim:` numbers (tests/golden/ssim_ref.npz, written by tests/golden/gen_ssim_golden.py from `appencoder -ssim` runs):
the definition is accepted only if it reproduces every printed number of every case - plane sizes that are no multiple of 8 and multi-picture runs included."""
import re

import numpy as np
import pytest

import ssim_ref
from golden_io import load_cases

CASES = load_cases("ssim_ref")
BOUND = 6e-5                     # half a unit of the last printed digit (four decimals) + float slack
LINE = rb"\t ssim: \d+\.\d{4}\t\d\.\d{4}\t\d\.\d{4}\t\d\.\d{4}\n"


def _name(c):
    return bytes(c["name"]).decode()


def test_fixture_covers_the_questions():
    names = {_name(c) for c in CASES}
    sizes = {(c["W"], c["H"]) for c in CASES}
    assert {(64, 64), (72, 40), (136, 72), (200, 136)} <= sizes          # chroma 36x20, 68x36, 100x68: partial windows both ways
    assert any(c["N"] > 1 for c in CASES) and "flat_64x64" in names and "smooth_64x64_qp4" in names


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_spec_reproduces_printed_numbers(case):
    got = ssim_ref.stream_ssim(case["src"], case["rec"], case["W"], case["H"])
    diff = np.abs(got - case["printed"][1:])
    print(_name(case), "spec", got, "printed", case["printed"][1:], "max |diff|", diff.max())
    assert (diff <= BOUND).all()


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_line_format(case):
    line = case["line"].tobytes()
    assert re.fullmatch(LINE, line), line
    assert line == b"\t ssim: %.4f\t%.4f\t%.4f\t%.4f\n" % tuple(case["printed"])


def test_partial_windows_are_dropped():
    """100x68 chroma: 12 x 8 whole windows; the last 4 columns / rows enter no window"""
    c = next(c for c in CASES if (c["W"], c["H"]) == (200, 136))
    res = ssim_ref.picture_ssim(c["src"][0], c["rec"][0], 200, 136)
    assert [n for n, _, _ in res] == [25 * 17, 12 * 8, 12 * 8]
    a = c["src"][0].copy(); pu = ssim_ref.planes_of(a, 200, 136)[1]
    pu[:, 96:] ^= 0xFF; pu[64:, :] ^= 0xFF                                  # (a view: changes a)
    assert ssim_ref.picture_ssim(a, c["rec"][0], 200, 136)[1] == res[1]


def test_fixed_point_sum_and_identity():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (40, 72), dtype=np.uint8); b = rng.integers(0, 256, (40, 72), dtype=np.uint8)
    n, mean, fixed = ssim_ref.plane_ssim(a, b)
    assert n == 45 and abs(fixed / ssim_ref.FIX / n - mean) <= 2.0 ** -31
    assert ssim_ref.plane_ssim(a, a) == (45, 1.0, 45 << 30)
    z = np.zeros((8, 8), np.uint8)
    n, mean, fixed = ssim_ref.plane_ssim(z, z + 255)                        # flat 0 against flat 255: C1 / (255^2 + C1)
    assert abs(mean - ssim_ref.C1 / (255.0 ** 2 + ssim_ref.C1)) < 1e-15
