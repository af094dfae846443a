"""CPU: the host's plain-C reducer and rasteriser of ROI maps (ks265codec_amd/host/ks265_roi.h) under the sanitizers, against tests/roi_map_ref.py word for word.
tests/roi_reduce_main.c is a stand-alone program built with -fsanitize=address,undefined and run as a child process: the map sits in a heap block of exactly its extent,
so a read past the map is a sanitizer report."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import roi_cases
import roi_map_ref as R

from host_harness import build_host_program


@pytest.fixture(scope="module")
def exe():
    return build_host_program("roi_reduce_main.c")


def _reduce(exe, tmp_path, m, lb, w, h, pad_elems, offset):
    """the program's records for map m laid out with pad_elems elements behind every row, offset bytes into its block"""
    es = m.dtype.itemsize
    rows, cols = m.shape
    pitch = (cols + pad_elems) * es
    buf = np.full(offset + pitch * (rows - 1) + cols * es, 0xA5, np.uint8)
    for r in range(rows):
        buf[offset + r * pitch:offset + r * pitch + cols * es] = m[r].view(np.uint8)
    src, dst = str(tmp_path / "map.bin"), str(tmp_path / "rec.bin")
    buf.tofile(src)
    r = subprocess.run([exe, "reduce", str(R.FLOAT32 if m.dtype == np.float32 else R.INT8), str(lb), str(w), str(h), str(pitch), str(offset), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-400:] + r.stderr[-3000:]
    return np.fromfile(dst, np.int32)


@pytest.mark.parametrize("dtype", [np.int8, np.float32])
@pytest.mark.parametrize("lb", range(7))
def test_reducer_equals_the_spec(exe, tmp_path, lb, dtype):
    for w, h in ((64, 64), (72, 72), (200, 136)):
        m = roi_cases.special_map(1000 * lb + w, w, h, lb, dtype)
        exp = R.reduce(m, w, h, lb)
        for pad, off in ((0, 0), (1, 0), (3, 1), (0, 5)):                 # pitches that are no multiple of 16, 4 or (float) of anything but the element; odd addresses
            got = _reduce(exe, tmp_path, m, lb, w, h, pad, off)
            assert (got == exp).all(), (w, h, lb, pad, off, np.flatnonzero(got != exp)[:8])


def test_reducer_element_conversion_on_every_special_value(exe, tmp_path):
    """one element per CTU (log2_block 6): the record is the element's Q8 value itself"""
    sp = np.concatenate([roi_cases.F32_SPECIALS, (np.arange(-40, 41) / np.float32(512)).astype(np.float32), np.float32([50.99, -50.99, 12.345678, -7.000001])])
    m = sp.reshape(1, -1).astype(np.float32)
    w = 64 * m.shape[1]
    got = _reduce(exe, tmp_path, m, 6, w, 64, 0, 0)
    assert (got == R.to_q8(m).reshape(-1)).all()
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)            # any bit pattern: denormals, NaN payloads, huge exponents
    m = bits.view(np.float32).reshape(1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        exp = R.to_q8(m).reshape(-1)
    assert (_reduce(exe, tmp_path, m, 6, 64 * 4096, 64, 0, 0) == exp).all()
    m = (rng.integers(-13100 * 2, 13100 * 2, 4096) / np.float32(512)).astype(np.float32).reshape(1, -1)      # every second one a tie
    assert (_reduce(exe, tmp_path, m, 6, 64 * 4096, 64, 0, 0) == R.to_q8(m).reshape(-1)).all()


def test_reducer_means_of_exactly_half(exe, tmp_path):
    for k in (-3, -1, 0, 4):
        for lb in (0, 3, 5):
            m = roi_cases.half_mean_map(128, 64, lb, k)
            exp = R.reduce(m, 128, 64, lb)
            assert exp.tolist() == [k + 1, k + 1]
            assert (_reduce(exe, tmp_path, m, lb, 128, 64, 1, 4) == exp).all()


def test_reducer_refuses_bad_descriptions(exe, tmp_path):
    (tmp_path / "x.bin").write_bytes(b"\0" * 64)
    for args in (["2", "0", "64", "64", "64"], ["0", "7", "64", "64", "64"], ["0", "-1", "64", "64", "64"], ["0", "0", "64", "64", "63"], ["1", "0", "64", "64", "258"], ["1", "0", "64", "64", "252"]):
        r = subprocess.run([exe, "reduce", *args, "0", str(tmp_path / "x.bin"), str(tmp_path / "y.bin")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout == "refused\n", (args, r.stdout, r.stderr[-2000:])


RECTS = [
    ((200, 136), [(0, 0, 64, 64, -6), (64, 0, 136, 136, 4)]),
    ((200, 136), [(0, 0, 200, 136, 3), (17, 17, 1, 1, -2), (500, 0, 10, 10, 9), (-8, -8, 9, 9, 7), (190, 130, 100, 100, -60), (15, 0, 2, 136, 60), (0, 0, 0, 5, 1), (3, 3, -4, 5, 1)]),
    ((128, 72), []),
    ((72, 72), [(71, 71, 1, 1, 5), (0, 64, 16, 8, -5)]),
]


@pytest.mark.parametrize("size,rects", RECTS)
def test_rasteriser_equals_the_spec_and_reduces_to_it(exe, tmp_path, size, rects):
    w, h = size
    exp = R.rasterise(rects, w, h)
    for pad in (0, 5):
        dst = str(tmp_path / "raster.bin")
        r = subprocess.run([exe, "raster", str(w), str(h), str(exp.shape[1] + pad), dst, *["%d:%d:%d:%d:%d" % t for t in rects]], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-400:] + r.stderr[-3000:]
        got = np.fromfile(dst, np.int8).reshape(exp.shape)
        assert (got == exp).all()
    assert (_reduce(exe, tmp_path, exp, 4, w, h, 2, 3) == R.reduce(exp, w, h, 4)).all()


def test_rasteriser_refuses_a_ninth_rectangle(exe, tmp_path):
    r = subprocess.run([exe, "raster", "64", "64", "4", str(tmp_path / "r.bin"), *["0:0:8:8:1"] * 9], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "refused\n", r.stdout + r.stderr[-2000:]
