"""CPU: properties of tests/yuv_hibit_ref.py, the specification of the YUV family of the device input (KS265_IN_YUV, include/ks265_hip.h):
  * depth 8 4:2:0 planar / semi-planar is, byte for byte, yuv_convert_ref's I420 repack / NV12 deinterleave;
  * a depth-d picture whose every sample is u8 << (d - 8) gives exactly the 8-bit picture's result, for all three subsamplings and both alignments;
  * 4:2:2 with equal row pairs and 4:4:4 with constant chroma are identities;
  * msb = 0 ignores the high stray bits and msb = 1 the low ones;
  * all-maximum input gives 255, not 0; ties round up, once;
  * the codes: the names of the header, what is valid and what is not."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import yuv_convert_ref as cref
import yuv_hibit_ref as yh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 24, 6


def test_depth8_420_is_the_existing_repack():
    rng = np.random.default_rng(1)
    y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
    assert (yh.to_i420([y, u, v], yh.PLANAR, yh.S420, 8) == np.concatenate([y.ravel(), u.ravel(), v.ravel()])).all()
    uv = rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    assert (yh.to_i420([y, uv], yh.SEMI, yh.S420, 8) == cref.nv12_to_i420(y, uv)).all()


@pytest.mark.parametrize("layout,sub", yh.SHAPES, ids=[f"{yh.LAYOUT_NAMES[l]}{yh.SUB_NAMES[s]}" for l, s in yh.SHAPES])
@pytest.mark.parametrize("depth", [9, 10, 12, 16])
def test_shifted_8bit_pictures_give_the_8bit_result(layout, sub, depth):
    rng = np.random.default_rng(depth)
    p8 = yh.random_planes(rng, layout, sub, 8, 0, W, H)
    p8[0][0, :4] = (0, 255, 255, 0)
    exp = yh.to_i420(p8, layout, sub, 8)
    wide = [p.astype(np.uint16) << (depth - 8) for p in p8]
    assert (yh.to_i420(wide, layout, sub, depth, 0) == exp).all()
    assert (yh.to_i420([p << (16 - depth) for p in wide], layout, sub, depth, 1) == exp).all()


@pytest.mark.parametrize("depth", [8, 10])
def test_422_of_equal_row_pairs_and_444_of_constant_chroma_are_identities(depth):
    rng = np.random.default_rng(3)
    hi = 1 << depth
    dt = np.uint8 if depth == 8 else np.uint16
    y = (rng.integers(0, 256, (H, W)) << (depth - 8)).astype(dt)
    c = (rng.integers(0, 256, (2, H // 2, W // 2)) << (depth - 8)).astype(dt)
    exp = np.concatenate([(y >> (depth - 8)).ravel(), (c >> (depth - 8)).ravel()]).astype(np.uint8)
    got = yh.to_i420([y, np.repeat(c[0], 2, 0), np.repeat(c[1], 2, 0)], yh.PLANAR, yh.S422, depth)
    assert (got == exp).all()
    for k in (0, 37 << (depth - 8), hi - 1):
        u, v = np.full((H, W), k, dt), np.full((H, W), hi - 1 - k, dt)
        got = yh.to_i420([y, u, v], yh.PLANAR, yh.S444, depth)
        s = depth - 8
        rnd = lambda n: min(255, (n + (1 << s >> 1)) >> s)
        assert (got[W * H:W * H * 5 // 4] == rnd(k)).all() and (got[W * H * 5 // 4:] == rnd(hi - 1 - k)).all()
    # replicated 2 x 2 chroma: the (1, 2, 1) filter sees c(i - 1), c(i), c(i) - an identity only where the left neighbour equals the sample, so a 2 x 2 replication of a
    # plane that is constant along its rows comes back as it was
    rows = (rng.integers(0, 256, (H // 2, 1)) << (depth - 8)).astype(dt).repeat(W // 2, 1)
    got = yh.to_i420([y, np.repeat(np.repeat(rows, 2, 0), 2, 1), np.repeat(np.repeat(rows, 2, 0), 2, 1)], yh.PLANAR, yh.S444, depth)
    assert (got[W * H:W * H * 5 // 4].reshape(H // 2, W // 2) == rows >> (depth - 8)).all()


@pytest.mark.parametrize("layout,sub", yh.SHAPES, ids=[f"{yh.LAYOUT_NAMES[l]}{yh.SUB_NAMES[s]}" for l, s in yh.SHAPES])
def test_stray_bits_on_the_unused_side_are_ignored(layout, sub):
    for depth in (10, 12):
        for msb in (0, 1):
            clean = yh.random_planes(np.random.default_rng(7), layout, sub, depth, msb, W, H, stray=False)
            junk = ((1 << (16 - depth)) - 1) << (0 if msb else depth)
            rng = np.random.default_rng(8)
            dirty = [p | (rng.integers(0, 65536, p.shape).astype(np.uint16) & np.uint16(junk)) for p in clean]
            assert all((a & np.uint16(junk) == 0).all() for a in clean) and all((a != b).any() for a, b in zip(clean, dirty))
            assert (yh.to_i420(clean, layout, sub, depth, msb) == yh.to_i420(dirty, layout, sub, depth, msb)).all()
            all_junk = [np.full_like(p, junk) for p in clean]
            assert (yh.to_i420(all_junk, layout, sub, depth, msb) == 0).all()


@pytest.mark.parametrize("layout,sub", yh.SHAPES, ids=[f"{yh.LAYOUT_NAMES[l]}{yh.SUB_NAMES[s]}" for l, s in yh.SHAPES])
def test_all_maximum_input_gives_255(layout, sub):
    for depth in range(8, 17):
        for msb in ((0,) if depth == 8 else (0, 1)):
            planes = [np.full(s, 0xFF if depth == 8 else 0xFFFF, np.uint8 if depth == 8 else np.uint16) for s in yh.plane_shapes(layout, sub, W, H)]
            assert (yh.to_i420(planes, layout, sub, depth, msb) == 255).all(), (depth, msb)


def test_ties_round_up_once():
    # depth 10: 4n + 2 is halfway -> n + 1; 4:2:2 of (4n + 1, 4n + 2): S = 8n + 3 -> (S + 4) >> 3 = n (rounded twice it would be n + 1)
    y = np.full((2, 8), 4 * 50 + 2, np.uint16)
    u = np.array([[4 * 60 + 1] * 4, [4 * 60 + 2] * 4], np.uint16)
    v = np.array([[4 * 60 + 2] * 4, [4 * 60 + 2] * 4], np.uint16)
    got = yh.to_i420([y, u, v], yh.PLANAR, yh.S422, 10)
    assert (got[:16] == 51).all() and (got[16:20] == 60).all() and (got[20:] == 61).all()
    assert yh.to_i420([np.full((2, 8), 1023, np.uint16), u, v], yh.PLANAR, yh.S422, 10)[0] == 255            # (1023 + 2) >> 2 = 256: clipped


def test_codes_and_names():
    assert yh.code(0, 0, 8) == 0x1008 and yh.NAMED["P010"] == 0x1000 | 1 << 8 | 1 << 5 | 10
    assert all(c >= 4096 for c in yh.NAMED.values()) and len(set(yh.NAMED.values())) == len(yh.NAMED)
    for name, c in yh.NAMED.items():
        assert yh.decode(c) is not None, name
    valid = [c for c in range(0x1000, 0x1400) if yh.decode(c)]
    assert len(valid) == 6 * 17 + 2 * 17                               # planar and semi-planar x 3 subsamplings, packed x 4:2:2; depth 8 once, 9 .. 16 with both alignments
    for c in (0, 1, 2, 3, 7, 15, 16, 19, 4095, 0x1000, yh.code(0, 0, 7), yh.code(0, 0, 17), yh.code(0, 0, 8, 1), yh.code(2, 0, 8), yh.code(2, 2, 8), yh.code(3, 2, 10, 1),
              yh.code(0, 3, 8), 0x2008, 0x1408, 0x1008 | 1 << 16, -1):
        assert yh.decode(c) is None, hex(c)
    # the header's names are these codes
    for header in ("ks265_hip.h", "ks265_enc.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        found = dict(re.findall(r"#define KS265_IN_(\w+) KS265_IN_YUV\(([^)]*)\)", text))
        assert set(found) == set(yh.NAMED), header
        for name, args in found.items():
            assert yh.code(*[int(a) for a in args.split(",")]) == yh.NAMED[name], (header, name)
    from ks265codec_amd import lib as kl
    for name, c in yh.NAMED.items():
        assert getattr(kl, "IN_" + name) == c
