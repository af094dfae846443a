"""Properties of the scaler's specification (tests/yuv_scale_ref.py): the tables' sum rule and bound, identity, flatness, the chroma siting, clipping, and a cross-check of
the luma path against torch's antialiased resize on the CPU."""
from __future__ import annotations

import numpy as np
import pytest

import yuv_scale_ref as ys

FILTERS = [ys.TRIANGLE, ys.CATMULL_ROM]


def brute_table(S, D, filt, cosited):
    """the definition read literally, one output at a time"""
    q = 2 * max(S, D)
    R = q if filt == ys.TRIANGLE else 2 * q
    first, rows = [], []
    for j in range(D):
        taps = []
        for k in range(S):
            m = 2 * (k * D - j * S) if cosited else (2 * k + 1) * D - (2 * j + 1) * S
            x = abs(m)
            if x >= R:
                continue
            n = max(0, q - x) if filt == ys.TRIANGLE else (3 * x ** 3 - 5 * q * x ** 2 + 2 * q ** 3 if x < q else -x ** 3 + 5 * q * x ** 2 - 8 * q * q * x + 4 * q ** 3)
            taps.append((k, n))
        while taps[0][1] == 0:
            taps.pop(0)
        while taps[-1][1] == 0:
            taps.pop()
        assert [k for k, _ in taps] == list(range(taps[0][0], taps[0][0] + len(taps)))
        N = sum(n for _, n in taps)
        c = [(2 * 16384 * n + N) // (2 * N) for _, n in taps]
        best = max(n for _, n in taps)
        c[[n for _, n in taps].index(best)] += 16384 - sum(c)
        first.append(taps[0][0]); rows.append(c)
    T = max(len(r) for r in rows)
    return np.array(first, np.int32), np.array([r + [0] * (T - len(r)) for r in rows], np.int16), T


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("cosited", [False, True])
def test_tables_sum_rule_and_bound(filt, cosited):
    for S, D in ys.AXIS_PAIRS:
        first, c, T = ys.table(S, D, filt, cosited)                 # (raises when sum |c| > 2 * 16384)
        c = c.astype(np.int64)
        assert c.shape == (D, T) and T <= ys.MAX_TAPS, (S, D)
        assert (c.sum(axis=1) == 16384).all(), (S, D)
        assert (np.abs(c).sum(axis=1) <= 2 * 16384).all(), (S, D)
        assert first.min() >= 0 and (first + T - 1).min() >= 0 and first.max() <= S - 1, (S, D)
        cnt = T - (np.cumsum(c[:, ::-1] != 0, axis=1) == 0).sum(axis=1)     # the entries behind the last non-zero one are 0 by construction
        assert ((first + cnt - 1) <= S - 1).all(), (S, D)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("cosited", [False, True])
def test_tables_equal_the_definition_read_literally(filt, cosited):
    for S, D in [(p, d) for p, d in ys.AXIS_PAIRS if p * d <= 200 * 128]:
        first, c, T = ys.table(S, D, filt, cosited)
        bf, bc, bT = brute_table(S, D, filt, cosited)
        assert T == bT and (first == bf).all() and (c == bc).all(), (S, D)


def test_size_rules():
    assert ys.size_ok(3840, 2160, 1920, 1080) and ys.size_ok(3840, 2160, 1280, 720) and ys.size_ok(200, 136, 128, 72) and ys.size_ok(512, 256, 64, 32) and ys.size_ok(64, 64, 512, 512)
    for bad in [(520, 256, 64, 32), (64, 64, 520, 64), (132, 96, 64, 48), (128, 97, 64, 48), (128, 96, 60, 48), (128, 96, 64, 44), (8200, 96, 4096, 48), (0, 96, 64, 48)]:
        assert not ys.size_ok(*bad), bad
        with pytest.raises(ValueError):
            ys.tables(*bad)
    with pytest.raises(ValueError):
        ys.table(64, 32, 2)


@pytest.mark.parametrize("filt", FILTERS)
def test_identity_is_single_tap_and_exact(filt):
    t = ys.tables(64, 48, 64, 48, filt)
    for first, c, T in t.values():
        assert T == 1 and (c == 16384).all() and (first == np.arange(len(first))).all()
    src = np.random.default_rng(1).integers(0, 256, 64 * 48 * 3 // 2, dtype=np.uint8)
    assert (ys.scale_i420(src, 64, 48, 64, 48, filt) == src).all()


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("size", [(128, 96, 64, 48), (200, 136, 128, 72), (512, 256, 64, 32), (64, 64, 104, 88)])
def test_flat_stays_flat(filt, size):
    sw, sh, dw, dh = size
    for v in (0, 1, 16, 127, 128, 254, 255):
        out = ys.scale_i420(np.full(sw * sh * 3 // 2, v, np.uint8), sw, sh, dw, dh, filt)
        assert out.size == dw * dh * 3 // 2 and (out == v).all()


@pytest.mark.parametrize("filt", FILTERS)
def test_chroma_ramp_keeps_its_luma_positions(filt):
    S, D, H = 64, 32, 8                                             # chroma sample k sits on luma column 2k; the ramp is 4 levels per chroma sample
    ramp = np.broadcast_to((4 * np.arange(S)).astype(np.uint8), (H, S))
    want = 4.0 * 2 * np.arange(D)                                   # output j sits on destination luma column 2j = source luma column 4j = source chroma column 2j
    inner = slice(4, D - 4)                                         # (the dropped taps at the borders pull the ends inwards)
    cos = ys.scale_plane(ramp, ys.table(S, D, filt, True), ys.table(H, H, filt))
    assert np.abs(cos[0, inner] - want[inner]).max() <= 1
    cen = ys.scale_plane(ramp, ys.table(S, D, filt, False), ys.table(H, H, filt))
    assert np.abs(cen[0, inner] - (want[inner] + 2.0)).max() <= 1   # the centre mapping lands half a source chroma sample (a quarter destination sample) to the right: 2 levels
    assert np.abs(cen[0, inner] - want[inner]).min() >= 1


def test_checkerboard_clips_and_never_wraps():
    sw, sh = 64, 64
    yy, xx = np.mgrid[0:sh, 0:sw]
    for cell in (1, 2, 3):
        board = (((yy // cell + xx // cell) & 1) * 255).astype(np.uint8)
        for dw, dh in [(104, 88), (512, 512), (40, 24), (64, 64)]:
            tx, ty = ys.table(sw, dw, ys.CATMULL_ROM), ys.table(sh, dh, ys.CATMULL_ROM)
            out = ys.scale_plane(board, tx, ty).astype(np.int64)
            # the same sums in Python integers, unclipped: wherever they leave [0, 255] the output sits on the bound
            p = board.astype(np.int64)
            h = np.zeros((sh, dw), np.int64)
            for i in range(tx[2]):
                h += tx[1][:, i].astype(np.int64)[None, :] * p[:, np.minimum(tx[0] + i, sw - 1)]
            h = (h + 128) >> 8
            v = np.zeros((dh, dw), np.int64)
            for i in range(ty[2]):
                v += ty[1][:, i].astype(np.int64)[:, None] * h[np.minimum(ty[0] + i, sh - 1), :]
            raw = (v + (1 << 19)) >> 20
            assert (out == np.clip(raw, 0, 255)).all()
            if (dw, dh) == (104, 88) and cell >= 2:
                assert (raw < 0).any() and (raw > 255).any()        # the cubic does overshoot here: the clip is exercised
            assert (out[raw < 0] == 0).all() and (out[raw > 255] == 255).all()


@pytest.mark.parametrize("filt,mode", [(ys.TRIANGLE, "bilinear"), (ys.CATMULL_ROM, "bicubic")])
def test_luma_against_torch_antialiased_resize(filt, mode):
    """Bound 2 levels, derived: rounding the coefficients and the fix-up move the weight sum of an axis by at most 2 T 2^-15 (0.56 levels at T = 36), the intermediate adds
    2^-7 and the two roundings (ours, torch's result rounded here) the rest."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(7)
    for sw, sh, dw, dh in [(128, 96, 64, 48), (200, 136, 128, 72), (512, 256, 64, 32), (64, 64, 104, 88), (384, 216, 128, 72)]:
        src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        smooth = np.clip(128 + 100 * np.sin(np.arange(sw)[None, :] / 9.0) * np.cos(np.arange(sh)[:, None] / 7.0), 0, 255).astype(np.uint8)
        for pic in (src, smooth):
            ref = F.interpolate(torch.from_numpy(pic.astype(np.float32))[None, None], size=(dh, dw), mode=mode, antialias=True, align_corners=False)[0, 0].numpy()
            ref = np.clip(np.floor(ref + 0.5), 0, 255).astype(np.int64)
            got = ys.scale_plane(pic, ys.table(sw, dw, filt), ys.table(sh, dh, filt)).astype(np.int64)
            d = np.abs(got - ref)
            print(f"{mode} {sw}x{sh}->{dw}x{dh}: max {d.max()}, share at 2: {(d == 2).mean():.6f}, share at 1: {(d == 1).mean():.6f}")
            assert d.max() <= 2
