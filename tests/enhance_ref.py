"""TEST INFRASTRUCTURE: the specification of `vpp_edge` / `vpp_color` (include/ks265_enc.h), in exact integer arithmetic: every byte that ks265_input_enhance
(ks265codec_amd/csrc/input_enhance.hip), its CPU stand-in (tests/hip_stub_enhance.c) and the encoder host produce is held to this file.

One step, no state: the packed I420 picture of W x H (both multiples of 8: the coded size) and (edge_gain, edge_core, edge_limit, edge_over, color_gain) -> the enhanced picture.
  * luma (edge_gain > 0; S = the source plane as int, coordinates outside the plane clamped into it = edge replication, nothing outside the plane is read):
      h(x, y) = sum_i k[i] S(x + i - 2, y), k = (1, 4, 6, 4, 1);  v(x, y) = sum_j k[j] h(x, y + j - 2): the blur in 1/256 of a code, 0 .. 65280, no rounding in between
      d = 256 S - v;  a = max(0, |d| - 256 edge_core)  (coring, a soft threshold);  e = min(edge_limit, (edge_gain a + 2048) >> 12)  (edge_gain in 1/16);  o = S + sgn(d) e
      halo control: mn / mx = the minimum / maximum of S over the 3x3 neighbourhood (same clamping); the result is clip(o, max(0, mn - edge_over), min(255, mx + edge_over)).
  * chroma (color_gain > 0), pointwise per co-located (u, v): cu = u - 128, cv = v - 128, m = max(|cu|, |cv|), K = 8192 + color_gain (128 - m); every component becomes
      128 + sgn(c) ((|c| K + 4096) >> 13), clipped to 0 .. 255.  The gain falls linearly to 1 as the pair approaches full saturation; grey stays grey.
  * a gain of 0 leaves its planes as they are.
Ranges: edge_gain 0 .. 64, edge_core 0 .. 16, edge_limit 1 .. 64 (when edge_gain > 0), edge_over 0 .. 32, color_gain 0 .. 32 (at 64 the final clip would bind: 1984 of the
65 536 pairs); both gains 0 is no filter at all.  The levels (vpp_edge 1 / 2 / 3, vpp_color 1 / 2 / 3) are this build's choice; nobody has tried them on real footage."""
from __future__ import annotations

import numpy as np

K5 = (1, 4, 6, 4, 1)
EDGE_LEVELS = {1: (8, 2, 8, 2), 2: (16, 2, 16, 4), 3: (24, 3, 24, 8)}      # (gain, core, limit, over)
COLOR_LEVELS = {1: 8, 2: 16, 3: 32}


def level_params(edge: int, color: int):
    """(edge_gain, edge_core, edge_limit, edge_over, color_gain) of a handle's vpp_edge / vpp_color, None when both are 0"""
    if not edge and not color:
        return None
    return (EDGE_LEVELS[edge] if edge else (0, 0, 0, 0)) + (COLOR_LEVELS[color] if color else 0,)


def check_cfg(cfg, w, h):
    g, core, limit, over, cg = cfg
    return (w > 0 and h > 0 and w % 8 == 0 and h % 8 == 0 and w <= 8192 and h <= 8192 and 0 <= g <= 64 and 0 <= core <= 16 and 0 <= over <= 32 and 0 <= cg <= 32
            and (g == 0 or 1 <= limit <= 64) and (g > 0 or cg > 0))


def planes(p: np.ndarray, w: int, h: int):
    p = np.asarray(p, np.uint8).reshape(-1)
    assert p.size == w * h * 3 // 2
    return p[:w * h].reshape(h, w), p[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), p[w * h * 5 // 4:].reshape(h // 2, w // 2)


def _shift(a, dx, dy):
    """a(x + dx, y + dy) with the coordinates clamped into the plane"""
    h, w = a.shape
    return a[np.clip(np.arange(h) + dy, 0, h - 1)[:, None], np.clip(np.arange(w) + dx, 0, w - 1)[None, :]]


def blur256(s):
    """v: the 5x5 binomial blur of the plane in 1/256 of a code"""
    s = np.asarray(s).astype(np.int32)
    hp = sum(k * _shift(s, i - 2, 0) for i, k in enumerate(K5))
    return sum(k * _shift(hp, 0, j - 2) for j, k in enumerate(K5))


def min_max3(s):
    s = np.asarray(s).astype(np.int32)
    nb = [_shift(s, dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.minimum.reduce(nb), np.maximum.reduce(nb)


def enhance_luma(s, gain, core, limit, over):
    s = np.asarray(s).astype(np.int32)
    if gain <= 0:
        return s.astype(np.uint8)
    v = blur256(s)
    assert v.min() >= 0 and v.max() <= 65280
    d = 256 * s - v
    a = np.maximum(0, np.abs(d) - 256 * core)
    e = np.minimum(limit, (gain * a + 2048) >> 12)
    o = s + np.sign(d) * e
    mn, mx = min_max3(s)
    return np.clip(o, np.maximum(0, mn - over), np.minimum(255, mx + over)).astype(np.uint8)


def color_map(u, v, gain):
    """the chroma step on int arrays BEFORE the final clip: (u', v') as int"""
    cu, cv = np.asarray(u).astype(np.int32) - 128, np.asarray(v).astype(np.int32) - 128
    k = 8192 + gain * (128 - np.maximum(np.abs(cu), np.abs(cv)))
    return tuple(128 + np.sign(c) * ((np.abs(c) * k + 4096) >> 13) for c in (cu, cv))


def enhance_chroma(u, v, gain):
    if gain <= 0:
        return np.asarray(u, np.uint8).copy(), np.asarray(v, np.uint8).copy()
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in color_map(u, v, gain))


def enhance_picture(pic, w, h, cfg):
    """the enhanced packed picture"""
    assert check_cfg(cfg, w, h), (cfg, w, h)
    g, core, limit, over, cg = cfg
    y, u, v = planes(pic, w, h)
    u2, v2 = enhance_chroma(u, v, cg)
    return np.concatenate([enhance_luma(y, g, core, limit, over).ravel(), u2.ravel(), v2.ravel()])


def enhance_clip(pictures, w, h, cfg):
    return [enhance_picture(p, w, h, cfg) for p in pictures]
