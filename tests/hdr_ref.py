"""TEST INFRASTRUCTURE: the specification of `vpp_hdr` (include/ks265_enc.h), in exact integer arithmetic: every byte that ks265_input_hdr
(ks265codec_amd/csrc/input_hdr.hip), its CPU stand-in (tests/hip_stub_hdr.c) and the encoder host produce is held to this file.

One step, no state, luma only: the packed I420 picture of W x H (both multiples of 8, at most 8192: the coded size) and (gain, iters, slope, radius[3]) -> the picture with
its local contrast raised.  The smoother is the domain transform in its normalised-convolution form:
  * guidance: the luma Y that enters the filter, fixed over all iterations.  Along a line d[x] = 16 + slope |Y[x] - Y[x - 1]| (1/16 sample), ct = the running sum of d; d of
    a line's first sample plays no part - only differences of ct are ever used.
  * one 1-D pass of radius r (1/16 sample) over a plane J of 12-bit values (1/16 code; J starts as 16 Y): the window of sample x is every sample j of the same line with
    |ct[j] - ct[x]| <= r (contiguous: ct is strictly increasing; at most r // 16 samples a side, since d >= 16); out goes (2 S + n) // (2 n), S the sum of J over the window,
    n its size.  At the ends of a line the window simply ends.
  * iteration i = 1 .. iters (2 or 3): a pass along the rows, then one along the columns, both with radius[i - 1].  The last column pass gives the base B.
  * D = 16 Y - B;  out = clip(Y + sgn(gain D) ((|gain D| + 128) >> 8), 0, 255), gain in 1/16.  No tone curve on the base.  Chroma is not touched.
Ranges: gain 1 .. 80, iters 2 / 3, slope 0 .. 4096, every radius in use 16 .. 2480.  ct is kept in int64 here (8192 samples of 16 + 4096 * 255 pass 2^32); every other
value stays inside int32.  params() maps the SDK's doubles; the defaults (strength 1.0, iter 3, sigma_s 20, sigma_r 15) are this build's choice and nobody has tried them on
real footage."""
from __future__ import annotations

import math

import numpy as np

DEFAULTS = (1.0, 3, 20.0, 15.0)               # strength, iter, sigma_s, sigma_r of a field left at 0


def params(strength, iters, sigma_s, sigma_r):
    """(gain, iters, slope, (radius ...)) of the SDK's four doubles, a 0 taking this build's default; sigma_r is a percentage of the 8-bit range"""
    strength = float(strength) if strength else DEFAULTS[0]
    iters = int(iters) if iters else DEFAULTS[1]
    sigma_s = float(sigma_s) if sigma_s else DEFAULTS[2]
    sigma_r = float(sigma_r) if sigma_r else DEFAULTS[3]
    gain = int(math.floor(16 * strength + 0.5))
    slope = min(4096, int(math.floor(1600 * sigma_s / (255 * sigma_r) + 0.5)))
    radius = tuple(max(16, int(math.floor(16 * (3 * sigma_s * 2.0 ** (iters - i) / math.sqrt(4.0 ** iters - 1)) + 0.5))) for i in range(1, iters + 1))
    return gain, iters, slope, radius


def check_cfg(cfg, w, h):
    gain, iters, slope, radius = cfg
    return (w > 0 and h > 0 and w % 8 == 0 and h % 8 == 0 and w <= 8192 and h <= 8192 and 1 <= gain <= 80 and iters in (2, 3) and 0 <= slope <= 4096
            and len(radius) >= iters and all(16 <= r <= 2480 for r in radius[:iters]))


def work_bytes(w, h):
    """what ks265_input_hdr_work_bytes answers: the guidance copy and two 16-bit planes"""
    return 5 * w * h


def planes(p: np.ndarray, w: int, h: int):
    p = np.asarray(p, np.uint8).reshape(-1)
    assert p.size == w * h * 3 // 2
    return p[:w * h].reshape(h, w), p[w * h:]


def transform(y, slope):
    """ct along the rows of y (int64; column 0 holds 0: the first sample's d plays no part)"""
    y = np.asarray(y).astype(np.int64)
    d = 16 + slope * np.abs(np.diff(y, axis=1))
    return np.concatenate([np.zeros((y.shape[0], 1), np.int64), np.cumsum(d, axis=1)], axis=1)


def pass_rows(j, ct, r):
    """one pass along the rows of j (int) under ct"""
    j = np.asarray(j).astype(np.int64)
    n_lines, n = j.shape
    big = int(ct.max()) + r + 1                                         # lines kept apart: one searchsorted for the whole plane
    flat = (ct + big * np.arange(n_lines, dtype=np.int64)[:, None]).ravel()
    lo = np.searchsorted(flat, flat - r, "left")
    hi = np.searchsorted(flat, flat + r, "right")                       # one behind the window
    ps = np.concatenate([[0], np.cumsum(j.ravel())])
    s, cnt = ps[hi] - ps[lo], hi - lo
    assert s.max() < 2 ** 30 and cnt.min() >= 1
    return ((2 * s + cnt) // (2 * cnt)).reshape(n_lines, n)


def base_layer(y, iters, slope, radius):
    """B: the smoothed plane in 1/16 code"""
    y = np.asarray(y).astype(np.int64)
    ct_r, ct_c = transform(y, slope), transform(y.T, slope)
    j = 16 * y
    for i in range(iters):
        j = pass_rows(j, ct_r, radius[i])
        j = pass_rows(j.T, ct_c, radius[i]).T
    return j


def hdr_luma(y, cfg):
    gain, iters, slope, radius = cfg
    y = np.asarray(y).astype(np.int64)
    gd = gain * (16 * y - base_layer(y, iters, slope, radius))
    assert np.abs(gd).max() < 2 ** 30
    return np.clip(y + np.sign(gd) * ((np.abs(gd) + 128) >> 8), 0, 255).astype(np.uint8)


def hdr_picture(pic, w, h, cfg):
    """the filtered packed picture"""
    assert check_cfg(cfg, w, h), (cfg, w, h)
    y, c = planes(pic, w, h)
    return np.concatenate([hdr_luma(y, cfg).ravel(), c])


def hdr_clip(pictures, w, h, cfg):
    return [hdr_picture(p, w, h, cfg) for p in pictures]
