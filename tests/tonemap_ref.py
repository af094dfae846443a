"""Specification of tone mapping on the way in (ks265_input_tonemap of include/ks265_hip.h; ks265codec_amd/csrc/input_tonemap.hip; host/ks265_tonemap.h builds the same
tables in C): an HDR10 picture - SMPTE ST 2084 "PQ", BT.2020 primaries and non-constant-luminance matrix, 4:2:0 of 10 to 16 bits, planar or semi-planar
(tests/yuv_hibit_ref.py describes the layouts) - to the encoder's packed 8-bit I420 in BT.709, limited range.

model() is the colour pipeline in float64, per luma sample:
  1  chroma up to luma resolution at HEVC's default siting: an even column takes its chroma sample, an odd one the rounded mean of its two neighbours (the right edge
     clamps); both luma rows of a pair take chroma row i
  2  normalise at depth d: limited y = (Y - 16 2^(d-8)) / (219 2^(d-8)), c = (C - 128 2^(d-8)) / (224 2^(d-8)); full y = Y / (2^d - 1), c = (C - 2^(d-1)) / (2^d - 1)
  3  R' = y + 1.4746 cr, G' = y - 0.16455 cb - 0.57135 cr, B' = y + 1.8814 cb, each clamped to [0, 1]
  4  PQ EOTF to nits, x = min(L, peak) / white
  5  gain g = curve(m) / m on m = max(xR, xG, xB) (g = 1 at m = 0): bt2390 (BT.2390's EETF in PQ space), reinhard m (1 + m / P^2) / (1 + m), clip min(m, 1); P = peak / white
  6  BT.2020 -> BT.709 primaries on the linear values, times g, clamped to [0, 1]
  7  BT.709 OETF, q = round(65280 V)
  8  tests/yuv_float_ref.py q_to_i420(qr, qg, qb, MATRIX_BT709, False): the arithmetic float RGB tensors go through

to_i420() is the integer form every byte of the kernel, the CPU stand-in and the host are held to.  Three tables per (curve, peak, white), every entry from math.pow
(the C library's pow: the C host builds the same integers):
  E[4096]  uint32  the linear light x of PQ code i / 4095 in 1 / 2^20 (at most 125 2^20 < 2^27)
  G[4096]  uint16  the gain in 1 / 2^15 at the linear light of code i, read at the LARGEST of a pixel's three codes (the EOTF is monotonic: the largest linear component),
                   so the index lies in the perceptual domain; g <= 1 for all three curves
  O[4097]  uint16  q of linear light i / 4096, read with linear interpolation (the OETF's linear toe is interpolated exactly)
and the arithmetic, with the width every step is computed in:
  chroma   odd columns (C[k] + C[min(k + 1, W/2 - 1)] + 1) >> 1                                                                      int32
  codes    R12 = clamp((ky (Y - yoff) + krv (Cr - coff) + 2^16) >> 17, 0, 4095), G12 and B12 alike; k* = round(4095 2^17 coefficient / range).  The luma product is at
           most 4095 256 / 219 2^17 < 6.3e8 at every depth and the chroma products together at most 5.8e8: the sum fits                 int32
  gain     t = min((E[c12] G[max(R12, G12, B12)] + 2^18) >> 19, 65536): linear light after the curve in 1 / 2^16; the product is below 2^42    uint64
  matrix   v = clamp((m0 tR + m1 tG + m2 tB + 2^9) >> 10, 0, 2^20) with the rows in 1 / 2^14, each summing to EXACTLY 16384 (the rounding remainder goes to the
           diagonal): equal t give v = 16 t in all three channels, so neutral chroma in gives U = V = 128 out.  |sum| <= 27206 65536 < 1.8e9                 int32
  OETF     i = v >> 8, f = v & 255, q = (O[i] (256 - f) + O[i + 1] f + 128) >> 8 (i = 4096 has f = 0: O[4097] is never read);  65280 256 < 2^24              int32
  q_to_i420 as tests/yuv_float_ref.py has it                                                                                                                int64
"""
from __future__ import annotations

import functools
import math

import numpy as np

import yuv_float_ref as yf
import yuv_hibit_ref as yh

BT2390, REINHARD, CLIP = 0, 1, 2
CURVES = {"bt2390": BT2390, "reinhard": REINHARD, "clip": CLIP}
TRANSFER_PQ = 16
M1, M2, C1, C2, C3 = 0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875
NCL = (1.4746, 0.16455, 0.57135, 1.8814)                               # R' from cr; G' from cb and cr; B' from cb
PRIM = ((1.660491, -0.587641, -0.072850), (-0.124550, 1.132900, -0.008349), (-0.018151, -0.100579, 1.118730))
SH_CODE, E_ONE, G_ONE, T_ONE, M_ONE, V_ONE = 17, 1 << 20, 1 << 15, 1 << 16, 1 << 14, 1 << 20


def cfg_ok(curve: int, peak: float, white: float) -> bool:
    return curve in (BT2390, REINHARD, CLIP) and 100.0 <= peak <= 10000.0 and 80.0 <= white <= 1000.0 and white <= peak


def pq_eotf(e: float) -> float:
    """non-linear [0, 1] -> nits"""
    p = math.pow(e, 1.0 / M2)
    n = p - C1
    if n < 0.0:
        n = 0.0
    return 10000.0 * math.pow(n / (C2 - C3 * p), 1.0 / M1)


def pq_inv(nits: float) -> float:
    y = math.pow(nits / 10000.0, M1)
    return math.pow((C1 + C2 * y) / (1.0 + C3 * y), M2)


def curve_of(m: float, curve: int, peak: float, white: float) -> float:
    """the tone curve on linear light m (1 = white), 0 <= m <= peak / white"""
    if curve == CLIP:
        return m if m < 1.0 else 1.0
    if curve == REINHARD:
        P = peak / white
        return m * (1.0 + m / (P * P)) / (1.0 + m)
    top = pq_inv(peak)
    e1 = pq_inv(m * white) / top
    ml = pq_inv(white) / top
    ks = 1.5 * ml - 0.5
    e2 = e1
    if e1 > ks and ks < 1.0:
        t = (e1 - ks) / (1.0 - ks)
        t2 = t * t
        t3 = t2 * t
        e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * ml
    return pq_eotf(e2 * top) / white


def gain_of(m: float, curve: int, peak: float, white: float) -> float:
    return curve_of(m, curve, peak, white) / m if m > 0.0 else 1.0


def oetf709(L: float) -> float:
    return 4.5 * L if L < 0.018 else 1.099 * math.pow(L, 0.45) - 0.099


def _rnd(x: float) -> int:
    return int(math.floor(x + 0.5))


@functools.lru_cache(maxsize=None)
def tables(curve: int, peak: float, white: float):
    """(E uint32[4096], G uint16[4096], O uint16[4097], M int32[3][3])"""
    assert cfg_ok(curve, peak, white)
    E, G = np.zeros(4096, np.uint32), np.zeros(4096, np.uint16)
    for i in range(4096):
        L = pq_eotf(i / 4095.0)
        if L > peak:
            L = peak
        x = L / white
        E[i] = _rnd(x * E_ONE)
        g = _rnd(gain_of(x, curve, peak, white) * G_ONE)
        G[i] = min(max(g, 0), G_ONE)
    O = np.array([_rnd(65280.0 * oetf709(i / 4096.0)) for i in range(4097)], np.uint16)
    M = np.zeros((3, 3), np.int32)
    for r in range(3):
        for c in range(3):
            M[r, c] = _rnd(PRIM[r][c] * M_ONE)
        M[r, r] += M_ONE - int(M[r].sum())
    for t in (E, G, O, M):
        t.setflags(write=False)
    return E, G, O, M


def norm_coef(depth: int, full_range: bool):
    """(yoff, coff, ky, krv, kgu, kgv, kbu) of the code step"""
    s = depth - 8
    ys, cs, yoff = ((1 << depth) - 1, (1 << depth) - 1, 0) if full_range else (219 << s, 224 << s, 16 << s)
    one = 4095.0 * (1 << SH_CODE)
    return (yoff, 1 << (depth - 1), _rnd(one / ys), _rnd(NCL[0] * one / cs), _rnd(NCL[1] * one / cs), _rnd(NCL[2] * one / cs), _rnd(NCL[3] * one / cs))


def _upsample(c: np.ndarray) -> np.ndarray:
    """(H/2, W/2) chroma -> (H, W) at luma resolution (step 1), integers"""
    nxt = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    full = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    full[:, 0::2] = c
    full[:, 1::2] = (c + nxt + 1) >> 1
    return np.repeat(full, 2, axis=0)


def _samples(planes, layout: int, depth: int, msb: int):
    y, u, v = (yh.normalise(p, depth, msb).astype(np.int64) for p in yh.split(planes, layout))
    H, W = y.shape
    assert W % 2 == 0 and H % 2 == 0 and u.shape == v.shape == (H // 2, W // 2)
    return y, _upsample(u), _upsample(v)


def to_q(planes, layout: int, depth: int, msb: int, curve: int = BT2390, peak: float = 1000.0, white: float = 203.0, full_range: bool = False):
    """the integer form up to q: three (H, W) int64 planes"""
    assert layout in (yh.PLANAR, yh.SEMI) and 10 <= depth <= 16
    E, G, O, M = tables(curve, float(peak), float(white))
    Y, U, V = _samples(planes, layout, depth, msb)
    yoff, coff, ky, krv, kgu, kgv, kbu = norm_coef(depth, full_range)
    ly, cb, cr = ky * (Y - yoff) + (1 << (SH_CODE - 1)), U - coff, V - coff
    sums = [ly + krv * cr, ly - kgu * cb - kgv * cr, ly + kbu * cb]
    for c in sums:
        assert np.abs(c).max() < 1 << 31
    code = [np.clip(c >> SH_CODE, 0, 4095) for c in sums]
    g = G[np.maximum(np.maximum(code[0], code[1]), code[2])].astype(np.int64)
    t = [np.minimum((E[c].astype(np.int64) * g + (1 << 18)) >> 19, T_ONE) for c in code]
    out = []
    for r in range(3):
        s = int(M[r, 0]) * t[0] + int(M[r, 1]) * t[1] + int(M[r, 2]) * t[2] + (1 << 9)
        assert np.abs(s).max() < 1 << 31
        v = np.clip(s >> 10, 0, V_ONE)
        i, f = v >> 8, v & 255
        out.append((O[i].astype(np.int64) * (256 - f) + O[np.minimum(i + 1, 4096)].astype(np.int64) * f + 128) >> 8)
    return out


def to_i420(planes, layout: int, depth: int, msb: int = 0, curve: int = BT2390, peak: float = 1000.0, white: float = 203.0, full_range: bool = False) -> np.ndarray:
    """the planes of a picture (tests/yuv_hibit_ref.py plane_shapes, 4:2:0) -> packed I420, one flat uint8 array: the specification"""
    return yf.q_to_i420(*to_q(planes, layout, depth, msb, curve, peak, white, full_range), yf.MATRIX_BT709, False)


def model(planes, layout: int, depth: int, msb: int = 0, curve: int = BT2390, peak: float = 1000.0, white: float = 203.0, full_range: bool = False) -> np.ndarray:
    """the colour pipeline in float64 -> packed I420"""
    Y, U, V = (p.astype(np.float64) for p in _samples(planes, layout, depth, msb))
    s = depth - 8
    if full_range:
        y, cb, cr = Y / ((1 << depth) - 1), (U - (1 << (depth - 1))) / ((1 << depth) - 1), (V - (1 << (depth - 1))) / ((1 << depth) - 1)
    else:
        y, cb, cr = (Y - (16 << s)) / (219 << s), (U - (128 << s)) / (224 << s), (V - (128 << s)) / (224 << s)
    nl = [np.clip(y + NCL[0] * cr, 0, 1), np.clip(y - NCL[1] * cb - NCL[2] * cr, 0, 1), np.clip(y + NCL[3] * cb, 0, 1)]
    p = [np.power(e, 1 / M2) for e in nl]
    x = [np.minimum(10000.0 * np.power(np.maximum(q - C1, 0) / (C2 - C3 * q), 1 / M1), peak) / white for q in p]
    m = np.maximum(np.maximum(x[0], x[1]), x[2])
    if curve == CLIP:
        cv = np.minimum(m, 1.0)
    elif curve == REINHARD:
        P = peak / white
        cv = m * (1 + m / (P * P)) / (1 + m)
    else:
        pinv = lambda n: np.power((C1 + C2 * np.power(n / 10000.0, M1)) / (1 + C3 * np.power(n / 10000.0, M1)), M2)
        top, ml = pq_inv(peak), pq_inv(white) / pq_inv(peak)
        ks = 1.5 * ml - 0.5
        e1 = pinv(m * white) / top
        t = np.clip((e1 - ks) / (1 - ks), 0, 1) if ks < 1.0 else np.zeros_like(e1)
        sp = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1 - ks) + (-2 * t ** 3 + 3 * t ** 2) * ml
        e2 = np.where((e1 > ks) & (ks < 1.0), sp, e1)
        pe = np.power(e2 * top, 1 / M2)
        cv = 10000.0 * np.power(np.maximum(pe - C1, 0) / (C2 - C3 * pe), 1 / M1) / white
    with np.errstate(all="ignore"):
        g = np.where(m > 0, cv / np.where(m > 0, m, 1.0), 1.0)
    q = []
    for r in range(3):
        L = np.clip((PRIM[r][0] * x[0] + PRIM[r][1] * x[1] + PRIM[r][2] * x[2]) * g, 0, 1)
        Vv = np.where(L < 0.018, 4.5 * L, 1.099 * np.power(L, 0.45) - 0.099)
        q.append(np.floor(65280.0 * Vv + 0.5).astype(np.int64))
    return yf.q_to_i420(q[0], q[1], q[2], yf.MATRIX_BT709, False)


def grey_ramp(depth: int = 10, layout: int = yh.SEMI, msb: int = 1, chroma: int | None = None) -> list:
    """every luma code of `depth` once (a 2^(depth-5) x 32 picture) under neutral chroma, as stored elements"""
    n = 1 << depth
    sh = 16 - depth if msb else 0
    y = (np.arange(n, dtype=np.int64).reshape(-1, 32) << sh).astype(np.uint16)
    c = np.full((y.shape[0] // 2, 16), (n >> 1 if chroma is None else chroma) << sh, np.uint16)
    return [y, np.repeat(c, 2, axis=1)] if layout == yh.SEMI else [y, c, c.copy()]


def primaries(depth: int, layout: int, msb: int, W: int, H: int, full_range: bool = False) -> list:
    """saturated BT.2020 primaries and secondaries at full signal in vertical bars (non-linear R'G'B' of 0 / 1 through the NCL matrix), as stored elements"""
    Kr, Kb = 0.2627, 0.0593
    Kg = 1 - Kr - Kb
    s = depth - 8
    cols = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1), (0, 0, 0)]
    yv, uv, vv = [], [], []
    for r, g, b in cols:
        yy = Kr * r + Kg * g + Kb * b
        cb, cr = (b - yy) / 1.8814, (r - yy) / 1.4746
        if full_range:
            mx = (1 << depth) - 1
            yv.append(round(yy * mx)); uv.append(round(cb * mx) + (1 << (depth - 1))); vv.append(round(cr * mx) + (1 << (depth - 1)))
        else:
            yv.append(round(yy * (219 << s)) + (16 << s)); uv.append(round(cb * (224 << s)) + (128 << s)); vv.append(round(cr * (224 << s)) + (128 << s))
    sh = 16 - depth if msb else 0
    bar = lambda vals, n: (np.clip(np.array([vals[min(x * len(cols) // n, len(cols) - 1)] for x in range(n)], np.int64), 0, (1 << depth) - 1) << sh).astype(np.uint16)
    y = np.tile(bar(yv, W), (H, 1))
    u, v = np.tile(bar(uv, W // 2), (H // 2, 1)), np.tile(bar(vv, W // 2), (H // 2, 1))
    if layout == yh.SEMI:
        c = np.empty((H // 2, W), np.uint16)
        c[:, 0::2], c[:, 1::2] = u, v
        return [y, c]
    return [y, u, v]
