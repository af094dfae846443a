"""Specification of the device-input scaler (ks265codec_amd/csrc/input_scale.hip, ks265codec_amd/host/ks265_scale.h): a packed I420 picture of one size into a packed
I420 picture of another, separable, in exact integer arithmetic.

  per axis  S source samples, D destination samples, S / D and D / S at most 8; q = 2 max(S, D)
  siting    centre:  m = (2k + 1) D - (2j + 1) S     luma both ways, chroma vertically
            cosited: m = 2 (k D - j S)               chroma horizontally (HEVC's default siting, as yuv_convert_ref.py and yuv_output_ref.py assume), with the chroma
                                                     planes' own S and D: a chroma sample keeps its place on the luma grid
  weights   int64, x = |m|:   0 triangle     n = max(0, q - x)                                  support q
                              1 Catmull-Rom  n = 3 x^3 - 5 q x^2 + 2 q^3          x < q         support 2 q
                                             n = -x^3 + 5 q x^2 - 8 q^2 x + 4 q^3  q <= x < 2 q
  taps      of output j: the k in [0, S) with x inside the support (taps outside the source are dropped, not replicated), less the leading and the trailing ones of
            weight 0 (the cubic's zero at x = q: with S = D only k = j stays).  first[j] = the lowest, T = the largest count of the axis (at most MAX_TAPS)
  Q14       N = sum n;  c = floor((2 * 16384 n + N) / (2 N));  16384 - sum c goes to the first tap with the largest n.  Entries behind an output's count are 0.
            A table with sum |c| > 2 * 16384 for any output is refused (ValueError)
  samples   int32:  h(y, j) = (sum_i cx[j][i] p(y, first_x[j] + i) + 128) >> 8        (6 fractional bits, |h| <= 32640)
                    v       = sum_i cy[r][i] h(first_y[r] + i, j)                      (|v| < 2^31)
                    out     = clip255((v + 2^19) >> 20)
  sources   I420 and NV12 scale their planes; RGB is converted to I420 at the source's size first (yuv_convert_ref.rgb_to_i420, unchanged) and that picture is scaled.
"""
from __future__ import annotations

import numpy as np

TRIANGLE, CATMULL_ROM = 0, 1
MAX_TAPS = 36
MAX_DIM = 8192
MAX_RATIO = 8
ONE = 16384


def size_ok(sw: int, sh: int, dw: int, dh: int) -> bool:
    """the size rules: source width a multiple of 8 and height even, destination multiples of 8, both at most 8192, ratios at most 8 either way"""
    if sw <= 0 or sh <= 0 or dw <= 0 or dh <= 0 or sw % 8 or sh % 2 or dw % 8 or dh % 8 or max(sw, sh, dw, dh) > MAX_DIM:
        return False
    return sw <= MAX_RATIO * dw and dw <= MAX_RATIO * sw and sh <= MAX_RATIO * dh and dh <= MAX_RATIO * sh


def weights(x: np.ndarray, q: int, filt: int) -> np.ndarray:
    """n of |m| = x (int64); x is limited to the support first, so that no power leaves int64"""
    x = np.minimum(np.asarray(x, np.int64), np.int64(2 * q))
    q = np.int64(q)
    if filt == TRIANGLE:
        return np.maximum(np.int64(0), q - x)
    inner = 3 * x * x * x - 5 * q * x * x + 2 * q * q * q
    outer = -x * x * x + 5 * q * x * x - 8 * q * q * x + 4 * q * q * q
    return np.where(x < q, inner, np.where(x < 2 * q, outer, np.int64(0)))


def table(S: int, D: int, filt: int = CATMULL_ROM, cosited: bool = False):
    """(first int32[D], coef int16[D, T], T) of one axis"""
    if filt not in (TRIANGLE, CATMULL_ROM) or S <= 0 or D <= 0 or S > MAX_RATIO * D or D > MAX_RATIO * S or max(S, D) > MAX_DIM:
        raise ValueError("scale: filter 0 or 1, ratios at most 8, lengths at most 8192")
    q = 2 * max(S, D)
    R = q if filt == TRIANGLE else 2 * q
    j = np.arange(D, dtype=np.int64)
    a = 2 * D                                                   # m = a k + b
    b = -2 * j * S if cosited else D - (2 * j + 1) * S
    lo = np.maximum((-R - b) // a + 1, 0)                       # a k + b > -R
    hi = np.minimum(-((b - R) // a) - 1, S - 1)                 # a k + b < R
    T0 = int((hi - lo).max()) + 1
    i = np.arange(T0, dtype=np.int64)
    k = lo[:, None] + i[None, :]
    valid = k <= hi[:, None]
    n = np.where(valid, weights(np.abs(a * k + b[:, None]), q, filt), 0)
    nz = n != 0
    assert nz.any(axis=1).all()
    lead = nz.argmax(axis=1)                                    # leading taps of weight 0
    last = T0 - 1 - nz[:, ::-1].argmax(axis=1)
    cnt = last - lead + 1
    T = int(cnt.max())
    if T > MAX_TAPS:
        raise ValueError("scale: more taps than MAX_TAPS")
    idx = np.minimum(lead[:, None] + np.arange(T)[None, :], T0 - 1)
    live = np.arange(T)[None, :] < cnt[:, None]
    n = np.where(live, np.take_along_axis(n, idx, axis=1), 0)
    first = lo + lead
    N = n.sum(axis=1, keepdims=True)
    assert (N > 0).all()
    c = np.where(live, (2 * ONE * n + N) // (2 * N), 0)
    fix = ONE - c.sum(axis=1)
    c[np.arange(D), n.argmax(axis=1)] += fix                    # argmax: the first of the largest
    if (np.abs(c).sum(axis=1) > 2 * ONE).any():
        raise ValueError("scale: sum |c| above 2 * 16384")
    assert (c.sum(axis=1) == ONE).all() and np.abs(c).max() < 32768
    return first.astype(np.int32), c.astype(np.int16), T


def tables(sw: int, sh: int, dw: int, dh: int, filt: int = CATMULL_ROM) -> dict:
    """the four tables of a picture: luma x, luma y, chroma x (cosited), chroma y"""
    if not size_ok(sw, sh, dw, dh):
        raise ValueError("scale: size outside the rules")
    return {"lx": table(sw, dw, filt), "ly": table(sh, dh, filt), "cx": table(sw // 2, dw // 2, filt, True), "cy": table(sh // 2, dh // 2, filt)}


def scale_plane(p: np.ndarray, tx, ty) -> np.ndarray:
    """one (H, W) uint8 plane through the table of its x axis, then of its y axis"""
    fx, cx, Tx = tx
    fy, cy, Ty = ty
    p = np.asarray(p, np.int32)
    H, W = p.shape
    acc = np.zeros((H, len(fx)), np.int32)
    for i in range(Tx):                                         # (entries behind an output's count are 0: the clamped index is never weighted)
        acc += cx[:, i].astype(np.int32)[None, :] * p[:, np.minimum(fx + i, W - 1)]
    h = (acc + np.int32(128)) >> 8
    assert np.abs(h).max() <= 32640
    v = np.zeros((len(fy), len(fx)), np.int64)
    for i in range(Ty):
        v += cy[:, i].astype(np.int64)[:, None] * h[np.minimum(fy + i, H - 1), :]
    assert np.abs(v).max() < 2 ** 31 - 2 ** 19
    return np.clip((v.astype(np.int32) + np.int32(1 << 19)) >> 20, 0, 255).astype(np.uint8)


def scale_i420(i420: np.ndarray, sw: int, sh: int, dw: int, dh: int, filt: int = CATMULL_ROM) -> np.ndarray:
    """packed I420 sw x sh (flat uint8) -> packed I420 dw x dh"""
    t = tables(sw, sh, dw, dh, filt)
    i420 = np.asarray(i420, np.uint8).ravel()
    assert i420.size == sw * sh * 3 // 2
    n = sw * sh
    y = scale_plane(i420[:n].reshape(sh, sw), t["lx"], t["ly"])
    u = scale_plane(i420[n:n + n // 4].reshape(sh // 2, sw // 2), t["cx"], t["cy"])
    v = scale_plane(i420[n + n // 4:].reshape(sh // 2, sw // 2), t["cx"], t["cy"])
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def scale_rgb(r: np.ndarray, g: np.ndarray, b: np.ndarray, dw: int, dh: int, filt: int = CATMULL_ROM, matrix: int = 0, full_range: bool = False) -> np.ndarray:
    """three (H, W) uint8 planes -> packed I420 dw x dh: the conversion at the source's size, then the scaler"""
    from yuv_convert_ref import rgb_to_i420
    sh, sw = r.shape
    return scale_i420(rgb_to_i420(r, g, b, matrix, full_range), sw, sh, dw, dh, filt)


# the axis pairs (S, D) every table test walks: the ladder (2160p -> 1080p, 720p; 1080p -> 720p), odd ratios, ratio 8 both ways, S = D, short axes
AXIS_PAIRS = [(3840, 1920), (3840, 1280), (2160, 1080), (2160, 720), (1920, 1280), (1080, 720), (1920, 960), (1080, 540), (200, 128), (136, 72), (100, 64), (68, 36),
              (512, 64), (256, 32), (64, 512), (8, 64), (4, 32), (64, 104), (64, 88), (32, 52), (32, 44), (64, 64), (8, 8), (4, 4), (4096, 2048), (16, 8), (2048, 1024),
              (8192, 1024), (1024, 8192), (8192, 8192), (7, 5), (5, 7), (1, 1), (1, 8), (8, 1), (24, 16), (1000, 136)]
