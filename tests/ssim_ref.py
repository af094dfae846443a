"""The SSIM of the reference's `-ssim` line, in NumPy: the specification the device kernel (ks265_ssim_picture) and the encoder's ` ssim:` line are
checked against, itself pinned on the reference's printed numbers by tests/test_ssim_ref.py (tests/golden/ssim_ref.npz).

Per plane: 8x8 windows, non-overlapping, from sample (0, 0); a window that does not lie wholly inside the plane is dropped (a 100x68 chroma plane has 12 x 8 windows).
Per window, from the exact integer sums sa = sum a, sb = sum b, saa = sum a^2, sbb = sum b^2, sab = sum a b (n = 64 samples):
    mu_a = sa / n, var_a = saa / n - mu_a^2 (population), cov = sab / n - mu_a mu_b
    ssim = (2 mu_a mu_b + C1) (2 cov + C2) / ((mu_a^2 + mu_b^2 + C1) (var_a + var_b + C2)),  C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2
which this file evaluates with everything multiplied through by n^2 = 4096, so that the four factors are exact in float64 up to the constants' rounding:
    ssim = (2 sa sb + n^2 C1) (2 (n sab - sa sb) + n^2 C2) / ((sa^2 + sb^2 + n^2 C1) (n (saa + sbb) - sa^2 - sb^2 + n^2 C2))
Plane value = mean over the plane's windows; stream value = mean over the pictures of the plane values."""
from __future__ import annotations

import numpy as np

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2
K1 = 4096.0 * C1                  # the constants at the scale of the integer forms (x n^2); the device kernel holds the same two doubles
K2 = 4096.0 * C2
FIX = 1 << 30                     # fixed point of the device's per-plane sums


def window_sums(a: np.ndarray, b: np.ndarray):
    """a, b: uint8 [h, w].  Returns the five int64 arrays [h // 8, w // 8] of the whole windows."""
    h, w = a.shape
    nh, nw = h // 8, w // 8
    A = a[:nh * 8, :nw * 8].astype(np.int64).reshape(nh, 8, nw, 8)
    B = b[:nh * 8, :nw * 8].astype(np.int64).reshape(nh, 8, nw, 8)
    s = lambda x: x.sum(axis=(1, 3))
    return s(A), s(B), s(A * A), s(B * B), s(A * B)


def window_ssim(sa, sb, saa, sbb, sab) -> np.ndarray:
    """float64 SSIM of every window from its integer sums (the order of operations is the device kernel's)"""
    sa = np.asarray(sa, np.int64); sb = np.asarray(sb, np.int64)
    pab = (sa * sb).astype(np.float64)                         # < 2^28: exact
    paa = (sa * sa + sb * sb).astype(np.float64)               # < 2^29: exact
    cov = (64 * np.asarray(sab, np.int64) - sa * sb).astype(np.float64)
    var = (64 * (np.asarray(saa, np.int64) + np.asarray(sbb, np.int64)) - sa * sa - sb * sb).astype(np.float64)
    num = (2.0 * pab + K1) * (2.0 * cov + K2)
    den = (paa + K1) * (var + K2)
    return num / den


def plane_ssim(a: np.ndarray, b: np.ndarray):
    """(windows, mean SSIM, sum over the windows of llrint(ssim * 2^30)) of one plane"""
    v = window_ssim(*window_sums(a, b))
    fixed = int(np.rint(v * FIX).astype(np.int64).sum())       # rint: to nearest even, as llrint in the default rounding mode
    return v.size, float(v.mean()) if v.size else 0.0, fixed


def planes_of(i420: np.ndarray, W: int, H: int):
    i420 = np.asarray(i420, np.uint8).reshape(-1)
    return (i420[:W * H].reshape(H, W), i420[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), i420[W * H * 5 // 4:W * H * 3 // 2].reshape(H // 2, W // 2))


def picture_ssim(a_i420: np.ndarray, b_i420: np.ndarray, W: int, H: int):
    """three (windows, mean, fixed sum) tuples: Y, U, V"""
    return [plane_ssim(pa, pb) for pa, pb in zip(planes_of(a_i420, W, H), planes_of(b_i420, W, H))]


def stream_ssim(a: np.ndarray, b: np.ndarray, W: int, H: int) -> np.ndarray:
    """a, b: [pictures, W * H * 3 / 2].  The three numbers of the ` ssim:` line: the mean over the pictures of the plane values."""
    a = np.asarray(a, np.uint8).reshape(-1, W * H * 3 // 2); b = np.asarray(b, np.uint8).reshape(-1, W * H * 3 // 2)
    return np.mean([[m for _, m, _ in picture_ssim(x, y, W, H)] for x, y in zip(a, b)], axis=0)
