"""Specification of the overlay stage (ks265codec_amd/csrc/input_overlay.hip, ks265_enc_set_overlay of include/ks265_enc.h): pictures of RGB plus alpha - logos,
captions, a picture in picture - blended onto the packed I420 picture of an input slot in exact integer arithmetic, next to tests/yuv_convert_ref.py (its matrices, its
ranges, its Q16 coefficients, its chroma filter) and tests/yuv_float_ref.py (q of a float sample).

  overlay  w x h samples (both even, >= 2) with the top-left corner at (x, y) of the picture (both even, any sign, may reach past the picture: what lies outside the
           window is clipped).  8-bit codes R, G, B, a; no alpha channel: a = 255.  Float samples are reduced to codes first: code = (q + 128) >> 8 (q of yuv_float_ref),
           so a float32 overlay u8 / 255 IS the u8 overlay.  opacity 0 .. 256:  A = (a * opacity + 128) >> 8  (0 .. 255).
  luma     Y' = clip255((Y (255 - A) 65536 + A (cy . RGB + (oy << 16)) + 255 * 32768) // (255 * 65536))
  chroma   premultiplied, so the colour of a transparent pixel never bleeds into its neighbours: SA, SAR, SAG, SAB = the (1, 2, 1) x (1, 1) sums (weight 8, HEVC's default
           siting) of A, A R, A G, A B over the OVERLAY AS A PICTURE OF ITS OWN - columns clamp to the overlay's edges as yuv_convert_ref's chroma_sum clamps them; the
           sums never look at the picture, so clipping removes samples and changes none of those that remain.  With D = 2040 * 65536 (SA <= 8 * 255):
           Cb' = clip255((Cb (2040 - SA) 65536 + cb . (SAR, SAG, SAB) + 128 * 65536 * SA + D // 2) // D),  Cr' the same with cr.
           Chroma sample (i, j) of the overlay lands on chroma sample (y / 2 + i, x / 2 + j) of the picture.
  window   the rectangle is clipped to win_w x win_h (both even): the picture's size, or on a handle whose size is no multiple of 8 picWidth x picHeight inside the coded
           picture - the padding keeps the bytes it had.
  order    several overlays are blended one after the other in ascending slot number; where they overlap the later one lies on top of the earlier one's result.
  int64 throughout, floor division.

A = 0 (or opacity 0) leaves every byte as it was; A = 255 everywhere gives exactly yuv_convert_ref.rgb_to_i420 of the overlay (the 255 and the 2040 cancel)."""
from __future__ import annotations

import numpy as np

import yuv_float_ref as yf
from yuv_convert_ref import MATRIX_BT601, MATRIX_BT709, coefficients  # noqa: F401

D = 2040 * 65536


def codes(samples: np.ndarray, fmt: int | None = None) -> np.ndarray:
    """samples of a format -> 8-bit codes (int64): uint8 as they are (fmt None), float samples (yuv_float_ref's formats) through q"""
    if fmt is None:
        assert np.asarray(samples).dtype == np.uint8
        return np.asarray(samples, np.int64)
    return (yf.q(yf.to_f32(samples, fmt)) + 128) >> 8


def overlay(r, g, b, a=None, x=0, y=0, opacity=256, matrix=MATRIX_BT709, full_range=False) -> dict:
    """an overlay of (h, w) planes of codes (codes()); a None: opaque"""
    r, g, b = (np.asarray(c, np.int64) for c in (r, g, b))
    a = np.full(r.shape, 255, np.int64) if a is None else np.asarray(a, np.int64)
    h, w = r.shape
    assert r.shape == g.shape == b.shape == a.shape and w >= 2 and h >= 2 and not (w | h | x | y) & 1 and 0 <= opacity <= 256
    return {"r": r, "g": g, "b": b, "a": a, "x": x, "y": y, "opacity": opacity, "matrix": matrix, "full_range": full_range}


def effective_alpha(a: np.ndarray, opacity: int) -> np.ndarray:
    return (np.asarray(a, np.int64) * opacity + 128) >> 8


def chroma_sum(C: np.ndarray) -> np.ndarray:
    """yuv_convert_ref's (1, 2, 1) x (1, 1) sum, in int64"""
    left = np.concatenate([C[:, :1], C[:, :-1]], axis=1)
    right = np.concatenate([C[:, 1:], C[:, -1:]], axis=1)
    hsum = (left + 2 * C + right)[:, 0::2]
    return hsum[0::2] + hsum[1::2]


def overlay_luma(ov: dict) -> np.ndarray:
    """the overlay's own luma, cy . RGB + (oy << 16) rounded as yuv_convert_ref rounds it (int64, clipped): what Y' moves towards"""
    k = coefficients(ov["matrix"], ov["full_range"])
    return np.clip((k["cy"][0] * ov["r"] + k["cy"][1] * ov["g"] + k["cy"][2] * ov["b"] + (k["oy"] << 16) + 32768) >> 16, 0, 255)


def blend_one(i420: np.ndarray, W: int, H: int, ov: dict, win_w: int | None = None, win_h: int | None = None) -> np.ndarray:
    """one overlay onto a packed I420 picture of W x H (flat uint8), clipped to the window; returns a new array"""
    win_w = W if win_w is None else win_w
    win_h = H if win_h is None else win_h
    assert not (W | H | win_w | win_h) & 1 and win_w <= W and win_h <= H
    out = np.array(i420, np.uint8).copy()
    npx = W * H
    Y = out[:npx].reshape(H, W)
    U = out[npx:npx + npx // 4].reshape(H // 2, W // 2)
    V = out[npx + npx // 4:].reshape(H // 2, W // 2)
    k = coefficients(ov["matrix"], ov["full_range"])
    R, G, B = ov["r"], ov["g"], ov["b"]
    A = effective_alpha(ov["a"], ov["opacity"])
    h, w = R.shape
    x, y = ov["x"], ov["y"]
    # the part of the overlay that lies inside the window: rows r0 .. r1, columns c0 .. c1 of the overlay (all even)
    c0, c1, r0, r1 = max(0, -x), min(w, win_w - x), max(0, -y), min(h, win_h - y)
    if c0 >= c1 or r0 >= r1:
        return out
    lum = k["cy"][0] * R + k["cy"][1] * G + k["cy"][2] * B + (k["oy"] << 16)
    sel = (slice(r0, r1), slice(c0, c1))
    dst = (slice(y + r0, y + r1), slice(x + c0, x + c1))
    Yn = (Y[dst].astype(np.int64) * (255 - A[sel]) * 65536 + A[sel] * lum[sel] + 255 * 32768) // (255 * 65536)
    Y[dst] = np.clip(Yn, 0, 255).astype(np.uint8)
    SA, SAR, SAG, SAB = chroma_sum(A), chroma_sum(A * R), chroma_sum(A * G), chroma_sum(A * B)
    csel = (slice(r0 // 2, r1 // 2), slice(c0 // 2, c1 // 2))
    cdst = (slice((y + r0) // 2, (y + r1) // 2), slice((x + c0) // 2, (x + c1) // 2))
    for P, c in ((U, k["cb"]), (V, k["cr"])):
        Cn = (P[cdst].astype(np.int64) * (2040 - SA[csel]) * 65536 + c[0] * SAR[csel] + c[1] * SAG[csel] + c[2] * SAB[csel] + 128 * 65536 * SA[csel] + D // 2) // D
        P[cdst] = np.clip(Cn, 0, 255).astype(np.uint8)
    return out


def blend(i420: np.ndarray, W: int, H: int, overlays, win_w: int | None = None, win_h: int | None = None) -> np.ndarray:
    """the overlays (a list in ascending slot order; None entries are empty slots) onto a packed I420 picture"""
    out = np.array(i420, np.uint8).copy()
    for ov in overlays:
        if ov is not None:
            out = blend_one(out, W, H, ov, win_w, win_h)
    return out
