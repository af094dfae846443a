"""TEST INFRASTRUCTURE: the specification of `vpp_denoise` / `vpp_recur_filter` (include/ks265_enc.h), in exact integer arithmetic: every byte that
ks265_input_denoise (ks265codec_amd/csrc/input_denoise.hip), its CPU stand-in (tests/hip_stub_denoise.c) and the encoder host produce is held to this file.

One step: the current packed I420 picture C of W x H (both multiples of 8: the coded size), the previous FILTERED picture P (the history) or None, thr T in 1..64 and
weight wmax in 1..30 (1/32 units) -> the filtered picture O, which is also the next history.
  * no history: O = C; every block reports the vector (0, 0), gated, SAD 0.
  * motion: luma blocks of 16x16 on a grid from (0, 0), the edge blocks the 8-wide / 8-tall remainder.  Candidates: integer (dx, dy), |dx|, |dy| <= RANGE = 8, whose displaced
    block lies wholly inside the picture (0 <= bx + dx, bx + dx + bw <= W, the same for y) - nothing outside the picture is ever read, the picture is not padded.
    cost = SAD(C block, P block at +d) + LAMBDA (|dx| + |dy|), LAMBDA = 16; the winner is the smallest (cost, |dx| + |dy|, dy, dx).  (0, 0) is always valid.
  * gate: winner's plain SAD >= T bw bh -> the block is C's, luma and both chroma planes.
  * luma: d = |c - p|, w = min(wmax, (2 wmax max(0, T - d)) // T), o = (c (32 - w) + p w + 16) >> 5, p = P at +d.
  * chroma, the plane's bw/2 x bh/2 block at (bx/2, by/2): whole-sample vector (dx >> 1, dy >> 1) (arithmetic), fx = dx & 1, fy = dy & 1,
    p = (h[y, x] + h[y, x + fx] + h[y + fy, x] + h[y + fy, x + fx] + 2) >> 2, the same blend with the threshold (T + 1) >> 1.
    The luma validity rule keeps every chroma read inside the plane: bx, bw, W even, so 0 <= bx + dx gives 0 <= bx/2 + (dx >> 1) (the floor of a non-negative half), and
    bx + dx + bw <= W with dx = 2 m + fx gives bx/2 + m + bw/2 <= (W - fx) / 2, i.e. the last column read, bx/2 + m + bw/2 - 1 + fx, is at most W/2 - 1.  chroma_reads()
    returns the index ranges and filter_picture asserts them.
blocks: one row per 16x16 block in raster order, (dx + 8 | (dy + 8) << 8 | gated << 16, plain SAD) - what ks265_input_denoise writes into dev_blocks."""
from __future__ import annotations

import numpy as np

RANGE, LAMBDA = 8, 16
LEVELS = {1: (6, 16), 2: (10, 20), 3: (16, 24)}


def level_params(denoise: int, recur: float = 0.0):
    """(T, wmax) of a handle's vpp_denoise / vpp_recur_filter, None when both are 0"""
    if not denoise and not recur > 0:
        return None
    t, w = LEVELS[denoise] if denoise else (10, 20)
    if recur > 0:
        w = min(30, max(1, int(np.floor(recur + 0.5))))
    return t, w


def planes(p: np.ndarray, w: int, h: int):
    p = np.asarray(p, np.uint8).reshape(-1)
    assert p.size == w * h * 3 // 2
    return p[:w * h].reshape(h, w), p[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), p[w * h * 5 // 4:].reshape(h // 2, w // 2)


def block_grid(w: int, h: int):
    """(bx, by, bw, bh) of every block, raster order"""
    return [(bx, by, min(16, w - bx), min(16, h - by)) for by in range(0, h, 16) for bx in range(0, w, 16)]


def candidates(bx, by, bw, bh, w, h):
    """the valid vectors as arrays dx, dy (any order)"""
    d = np.arange(-RANGE, RANGE + 1)
    dx, dy = np.meshgrid(d, d)
    dx, dy = dx.ravel(), dy.ravel()
    ok = (bx + dx >= 0) & (bx + dx + bw <= w) & (by + dy >= 0) & (by + dy + bh <= h)
    return dx[ok], dy[ok]


def search(cy, py, bx, by, bw, bh):
    """(dx, dy, plain SAD) of the block's winner"""
    h, w = cy.shape
    dx, dy = candidates(bx, by, bw, bh, w, h)
    ry, rx = np.arange(bh)[:, None], np.arange(bw)[None, :]
    ref = py[(by + dy)[:, None, None] + ry, (bx + dx)[:, None, None] + rx].astype(np.int32)       # candidates x bh x bw
    sad = np.abs(ref - cy[by:by + bh, bx:bx + bw].astype(np.int32)).sum(axis=(1, 2))
    l1 = np.abs(dx) + np.abs(dy)
    k = np.lexsort((dx, dy, l1, sad + LAMBDA * l1))[0]                  # the last key is the primary one
    return int(dx[k]), int(dy[k]), int(sad[k])


def blend(c, p, thr, wmax):
    c, p = c.astype(np.int32), p.astype(np.int32)
    w = np.minimum(wmax, (2 * wmax * np.maximum(0, thr - np.abs(c - p))) // thr)
    return ((c * (32 - w) + p * w + 16) >> 5).astype(np.uint8)


def chroma_reads(bx, by, bw, bh, dx, dy):
    """(x first, x last, y first, y last) of the chroma samples the block's prediction reads"""
    x0, y0 = bx // 2 + (dx >> 1), by // 2 + (dy >> 1)
    return x0, x0 + bw // 2 - 1 + (dx & 1), y0, y0 + bh // 2 - 1 + (dy & 1)


def chroma_pred(hp, bx, by, bw, bh, dx, dy):
    x0, x1, y0, y1 = chroma_reads(bx, by, bw, bh, dx, dy)
    assert 0 <= x0 and x1 < hp.shape[1] and 0 <= y0 and y1 < hp.shape[0], "a chroma read outside the plane"
    fx, fy, cw, ch = dx & 1, dy & 1, bw // 2, bh // 2
    a = hp[y0:y1 + 1, x0:x1 + 1].astype(np.int32)
    return (a[:ch, :cw] + a[:ch, fx:fx + cw] + a[fy:fy + ch, :cw] + a[fy:fy + ch, fx:fx + cw] + 2) >> 2


def filter_picture(cur, hist, w, h, thr, wmax):
    """(O packed, blocks int32 [n, 2])"""
    assert w > 0 and h > 0 and w % 8 == 0 and h % 8 == 0 and 1 <= thr <= 64 and 1 <= wmax <= 30
    cur = np.asarray(cur, np.uint8).reshape(-1)
    grid = block_grid(w, h)
    blocks = np.zeros((len(grid), 2), np.int32)
    if hist is None:
        blocks[:, 0] = 8 | 8 << 8 | 1 << 16
        return cur.copy(), blocks
    out = cur.copy()
    c3, p3, o3 = planes(cur, w, h), planes(hist, w, h), planes(out, w, h)
    tc = (thr + 1) >> 1
    for i, (bx, by, bw, bh) in enumerate(grid):
        dx, dy, sad = search(c3[0], p3[0], bx, by, bw, bh)
        gated = sad >= thr * bw * bh
        blocks[i] = (dx + 8) | (dy + 8) << 8 | int(gated) << 16, sad
        if gated:
            continue
        o3[0][by:by + bh, bx:bx + bw] = blend(c3[0][by:by + bh, bx:bx + bw], p3[0][by + dy:by + dy + bh, bx + dx:bx + dx + bw], thr, wmax)
        for k in (1, 2):
            cb = c3[k][by // 2:(by + bh) // 2, bx // 2:(bx + bw) // 2]
            o3[k][by // 2:(by + bh) // 2, bx // 2:(bx + bw) // 2] = blend(cb, chroma_pred(p3[k], bx, by, bw, bh, dx, dy), tc, wmax)
    return out, blocks


def filter_clip(pictures, w, h, thr, wmax, reset_at=()):
    """the recursion over a clip: picture t's history is picture t - 1's output; none for the first and for every t in reset_at"""
    out, hist = [], None
    for t, p in enumerate(pictures):
        if t in reset_at:
            hist = None
        hist, _ = filter_picture(p, hist, w, h, thr, wmax)
        out.append(hist)
    return out


def vectors(blocks):
    b = np.asarray(blocks)[:, 0]
    return (b & 255) - 8, (b >> 8 & 255) - 8, b >> 16 & 1


def psnr(a, b):
    e = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if e == 0 else 10 * np.log10(255.0 ** 2 / e)


def synthetic_clip(w=104, h=72, n=10, seed=5, sigma=4.0, pan=(3, 1)):
    """(clean, noisy): n packed I420 pictures each.  A field of uniform random values on a 4x4-replicated grid, box-blurred with 5 taps along both axes, panned by `pan` per
    picture; U = the 2x2 luma mean / 2 + 64, V = 255 - U; the noise is Gaussian, rounded and clipped"""
    rng = np.random.default_rng(seed)
    fw, fh = w + pan[0] * n + 16, h + pan[1] * n + 16
    f = np.repeat(np.repeat(rng.integers(0, 256, ((fh + 3) // 4, (fw + 3) // 4)).astype(np.float64), 4, axis=0), 4, axis=1)[:fh, :fw]
    k = np.ones(5) / 5
    f = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, f)
    f = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, f)
    clean, noisy = [], []
    for t in range(n):
        y = f[8 + pan[1] * t:8 + pan[1] * t + h, 8 + pan[0] * t:8 + pan[0] * t + w]
        u = (y[0::2, 0::2] + y[0::2, 1::2] + y[1::2, 0::2] + y[1::2, 1::2]) / 4 / 2 + 64
        pl = [y, u, 255 - u]
        clean.append(np.concatenate([np.clip(np.rint(q), 0, 255).astype(np.uint8).ravel() for q in pl]))
        noisy.append(np.concatenate([np.clip(np.rint(q + rng.normal(0, sigma, q.shape)), 0, 255).astype(np.uint8).ravel() for q in pl]))
    return clean, noisy
