"""The specification of the analysis output (include/ks265_hip.h ks265_analysis_*), in numpy, and the input generators the CPU and GPU tests share.

A picture of W x H has w8 x h8 = W / 8 x H / 8 blocks of 8 x 8 luma samples and cc x cr = ceil(W / 64) x ceil(H / 64) CTUs.  From the picture's CU map (one ks265_cu8 record
per block), its per-CTU QP map, the POC deltas of its reference lists, and the source and reconstructed pictures:

  mv   int16 [2][h8][w8][2]   list L's vector (x, y) in quarter samples; (0, 0) where the block does not use the list or is intra
  ref  int8  [2][h8][w8]      POC(reference the block uses in list L) - POC(this picture); 0 = list unused or intra
  cu   uint8 [5][h8][w8]      kind (0 intra, 1 L0, 2 L1, 3 bi) | log2 CU size | partition (0 2Nx2N, 1 / 2 rectangular, 3 four TUs) | cbf (bit 0 Y, 1 Cb, 2 Cr) |
                              intra luma mode (255 = none)
  qp   int8  [cr][cc]         the CTU's QP
  sse  int32 [3][h8][w8]      squared error of the block's 8 x 8 luma, 4 x 4 Cb and 4 x 4 Cr samples

Skip and merge flags are decided by the slice writer on the host and never exist on the device: they are not part of the analysis."""
from __future__ import annotations

import numpy as np

CU8 = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("mv1x", "<i2"), ("mv1y", "<i2"), ("log2_cu", "u1"), ("cbf", "u1"), ("pred_mode", "u1"), ("inter_dir", "u1")])
SSE_MAX_LUMA, SSE_MAX_CHROMA = 64 * 255 * 255, 16 * 255 * 255


def dims(W: int, H: int):
    return W // 8, H // 8, (W + 63) // 64, (H + 63) // 64


def block_sse(a: np.ndarray, b: np.ndarray, n: int) -> np.ndarray:
    """sum of (a - b)^2 over the n x n blocks of two equal planes"""
    d = a.astype(np.int64) - b.astype(np.int64)
    h, w = d.shape
    return (d * d).reshape(h // n, n, w // n, n).sum(axis=(1, 3)).astype(np.int32)


def planes(i420: np.ndarray, W: int, H: int):
    i420 = np.asarray(i420, np.uint8).reshape(-1)
    return i420[:W * H].reshape(H, W), i420[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), i420[W * H * 5 // 4:W * H * 3 // 2].reshape(H // 2, W // 2)


def analysis(cu8_records, qp_map, picture_qp: int, deltas, src_i420, recon_i420, W: int, H: int) -> dict:
    """the five arrays; cu8_records: h8 * w8 CU8 records in raster order; qp_map: cr * cc int8 or None; deltas[L][i]: POC delta of list L's picture i"""
    w8, h8, cc, cr = dims(W, H)
    r = np.asarray(cu8_records).view(CU8).reshape(h8, w8)
    d = np.asarray(deltas, np.int8).reshape(2, 4)
    intra = r["pred_mode"] != 0
    direction = np.where(intra, 0, r["inter_dir"] & 3).astype(np.uint8)
    use = [(direction & 1) != 0, (direction & 2) != 0]
    idx = [(r["inter_dir"] >> 4) & 3, (r["inter_dir"] >> 6) & 3]
    mv = np.zeros((2, h8, w8, 2), np.int16)
    ref = np.zeros((2, h8, w8), np.int8)
    for L, (fx, fy) in enumerate((("mvx", "mvy"), ("mv1x", "mv1y"))):
        mv[L, ..., 0] = np.where(use[L], r[fx], 0)
        mv[L, ..., 1] = np.where(use[L], r[fy], 0)
        ref[L] = np.where(use[L], d[L][idx[L]], 0)
    cu = np.zeros((5, h8, w8), np.uint8)
    cu[0] = direction
    cu[1] = r["log2_cu"] & 15
    cu[2] = (r["log2_cu"] >> 4) & 3
    cu[3] = r["cbf"]
    cu[4] = np.where(r["pred_mode"] == 2, r["mvx"].astype(np.int32) & 255, 255)
    if qp_map is None:
        qp = np.full((cr, cc), picture_qp, np.int8)
    else:
        qp = np.asarray(qp_map, np.int8).reshape(cr, cc).copy()
    s, t = planes(src_i420, W, H), planes(recon_i420, W, H)
    sse = np.stack([block_sse(s[0], t[0], 8), block_sse(s[1], t[1], 4), block_sse(s[2], t[2], 4)])
    return {"mv": mv, "ref": ref, "cu": cu, "qp": qp, "sse": sse}


# ------------------------------------------------------------------ generators

DELTAS = ((-1, -3, -7, -128), (1, 2, 5, 127))          # distinct, non-zero, the int8 extremes included


def make_cu8(W: int, H: int, seed: int = 0) -> np.ndarray:
    """h8 * w8 records that walk, block after block, through: every kind (L0, L1, bi, the flat intra stand-in, intra with a mode), every (idx0, idx1) pair within each kind,
    CU sizes 3 .. 6, the four partition codes, every cbf; vectors random over int16 with +-32767 planted; intra records carry junk in the fields an intra block must not
    show (list-1 vector, inter_dir)"""
    w8, h8, _, _ = dims(W, H)
    n = w8 * h8
    rng = np.random.default_rng(seed)
    k = np.arange(n) + seed
    r = np.zeros(n, CU8)
    kind = k % 5                                        # 0 L0, 1 L1, 2 bi, 3 pred_mode 1, 4 pred_mode 2
    pair = (k // 5) % 16
    r["pred_mode"] = np.where(kind == 3, 1, np.where(kind == 4, 2, 0))
    direction = np.where(kind < 3, kind + 1, rng.integers(0, 4, n))
    r["inter_dir"] = direction | (pair & 3) << 4 | (pair >> 2) << 6
    r["log2_cu"] = (3 + k % 4) | ((k // 3) % 4) << 4
    r["cbf"] = (k // 2) % 8
    for f in ("mvx", "mvy", "mv1x", "mv1y"):
        v = rng.integers(-32767, 32768, n)
        ext = rng.integers(0, 6, n)
        r[f] = np.where(ext == 0, 32767, np.where(ext == 1, -32767, v))
    r["mvx"] = np.where(kind == 4, (k // 5) % 35, r["mvx"])
    return r


def make_pictures(W: int, H: int, seed: int = 0, extreme: bool = False):
    """(source, reconstruction) as packed I420: random bytes, or 0 against 255 (every block's sse at its maximum)"""
    n = W * H * 3 // 2
    if extreme:
        return np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
    rng = np.random.default_rng(seed + 1000)
    return rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)


def make_qp_map(W: int, H: int, seed: int = 0) -> np.ndarray:
    _, _, cc, cr = dims(W, H)
    return np.random.default_rng(seed + 2000).integers(-128, 128, cc * cr).astype(np.int8)


def moving_window_clip(W: int, H: int, n: int, dx: int = 6, dy: int = -2, seed: int = 7) -> list:
    """n packed I420 pictures: a W x H crop window that moves by (dx, dy) samples per picture over one larger low-pass filtered noise image, so the content moves by
    (-dx, -dy) and a block of picture t lies at +(dx, dy) in picture t - 1: its list-0 vector is (4 dx, 4 dy) quarter samples"""
    m = 16 + max(abs(dx), abs(dy)) * n
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (H + 2 * m, W + 2 * m)).astype(np.float64)
    for _ in range(3):                                  # three (1, 2, 1) / 4 passes each way: texture a few samples wide, nothing periodic
        big = (np.roll(big, 1, 0) + 2 * big + np.roll(big, -1, 0)) / 4
        big = (np.roll(big, 1, 1) + 2 * big + np.roll(big, -1, 1)) / 4
    big = (big - big.mean()) * (60.0 / big.std()) + 128
    big = np.clip(np.rint(big), 0, 255).astype(np.uint8)
    out = []
    for t in range(n):
        x0, y0 = m + dx * t, m + dy * t                 # inside the margin either way: m > max(|dx|, |dy|) n
        y = big[y0:y0 + H, x0:x0 + W]
        c = y.reshape(H // 2, 2, W // 2, 2).astype(np.int32).sum(axis=(1, 3))
        u = ((c + 2) >> 2).astype(np.uint8)
        out.append(np.concatenate([y.reshape(-1), u.reshape(-1), (255 - u).reshape(-1)]))
    return out
