"""The specification of pictures whose size is no multiple of 8 (ks265codec_amd/csrc/picture_window.hip), in numpy.

A picture is a packed I420 byte array: Y (h x w), then U and V (h/2 x w/2).  The source size W x H is even; the coded size is W and H rounded up to the minimum CU size, 8.
  pad_i420    np.pad(..., mode="edge") per plane: the last column and the last row replicated, on the right and at the bottom only
  crop_i420   the top-left W x H of every plane
  sse3        the three planes' sums of squared differences (exact integers)
  sse_window  sse3 of the crops; sse_strips what the padding contributes: sse_window + sse_strips = sse3 of the coded pictures
  conf_window the SPS's conf_win_{left,right,top,bottom}_offset, in chroma units (4:2:0: luma samples / 2)
"""
from __future__ import annotations

import numpy as np


def coded_size(w: int, h: int) -> tuple[int, int]:
    return (w + 7) & ~7, (h + 7) & ~7


def planes(pic: np.ndarray, w: int, h: int) -> list[np.ndarray]:
    """views of the Y, U, V planes of a packed I420 picture"""
    pic = np.asarray(pic, np.uint8).reshape(-1)
    assert w > 0 and h > 0 and w % 2 == 0 and h % 2 == 0 and pic.size == w * h * 3 // 2
    n, c = w * h, (w // 2) * (h // 2)
    return [pic[:n].reshape(h, w), pic[n:n + c].reshape(h // 2, w // 2), pic[n + c:].reshape(h // 2, w // 2)]


def pack(pl) -> np.ndarray:
    return np.concatenate([np.ascontiguousarray(p, np.uint8).reshape(-1) for p in pl])


def pad_planes(pl, w: int, h: int) -> np.ndarray:
    """Y, U, V planes of a w x h picture (any row layout) -> the packed I420 picture of the coded size"""
    cw, ch = coded_size(w, h)
    out = []
    for k, p in enumerate(pl):
        s = 1 if k == 0 else 2
        assert p.shape == (h // s, w // s)
        out.append(np.pad(p, ((0, (ch - h) // s), (0, (cw - w) // s)), mode="edge"))
    return pack(out)


def pad_i420(pic: np.ndarray, w: int, h: int) -> np.ndarray:
    return pad_planes(planes(pic, w, h), w, h)


def nv12_planes(y: np.ndarray, uv: np.ndarray) -> list[np.ndarray]:
    """Y (h x w) and interleaved UV (h/2 x w) -> Y, U, V"""
    return [y, uv[:, 0::2], uv[:, 1::2]]


def crop_i420(pic: np.ndarray, cw: int, ch: int, w: int, h: int) -> np.ndarray:
    assert w <= cw and h <= ch
    return pack([p[:h // s, :w // s] for p, s in zip(planes(pic, cw, ch), (1, 2, 2))])


def sse3(a: np.ndarray, b: np.ndarray, w: int, h: int) -> list[int]:
    return [int(((p.astype(np.int64) - q.astype(np.int64)) ** 2).sum()) for p, q in zip(planes(a, w, h), planes(b, w, h))]


def sse_window(a: np.ndarray, b: np.ndarray, cw: int, ch: int, w: int, h: int) -> list[int]:
    return sse3(crop_i420(a, cw, ch, w, h), crop_i420(b, cw, ch, w, h), w, h)


def sse_strips(a: np.ndarray, b: np.ndarray, cw: int, ch: int, w: int, h: int) -> list[int]:
    """the squared error of the samples outside the window: columns w .. of every row, rows h .. of the window's columns"""
    out = []
    for p, q, s in zip(planes(a, cw, ch), planes(b, cw, ch), (1, 2, 2)):
        d = (p.astype(np.int64) - q.astype(np.int64)) ** 2
        out.append(int(d[:, w // s:].sum() + d[h // s:, :w // s].sum()))
    return out


def conf_window(w: int, h: int) -> tuple[int, int, int, int]:
    cw, ch = coded_size(w, h)
    return 0, (cw - w) // 2, 0, (ch - h) // 2


def psnr(sse: int, samples: int) -> float:
    """as the encoder's lines and Encoder.quality() print it: 99.0 for a zero sum"""
    return 99.0 if sse == 0 else 10.0 * np.log10(255.0 * 255.0 * samples / sse)
