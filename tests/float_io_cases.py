"""Shared by the tests of the float sample formats (tests/yuv_float_ref.py): samples as bit patterns, pictures placed into raw buffers in every layout, the descriptor of each.
Nothing here needs a GPU; the GPU tests upload the buffers as bytes."""
from __future__ import annotations

import ctypes as C

import numpy as np

import yuv_float_ref as fref

FORMATS = (fref.IN_RGB_F16, fref.IN_RGB_BF16, fref.IN_RGB_F32)
NAMES = {fref.IN_RGB_F16: "f16", fref.IN_RGB_BF16: "bf16", fref.IN_RGB_F32: "f32"}
# name -> (elements per pixel, element index of R, G, B inside the pixel); planar: three planes
PIXELS = {"planar": (1, None), "hwc": (3, (0, 1, 2)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0))}
ONE = {fref.IN_RGB_F16: 0x3C00, fref.IN_RGB_BF16: 0x3F80, fref.IN_RGB_F32: 0x3F800000}
KS265_OK, KS265_POINTER, KS265_NOTSUPPORTED = 0, -3, -4


class InDesc(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


def elem_dtype(fmt: int):
    return np.uint32 if fmt == fref.IN_RGB_F32 else np.uint16


def bits_to_f32(bits: np.ndarray, fmt: int) -> np.ndarray:
    """bit patterns (uint16 / uint32) -> the samples as float32"""
    if fmt == fref.IN_RGB_F32:
        return np.ascontiguousarray(bits, np.uint32).view(np.float32)
    if fmt == fref.IN_RGB_BF16:
        return fref.bf16_to_f32(bits)
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float32)


def f32_to_bits(x: np.ndarray, fmt: int) -> np.ndarray:
    """float32 samples -> the bit patterns of the format (round to nearest even)"""
    x = np.ascontiguousarray(x, np.float32)
    if fmt == fref.IN_RGB_F32:
        return x.view(np.uint32)
    if fmt == fref.IN_RGB_BF16:
        return fref.f32_to_bf16(x)
    return x.astype(np.float16).view(np.uint16)


def sample_bits(code: np.ndarray, fmt: int) -> np.ndarray:
    """the bit patterns of the output samples of bytes `code`"""
    s = fref.code_to_sample(code, fmt)
    return s.view(np.uint32) if fmt == fref.IN_RGB_F32 else s.view(np.uint16)


def layout(fmt: int, pixel: str, W: int, H: int, pad: int, off: int, fill: int = 0xA5):
    """an empty picture in a raw buffer: returns (buf, views, plane offsets, pitch, step) - buf a uint8 array filled with `fill`, views[c] an (H, W) element view of channel c
    inside it, the offsets of pixel (0, 0)'s R, G, B in bytes from buf's start, pitch and step in bytes.  `pad` elements lie behind every row, `off` elements in front of the
    picture (off = 0: the picture begins where the buffer does)."""
    E = elem_dtype(fmt)
    es = E().itemsize
    n, order = PIXELS[pixel]
    row = W * (n if order is not None else 1) + pad                    # elements
    planes = 1 if order is not None else 3
    total = off + planes * H * row + 8
    buf = np.full(total * es, fill, np.uint8)
    el = buf.view(E)
    if order is None:
        views = [el[off + k * H * row: off + (k + 1) * H * row].reshape(H, row)[:, :W] for k in range(3)]
        offs = [(off + k * H * row) * es for k in range(3)]
        step = es
    else:
        px = el[off: off + H * row].reshape(H, row)[:, :W * n].reshape(H, W, n)
        assert np.shares_memory(px, buf)
        views = [px[:, :, order[k]] for k in range(3)]
        offs = [(off + order[k]) * es for k in range(3)]
        step = n * es
    return buf, views, offs, row * es, step


def describe(fmt: int, W: int, H: int, base: int, offs, pitch: int, step: int, matrix: int = 0, full: int = 0) -> InDesc:
    d = InDesc()
    d.format, d.width, d.height, d.pixel_step, d.matrix, d.full_range = fmt, W, H, step, matrix, int(full)
    for k in range(3):
        d.plane[k] = base + offs[k]
    d.pitch[0] = pitch
    return d


def random_bits(rng, fmt: int, shape) -> np.ndarray:
    """samples that exercise the range: most in [0, 1], some beyond it on both sides, a few special values"""
    x = rng.random(shape, dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
    flat = x.reshape(-1)
    sp = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.0, -1.0, 1e-40, 6e-8, 1 / 512, 3 / 512, 1 / 255, 254 / 255])
    idx = rng.integers(0, flat.size, 4 * sp.size)
    flat[idx] = np.tile(sp, 4)
    with np.errstate(all="ignore"):
        return f32_to_bits(x, fmt)
