"""GPU: the encoder's packed I420 into float RGB pictures (ks265_output_convert with KS265_IN_RGB_F16 / _BF16 / _F32, ks265codec_amd/csrc/output_convert.hip) against the
definition in tests/yuv_float_ref.py - the byte tests/yuv_output_ref.py defines, over 255, correctly rounded - bit pattern for bit pattern:
  * every type x planar / HWC / four-element pixels in both orders x both matrices x both ranges, at 8x2, 26x6 (a ragged right edge) and 520x10, the picture on 16 bytes and
    off them by one element, a pitch that is no multiple of 16;
  * a full-range grey ramp drives every channel through all 256 codes (the kernel's division, exhaustively); a random picture covers the rest;
  * the fourth element of a four-element pixel is 1.0; every byte behind a row and around the picture keeps its 0xA5;
  * refusals enqueue nothing."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import float_io_cases as fc  # noqa: E402
import yuv_convert_ref as cref  # noqa: E402
import yuv_float_ref as fref  # noqa: E402
import yuv_output_ref as oref  # noqa: E402

SHAPES = [(8, 2), (26, 6), (520, 10)]
PLACES = [(0, 8), (1, 8), (0, 3)]             # (elements in front of the picture, elements behind every row)
CASES = [(m, f) for m in (cref.MATRIX_BT709, cref.MATRIX_BT601) for f in (0, 1)]


@pytest.fixture(scope="module")
def hip():
    from ks265codec_amd.lib import load_library
    lib = load_library()
    lib.ks265_last_error.restype = C.c_char_p
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    yield lib, h
    lib.ks265_destroy(h)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pictures(W, H):
    """a full-range grey ramp (U = V = 128: R = G = B = Y, all 256 codes where the picture has 256 samples) and a random picture"""
    n = W * H
    ramp = np.concatenate([(np.arange(n) * 7 % 256).astype(np.uint8), np.full(n // 2, 128, np.uint8)])
    rnd = np.random.default_rng(n).integers(0, 256, n * 3 // 2, dtype=np.uint8)
    return [("ramp", ramp), ("random", rnd)]


def _expected(fmt, pixel, planes, W, H, pad, off):
    """the whole destination buffer as it must look afterwards: 0xA5 everywhere but the samples (and the fourth elements)"""
    buf, views, offs, pitch, step = fc.layout(fmt, pixel, W, H, pad, off)
    n, order = fc.PIXELS[pixel]
    if n == 4:                                                          # the element no channel names, through a view of the whole pixels
        E = fc.elem_dtype(fmt)
        row = pitch // E().itemsize
        px = buf.view(E)[off: off + H * row].reshape(H, row)[:, :W * 4].reshape(H, W, 4)
        assert np.shares_memory(px, buf)
        px[:, :, 3] = fc.ONE[fmt]
    for k in range(3):
        views[k][:] = fc.sample_bits(planes[k], fmt)
    return buf, offs, pitch, step


def _convert(hip, src_dev, desc, size, want=0):
    lib, h = hip
    dst = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    for k in range(3):
        desc.plane[k] = (desc.plane[k] or 0) + dst.data_ptr()
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = lib.ks265_output_convert(h, C.c_void_p(src_dev.data_ptr()), C.byref(desc))
    assert rc == want, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    return dst.cpu().numpy()


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("fmt", fc.FORMATS, ids=[fc.NAMES[f] for f in fc.FORMATS])
def test_every_layout_equals_the_definition(hip, fmt, W, H):
    for label, pic in _pictures(W, H):
        src = _dev(pic)
        for matrix, full in CASES:
            planes = oref.i420_to_rgb(pic, W, H, matrix, bool(full))
            if label == "ramp" and full and W * H >= 256:
                assert all(len(np.unique(c)) == 256 for c in planes)
            for pixel in fc.PIXELS:
                for off, pad in PLACES:
                    exp, offs, pitch, step = _expected(fmt, pixel, planes, W, H, pad, off)
                    got = _convert(hip, src, fc.describe(fmt, W, H, 0, offs, pitch, step, matrix, full), exp.size)
                    assert (got == exp).all(), (fc.NAMES[fmt], label, pixel, matrix, full, off, pad, int((got != exp).sum()))


@pytest.mark.parametrize("fmt", fc.FORMATS, ids=[fc.NAMES[f] for f in fc.FORMATS])
def test_float_times_255_is_the_uint8_reconstruction(hip, fmt):
    """what the definition is for, through torch's own types: the uint8 kernel's picture equals the float kernel's x 255 (exactly for float32)"""
    W, H = 64, 16
    pic = _pictures(W, H)[1][1]
    src = _dev(pic)
    dt = {fref.IN_RGB_F16: torch.float16, fref.IN_RGB_BF16: torch.bfloat16, fref.IN_RGB_F32: torch.float32}[fmt]
    es = fref.ELEM_SIZE[fmt]
    lib, h = hip
    u8 = torch.zeros((3, H, W), dtype=torch.uint8, device="cuda")
    fl = torch.zeros((3, H, W), dtype=dt, device="cuda")
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    d8 = fc.describe(2, W, H, u8.data_ptr(), [k * W * H for k in range(3)], W, 1)
    df = fc.describe(fmt, W, H, fl.data_ptr(), [es * k * W * H for k in range(3)], es * W, es)
    assert lib.ks265_output_convert(h, C.c_void_p(src.data_ptr()), C.byref(d8)) == 0
    assert lib.ks265_output_convert(h, C.c_void_p(src.data_ptr()), C.byref(df)) == 0
    assert lib.ks265_synchronize(h) == 0
    assert torch.equal(fl.cpu(), (u8.cpu().float() / 255).to(dt))      # (the division on the host: it is correctly rounded there, torch's GPU kernel multiplies by 1 / 255)
    assert torch.equal((fl.float() * 255).round().to(torch.uint8), u8)
    if fmt == fref.IN_RGB_F32:
        assert torch.equal(fl * 255, u8.float())


def test_refusals_enqueue_nothing(hip):
    lib, h = hip
    W, H = 8, 2
    src = _dev(_pictures(W, H)[1][1])
    for fmt in fc.FORMATS:
        es = fref.ELEM_SIZE[fmt]
        buf, views, offs, pitch, step = fc.layout(fmt, "rgba", W, H, 8, 0)
        ok = lambda: fc.describe(fmt, W, H, 0, offs, pitch, step)
        assert not (_convert(hip, src, ok(), buf.size) == 0xA5).all()
        bad = []
        x = ok(); x.plane[1] = x.plane[1] + 1; bad.append((x, fc.KS265_NOTSUPPORTED))               # a pointer off its element size
        x = ok(); x.pitch[0] = pitch + 1; bad.append((x, fc.KS265_NOTSUPPORTED))                    # the pitch
        x = ok(); x.pixel_step = 2 * es; bad.append((x, fc.KS265_NOTSUPPORTED))                     # a step that is none of 1, 3, 4 elements
        x = ok(); x.pixel_step = 4 * es + 1; bad.append((x, fc.KS265_NOTSUPPORTED))
        x = ok(); x.plane[2] = x.plane[1]; bad.append((x, fc.KS265_NOTSUPPORTED))                   # two channels on one element of a four-element pixel
        x = ok(); x.plane[2] = 4 * es; bad.append((x, fc.KS265_NOTSUPPORTED))                       # a channel in the next pixel
        x = ok(); x.matrix = 2; bad.append((x, fc.KS265_NOTSUPPORTED))
        x = ok(); x.width = 7; bad.append((x, fc.KS265_NOTSUPPORTED))
        x = ok(); x.pitch[0] = W * step - es; bad.append((x, fc.KS265_POINTER))                     # a pitch below the row
        for x, want in bad:
            assert (_convert(hip, src, x, buf.size, want) == 0xA5).all(), "a refused picture enqueued something"
        host = np.zeros(buf.size, np.uint8)                                                         # host memory
        x = fc.describe(fmt, W, H, host.ctypes.data, offs, pitch, step)
        assert lib.ks265_output_validate(h, C.byref(x)) == fc.KS265_POINTER
        assert lib.ks265_output_convert(h, C.c_void_p(src.data_ptr()), C.byref(x)) == fc.KS265_POINTER
        # a buffer one element short: a page of its own that the B plane's last sample ends with - and then one element later
        page = C.c_void_p()
        assert lib.ks265_dev_malloc(h, C.byref(page), C.c_size_t(4096)) == 0
        row = W * es
        for shift, want in ((0, 0), (es, fc.KS265_POINTER)):
            assert lib.ks265_memset_async(h, page, 0xA5, C.c_size_t(4096)) == 0
            x = fc.describe(fmt, W, H, page.value, [0, 512, 4096 - (2048 + row) + shift], 2048, es)
            assert lib.ks265_output_convert(h, C.c_void_p(src.data_ptr()), C.byref(x)) == want
            got = torch.zeros(4096, dtype=torch.uint8, device="cuda")
            assert lib.ks265_memcpy_d2d_async(h, C.c_void_p(got.data_ptr()), page, C.c_size_t(4096)) == 0
            assert lib.ks265_synchronize(h) == 0
            assert bool((got.cpu().numpy() == 0xA5).all()) == bool(want)
        assert lib.ks265_dev_free(h, page) == 0
        assert (host == 0).all()
