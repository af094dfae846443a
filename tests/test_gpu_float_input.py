"""GPU: float RGB pictures into the encoder's packed I420 (ks265_input_convert with KS265_IN_RGB_F16 / _BF16 / _F32, ks265codec_amd/csrc/input_convert.hip) against
tests/yuv_float_ref.py, byte for byte:
  * every type x planar / HWC / four-element pixels in RGBA and BGRA order x both matrices x both ranges, at 8x2 (one thread), 24x6 and 520x10 (a second block in x and in y),
    pitches above the row, the picture on 16 bytes and off them by one element (the element path; the clamped left column at x0 = 0), a pitch that is no multiple of 16;
    0xA5 guards on both sides of the destination stay, the source is the same bytes afterwards;
  * exhaustively: every bit pattern of the 16-bit types (every NaN, infinity, denormal), 2^20 random bit patterns of float32 plus the special values;
  * u8 / 255 as float32 converts to the bytes the uint8 path makes of u8;
  * refusals enqueue nothing; a float source through the scaler's scratch picture."""
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
import yuv_scale_ref as ys  # noqa: E402

SLACK = 256
SHAPES = [(8, 2), (24, 6), (520, 10)]
PLACES = [(0, 8), (1, 8), (0, 3)]             # (elements in front of the picture, elements behind every row): on 16 bytes; off them by one element; rows that alternate
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


def _convert(hip, desc, W, H, want=0):
    """ks265_input_convert into a destination with SLACK bytes of 0xA5 on both sides; the picture (or, for a refusal, None after checking that nothing was written)"""
    lib, h = hip
    n = W * H * 3 // 2
    dst = torch.full((n + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = lib.ks265_input_convert(h, C.byref(desc), C.c_void_p(dst.data_ptr() + SLACK))
    assert rc == want, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    assert (out[:SLACK] == 0xA5).all() and (out[SLACK + n:] == 0xA5).all(), "bytes written outside the picture"
    if want:
        assert (out == 0xA5).all(), "a refused picture enqueued something"
        return None
    return out[SLACK:SLACK + n]


def _run(hip, fmt, pixel, bits, W, H, pad, off, matrix, full):
    buf, views, offs, pitch, step = fc.layout(fmt, pixel, W, H, pad, off, fill=0x3B)
    for k in range(3):
        views[k][:] = bits[k]
    d = _dev(buf)
    got = _convert(hip, fc.describe(fmt, W, H, d.data_ptr(), offs, pitch, step, matrix, full), W, H)
    assert (d.cpu().numpy() == buf).all(), "the source changed"
    return got


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("fmt", fc.FORMATS, ids=[fc.NAMES[f] for f in fc.FORMATS])
def test_every_layout_equals_the_specification(hip, fmt, W, H):
    bits = fc.random_bits(np.random.default_rng(W + fmt), fmt, (3, H, W))
    f = [fc.bits_to_f32(b, fmt) for b in bits]
    for matrix, full in CASES:
        exp = fref.rgbf_to_i420(*f, matrix, bool(full))
        for pixel in fc.PIXELS:
            for off, pad in PLACES:
                got = _run(hip, fmt, pixel, bits, W, H, pad, off, matrix, full)
                assert (got == exp).all(), (fc.NAMES[fmt], pixel, matrix, full, off, pad, int((got != exp).sum()))


@pytest.mark.parametrize("fmt", [fref.IN_RGB_F16, fref.IN_RGB_BF16], ids=["f16", "bf16"])
def test_all_65536_bit_patterns(hip, fmt):
    W, H = 512, 128
    i = np.arange(65536, dtype=np.uint32)
    bits = [i.astype(np.uint16).reshape(H, W), i[::-1].astype(np.uint16).reshape(H, W), ((i * 40503 + 12345) & 0xFFFF).astype(np.uint16).reshape(H, W)]
    assert len(np.unique(bits[2])) == 65536
    f = [fc.bits_to_f32(b, fmt) for b in bits]
    for matrix, full, pixel in ((cref.MATRIX_BT709, 0, "planar"), (cref.MATRIX_BT601, 1, "bgra")):
        exp = fref.rgbf_to_i420(*f, matrix, bool(full))
        got = _run(hip, fmt, pixel, bits, W, H, 8, 0, matrix, full)
        assert (got == exp).all(), (pixel, int((got != exp).sum()))


def test_float32_random_bit_patterns_and_special_values(hip):
    W, H = 1024, 344                                                    # 3 x 352256 samples: more than 2^20
    rng = np.random.default_rng(32)
    bits = rng.integers(0, 2 ** 32, (3, H, W), dtype=np.uint64).astype(np.uint32)
    sp = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -1e-30, 1.0, 1.0000001, 2.0, 3e38, 1e-45, 1.1754942e-38, 1 / 512, 3 / 512, 5 / 512, 1 / 255]).view(np.uint32)
    for k in range(3):
        bits[k, k, :sp.size] = np.roll(sp, k)
    bits[0, 5, :256] = (np.arange(256, dtype=np.float32) / np.float32(255)).view(np.uint32)
    f = [fc.bits_to_f32(b, fref.IN_RGB_F32) for b in bits]
    exp = fref.rgbf_to_i420(*f, cref.MATRIX_BT709, False)
    for pixel in ("planar", "rgba"):
        got = _run(hip, fref.IN_RGB_F32, pixel, bits, W, H, 4, 0, cref.MATRIX_BT709, 0)
        assert (got == exp).all(), (pixel, int((got != exp).sum()))


@pytest.mark.parametrize("W,H", [(24, 6), (520, 10)])
def test_u8_over_255_gives_the_bytes_of_the_uint8_path(hip, W, H):
    u8 = np.random.default_rng(H).integers(0, 256, (3, H, W), dtype=np.uint8)
    u8[:, :2, :8] = np.array([0, 255, 0], np.uint8)[:, None, None]
    t = _dev(u8)
    f32 = _dev(u8.astype(np.float32) / np.float32(255))                 # (divided on the host: correctly rounded)
    for matrix, full in CASES:
        exp = cref.rgb_to_i420(*u8, matrix, bool(full))
        d8 = fc.describe(2, W, H, t.data_ptr(), [k * W * H for k in range(3)], W, 1, matrix, full)
        df = fc.describe(fref.IN_RGB_F32, W, H, f32.data_ptr(), [4 * k * W * H for k in range(3)], 4 * W, 4, matrix, full)
        a, b = _convert(hip, d8, W, H), _convert(hip, df, W, H)
        assert (a == exp).all() and (b == exp).all(), (matrix, full, int((b != exp).sum()))


def test_refusals_enqueue_nothing(hip):
    lib, h = hip
    W, H = 8, 2
    for fmt in fc.FORMATS:
        es = fref.ELEM_SIZE[fmt]
        buf, views, offs, pitch, step = fc.layout(fmt, "rgba", W, H, 8, 0, fill=0)
        d = _dev(buf)
        ok = lambda: fc.describe(fmt, W, H, d.data_ptr(), offs, pitch, step)
        assert _convert(hip, ok(), W, H) is not None
        bad = []
        x = ok(); x.plane[1] = x.plane[1] + 1; bad.append((x, fc.KS265_NOTSUPPORTED))               # a pointer off its element size
        x = ok(); x.pixel_step = step + 1; bad.append((x, fc.KS265_NOTSUPPORTED))                   # the step
        x = ok(); x.pitch[0] = pitch + 1; bad.append((x, fc.KS265_NOTSUPPORTED))                    # the pitch
        x = ok(); x.pixel_step = 64 + es; x.pitch[0] = W * (64 + es); bad.append((x, fc.KS265_NOTSUPPORTED))   # a step above 64
        x = ok(); x.pixel_step = 0; bad.append((x, fc.KS265_NOTSUPPORTED))
        x = ok(); x.matrix = 2; bad.append((x, fc.KS265_NOTSUPPORTED))
        x = ok(); x.width = 12; bad.append((x, fc.KS265_NOTSUPPORTED))
        x = ok(); x.pitch[0] = W * step - es; bad.append((x, fc.KS265_POINTER))                     # a pitch below the row
        x = ok(); x.plane[2] = None; bad.append((x, fc.KS265_POINTER))
        host = np.zeros(buf.size, np.uint8)
        bad.append((fc.describe(fmt, W, H, host.ctypes.data, offs, pitch, step), fc.KS265_POINTER))  # host memory
        for x, want in bad:
            assert lib.ks265_input_validate(h, C.byref(x)) == want
            _convert(hip, x, W, H, want)
        # a buffer one element short: a page of its own, the B channel's last sample ends with it - and then one element later
        page = C.c_void_p()
        assert lib.ks265_dev_malloc(h, C.byref(page), C.c_size_t(4096)) == 0
        assert lib.ks265_memset_async(h, page, 0, C.c_size_t(4096)) == 0 and lib.ks265_synchronize(h) == 0
        row = (W - 1) * es + es
        fits = fc.describe(fmt, W, H, page.value, [0, 64, 4096 - (2048 + row)], 2048, es)
        assert _convert(hip, fits, W, H) is not None
        short = fc.describe(fmt, W, H, page.value, [0, 64, 4096 - (2048 + row) + es], 2048, es)
        _convert(hip, short, W, H, fc.KS265_POINTER)
        assert lib.ks265_dev_free(h, page) == 0
    for code in (3, 7, 15, 19):                                          # the codes around the three
        x = fc.describe(code, W, H, d.data_ptr(), offs, pitch, step)
        assert lib.ks265_input_validate(h, C.byref(x)) == fc.KS265_NOTSUPPORTED


def test_float_source_through_the_scaler(hip):
    lib, h = hip
    SW, SH, DW, DH = 48, 20, 32, 16
    fmt = fref.IN_RGB_F16
    bits = fc.random_bits(np.random.default_rng(48), fmt, (3, SH, SW))
    exp = ys.scale_i420(fref.rgbf_to_i420(*[fc.bits_to_f32(b, fmt) for b in bits]), SW, SH, DW, DH, 1)
    buf, views, offs, pitch, step = fc.layout(fmt, "hwc", SW, SH, 5, 0)
    for k in range(3):
        views[k][:] = bits[k]
    d = _dev(buf)
    plan = C.c_void_p()
    assert lib.ks265_scale_plan_create(h, SW, SH, DW, DH, 1, C.byref(plan)) == 0
    scratch = torch.zeros(SW * SH * 3 // 2, dtype=torch.uint8, device="cuda")
    dst = torch.full((DW * DH * 3 // 2 + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    desc = fc.describe(fmt, SW, SH, d.data_ptr(), offs, pitch, step)
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert lib.ks265_input_scale_validate(h, plan, C.byref(desc)) == 0
    rc = lib.ks265_input_scale(h, plan, C.byref(desc), C.c_void_p(scratch.data_ptr()), C.c_void_p(dst.data_ptr() + SLACK))
    assert rc == 0, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    assert lib.ks265_scale_plan_destroy(h, plan) == 0
    assert (out[:SLACK] == 0xA5).all() and (out[-SLACK:] == 0xA5).all()
    assert (out[SLACK:-SLACK] == exp).all()
