"""GPU: every alignment branch of the picture conversion kernels' loaders and stores, reached on purpose (ks265codec_amd/csrc/convert_dev.h and the five files that include it).
Each way in and each way out runs with every source plane (destination plane on the way out) at allocation offset k x element size for k = 0 .. 16 and a pitch that is a
multiple of 16, so every row of a case takes the same branch: 16-, 8-, 4-byte and element-wise accesses each have cases of their own.  32x4: the 16-column repack with exactly
two threads per row; 24x6: the 8-column kernels, H / 2 no multiple of the block's 4 rows; 22x6: pad and crop.  The expectations are the reference modules'; every comparison is
exact equality, and the 0xA5 around every destination must be intact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import picture_window_ref as pw  # noqa: E402
import yuv_convert_ref as cref  # noqa: E402
import yuv_float_ref as fref  # noqa: E402
import yuv_hibit_ref as href  # noqa: E402
import yuv_output_ref as oref  # noqa: E402
from ks265codec_amd.lib import IN_I420, IN_NV12, IN_RGB, IN_RGB_F16, IN_RGB_F32, InDesc  # noqa: E402

OFFSETS = range(17)
SLACK = 64
CANARY = 0xA5


@pytest.fixture(scope="module")
def hip():
    from ks265codec_amd.lib import load_library
    lib = load_library()
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    yield lib, h
    lib.ks265_destroy(h)


def _pitch(row_bytes: int) -> int:
    return (row_bytes + 15) // 16 * 16 + 16


def _host_buffer(plane: np.ndarray, off: int, fill: int) -> np.ndarray:
    """a plane (2-D, any element type) as bytes at offset `off` of a buffer of `fill`, rows _pitch apart, SLACK bytes behind the last row"""
    rows = np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape[0], -1)
    n, rb = rows.shape
    buf = np.full(off + _pitch(rb) * (n - 1) + rb + SLACK, fill, np.uint8)
    for r in range(n):
        buf[off + r * _pitch(rb): off + r * _pitch(rb) + rb] = rows[r]
    return buf


def _device(buf: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0                                       # the offsets below are offsets from a 16-byte boundary
    return t


def _desc(fmt, w, h, ptrs, pitches, step=0, matrix=0, full=0) -> InDesc:
    d = InDesc()
    d.format, d.width, d.height, d.pixel_step, d.matrix, d.full_range = fmt, w, h, step, matrix, full
    for k, p in enumerate(ptrs):
        d.plane[k] = p
    for k, s in enumerate(pitches):                                     # (RGB: one pitch for the three channel pointers)
        d.pitch[k] = s
    return d


def _sources(planes, off: int):
    """every plane in a device buffer of its own at byte offset `off`: (tensors to keep alive, addresses, pitches)"""
    devs = [_device(_host_buffer(p, off, 0x3C)) for p in planes]
    return devs, [d.data_ptr() + off for d in devs], [_pitch(p.shape[1] * p.dtype.itemsize) for p in planes]


def _run_in(hip, call, n: int) -> np.ndarray:
    """call(destination address) into a 16-byte aligned packed picture of n bytes with the canary on both sides"""
    lib, h = hip
    dst = torch.full((SLACK + n + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0 and SLACK % 16 == 0
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = call(C.c_void_p(dst.data_ptr() + SLACK))
    assert rc == 0, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    assert (out[:SLACK] == CANARY).all() and (out[SLACK + n:] == CANARY).all(), "bytes written outside the picture"
    return out[SLACK:SLACK + n]


def _convert(hip, desc: InDesc, w: int, h: int) -> np.ndarray:
    return _run_in(hip, lambda p: hip[0].ks265_input_convert(hip[1], C.byref(desc), p), w * h * 3 // 2)


def _i420(rng, w, h):
    pic = rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    return pic, [pic[:w * h].reshape(h, w), pic[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), pic[w * h * 5 // 4:].reshape(h // 2, w // 2)]


# ------------------------------------------------------------------ ways in

@pytest.mark.parametrize("w,h", [(32, 4), (24, 6)])
@pytest.mark.parametrize("nv12", [False, True], ids=["i420", "nv12"])
def test_in_i420_and_nv12(hip, w, h, nv12):
    pic, (y, u, v) = _i420(np.random.default_rng(w + nv12), w, h)
    planes = [y, np.stack([u, v], axis=2).reshape(h // 2, w)] if nv12 else [y, u, v]
    for k in OFFSETS:
        devs, ptrs, pitches = _sources(planes, k)
        got = _convert(hip, _desc(IN_NV12 if nv12 else IN_I420, w, h, ptrs, pitches), w, h)
        assert (got == pic).all(), (k, np.flatnonzero(got != pic)[:8])


def _rgb8(rng, w, h):
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]


def test_in_rgb_planar(hip):
    w, h = 24, 6
    rgb = _rgb8(np.random.default_rng(1), w, h)
    exp = cref.rgb_to_i420(*rgb, cref.MATRIX_BT709, False)
    for k in OFFSETS:
        devs, ptrs, pitches = _sources(rgb, k)
        got = _convert(hip, _desc(IN_RGB, w, h, ptrs, pitches[:1], step=1, matrix=cref.MATRIX_BT709), w, h)
        assert (got == exp).all(), (k, np.flatnonzero(got != exp)[:8])


def test_in_rgba(hip):
    w, h = 24, 6
    rng = np.random.default_rng(2)
    rgb = _rgb8(rng, w, h)
    exp = cref.rgb_to_i420(*rgb, cref.MATRIX_BT601, True)
    px = np.stack([*rgb, rng.integers(0, 256, (h, w), dtype=np.uint8)], axis=2).reshape(h, w * 4)
    for k in OFFSETS:
        devs, ptrs, pitches = _sources([px], k)
        got = _convert(hip, _desc(IN_RGB, w, h, [ptrs[0] + c for c in range(3)], pitches, step=4, matrix=cref.MATRIX_BT601, full=1), w, h)
        assert (got == exp).all(), (k, np.flatnonzero(got != exp)[:8])


def _float_rgb(rng, w, h, dtype):
    """samples below 0, inside [0, 1] and above 1"""
    return [rng.uniform(-0.1, 1.1, (h, w)).astype(dtype) for _ in range(3)]


def test_in_f16_planar(hip):
    w, h = 24, 6
    rgb = _float_rgb(np.random.default_rng(3), w, h, np.float16)
    exp = fref.rgbf_to_i420(*(fref.to_f32(c, IN_RGB_F16) for c in rgb), cref.MATRIX_BT709, False)
    for k in OFFSETS:
        devs, ptrs, pitches = _sources(rgb, 2 * k)
        got = _convert(hip, _desc(IN_RGB_F16, w, h, ptrs, pitches[:1], step=2, matrix=cref.MATRIX_BT709), w, h)
        assert (got == exp).all(), (k, np.flatnonzero(got != exp)[:8])


def test_in_f32_rgba(hip):
    w, h = 24, 6
    rng = np.random.default_rng(4)
    rgb = _float_rgb(rng, w, h, np.float32)
    exp = fref.rgbf_to_i420(*rgb, cref.MATRIX_BT601, True)
    px = np.stack([*rgb, rng.uniform(0, 1, (h, w)).astype(np.float32)], axis=2).reshape(h, w * 4)
    for k in OFFSETS:
        devs, ptrs, pitches = _sources([px], 4 * k)
        got = _convert(hip, _desc(IN_RGB_F32, w, h, [ptrs[0] + 4 * c for c in range(3)], pitches, step=16, matrix=cref.MATRIX_BT601, full=1), w, h)
        assert (got == exp).all(), (k, np.flatnonzero(got != exp)[:8])


@pytest.mark.parametrize("name,layout,sub,depth,msb", [("p010", href.SEMI, href.S420, 10, 1), ("planar444_16", href.PLANAR, href.S444, 16, 0)])
def test_in_high_bit_depth(hip, name, layout, sub, depth, msb):
    w, h = 24, 6
    planes = href.random_planes(np.random.default_rng(depth), layout, sub, depth, msb, w, h)
    exp = href.to_i420(planes, layout, sub, depth, msb)
    for k in OFFSETS:
        devs, ptrs, pitches = _sources(planes, 2 * k)
        got = _convert(hip, _desc(href.code(layout, sub, depth, msb), w, h, ptrs, pitches), w, h)
        assert (got == exp).all(), (name, k, np.flatnonzero(got != exp)[:8])


@pytest.mark.parametrize("nv12", [False, True], ids=["i420", "nv12"])
def test_in_pad(hip, nv12):
    w, h = 22, 6
    cw, ch = pw.coded_size(w, h)
    pic, (y, u, v) = _i420(np.random.default_rng(5 + nv12), w, h)
    exp = pw.pad_planes([y, u, v], w, h)
    planes = [y, np.stack([u, v], axis=2).reshape(h // 2, w)] if nv12 else [y, u, v]
    for k in OFFSETS:
        devs, ptrs, pitches = _sources(planes, k)
        desc = _desc(IN_NV12 if nv12 else IN_I420, w, h, ptrs, pitches)
        got = _run_in(hip, lambda p: hip[0].ks265_input_pad(hip[1], C.byref(desc), cw, ch, p), cw * ch * 3 // 2)
        assert (got == exp).all(), (k, np.flatnonzero(got != exp)[:8])


# ------------------------------------------------------------------ ways out

def _run_out(hip, call, expected: list, off: int):
    """call(addresses, pitches) writes planes; each destination is a buffer of the canary in which exactly the bytes of `expected` (at offset `off`, rows _pitch apart) may change"""
    lib, h = hip
    want = [_host_buffer(p, off, CANARY) for p in expected]
    devs = [_device(np.full(b.size, CANARY, np.uint8)) for b in want]
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = call([d.data_ptr() + off for d in devs], [_pitch(p.shape[1] * p.dtype.itemsize) for p in expected])
    assert rc == 0, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    for n, (d, b) in enumerate(zip(devs, want)):
        got = d.cpu().numpy()
        assert (got == b).all(), (off, n, np.flatnonzero(got != b)[:8])


@pytest.mark.parametrize("w,h", [(32, 4), (24, 6)])
@pytest.mark.parametrize("nv12", [False, True], ids=["i420", "nv12"])
def test_out_i420_and_nv12(hip, w, h, nv12):
    pic, (y, u, v) = _i420(np.random.default_rng(6 + w + nv12), w, h)
    src = _device(pic)
    expected = [y, oref.i420_to_nv12(pic, w, h)[h:]] if nv12 else [y, u, v]
    for k in OFFSETS:
        _run_out(hip, lambda ptrs, pitches: hip[0].ks265_output_convert(hip[1], C.c_void_p(src.data_ptr()), C.byref(_desc(IN_NV12 if nv12 else IN_I420, w, h, ptrs, pitches))),
                 expected, k)


def test_out_rgba(hip):
    w, h = 24, 6
    pic, _ = _i420(np.random.default_rng(7), w, h)
    src = _device(pic)
    r, g, b = oref.i420_to_rgb(pic, w, h, cref.MATRIX_BT709, False)
    px = np.stack([r, g, b, np.full_like(r, 255)], axis=2).reshape(h, w * 4)
    for k in OFFSETS:
        _run_out(hip, lambda ptrs, pitches: hip[0].ks265_output_convert(hip[1], C.c_void_p(src.data_ptr()), C.byref(
            _desc(IN_RGB, w, h, [ptrs[0] + c for c in range(3)], pitches, step=4, matrix=cref.MATRIX_BT709))), [px], k)


def test_out_f16_rgba(hip):
    w, h = 24, 6
    pic, _ = _i420(np.random.default_rng(8), w, h)
    src = _device(pic)
    r, g, b = fref.i420_to_rgbf(pic, w, h, IN_RGB_F16, cref.MATRIX_BT601, True)
    px = np.stack([r, g, b, np.ones_like(r)], axis=2).reshape(h, w * 4)
    for k in OFFSETS:
        _run_out(hip, lambda ptrs, pitches: hip[0].ks265_output_convert(hip[1], C.c_void_p(src.data_ptr()), C.byref(
            _desc(IN_RGB_F16, w, h, [ptrs[0] + 2 * c for c in range(3)], pitches, step=8, matrix=cref.MATRIX_BT601, full=1))), [px], 2 * k)


def test_out_crop(hip):
    lib, hd = hip
    w, h = 22, 6
    cw, ch = pw.coded_size(w, h)
    pic = np.random.default_rng(9).integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8)
    src = _device(pic)
    exp = pw.crop_i420(pic, cw, ch, w, h)
    n = w * h * 3 // 2
    for k in OFFSETS:
        dst = _device(np.full(k + n + SLACK, CANARY, np.uint8))
        assert lib.ks265_wait_external(hd, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        rc = lib.ks265_output_crop(hd, C.c_void_p(src.data_ptr()), cw, ch, w, h, C.c_void_p(dst.data_ptr() + k))
        assert rc == 0, (rc, lib.ks265_last_error(hd))
        assert lib.ks265_synchronize(hd) == 0
        out = dst.cpu().numpy()
        assert (out[:k] == CANARY).all() and (out[k + n:] == CANARY).all(), "bytes written outside the picture"
        assert (out[k:k + n] == exp).all(), (k, np.flatnonzero(out[k:k + n] != exp)[:8])
