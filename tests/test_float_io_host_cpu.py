"""CPU: float pictures (KS265_IN_RGB_F16 / _BF16 / _F32, include/ks265_enc.h) through the real encoder host, against the stand-in of the device library WITH the float formats
(tests/hip_stub_float.c), 128x72:
  * a float32 planar clip through ks265_enc_encode_device_frame writes, byte for byte, the stream of the same clip handed in as host I420 made by tests/yuv_float_ref.py - one
    and two GOP lanes; the same through ks265_enc_encode_device_frame_scaled;
  * ks265_enc_get_device_recon into a float16 planar picture and into a four-element float32 picture equals the definition;
  * a float picture whose pointer is off its element size is QY_NOTSUPPORTED, shows no device call and leaves a pending ROI map pending;
  * the stand-in's two conversion routines in a program of their own under -fsanitize=address,undefined, over ragged shapes in buffers of exactly their extent, equal
    the specification (no sanitizer touches anything loaded into Python)."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

import float_io_cases as fc
import yuv_float_ref as fref
import yuv_output_ref as oref
import yuv_scale_ref as ys
from host_harness import QY_NOTSUPPORTED, QY_OK, QY_POINTER, Nal, Picture, Roi, build_host_lib, build_host_program, dev_pic, device_picture, drive, host_picture, load_host_lib
from host_harness import open_handle as open_at

W, H, SW, SH, N = 128, 72, 256, 144, 17


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_host_lib(build_host_lib("hip_stub_float.c"), call_log=str(tmp_path_factory.mktemp("stubfloat") / "calls.log"))


def open_handle(lib, params=(), lanes=1, roi=False, devrecon=False):
    return open_at(lib, W, H, params=params, lanes=lanes, roi=roi, defaults=("devrecon",) if devrecon else ())


def float_pic(buf: np.ndarray, fmt, offs, pitch, step, pts=0):
    return dev_pic([buf], offs, (pitch,), fmt, pts, step)


def session(lib, pictures, lanes=1, scaled=None, params=(), fetch=None):
    """one handle fed `pictures`: flat uint8 arrays are host I420 pictures (QY265EncoderEncodeFrame), tuples (buf, fmt, offs, pitch, step) float pictures in "device" memory
    (scaled=(sw, sh, filter): through the scaled entry).  fetch(h): called after every call that may have handed pictures out.  The stream."""
    h = open_handle(lib, params=params, lanes=lanes, devrecon=fetch is not None)
    if any(isinstance(p, tuple) for p in pictures) or fetch:
        assert lib.ks265_enc_enable_device_input(h) == QY_OK
    if scaled:
        assert lib.ks265_enc_enable_device_scale(h, scaled[0], scaled[1]) == QY_OK
    submits = (device_picture(lib, h, [p[0]], p[2], (p[3],), p[1], t, p[4], scaled=scaled) if isinstance(p, tuple) else host_picture(lib, h, p, W, H, t) for t, p in enumerate(pictures))
    return drive(lib, h, submits, after=fetch and (lambda: fetch(h)))


def float_clip(fmt, pixel, w, h, n, seed, pad=3):
    """n pictures as (buf, fmt, offs, pitch, step) and their samples as float32 (n, 3, h, w)"""
    rng = np.random.default_rng(seed)
    base = rng.random((3, h, w), dtype=np.float32)
    pics, samples = [], []
    for t in range(n):
        x = np.clip(np.roll(base, (2 * t, 3 * t), (1, 2)) * np.float32(1.2) - np.float32(0.1) + rng.random((3, h, w), dtype=np.float32) * np.float32(0.02), -0.05, 1.05).astype(np.float32)
        bits = fc.f32_to_bits(x, fmt)
        buf, views, offs, pitch, step = fc.layout(fmt, pixel, w, h, pad, 0, fill=0x3B)
        for k in range(3):
            views[k][:] = bits[k]
        pics.append((buf, fmt, offs, pitch, step))
        samples.append(np.stack([fc.bits_to_f32(b, fmt) for b in bits]))
    return pics, samples


@pytest.mark.parametrize("lanes", [1, 2])
def test_float32_planar_clip_writes_the_stream_of_its_reference_conversion(lib, lanes):
    params = (("iper", 8),) if lanes == 2 else ()
    pics, samples = float_clip(fref.IN_RGB_F32, "planar", W, H, N, 41)
    host = [fref.rgbf_to_i420(*s) for s in samples]
    got, exp = session(lib, pics, lanes, params=params), session(lib, host, lanes, params=params)
    assert len(got) > 1000 and got == exp
    assert session(lib, [fref.rgbf_to_i420(*s, full_range=True) for s in samples], lanes, params=params) != exp   # the comparison can tell conversions apart


def test_scaled_entry_takes_float_pictures(lib):
    pics, samples = float_clip(fref.IN_RGB_F32, "planar", SW, SH, 9, 43)
    host = [ys.scale_i420(fref.rgbf_to_i420(*s), SW, SH, W, H, 1) for s in samples]
    got, exp = session(lib, pics, scaled=(SW, SH, 1)), session(lib, host)
    assert len(got) > 1000 and got == exp
    pics16, samples16 = float_clip(fref.IN_RGB_BF16, "bgra", SW, SH, 3, 44)
    host16 = [ys.scale_i420(fref.rgbf_to_i420(*s), SW, SH, W, H, 0) for s in samples16]
    assert session(lib, pics16, scaled=(SW, SH, 0)) == session(lib, host16)


def test_device_recon_into_float_pictures_equals_the_definition(lib):
    pics, _ = float_clip(fref.IN_RGB_F32, "planar", W, H, 7, 45)

    def fetcher(out, fmt, pixel):
        def fetch(h):
            info = Picture()
            while lib.ks265_enc_device_recon_pending(h) > 0:
                if fmt == 0:
                    buf = np.full(W * H * 3 // 2, 0xA5, np.uint8)
                    offs, pitch, step = [0, W * H, W * H * 5 // 4], W, 0
                else:
                    buf, _, offs, pitch, step = fc.layout(fmt, pixel, W, H, 5, 1)
                d = float_pic(buf, fmt, offs, pitch, step)
                if fmt == 0:
                    d.pitch[1] = d.pitch[2] = W // 2
                assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.byref(info)) == QY_OK
                out.append((info.poc, buf))
        return fetch
    i420, f16, f32 = [], [], []
    streams = {session(lib, pics, fetch=fetcher(out, fmt, pixel)) for out, fmt, pixel in ((i420, 0, None), (f16, fref.IN_RGB_F16, "planar"), (f32, fref.IN_RGB_F32, "bgra"))}
    assert len(streams) == 1 and len(i420) == len(f16) == len(f32) == 7
    for (poc, pic), (p16, b16), (p32, b32) in zip(i420, f16, f32):
        assert poc == p16 == p32
        planes = oref.i420_to_rgb(pic, W, H)
        for fmt, pixel, got in ((fref.IN_RGB_F16, "planar", b16), (fref.IN_RGB_F32, "bgra", b32)):
            exp, views, offs, pitch, step = fc.layout(fmt, pixel, W, H, 5, 1)
            for k in range(3):
                views[k][:] = fc.sample_bits(planes[k], fmt)
            if pixel == "bgra":
                E = fc.elem_dtype(fmt)
                exp.view(E)[1:1 + H * (pitch // 4)].reshape(H, pitch // 4)[:, 3:W * 4:4] = fc.ONE[fmt]
            assert (got == exp).all(), (fc.NAMES[fmt], pixel, int((got != exp).sum()))


def test_a_misaligned_float_picture_is_refused_and_keeps_the_map(lib):
    h = open_handle(lib, roi=True)
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()
    (buf, fmt, offs, pitch, step), = float_clip(fref.IN_RGB_F32, "planar", W, H, 1, 47)[0]
    m = np.full(((H + 7) // 8, (W + 7) // 8), 3, np.int8)               # a map in "device" memory: its reduction shows in the call log
    r = Roi()
    r.type, r.log2_block, r.device, r.data, r.pitch, r.stream = 0, 3, 0, m.ctypes.data, m.strides[0], None
    assert lib.ks265_enc_set_next_roi(h, C.byref(r)) == QY_OK
    before = sum(1 for _ in open(lib.call_log_path))
    bad = []
    p = float_pic(buf, fmt, offs, pitch, step); p.plane[1] = p.plane[1] + 2; bad.append((p, QY_NOTSUPPORTED))
    p = float_pic(buf, fmt, offs, pitch, step); p.pitch[0] = pitch + 2; bad.append((p, QY_NOTSUPPORTED))
    p = float_pic(buf, fmt, offs, pitch, step); p.pixel_step = 68; bad.append((p, QY_NOTSUPPORTED))
    p = float_pic(buf, fmt, offs, pitch, step); p.format = 19; bad.append((p, QY_NOTSUPPORTED))
    p = float_pic(buf, fmt, offs, pitch, step); p.pitch[0] = 4 * W - 4; bad.append((p, QY_POINTER))
    for p, want in bad:
        assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(p), C.byref(outp)) == want
        assert nn.value == 0 and lib.QY265EncoderDelayedFrames(h) == 0
    assert sum(1 for _ in open(lib.call_log_path)) == before, "a refused picture enqueued something"
    ok = float_pic(buf, fmt, offs, pitch, step)
    for _ in range(2):
        assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(ok), C.byref(outp)) == QY_OK
    new = open(lib.call_log_path).read().split("\n")[before:]
    assert sum("ks265_roi_reduce" in l for l in new) == 1, "the pending map went with the first picture that was taken"
    assert sum("ks265_input_convert" in l for l in new) == 2
    lib.QY265EncoderClose(h)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


@pytest.fixture(scope="module")
def sanitized():
    return build_host_program("float_stub_main.c")


@pytest.mark.parametrize("fmt", fc.FORMATS, ids=[fc.NAMES[f] for f in fc.FORMATS])
def test_conversion_routines_under_the_sanitizers(sanitized, tmp_path, fmt):
    es = fref.ELEM_SIZE[fmt]
    src_f, dst_f = str(tmp_path / "src.bin"), str(tmp_path / "dst.bin")

    def run(*args):
        r = subprocess.run([sanitized, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return np.fromfile(dst_f, np.uint8)
    for (w, h), (wo, ho) in zip([(8, 2), (24, 6), (520, 10)], [(8, 2), (26, 6), (520, 10)]):
        for pixel, matrix, full in (("planar", 0, 0), ("bgra", 1, 1), ("hwc", 0, 1)):
            n, order = fc.PIXELS[pixel]
            # input: the source ends with its last sample
            bits = fc.random_bits(np.random.default_rng(w + fmt), fmt, (3, h, w))
            buf, views, offs, pitch, step = fc.layout(fmt, pixel, w, h, 3, 0)
            for k in range(3):
                views[k][:] = bits[k]
            buf[:max(offs) + (h - 1) * pitch + (w - 1) * step + es].tofile(src_f)
            got = run("in", fmt, w, h, step, pitch, *offs, matrix, full, src_f, dst_f)
            assert (got == fref.rgbf_to_i420(*[fc.bits_to_f32(b, fmt) for b in bits], matrix, bool(full))).all(), ("in", pixel, w, h)
            # output: the destination ends with its last row
            pic = np.random.default_rng(wo).integers(0, 256, wo * ho * 3 // 2, dtype=np.uint8)
            pic.tofile(src_f)
            exp, views, offs, pitch, step = fc.layout(fmt, pixel, wo, ho, 3, 0)
            for k, c in enumerate(oref.i420_to_rgb(pic, wo, ho, matrix, bool(full))):
                views[k][:] = fc.sample_bits(c, fmt)
            one = -1
            if n == 4:
                exp.view(fc.elem_dtype(fmt))[:ho * (pitch // es)].reshape(ho, pitch // es)[:, 3:wo * 4:4] = fc.ONE[fmt]
                one = 3 * es
            size = (min(offs) if n > 1 else max(offs)) + (ho - 1) * pitch + wo * n * es
            got = run("out", fmt, wo, ho, step, pitch, *offs, matrix, full, src_f, dst_f, size, one)
            assert (got == exp[:size]).all(), ("out", pixel, wo, ho)
