"""CPU: ks265_enc_enable_device_scale / ks265_enc_encode_device_frame_scaled (include/ks265_enc.h) in the encoder host, against the stand-in of the device library WITH device
input and the scaler (tests/hip_stub_scale.c):
  * every refusal, each leaving nothing enqueued (the stand-in's call log does not grow) and a pending ROI map pending;
  * a handle fed 17 random 128x96 pictures through the scaled entry into a 64x48 encoder writes, byte for byte, the stream of a handle fed the same pictures pre-scaled by
    tests/yuv_scale_ref.py through the plain entry - both filters, an RGBA source, one and two GOP lanes, `roi` on;
  * the plan cache: five source sizes in turn, four plans kept, the least recently used one replaced, nothing alive after close."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import yuv_convert_ref as cref
import yuv_scale_ref as ys
from host_harness import IN_I420, IN_RGB, LOG_CB, QY_NOTSUPPORTED, QY_OK, QY_POINTER, Nal, Picture, Roi, build_host_lib, calls, dev_pic, device_picture, drive, load_host_lib, preceded
from host_harness import open_handle as open_at

W, H, SW, SH, N = 64, 48, 128, 96, 17


def _load(d, defines=()):
    lib = load_host_lib(build_host_lib("hip_stub_scale.c", defines), call_log=str(d / "calls.log"))
    lib.ks265_stub_creating_calls.restype = C.c_long
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return _load(tmp_path_factory.mktemp("stubscale"))


@pytest.fixture(scope="module")
def lib_without(tmp_path_factory):
    return _load(tmp_path_factory.mktemp("stubnoscale"), ("KS265_STUB_NO_SCALE",))


def open_handle(lib, w=W, h=H, **kw):
    return open_at(lib, w, h, **kw)


def i420_args(w, h):
    return (0, w * h, w * h * 5 // 4), (w, w // 2, w // 2), IN_I420


def i420_pic(a: np.ndarray, w: int, h: int, pts=0):
    return dev_pic([a], *i420_args(w, h), pts)


def roi_of(t):
    m = np.random.default_rng(500 + t).integers(-8, 9, ((H + 15) // 16, (W + 15) // 16)).astype(np.int8)
    r = Roi()
    r.type, r.log2_block, r.device, r.data, r.pitch, r.stream = 0, 4, -1, m.ctypes.data, m.strides[0], None
    return m, r


def session(lib, pictures, scaled, filt=1, rgba=False, lanes=1, roi=False, params=()):
    """one handle fed `pictures` (scaled: sources of SW x SH through the scaled entry; else pictures of W x H through the plain entry); its stream"""
    lines = []
    cb = LOG_CB(lambda m: lines.append(m.decode()))
    lib.QY265SetLogPrintf(cb)
    h = open_handle(lib, params=params, lanes=lanes, roi=roi)
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    if scaled:
        assert lib.ks265_enc_enable_device_scale(h, SW, SH) == QY_OK

    def picture(t, a):
        if scaled and rgba:
            put = device_picture(lib, h, [a], (0, 1, 2), (SW * 4,), IN_RGB, t, step=4, scaled=(SW, SH, filt))
        else:
            put = device_picture(lib, h, [a], *i420_args(*((SW, SH) if scaled else (W, H))), t, scaled=(SW, SH, filt) if scaled else None)
        return preceded(lambda: set_map(t), put) if roi and t % 3 != 2 else put

    def set_map(t, keep=[]):
        keep[:] = roi_of(t)                                             # (the map stays the caller's until the picture is taken)
        assert lib.ks265_enc_set_next_roi(h, C.byref(keep[1])) == QY_OK

    bs = drive(lib, h, (picture(t, a) for t, a in enumerate(pictures)))
    lib.QY265SetLogPrintf(None)
    return bs, "".join(lines)


_SRC = {}


def sources(rgba: bool):
    if rgba not in _SRC:
        rng = np.random.default_rng(21 + rgba)
        _SRC[rgba] = rng.integers(0, 256, (N, SH, SW, 4), dtype=np.uint8) if rgba else rng.integers(0, 256, (N, SW * SH * 3 // 2), dtype=np.uint8)
    return _SRC[rgba]


def prescaled(rgba: bool, filt: int):
    src = sources(rgba)
    if rgba:
        return [ys.scale_rgb(p[:, :, 0], p[:, :, 1], p[:, :, 2], W, H, filt, cref.MATRIX_BT709, False) for p in src]
    return [ys.scale_i420(p, SW, SH, W, H, filt) for p in src]


@pytest.mark.parametrize("filt,rgba,lanes,roi", [(1, False, 1, False), (0, False, 1, False), (1, True, 1, False), (0, True, 1, False), (1, False, 2, False), (1, False, 1, True),
                                                  (0, True, 2, True)])
def test_scaled_entry_equals_prescaled_pictures(lib, filt, rgba, lanes, roi):
    params = (("iper", 8),) if lanes == 2 else ()
    got, log = session(lib, sources(rgba), True, filt, rgba, lanes, roi, params)
    exp, _ = session(lib, prescaled(rgba, filt), False, filt, False, lanes, roi, params)
    assert lanes == 1 or "2 GOP lanes" in log
    assert len(got) > 1000 and got == exp
    other, _ = session(lib, prescaled(rgba, 1 - filt), False, filt, False, lanes, roi, params)
    assert other != exp                                                 # the comparison can tell the filters apart


def test_own_size_is_the_plain_entry(lib):
    pics = prescaled(False, 1)
    exp, _ = session(lib, pics, False)
    h = open_handle(lib, lanes=1)
    assert lib.ks265_enc_enable_device_input(h) == QY_OK               # (the switch is not even on)
    assert drive(lib, h, (device_picture(lib, h, [a], *i420_args(W, H), t, scaled=(W, H, 1)) for t, a in enumerate(pics))) == exp


def test_enable_refusals(lib, lib_without):
    h = open_handle(lib)
    assert lib.ks265_enc_enable_device_scale(h, SW, SH) == QY_NOTSUPPORTED          # device input is off
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    live = [lib.ks265_stub_live(k) for k in range(5)]
    for bad in [(132, 96), (128, 97), (0, 96), (128, -2), (8200, 96), (W * 8 + 8, 96), (128, H * 8 + 2)]:
        assert lib.ks265_enc_enable_device_scale(h, *bad) == QY_NOTSUPPORTED, bad
    assert [lib.ks265_stub_live(k) for k in range(5)] == live
    assert lib.ks265_enc_enable_device_scale(h, SW, SH) == QY_OK
    now = [lib.ks265_stub_live(k) for k in range(5)]
    assert now[3] == live[3] + 1 and now[:3] + now[4:] == live[:3] + live[4:]       # one device block per lane: the RGB scratch picture, nothing else
    assert lib.ks265_enc_enable_device_scale(h, SW, SH) == QY_OK and lib.ks265_enc_enable_device_scale(h, SW * 2, SH) == QY_NOTSUPPORTED
    lib.QY265EncoderClose(h)
    h = open_handle(lib)                                                            # after the first picture
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()
    a = prescaled(False, 1)[0]
    assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(i420_pic(a, W, H)), C.byref(outp)) == QY_OK
    assert lib.ks265_enc_enable_device_scale(h, SW, SH) == QY_NOTSUPPORTED
    lib.QY265EncoderClose(h)
    # a device library with device input and without the scaler: one log line
    lines = []
    cb = LOG_CB(lambda m: lines.append(m.decode()))
    lib_without.QY265SetLogPrintf(cb)
    h = open_handle(lib_without)
    assert lib_without.ks265_enc_enable_device_input(h) == QY_OK
    assert lib_without.ks265_enc_enable_device_scale(h, SW, SH) == QY_NOTSUPPORTED
    src = sources(False)[0]
    assert lib_without.ks265_enc_encode_device_frame_scaled(h, C.byref(nal), C.byref(nn), C.byref(i420_pic(src, SW, SH)), SW, SH, 1, C.byref(outp)) == QY_NOTSUPPORTED
    lib_without.QY265EncoderClose(h)
    lib_without.QY265SetLogPrintf(None)
    assert "".join(lines).count("ks265enc: input scaling is unavailable: ") == 1


def test_picture_refusals_enqueue_nothing_and_keep_the_map(lib):
    h = open_handle(lib, roi=True, lanes=1)
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()
    src = sources(False)[0].copy()
    big = np.zeros(1024 * 96 * 3 // 2, np.uint8)
    before = calls(lib)
    assert lib.ks265_enc_encode_device_frame_scaled(h, C.byref(nal), C.byref(nn), C.byref(i420_pic(src, SW, SH)), SW, SH, 1, C.byref(outp)) == QY_NOTSUPPORTED   # the switch is off
    assert lib.ks265_enc_enable_device_scale(h, SW, SH) == QY_OK
    m = np.full(((H + 7) // 8, (W + 7) // 8), 3, np.int8)                               # a map in "device" memory: its reduction shows in the call log
    r = Roi()
    r.type, r.log2_block, r.device, r.data, r.pitch, r.stream = 0, 3, 0, m.ctypes.data, m.strides[0], None
    assert lib.ks265_enc_set_next_roi(h, C.byref(r)) == QY_OK
    ok = i420_pic(src, SW, SH)
    cases = [(ok, 132, 96, 1, QY_NOTSUPPORTED), (ok, 128, 95, 1, QY_NOTSUPPORTED), (ok, 120, 96, 2, QY_NOTSUPPORTED), (ok, 128, 96, 2, QY_NOTSUPPORTED), (ok, 128, 96, -1, QY_NOTSUPPORTED),
             (i420_pic(big, 1024, 96), 1024, 96, 1, QY_NOTSUPPORTED),                   # above the maximum (and a ratio above 8)
             (ok, 8, 2, 1, QY_NOTSUPPORTED)]                                            # a ratio of 8 is allowed, 24 is not
    p = i420_pic(src, SW, SH); p.plane[1] = None
    cases.append((p, SW, SH, 1, QY_POINTER))
    p = i420_pic(src, SW, SH); p.pitch[0] = SW - 8
    cases.append((p, SW, SH, 1, QY_POINTER))
    p = i420_pic(src, SW, SH); p.device = 1
    cases.append((p, SW, SH, 1, QY_NOTSUPPORTED))
    p = i420_pic(src, SW, SH); p.format = 7
    cases.append((p, SW, SH, 1, QY_NOTSUPPORTED))
    for pic, sw, sh, filt, code in cases:
        assert lib.ks265_enc_encode_device_frame_scaled(h, C.byref(nal), C.byref(nn), C.byref(pic), sw, sh, filt, C.byref(outp)) == code, (sw, sh, filt)
        assert nn.value == 0 and lib.QY265EncoderDelayedFrames(h) == 0
    assert calls(lib) == before, "a refused picture enqueued something"
    assert lib.ks265_enc_encode_device_frame_scaled(h, C.byref(nal), C.byref(nn), C.byref(ok), SW, SH, 1, C.byref(outp)) == QY_OK
    new = open(lib.call_log_path).read().split("\n")[before:]
    assert sum("ks265_roi_reduce" in l for l in new) == 1, "the pending map went with the first picture that was taken"
    assert sum("ks265_input_scale" in l for l in new) == 1 and not any("ks265_input_convert" in l for l in new)
    assert lib.ks265_enc_encode_device_frame_scaled(h, C.byref(nal), C.byref(nn), C.byref(ok), SW, SH, 1, C.byref(outp)) == QY_OK
    assert sum("ks265_roi_reduce" in l for l in open(lib.call_log_path).read().split("\n")[before:]) == 1
    lib.QY265EncoderClose(h)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


def test_plan_cache_keeps_four_and_leaks_nothing(lib):
    h = open_handle(lib, lanes=1, params=(("bframes", 0),))
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    assert lib.ks265_enc_enable_device_scale(h, 256, 192) == QY_OK
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()
    sizes = [(128, 96), (96, 64), (256, 192), (72, 56), (104, 80)]
    buf = np.random.default_rng(3).integers(0, 256, 256 * 192 * 3 // 2, dtype=np.uint8)

    def put(k, filt=1):
        sw, sh = sizes[k]
        before = lib.ks265_stub_creating_calls(), lib.ks265_stub_live(3), calls(lib)
        assert lib.ks265_enc_encode_device_frame_scaled(h, C.byref(nal), C.byref(nn), C.byref(i420_pic(buf, sw, sh)), sw, sh, filt, C.byref(outp)) == QY_OK
        new = open(lib.call_log_path).read().split("\n")[before[2]:]
        assert sum("ks265_input_scale" in l for l in new) == 1
        return lib.ks265_stub_creating_calls() - before[0], lib.ks265_stub_live(3) - before[1]

    assert [put(k) for k in range(4)] == [(1, 1)] * 4                   # four sizes: four plans
    assert [put(k) for k in (0, 1, 2, 3, 3, 0)] == [(0, 0)] * 6         # all cached
    assert put(4) == (1, 0)                                             # a fifth: created, the least recently used one (size 1) destroyed
    assert [put(k) for k in (0, 2, 3, 4)] == [(0, 0)] * 4
    assert put(1) == (1, 0)                                             # size 1 had gone; now size 0 goes
    assert put(1, filt=0) == (1, 0)                                     # the filter is part of the key
    assert put(0) == (1, 0)
    while lib.QY265EncoderDelayedFrames(h) > 0:
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == QY_OK
    lib.QY265EncoderClose(h)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5, "contexts, frame objects, events, device and pinned blocks"
