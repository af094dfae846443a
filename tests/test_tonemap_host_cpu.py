"""CPU: tone mapping on the way in (ks265_enc_enable_tonemap, include/ks265_enc.h) through the real encoder host, against the stand-in of the device library WITH the
entries (tests/hip_stub_tonemap.c):
  * the stand-in's routine gives tests/tonemap_ref.py's bytes on the shapes of the GPU test - formats, ranges, curves, peaks - and refuses what the device library refuses;
  * P010 and I010 pictures on a tone-mapping handle at 64x48 and 136x72, default GOP and zero latency, one lane and two: byte for byte the stream of the reference-mapped
    8-bit I420 pictures on a plain device-input handle; the same through the scaled entry, 128x96 to 64x48.  ON THE PARENT COMMIT THIS TEST FAILS: the library has no
    ks265_enc_enable_tonemap (an AttributeError, not a skip);
  * every refusal returns its code, adds nothing to the stand-in's call log and leaves the handle usable; a stand-in without the entries: QY_NOTSUPPORTED and ONE log line;
  * off is the parent: a zero-latency device-input session that never enables tone mapping writes the call log of the same session on the stub this one includes;
  * tests/tonemap_main.c, the routine and the table builder under -fsanitize=address,undefined as a program of its own, rows ending where their blocks end."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

import tonemap_ref as tm
import yuv_hibit_ref as yh
from host_harness import (QY_NOTSUPPORTED, QY_OK, QY_POINTER, Nal, Picture, build_host_lib, build_host_program, calls, dev_pic, device_picture, drive, i420_picture, load_host_lib,
                          logged, nal_bytes, open_handle, same_calls)

KS265_POINTER, KS265_NOTSUPPORTED = -3, -4
FORMATS = {"P010": (yh.SEMI, 10, 1), "I010": (yh.PLANAR, 10, 0), "P012": (yh.SEMI, 12, 1), "P016": (yh.SEMI, 16, 1)}
SHAPES = [(8, 2), (24, 6), (72, 34), (520, 4)]
SETTINGS = [(curve, full, peak) for curve in tm.CURVES.values() for full in (0, 1) for peak in (1000.0, 4000.0)]


class Tonemap(C.Structure):                   # ks265_tonemap
    _fields_ = [("transfer", C.c_int), ("curve", C.c_int), ("full_range", C.c_int), ("peak_nits", C.c_double), ("white_nits", C.c_double)]


class TonemapCfg(C.Structure):                # ks265_tonemap_cfg
    _fields_ = [("transfer", C.c_int32), ("curve", C.c_int32), ("full_range", C.c_int32), ("peak_nits", C.c_double), ("white_nits", C.c_double)]


class InDesc(C.Structure):                    # ks265_in_desc
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3), ("pixel_step", C.c_int32),
                ("matrix", C.c_int32), ("full_range", C.c_int32)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_host_lib(build_host_lib("hip_stub_tonemap.c"), call_log=str(tmp_path_factory.mktemp("stubtm") / "calls.log"))


@pytest.fixture(scope="module")
def without(tmp_path_factory):
    """the stand-in without the entries: the device library of the parent"""
    return load_host_lib(build_host_lib("hip_stub_overlay.c"), call_log=str(tmp_path_factory.mktemp("stubnotm") / "calls.log"))


def code_of(name):
    layout, depth, msb = FORMATS[name]
    return yh.code(layout, yh.S420, depth, msb)


def hdr_planes(seed, name, w, h):
    layout, depth, msb = FORMATS[name]
    return yh.random_planes(np.random.default_rng(seed), layout, yh.S420, depth, msb, w, h)


def desc_of(code, w, h, bufs, offs, pitches):
    d = InDesc()
    d.format, d.width, d.height = code, w, h
    for k, off in enumerate(offs):
        d.plane[k], d.pitch[k] = bufs[k].ctypes.data + off, pitches[k]
    return d


def aligned(n, fill=0xA5):
    buf = np.full(n + 16 + 32, fill, np.uint8)
    off = -buf.ctypes.data % 16 + 16
    return buf, off


# ------------------------------------------------------------------ the stand-in's routine

@pytest.mark.parametrize("name", sorted(FORMATS))
def test_stand_in_equals_the_reference(lib, name):
    layout, depth, msb = FORMATS[name]
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    for curve, full, peak in SETTINGS:
        plan = C.c_void_p()
        assert lib.ks265_tonemap_plan_create(ctx, C.byref(TonemapCfg(16, curve, full, peak, 203.0)), C.byref(plan)) == 0
        for w, h in SHAPES:
            for content in ("random", "primaries", "ramp"):
                if content == "random":
                    pl = hdr_planes(w + curve, name, w, h)
                elif content == "primaries":
                    pl = tm.primaries(depth, layout, msb, w, h, bool(full))
                elif (w, h) == SHAPES[0] and depth < 16:               # every luma code once under neutral chroma, a picture of 32 columns
                    pl = tm.grey_ramp(depth, layout, msb)
                    h, w = pl[0].shape
                else:
                    continue
                bufs, offs, pitches = yh.lay_out(pl, 1, 3)
                buf, off = aligned(w * h * 3 // 2)
                n = w * h * 3 // 2
                assert lib.ks265_input_tonemap(ctx, plan, C.byref(desc_of(code_of(name), w, h, bufs, offs, pitches)), C.c_void_p(buf.ctypes.data + off)) == 0
                exp = tm.to_i420(pl, layout, depth, msb, curve, peak, 203.0, bool(full))
                assert (buf[off:off + n] == exp).all(), (curve, full, peak, w, h, content)
                assert (buf[:off] == 0xA5).all() and (buf[off + n:] == 0xA5).all()
        assert lib.ks265_tonemap_plan_destroy(ctx, plan) == 0
    lib.ks265_destroy(ctx)


def test_stand_in_refuses_what_the_library_refuses(lib):
    ctx, plan = C.c_void_p(), C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    for bad in (TonemapCfg(18, 0, 0, 1000.0, 203.0), TonemapCfg(16, 3, 0, 1000.0, 203.0), TonemapCfg(16, 0, 2, 1000.0, 203.0), TonemapCfg(16, 0, 0, 99.0, 80.0),
                TonemapCfg(16, 0, 0, 10001.0, 203.0), TonemapCfg(16, 0, 0, 1000.0, 79.0), TonemapCfg(16, 0, 0, 1000.0, 1001.0), TonemapCfg(16, 0, 0, 150.0, 203.0),
                TonemapCfg(16, 0, 0, 0.0, 0.0)):
        assert lib.ks265_tonemap_plan_create(ctx, C.byref(bad), C.byref(plan)) == KS265_NOTSUPPORTED and not plan.value
    assert lib.ks265_tonemap_plan_create(ctx, C.byref(TonemapCfg(16, 0, 0, 1000.0, 203.0)), C.byref(plan)) == 0
    w, h = 8, 2
    pl = hdr_planes(1, "P010", w, h)
    bufs, offs, pitches = yh.lay_out(pl, 0, 2)
    buf, off = aligned(w * h * 3 // 2)
    dst = C.c_void_p(buf.ctypes.data + off)
    ok = lambda code=code_of("P010"): desc_of(code, w, h, bufs, offs, pitches)
    cases = [(ok(c), KS265_NOTSUPPORTED) for c in (0, 1, 2, yh.code(1, 0, 8), yh.code(0, 0, 9), yh.code(1, 1, 10, 1), yh.code(1, 2, 10, 1), yh.code(2, 1, 10, 1), yh.code(1, 0, 17, 1), -1)]
    x = ok(); x.pitch[0] += 1; cases.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.plane[1] += 1; cases.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.width = 12; cases.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.height = 3; cases.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.pitch[1] = 2 * w - 2; cases.append((x, KS265_POINTER))
    x = ok(); x.plane[0] = None; cases.append((x, KS265_POINTER))
    before = calls(lib)
    for x, want in cases:
        assert lib.ks265_input_tonemap_validate(ctx, plan, C.byref(x)) == want, hex(x.format & 0xFFFFFFFF)
        assert lib.ks265_input_tonemap(ctx, plan, C.byref(x), dst) == want
    assert lib.ks265_input_tonemap(ctx, plan, C.byref(ok()), None) == KS265_POINTER
    assert lib.ks265_input_tonemap(ctx, plan, C.byref(ok()), C.c_void_p(dst.value + 4)) == KS265_NOTSUPPORTED
    assert calls(lib) == before and (buf == 0xA5).all()
    assert lib.ks265_input_tonemap(ctx, plan, C.byref(ok()), dst) == 0 and calls(lib) == before + 1
    assert lib.ks265_tonemap_plan_destroy(ctx, plan) == 0
    lib.ks265_destroy(ctx)


# ------------------------------------------------------------------ streams

def tonemap_handle(lib, w, h, tmo, scale=None, **kw):
    hd = open_handle(lib, w, h, **kw)
    assert lib.ks265_enc_enable_device_input(hd) == QY_OK
    if scale:
        assert lib.ks265_enc_enable_device_scale(hd, *scale) == QY_OK
    if tmo is not None:
        assert lib.ks265_enc_enable_tonemap(hd, C.byref(tmo)) == QY_OK
    return hd


def hdr_session(lib, name, w, h, clip, tmo, scaled=None, **kw):
    """the stream of HDR pictures `clip` (lists of planes, at the source's size) on a tone-mapping handle of w x h"""
    hd = tonemap_handle(lib, w, h, tmo, scale=scaled[:2] if scaled else None, **kw)
    laid = [yh.lay_out(pl, 1, 3) for pl in clip]
    return drive(lib, hd, (device_picture(lib, hd, b, o, p, code_of(name), t, full_range=1, scaled=scaled) for t, (b, o, p) in enumerate(laid)))   # (full_range of the picture: ignored for YUV)


def sdr_session(lib, w, h, mapped, sw, sh, scaled=None, **kw):
    """the stream of the mapped 8-bit pictures on a plain device-input handle"""
    hd = tonemap_handle(lib, w, h, None, scale=scaled[:2] if scaled else None, **kw)
    return drive(lib, hd, (i420_picture(lib, hd, p, sw, sh, t, scaled=scaled) for t, p in enumerate(mapped)))


def mapped_clip(name, clip, tmo):
    layout, depth, msb = FORMATS[name]
    return [tm.to_i420(pl, layout, depth, msb, tmo.curve, tmo.peak_nits or 1000.0, tmo.white_nits or 203.0, bool(tmo.full_range)) for pl in clip]


def moving_hdr(name, w, h, n, seed):
    """n HDR pictures with structure that moves: a PQ ramp, coloured bars and noise"""
    layout, depth, msb = FORMATS[name]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        top = (1 << depth) - 1
        y = np.clip((0.1 + 0.6 * ((xx + 3 * t) % w) / w + 0.1 * np.sin(0.2 * (yy + t))) * top + rng.integers(0, 1 << (depth - 6), (h, w)), 0, top).astype(np.int64)
        u = np.clip((0.5 + 0.3 * np.sin(0.1 * (xx[::2, ::2] + t))) * top, 0, top).astype(np.int64)
        v = np.clip((0.5 + 0.3 * np.cos(0.13 * (yy[::2, ::2] + 2 * t))) * top, 0, top).astype(np.int64)
        sh = 16 - depth if msb else 0
        y, u, v = ((p << sh).astype(np.uint16) for p in (y, u, v))
        if layout == yh.SEMI:
            c = np.empty((h // 2, w), np.uint16)
            c[:, 0::2], c[:, 1::2] = u, v
            out.append([y, c])
        else:
            out.append([y, u, v])
    return out


@pytest.mark.parametrize("latency", [b"default", b"zerolatency"])
@pytest.mark.parametrize("w,h", [(64, 48), (136, 72)])
@pytest.mark.parametrize("name", ["P010", "I010"])
def test_tone_mapped_stream_is_the_plain_stream_of_mapped_pictures(lib, name, w, h, latency):
    """fails on the parent commit: no ks265_enc_enable_tonemap there"""
    tmo = Tonemap(16, tm.BT2390 if name == "P010" else tm.REINHARD, int(name == "I010"), 0.0, 0.0)
    clip = moving_hdr(name, w, h, 5, 11)
    want = sdr_session(lib, w, h, mapped_clip(name, clip, tmo), w, h, lanes=1, latency=latency)
    assert len(want) > 200
    for lanes in (1, 2):
        assert hdr_session(lib, name, w, h, clip, tmo, lanes=lanes, latency=latency) == want, lanes
    plain = hdr_session(lib, name, w, h, clip, None, lanes=1, latency=latency)
    assert plain != want                                               # (without the call: the pictures are only rounded)


def test_two_lanes_with_short_gops_give_the_one_lane_bytes(lib):
    w, h, n = 64, 48, 9
    tmo = Tonemap(16, tm.CLIP, 0, 4000.0, 203.0)
    clip = moving_hdr("P010", w, h, n, 12)
    params = (("iper", 4), ("bframes", 0))
    want = sdr_session(lib, w, h, mapped_clip("P010", clip, tmo), w, h, lanes=1, params=params)
    assert hdr_session(lib, "P010", w, h, clip, tmo, lanes=2, params=params) == want
    assert hdr_session(lib, "P010", w, h, clip, tmo, lanes=1, params=params) == want


@pytest.mark.parametrize("name", ["P010", "I010"])
def test_through_the_scaled_entry(lib, name):
    sw, sh, w, h = 128, 96, 64, 48
    tmo = Tonemap(16, tm.BT2390, 0, 1000.0, 203.0)
    clip = moving_hdr(name, sw, sh, 5, 13)
    want = sdr_session(lib, w, h, mapped_clip(name, clip, tmo), sw, sh, scaled=(sw, sh, 1), lanes=1)
    for lanes in (1, 2):
        assert hdr_session(lib, name, w, h, clip, tmo, scaled=(sw, sh, 1), lanes=lanes) == want


# ------------------------------------------------------------------ refusals, and off

def test_refusals_leave_the_handle_usable(lib, without, capfd):
    w, h = 64, 48
    good = Tonemap(16, 0, 0, 0.0, 0.0)
    clip = moving_hdr("P010", w, h, 3, 14)
    want = sdr_session(lib, w, h, mapped_clip("P010", clip, good), w, h, lanes=1, latency=b"zerolatency")
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()

    hd = open_handle(lib, w, h, lanes=1, latency=b"zerolatency")
    (rcs, log) = logged(lib, lambda: [lib.ks265_enc_enable_tonemap(hd, C.byref(good)), lib.ks265_enc_enable_tonemap(None, C.byref(good)), lib.ks265_enc_enable_tonemap(hd, None)])
    assert rcs == [QY_NOTSUPPORTED, QY_POINTER, QY_POINTER] and not log          # before device input
    assert lib.ks265_enc_enable_device_input(hd) == QY_OK
    bad = [Tonemap(18, 0, 0, 0.0, 0.0), Tonemap(1, 0, 0, 0.0, 0.0), Tonemap(16, 3, 0, 0.0, 0.0), Tonemap(16, -1, 0, 0.0, 0.0), Tonemap(16, 0, 2, 0.0, 0.0), Tonemap(16, 0, 0, 99.0, 0.0),
           Tonemap(16, 0, 0, 10001.0, 0.0), Tonemap(16, 0, 0, 0.0, 79.0), Tonemap(16, 0, 0, 0.0, 1001.0), Tonemap(16, 0, 0, 150.0, 0.0), Tonemap(16, 0, 0, float("nan"), 0.0)]
    (rcs, log) = logged(lib, lambda: [lib.ks265_enc_enable_tonemap(hd, C.byref(b)) for b in bad])
    assert rcs == [QY_NOTSUPPORTED] * len(bad) and not log                        # a field out of range
    assert lib.ks265_enc_enable_tonemap(hd, C.byref(good)) == QY_OK
    assert lib.ks265_enc_enable_tonemap(hd, C.byref(good)) == QY_NOTSUPPORTED     # once

    def refused(planes, code, scaled=None):
        b, o, p = yh.lay_out(planes, 0, 0)
        d = dev_pic(b, o, p, code)
        if scaled:
            return lib.ks265_enc_encode_device_frame_scaled(hd, C.byref(nal), C.byref(nn), C.byref(d), scaled[0], scaled[1], 0, C.byref(outp))
        return lib.ks265_enc_encode_device_frame(hd, C.byref(nal), C.byref(nn), C.byref(d), C.byref(outp))

    p422 = yh.random_planes(np.random.default_rng(1), yh.SEMI, yh.S422, 10, 1, w, h)
    p444 = yh.random_planes(np.random.default_rng(1), yh.PLANAR, yh.S444, 12, 0, w, h)
    p9 = yh.random_planes(np.random.default_rng(1), yh.PLANAR, yh.S420, 9, 0, w, h)
    y210 = yh.random_planes(np.random.default_rng(1), yh.YUYV, yh.S422, 10, 1, w, h)
    (rcs, log) = logged(lib, lambda: [refused(p422, yh.code(yh.SEMI, yh.S422, 10, 1)), refused(p444, yh.code(yh.PLANAR, yh.S444, 12, 0)), refused(p9, yh.code(yh.PLANAR, yh.S420, 9, 0)),
                                      refused(y210, yh.code(yh.YUYV, yh.S422, 10, 1))])
    assert rcs == [QY_NOTSUPPORTED] * 4 and not log and nn.value == 0             # high-bit-depth YUV outside the list: never passed through unmapped
    laid = [yh.lay_out(pl, 1, 3) for pl in clip]
    subs = [device_picture(lib, hd, b, o, p, code_of("P010"), t) for t, (b, o, p) in enumerate(laid)]
    first = subs[0](nal, nn, outp)
    assert first == QY_OK
    head = nal_bytes(nal, nn)
    (rc, log) = logged(lib, lambda: lib.ks265_enc_enable_tonemap(hd, C.byref(good)))
    assert rc == QY_NOTSUPPORTED and not log                                      # after the first picture
    (rc, log) = logged(lib, lambda: refused(p422, yh.code(yh.SEMI, yh.S422, 10, 1)))
    assert rc == QY_NOTSUPPORTED and not log
    assert head + drive(lib, hd, subs[1:]) == want                                # the handle went on as if nothing had been asked

    # enabling after the first picture on a handle that never had it; a handle of 100x50
    hd = tonemap_handle(lib, w, h, None, lanes=1, latency=b"zerolatency")
    mapped = mapped_clip("P010", clip, good)
    assert i420_picture(lib, hd, mapped[0], w, h, 0)(nal, nn, outp) == QY_OK
    (rc, log) = logged(lib, lambda: lib.ks265_enc_enable_tonemap(hd, C.byref(good)))
    assert rc == QY_NOTSUPPORTED and not log
    drive(lib, hd, [i420_picture(lib, hd, mapped[1], w, h, 1)])
    hd = open_handle(lib, 100, 50, lanes=1, latency=b"zerolatency")
    assert lib.ks265_enc_enable_device_input(hd) == QY_OK
    (rc, log) = logged(lib, lambda: lib.ks265_enc_enable_tonemap(hd, C.byref(good)))
    assert rc == QY_NOTSUPPORTED and not log
    lib.QY265EncoderClose(hd)

    # a device library without the entries: one line, however often it is asked
    capfd.readouterr()
    hd = tonemap_handle(without, w, h, None, lanes=1, latency=b"zerolatency")
    assert [without.ks265_enc_enable_tonemap(hd, C.byref(good)) for _ in range(3)] == [QY_NOTSUPPORTED] * 3
    without.QY265EncoderClose(hd)
    said = capfd.readouterr()
    assert (said.out + said.err).count("ks265enc: tone mapping is unavailable: ") == 1


def test_off_is_the_parent_s_call_log(lib, without):
    """a device-input session that never enables tone mapping: the same calls, line for line, as on a device library that does not have the entries (zero latency: the call
    log of a GOP of B pictures depends on thread timing)"""
    w, h = 64, 48
    clip = moving_hdr("P010", w, h, 4, 15)
    logs = []
    for l in (lib, without):
        stream, log = logged(l, lambda: hdr_session(l, "P010", w, h, clip, None, lanes=1, latency=b"zerolatency"))
        logs.append((stream, same_calls(log)))
    assert logs[0] == logs[1]
    assert not any("tonemap" in ln for ln in logs[0][1])


# ------------------------------------------------------------------ under the sanitizers

@pytest.fixture(scope="module")
def sanitized():
    return build_host_program("tonemap_main.c")


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_routine_and_tables_under_the_sanitizers(sanitized, tmp_path, name):
    layout, depth, msb = FORMATS[name]
    for k, ((w, h), (curve, full, peak)) in enumerate(zip(SHAPES, [(0, 0, 1000.0), (1, 1, 4000.0), (2, 0, 1000.0), (0, 1, 4000.0)])):
        pl = hdr_planes(100 + k, name, w, h)
        (tmp_path / "in").write_bytes(b"".join(p.tobytes() for p in pl))
        r = subprocess.run([sanitized, str(layout), str(depth), str(msb), str(full), str(curve), repr(peak), "203.0", str(w), str(h), str(k), str(tmp_path / "in"), str(tmp_path / "out"),
                            str(tmp_path / "tab")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        got = np.frombuffer((tmp_path / "out").read_bytes(), np.uint8)
        assert (got == tm.to_i420(pl, layout, depth, msb, curve, peak, 203.0, bool(full))).all(), (w, h)
