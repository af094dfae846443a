"""CPU: overlays (ks265_enc_set_overlay, include/ks265_enc.h) through the real encoder host, against the stand-in of the device library WITH the two entries
(tests/hip_stub_overlay.c):
  * the stand-in's blend equals tests/overlay_ref.py byte for byte (formats, clipping, the window, eight overlays) and refuses what the device library refuses;
  * at 208x136, 9 pictures, zero latency and the default GOP: the stream of a handle with overlays - a host RGBA logo and a "device" float32 caption, clipped - equals the
    stream of a plain handle fed the pictures pre-blended by overlay_ref.  ON THE PARENT COMMIT THIS TEST FAILS: the library has no ks265_enc_set_overlay (an
    AttributeError, not a skip);
  * the same with two GOP lanes (the set travels with the picture: the one-lane bytes), with `denoise=2 edge=2` (pre-blended BEHIND the filters' references: neither the
    filters nor the denoiser's history see the overlay) and at 202x134 (clipped to the window, the padding keeps its bytes);
  * no overlay set: the call log is that of the same encode on a stand-in WITHOUT the entries (tests/hip_stub_hdr.c) and names no overlay call;
  * set, replace and clear between pictures take effect at exactly the next picture; KS265_OV_FORCED_ONLY follows bForceLogo and is never drawn for device pictures;
    a host overlay's buffer may be written over right after the set call;
  * every refusal returns its code and leaves the slot as it was; a stand-in without the entries: QY_NOTSUPPORTED and ONE log line; a handle without twins refuses its
    first overlay while pictures are in flight (one log line) and takes it after the flush - the pictures behind it carry it; GOP lanes on several GPUs and the KS265_GRAPH
    experiment refuse every set call and code the plain stream;
  * the CLI's -logo;
  * tests/overlay_main.c, the host and the stand-in under -fsanitize=address,undefined as a program of its own: its script of sets, replacements, refusals and bForceLogo,
    both latencies - the input slots it dumps are overlay_ref's, byte for byte, and its stream is the plain handle's of those pictures."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import enhance_ref as er
import overlay_ref as ovr
import picture_window_ref as pw
import window_sps as ws
import yuv_float_ref as yf
from host_harness import (QY_NOTSUPPORTED, QY_OK, QY_POINTER, DevPicture, Nal, Picture, build_host_cli, build_host_lib, build_host_program, drive, edgy_clip, host_picture,
                          i420_picture, load_host_lib, logged, nal_bytes, nals, open_handle, packed_yuv, same_calls, session)

W, H, N = 208, 136, 9
IN_RGB = 2
FORCED_ONLY = 1


class Overlay(C.Structure):                   # ks265_overlay
    _fields_ = [("rgb", DevPicture), ("width", C.c_int), ("height", C.c_int), ("alpha", C.c_void_p), ("x", C.c_int), ("y", C.c_int), ("opacity", C.c_int), ("flags", C.c_int)]


class OvDesc(C.Structure):                    # ks265_overlay_desc
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3), ("pixel_step", C.c_int32),
                ("matrix", C.c_int32), ("full_range", C.c_int32), ("alpha", C.c_void_p), ("x", C.c_int32), ("y", C.c_int32), ("opacity", C.c_int32)]


class OvCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("w", "h", "win_w", "win_h", "n")] + [(n, C.c_int32 * 8) for n in ("ow", "oh", "x", "y", "opacity", "format")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_host_lib(build_host_lib("hip_stub_overlay.c"), call_log=str(tmp_path_factory.mktemp("stubov") / "calls.log"))


@pytest.fixture(scope="module")
def without(tmp_path_factory):
    """the stand-in without the two entries: the device library of the parent"""
    return load_host_lib(build_host_lib("hip_stub_hdr.c"), call_log=str(tmp_path_factory.mktemp("stubnoov") / "calls.log"))


def ov_calls(lib):
    buf = (OvCall * 1024)()
    n = lib.ks265_stub_overlay_calls(buf, 1024)
    return [(c.w, c.h, c.win_w, c.win_h, [(c.ow[k], c.oh[k], c.x[k], c.y[k], c.opacity[k], c.format[k]) for k in range(c.n)]) for c in buf[:n]]


# ------------------------------------------------------------------ overlays as arrays

class Ov:
    """an overlay over an (h, w, n) array: `order` names the elements of R, G, B; alpha: element 3 or None; fmt: None = bytes, else yuv_float_ref's code"""

    def __init__(self, arr, order=(0, 1, 2), alpha=True, x=0, y=0, opacity=256, matrix=0, full=0, fmt=None, flags=0, device=-1):
        self.arr, self.order, self.alpha, self.x, self.y, self.opacity, self.matrix, self.full, self.fmt, self.flags, self.device = arr, order, alpha, x, y, opacity, matrix, full, fmt, flags, device

    def at(self, arr):
        o = Ov.__new__(Ov)
        o.__dict__.update(self.__dict__, arr=arr)
        return o

    def ref(self):
        ch = [ovr.codes(np.ascontiguousarray(self.arr[:, :, k]), self.fmt) for k in (*self.order, *([3] if self.alpha else []))]
        return ovr.overlay(ch[0], ch[1], ch[2], ch[3] if self.alpha else None, self.x, self.y, self.opacity, self.matrix, bool(self.full))

    def _fill(self, d, base):
        es = self.arr.strides[2]                                        # (between the channels: the element for HWC, a plane for a transposed CHW view)
        d.format = IN_RGB if self.fmt is None else self.fmt
        for k in range(3):
            d.plane[k] = base + self.order[k] * es
        d.pitch[0], d.pixel_step, d.matrix, d.full_range = self.arr.strides[0], self.arr.strides[1], self.matrix, self.full
        return base + 3 * es if self.alpha else None

    def c(self):
        """the ks265_overlay, reading the array where it lies"""
        o = Overlay()
        o.alpha = self._fill(o.rgb, self.arr.ctypes.data)
        o.rgb.device, o.rgb.stream = self.device, None
        o.width, o.height, o.x, o.y, o.opacity, o.flags = self.arr.shape[1], self.arr.shape[0], self.x, self.y, self.opacity, self.flags
        return o

    def desc(self, d):
        d.alpha = self._fill(d, self.arr.ctypes.data)
        d.width, d.height, d.x, d.y, d.opacity = self.arr.shape[1], self.arr.shape[0], self.x, self.y, self.opacity


def rgba8(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def floats(seed, w, h, dtype=np.float32):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.2, 1.2, (h, w, 4)).astype(np.float32)
    v[rng.uniform(size=v.shape) < 0.03] = np.nan
    v[rng.uniform(size=v.shape) < 0.03] = 9.0
    return v.astype(dtype)


def set_overlay(lib, hd, slot, ov):
    return lib.ks265_enc_set_overlay(hd, slot, C.byref(ov.c()) if ov is not None else None)


# ------------------------------------------------------------------ the stand-in's blend

def stub_blend(lib, ctx, w, h, pic, ovs, ww=None, wh=None):
    buf = np.zeros(pic.size + 16, np.uint8)
    off = -buf.ctypes.data % 16
    view = buf[off:off + pic.size]
    view[:] = pic
    descs = (OvDesc * len(ovs))()
    for d, o in zip(descs, ovs):
        o.desc(d)
    assert lib.ks265_input_overlay(ctx, descs, len(ovs), w, h, ww or w, wh or h, C.c_void_p(view.ctypes.data)) == 0
    return view.copy()


def test_stand_in_equals_the_reference(lib):
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    for (w, h, ww, wh) in ((72, 40, 72, 40), (208, 136, 202, 134)):
        pic = np.random.default_rng(w).integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
        t, f16, f32 = rgba8(1, 24, 16), floats(2, 40, 12, np.float16), floats(3, 16, 20)
        bf = yf.f32_to_bf16(np.nan_to_num(floats(4, 20, 8), nan=0.5)).reshape(8, 20, 4)
        planar = np.random.default_rng(5).integers(0, 256, (4, 10, 33), dtype=np.uint8)[:, :, 1:31].transpose(1, 2, 0)        # (h, w, 4) view of four planes at odd addresses
        cases = [[Ov(t, x=0, y=0)], [Ov(t, (2, 1, 0), x=-10, y=-6, opacity=200, matrix=1, full=1)], [Ov(t, alpha=False, x=ww - 10, y=wh - 6, opacity=77, full=1)], [Ov(t, x=w, y=0)],
                 [Ov(rgba8(6, 2, 2), x=ww - 2, y=wh - 2)], [Ov(f16, x=6, y=2, fmt=yf.IN_RGB_F16, matrix=1)], [Ov(f32, (2, 1, 0), x=30, y=-4, fmt=yf.IN_RGB_F32)],
                 [Ov(bf, x=14, y=24, opacity=255, fmt=yf.IN_RGB_BF16)],
                 [Ov(t, x=4 * k - 6, y=2 * k - 2, opacity=256 - 20 * k, matrix=k & 1, full=(k >> 1) & 1) if k % 3 else Ov(f32, x=2 * k, y=4 * k, fmt=yf.IN_RGB_F32, opacity=250) for k in range(8)]]
        for ovs in cases:
            exp = ovr.blend(pic, w, h, [o.ref() for o in ovs], ww, wh)
            assert (stub_blend(lib, ctx, w, h, pic, ovs, ww, wh) == exp).all(), (w, h, [(o.x, o.y, o.fmt) for o in ovs])
        pl = Ov(planar, x=8, y=8)
        d = (OvDesc * 1)()
        pl.desc(d[0])
        assert d[0].pixel_step == 1 and d[0].plane[0] % 2 == 1
        assert (stub_blend(lib, ctx, w, h, pic, [pl], ww, wh) == ovr.blend(pic, w, h, [pl.ref()], ww, wh)).all()
    lib.ks265_destroy(ctx)


def test_stand_in_refuses_what_the_library_refuses(lib):
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    t = rgba8(1, 24, 16)
    pic = np.zeros(72 * 40 * 3 // 2 + 16, np.uint8)
    p = C.c_void_p(pic.ctypes.data + (-pic.ctypes.data % 16))

    def rc(n=1, w=72, h=40, ww=72, wh=40, pic=p, **kw):
        d = (OvDesc * 8)()
        for k in range(min(n, 8)):
            Ov(t, x=8, y=4).desc(d[k])
            for name, v in kw.items():
                setattr(d[k], name, v)
        return lib.ks265_input_overlay(ctx, d, n, w, h, ww, wh, pic)
    assert rc() == 0
    pic[:] = 0
    for kw in (dict(n=0), dict(n=9), dict(w=70), dict(h=36), dict(ww=74), dict(ww=71), dict(wh=0), dict(width=23), dict(height=0), dict(x=7), dict(y=-3), dict(x=16386), dict(opacity=257),
               dict(opacity=-1), dict(format=0), dict(format=19), dict(pixel_step=0), dict(pixel_step=17), dict(matrix=2), dict(format=yf.IN_RGB_F32), dict(format=yf.IN_RGB_F16, pixel_step=8),
               dict(pic=C.c_void_p(p.value + 1))):
        assert rc(**kw) == -4, kw
    for kw in (dict(pitch=(C.c_int32 * 3)(92, 0, 0)), dict(pic=None), dict(plane=(C.c_void_p * 3)(None, t.ctypes.data, t.ctypes.data))):
        assert rc(**kw) == -3, kw
    assert not pic.any(), "a refused call wrote something"
    lib.ks265_destroy(ctx)


# ------------------------------------------------------------------ streams

CONFIGS = {"zerolatency": b"zerolatency", "gop8": b"default"}
_src = {}


def source(w=W, h=H, n=N, seed=301):
    if (w, h, n, seed) not in _src:
        _src[(w, h, n, seed)] = edgy_clip(w, h, n, seed)
    return _src[(w, h, n, seed)]


LOGO = Ov(rgba8(11, 48, 24), (2, 1, 0), x=W - 40, y=-4, opacity=192, matrix=1, full=1)                       # host memory, BGRA, clipped at the right and the top
CAPTION = Ov(floats(12, 96, 16), x=100, y=-8, fmt=yf.IN_RGB_F32, device=0)                                  # "device" memory, float32, clipped at the top, under the logo's left part
# (the stand-in's encoder looks at the first rows of a picture only: overlays that are to move a STREAM lie there; what the slots hold everywhere is compared through
# ks265_stub_overlay_dump, byte for byte)


def dumped(lib, path, fn):
    """(fn's result, the input slots the stand-in's overlay calls left behind meanwhile, one row per call)"""
    if os.path.exists(path):
        os.remove(path)
    lib.ks265_stub_overlay_dump(str(path).encode())
    try:
        out = fn()
    finally:
        lib.ks265_stub_overlay_dump(None)
    return out, np.fromfile(path, np.uint8)


def overlaid_session(lib, w, h, pictures, sets, lanes=1, latency=b"default", params=(), ways="csa", force=lambda t: 0):
    """session() of host_harness with overlays: sets = {t: [(slot, Ov or None), ...]} applied right in front of picture t; every host overlay is handed over as a copy that is
    written over as soon as the set call has returned, every device overlay as a copy that stays until the close"""
    hd = open_handle(lib, w, h, lanes=lanes, latency=latency, params=params)
    if set(ways) & set("dn"):
        assert lib.ks265_enc_enable_device_input(hd) == QY_OK
    keep = []

    def submit(t, p):
        way = ways[t % len(ways)]

        def go(nal, nn, outp):
            for slot, ov in sets.get(t, ()):
                mine = ov.at(ov.arr.copy()) if ov is not None else None
                assert set_overlay(lib, hd, slot, mine) == QY_OK, (t, slot)
                if mine is not None and mine.device < 0:
                    mine.arr[...] = 0x5A if mine.fmt is None else 0.25
                elif mine is not None:
                    keep.append(mine)
            if way in "dn":
                return i420_picture(lib, hd, p, w, h, t, nv12=way == "n", extra=5)(nal, nn, outp)
            if not force(t):
                return host_picture(lib, hd, p, w, h, t, way)(nal, nn, outp)
            pic, yuv = Picture(), packed_yuv(p, w, h)
            pic.yuv, pic.pts = C.pointer(yuv), t
            return lib.QY265EncoderEncodeFrame(hd, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), force(t))
        return go
    return drive(lib, hd, [submit(t, p) for t, p in enumerate(pictures)])


def blended(pictures, w, h, slots_at, ww=None, wh=None):
    """slots_at(t) -> the eight slots in force for picture t (Ov or None)"""
    return [ovr.blend(p, w, h, [o.ref() if o is not None else None for o in slots_at(t)], ww, wh) for t, p in enumerate(pictures)]


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_overlaid_stream_is_the_plain_stream_of_blended_pictures(lib, cfg, tmp_path):
    """fails on the parent commit: no ks265_enc_set_overlay there"""
    latency = CONFIGS[cfg]
    src = source()
    want = blended(src, W, H, lambda t: [LOGO, None, None, CAPTION])
    assert all((a != b).sum() > 1000 for a, b in zip(want, src))
    lib.ks265_stub_overlay_reset()
    exp = session(lib, W, H, want, ways="c", latency=latency)
    assert ov_calls(lib) == [], "a plain handle blends nothing"
    assert session(lib, W, H, src, ways="c", latency=latency) != exp
    bottom = Ov(rgba8(14, 64, 32), x=-20, y=H - 20, opacity=100)         # (seen by the slots alone)
    got, slots = dumped(lib, tmp_path / "slots.yuv", lambda: overlaid_session(lib, W, H, src, {0: [(0, LOGO), (3, CAPTION), (6, bottom)]}, latency=latency))
    assert (slots.reshape(N, -1) == np.array(blended(src, W, H, lambda t: [LOGO, None, None, CAPTION, None, None, bottom]))).all(), "the input slots are the reference's, byte for byte"
    lib.ks265_stub_overlay_reset()
    got = overlaid_session(lib, W, H, src, {0: [(0, LOGO), (3, CAPTION)]}, latency=latency)
    g, e = nals(got), nals(exp)
    assert len(g) == len(e) > N and all(a == b for a, b in zip(g, e)), cfg
    one = (W, H, W, H, [(48, 24, W - 40, -4, 192, IN_RGB), (96, 16, 100, -8, 256, yf.IN_RGB_F32)])
    assert ov_calls(lib) == [one] * N, "one call per picture, the overlays in slot order"
    # "device" pictures take the same way; the order of the SLOTS decides, not that of the calls
    assert overlaid_session(lib, W, H, src, {0: [(3, CAPTION), (0, LOGO)]}, latency=latency, ways="dn") == exp
    assert overlaid_session(lib, W, H, src, {0: [(3, LOGO), (0, CAPTION)]}, latency=latency) != exp


def test_two_lanes_give_the_one_lane_bytes(lib):
    n, iper = 40, 32
    src = source(n=n, seed=303)
    params = (("iper", iper),)
    sets = {0: [(0, LOGO)], 5: [(3, CAPTION)], 34: [(0, None)], 36: [(0, LOGO.at(LOGO.arr[:, ::-1].copy()))]}       # (also across the GOP boundary at 32: the set travels with the picture)
    lib.ks265_stub_overlay_reset()
    two = overlaid_session(lib, W, H, src, sets, lanes=2, params=params)
    assert len(ov_calls(lib)) == n
    one = overlaid_session(lib, W, H, src, sets, lanes=1, params=params)
    assert two == one
    at = lambda t: [LOGO if t < 34 else LOGO.at(LOGO.arr[:, ::-1]) if t >= 36 else None, None, None, CAPTION if t >= 5 else None]
    assert one == session(lib, W, H, blended(src, W, H, at), ways="c", lanes=1, params=params)


def test_behind_the_filters(lib):
    rng = np.random.default_rng(305)
    src = [np.clip(p.astype(np.int32) + np.rint(rng.normal(0, 3, p.shape)).astype(np.int32), 0, 255).astype(np.uint8) for p in source()]
    flt = er.enhance_clip(dr.filter_clip(src, W, H, *dr.level_params(2)), W, H, er.level_params(2, 0))
    want = blended(flt, W, H, lambda t: [LOGO, None, None, CAPTION])
    got, log = logged(lib, lambda: overlaid_session(lib, W, H, src, {0: [(0, LOGO), (3, CAPTION)]}, params=(("denoise", 2), ("edge", 2))))
    assert got == session(lib, W, H, want, ways="c")
    # the last step in front of the encoder, inside the bracket of the device overlay's stream, its event behind it; the denoiser's history never contains the overlay (blending in front of the filters is another stream)
    rows = [ln.split(" ") for ln in log]
    at = [i for i, f in enumerate(rows) if f[1] == "ks265_input_enhance"]
    assert len(at) == N
    for i in at:
        mine = [f for f in rows[i:] if f[0] == rows[i][0]][:6]
        want_calls = ["ks265_input_enhance", "ks265_event_record", "ks265_wait_external", "ks265_input_overlay", "ks265_event_record", "ks265_external_wait_event"]
        assert [f[1] for f in mine] == want_calls and {f[2] for f in mine} == {rows[i][2]} and len({f[4] for f in mine if f[4] != "-"}) == 1, mine
    pre = er.enhance_clip(dr.filter_clip(blended(src, W, H, lambda t: [LOGO, None, None, CAPTION]), W, H, *dr.level_params(2)), W, H, er.level_params(2, 0))
    assert got != session(lib, W, H, pre, ways="c")


def test_ragged_size_is_clipped_to_the_window(lib, tmp_path):
    w, h = 202, 134
    src = source(w, h)
    big, top = Ov(rgba8(13, 64, 32), x=w - 30, y=h - 20, opacity=230), Ov(rgba8(14, 64, 32), x=w - 30, y=-10)
    want = blended([pw.pad_i420(p, w, h) for p in src], W, H, lambda t: [big, top], w, h)
    assert all((a.reshape(-1)[:W * H].reshape(H, W)[:, w:] == pw.pad_i420(p, w, h)[:W * H].reshape(H, W)[:, w:]).all() for a, p in zip(want, src)), "the padding keeps its bytes"
    lib.ks265_stub_overlay_reset()
    got, slots = dumped(lib, tmp_path / "slots.yuv", lambda: overlaid_session(lib, w, h, src, {0: [(0, big), (1, top)]}, ways="csadn"))
    assert (slots.reshape(N, -1) == np.array(want)).all()
    assert ov_calls(lib) == [(W, H, w, h, [(64, 32, w - 30, h - 20, 230, IN_RGB), (64, 32, w - 30, -10, 256, IN_RGB)])] * N
    g, e = nals(got), nals(session(lib, W, H, want, ways="c"))
    assert len(g) == len(e) > N and all((a == b) == (t != ws.NAL_SPS) for (t, a), (_, b) in zip(g, e))


def test_no_overlay_is_the_parent_s_call_log(lib, without):
    """nothing set - and a slot set and cleared again before the first picture: the same calls, line for line, as on a device library that does not have the entries (zero
    latency: the call log of a GOP of B pictures depends on thread timing)"""
    for w, h, ways, params in ((W, H, "csadn", ()), (202, 134, "csa", ()), (W, H, "csa", (("denoise", 1), ("edge", 2)))):
        src = source(w, h, 5)
        lib.ks265_stub_overlay_reset()
        a, la = logged(lib, lambda: session(lib, w, h, src, ways=ways, latency=b"zerolatency", params=params))
        b, lb = logged(without, lambda: session(without, w, h, src, ways=ways, latency=b"zerolatency", params=params))
        assert a == b and len(a) > 500
        assert len(la) > 50 and not any("overlay" in ln for ln in la)
        assert same_calls(la) == same_calls(lb)
        assert ov_calls(lib) == []


def test_set_replace_and_clear_take_effect_at_the_next_picture(lib):
    src = source()
    moved = LOGO.at(LOGO.arr)
    moved.x, moved.y, moved.opacity = 20, 0, 256
    sets = {2: [(0, LOGO)], 4: [(0, moved), (7, CAPTION)], 6: [(0, None)], 7: [(7, None), (2, None)]}
    at = lambda t: [LOGO if t in (2, 3) else moved if t in (4, 5) else None] + [None] * 6 + [CAPTION if t in (4, 5, 6) else None]
    want = blended(src, W, H, at)
    lib.ks265_stub_overlay_reset()
    assert overlaid_session(lib, W, H, src, sets, latency=b"zerolatency") == session(lib, W, H, want, ways="c", latency=b"zerolatency")
    assert [len(c[4]) for c in ov_calls(lib)] == [1, 1, 2, 2, 1], "pictures 0, 1, 7 and 8 make no call"
    # the default GOP, the first overlay before the first picture (the twins are made while nothing is in flight)
    sets[0] = [(5, LOGO)]
    sets[1] = [(5, None)]
    at0 = lambda t: at(t)[:5] + [LOGO if t == 0 else None] + at(t)[6:]
    assert overlaid_session(lib, W, H, src, sets) == session(lib, W, H, blended(src, W, H, at0), ways="c")


def test_forced_only_follows_bforcelogo(lib):
    src = source()
    forced = LOGO.at(LOGO.arr)
    forced.flags = FORCED_ONLY
    force = lambda t: int(t in (1, 2, 6))
    sets = {0: [(0, forced), (1, CAPTION)]}
    want = blended(src, W, H, lambda t: [LOGO if force(t) else None, CAPTION])
    for latency in CONFIGS.values():
        assert overlaid_session(lib, W, H, src, sets, latency=latency, ways="c", force=force) == session(lib, W, H, want, ways="c", latency=latency)
    # never for device pictures; and with no such overlay set bForceLogo is without effect
    plain = blended(src, W, H, lambda t: [None, CAPTION])
    assert overlaid_session(lib, W, H, src, sets, latency=b"zerolatency", ways="d") == session(lib, W, H, plain, ways="c", latency=b"zerolatency")
    assert overlaid_session(lib, W, H, src, {}, latency=b"zerolatency", ways="c", force=lambda t: 1) == session(lib, W, H, src, ways="c", latency=b"zerolatency")


def test_refusals_leave_the_slot_as_it_was(lib, without, capfd):
    src = source()[:4]
    hd = open_handle(lib, W, H, lanes=1, latency=b"zerolatency")
    good = LOGO.at(LOGO.arr.copy())
    assert set_overlay(lib, hd, 2, good) == QY_OK

    def alt(**kw):
        o = good.c()
        for k, v in kw.items():
            if k in ("format", "device", "pixel_step", "matrix"):
                setattr(o.rgb, k, v)
            elif k == "pitch":
                o.rgb.pitch[0] = v
            elif k == "plane1":
                o.rgb.plane[1] = v
            else:
                setattr(o, k, v)
        return o
    refused = [(alt(x=7), QY_NOTSUPPORTED), (alt(y=-1), QY_NOTSUPPORTED), (alt(width=47), QY_NOTSUPPORTED), (alt(height=0), QY_NOTSUPPORTED), (alt(width=8194), QY_NOTSUPPORTED),
               (alt(x=16386), QY_NOTSUPPORTED), (alt(opacity=257), QY_NOTSUPPORTED), (alt(opacity=-1), QY_NOTSUPPORTED), (alt(flags=2), QY_NOTSUPPORTED), (alt(format=0), QY_NOTSUPPORTED),
               (alt(format=yf.IN_RGB_F32), QY_NOTSUPPORTED), (alt(pixel_step=0), QY_NOTSUPPORTED), (alt(pixel_step=65), QY_NOTSUPPORTED), (alt(matrix=2), QY_NOTSUPPORTED),
               (alt(device=1), QY_NOTSUPPORTED), (alt(device=-2), QY_NOTSUPPORTED), (alt(pitch=4 * 48 - 4), QY_POINTER), (alt(plane1=None), QY_POINTER)]
    for slot in (2, 4):
        for o, want in refused:
            assert lib.ks265_enc_set_overlay(hd, slot, C.byref(o)) == want, (slot, hex(want & 0xFFFFFFFF))
    for slot in (-1, 8):
        assert lib.ks265_enc_set_overlay(hd, slot, C.byref(good.c())) == QY_NOTSUPPORTED and lib.ks265_enc_set_overlay(hd, slot, None) == QY_NOTSUPPORTED
    assert lib.ks265_enc_set_overlay(None, 0, None) == QY_POINTER
    lib.ks265_stub_overlay_reset()
    got = drive(lib, hd, [host_picture(lib, hd, p, W, H, t) for t, p in enumerate(src)])
    assert ov_calls(lib) == [(W, H, W, H, [(48, 24, W - 40, -4, 192, IN_RGB)])] * 4, "slot 2 kept what it had, slot 4 stayed empty"
    assert got == session(lib, W, H, blended(src, W, H, lambda t: [None, None, LOGO]), ways="c", latency=b"zerolatency")
    # a device library without the entries: QY_NOTSUPPORTED, one log line, the handle goes on
    capfd.readouterr()
    hd = open_handle(without, W, H, lanes=1, latency=b"zerolatency", params=(("log", 0),))
    assert set_overlay(without, hd, 0, good) == QY_NOTSUPPORTED and set_overlay(without, hd, 1, good) == QY_NOTSUPPORTED and without.ks265_enc_set_overlay(hd, 0, None) == QY_NOTSUPPORTED
    assert drive(without, hd, [host_picture(without, hd, p, W, H, t) for t, p in enumerate(src)]) == session(lib, W, H, src, ways="c", latency=b"zerolatency")
    assert capfd.readouterr().out.count("ks265enc: overlays are unavailable: ") == 1
    # a handle without twins (no lookahead, no filter, no device input), the default GOP, four pictures handed in and held for their mini-GOP: the first overlay is refused
    # with one line, and nothing of it is drawn; after the flush it is taken, the twins are made then, and the pictures behind it carry it
    def two_halves(with_overlay, second):
        hd = open_handle(lib, W, H, lanes=1, params=(("log", 0),), env={"KS265_NO_AUTO_LOOKAHEAD": 1})
        nal, nn, outp, bs = C.POINTER(Nal)(), C.c_int(0), Picture(), bytearray()

        def flush():
            while lib.QY265EncoderDelayedFrames(hd) > 0:
                assert lib.QY265EncoderEncodeFrame(hd, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == QY_OK
                bs.extend(nal_bytes(nal, nn))
        for t, p in enumerate(src):
            assert host_picture(lib, hd, p, W, H, t)(nal, nn, outp) == QY_OK
            bs.extend(nal_bytes(nal, nn))
        if with_overlay:
            capfd.readouterr()
            assert set_overlay(lib, hd, 0, good) == QY_NOTSUPPORTED
            assert capfd.readouterr().out.count("pictures are in flight") == 1
        flush()
        if with_overlay:
            assert set_overlay(lib, hd, 0, good) == QY_OK
        for t, p in enumerate(second):
            assert host_picture(lib, hd, p, W, H, 4 + t)(nal, nn, outp) == QY_OK
            bs.extend(nal_bytes(nal, nn))
        flush()
        lib.QY265EncoderClose(hd)
        assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5, "the host overlay's copy and the twins go with the close"
        return bytes(bs)
    more = source()[4:8]
    lib.ks265_stub_overlay_reset()
    got = two_halves(True, more)
    assert len(ov_calls(lib)) == 4, "the four pictures behind the accepted set, none before"
    assert got == two_halves(False, blended(more, W, H, lambda t: [LOGO])) and got != two_halves(False, more)


def test_lanes_on_several_gpus_and_the_graph_experiment_refuse(lib, capfd):
    """GOP lanes on several GPUs: every set call is QY_NOTSUPPORTED, nothing is drawn, the stream is the plain one of the same handle.  The KS265_GRAPH experiment likewise"""
    n = 70
    src = source(n=n, seed=309)
    params = (("iper", 32), ("bframes", 0))
    for env in ({"KS265_GPUS": 2}, {"KS265_GRAPH": 1}):
        lanes = 2 if "KS265_GPUS" in env else 1

        def run(with_sets):
            hd = open_handle(lib, W, H, lanes=lanes, params=params, env=env)
            assert lib.ks265_enc_lanes(hd) == (4 if "KS265_GPUS" in env else 1), "KS265_GOP_LANES lanes per GPU"

            def put(t, p):
                def go(nal, nn, outp):
                    if with_sets and t in (0, 3, 40):
                        assert set_overlay(lib, hd, 0, LOGO.at(LOGO.arr.copy())) == QY_NOTSUPPORTED and set_overlay(lib, hd, 5, CAPTION.at(CAPTION.arr.copy())) == QY_NOTSUPPORTED
                        assert lib.ks265_enc_set_overlay(hd, 0, None) == QY_OK, "clearing an empty slot is nothing"
                    return host_picture(lib, hd, p, W, H, t)(nal, nn, outp)
                return go
            return drive(lib, hd, [put(t, p) for t, p in enumerate(src)])
        lib.ks265_stub_overlay_reset()
        got = run(True)
        assert ov_calls(lib) == [] and len(got) > 1000 and got == run(False), env


def test_cli_logo(lib, tmp_path):
    exe = build_host_cli("hip_stub_overlay.c")
    src = source()
    logo = rgba8(15, 48, 24)
    (tmp_path / "in.yuv").write_bytes(np.concatenate(src).tobytes())
    (tmp_path / "logo.rgba").write_bytes(logo.tobytes())
    (tmp_path / "want.yuv").write_bytes(np.concatenate(blended(src, W, H, lambda t: [Ov(logo, x=W - 40, y=0, opacity=200)])).tobytes())
    env = {k: v for k, v in os.environ.items() if not k.startswith("KS265_")}

    def run(yuv, out, *opts, ok=True):
        r = subprocess.run([exe, "-i", str(tmp_path / yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-rc", "0", "-qp", "30", "-threads", "3", "-b", str(tmp_path / out), *opts],
                           capture_output=True, text=True, timeout=120, env=env)
        assert (r.returncode == 0 and "H265 encoder passed!!!" in r.stdout) == ok, r.stdout[-800:] + r.stderr[-800:]
        return (tmp_path / out).read_bytes() if ok else r.stderr
    got = run("in.yuv", "a.265", "-logo", "%s:48:24:%d:0:200" % (tmp_path / "logo.rgba", W - 40))
    assert len(got) > 1000 and got == run("want.yuv", "b.265") and got != run("in.yuv", "c.265")
    assert run("in.yuv", "d.265", "-logo", "%s:48:24:0:0" % (tmp_path / "logo.rgba")) == run("in.yuv", "e.265", "-logo", "%s:48:24:0:0:256" % (tmp_path / "logo.rgba"))
    assert "bad value for -logo" in run("in.yuv", "f.265", "-logo", "logo.rgba:48", ok=False)
    assert "cannot read" in run("in.yuv", "f.265", "-logo", "%s:48:26:0:0" % (tmp_path / "logo.rgba"), ok=False)
    assert "refused" in run("in.yuv", "f.265", "-logo", "%s:48:24:1:0" % (tmp_path / "logo.rgba"), ok=False)


# ------------------------------------------------------------------ under the sanitizers

@pytest.fixture(scope="module")
def sanitized():
    """tests/overlay_main.c + the host + the stand-in, built once with -fsanitize=address,undefined"""
    return build_host_program("overlay_main.c", stub="hip_stub_overlay.c")


@pytest.mark.parametrize("latency", ["zerolatency", "default"])
def test_host_and_stand_in_under_the_sanitizers(lib, sanitized, tmp_path, latency):
    """the script in the header of tests/overlay_main.c, mirrored with overlay_ref: the input slots the stand-in dumped are the reference's, the stream is the plain one's"""
    n, lw, lh = 7, 48, 24
    src = source(n=n, seed=307)
    logo = rgba8(17, lw, lh)
    (tmp_path / "clip.yuv").write_bytes(np.concatenate(src).tobytes())
    (tmp_path / "logo.rgba").write_bytes(logo.tobytes())
    r = subprocess.run([sanitized, str(W), str(H), str(n), str(tmp_path / "clip.yuv"), str(tmp_path / "out.265"), str(tmp_path / "slots.yuv"), latency, str(tmp_path / "logo.rgba"),
                        str(lw), str(lh)], capture_output=True, text=True, timeout=300, env={**os.environ, "KS265_GOP_LANES": "1", "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    first, second, third = Ov(logo, x=8, y=4), Ov(logo, alpha=False, x=-4, y=-2, opacity=200), Ov(logo, x=40, y=20)
    forced = Ov(logo, (2, 1, 0), x=W - lw + 6, y=H - lh + 2, opacity=128, matrix=1, full=1)
    at = lambda t: [first if t < 2 else second if t < 4 else None, third if t >= 4 else None, None, None, None, forced if t & 1 else None]
    want = blended(src, W, H, at)
    slots = np.frombuffer((tmp_path / "slots.yuv").read_bytes(), np.uint8).reshape(n, -1)
    for t in range(n):
        assert (slots[t] == want[t]).all(), t
    assert (tmp_path / "out.265").read_bytes() == session(lib, W, H, want, ways="c", latency=latency.encode())
