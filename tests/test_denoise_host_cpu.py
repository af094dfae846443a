"""CPU: `vpp_denoise` / `vpp_recur_filter` through the real encoder host, against the stand-in of the device library WITH the two entries (tests/hip_stub_denoise.c):
  * the stand-in's filter equals tests/denoise_ref.py byte for byte - picture, history out and block words - on the shapes and contents of tests/test_gpu_denoise.py;
  * at 208x136, 17 pictures, with the default GOP, -bframes 0 and zero latency: every NAL unit of a `denoise=2` handle equals that of a plain handle fed the reference-filtered
    pictures, for every way in - contiguous and strided host planes, an acquired slot, "device" I420 and NV12, and the scaled entry;
  * the stand-in saw one call per picture, in display order, with the level's (thr, weight) at the coded size; the two history buffers are used ping-pong and only the first
    picture has none.  With two GOP lanes (-iper 32, 40 pictures: the host deals GOPs to lanes from a key period of 32 on) every chunk's first picture has none, and the
    stream is the two-lane plain handle's fed the per-chunk reference; at -iper 8 a handle asked for two lanes runs one and never restarts;
  * at 202x134 the filter sees 208x136, behind the pad;
  * against the plain stand-in (tests/hip_stub.c) a handle with either field set is refused with QY_NOTSUPPORTED; `recur=30` alone works (thr 10, weight 30); `denoise=4` and
    `recur=31` are QY265_PARAM_BAD_VALUE; values outside the ranges written into the structure are refused at open;
  * a handle with both fields 0 makes no denoise call;
  * tests/input_filter_main.c, the host and the stand-in under -fsanitize=address,undefined as a program of its own: 5 pictures at 202x134 with denoise=3, both latencies."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import picture_window_ref as pw
import window_sps as ws
import yuv_scale_ref as ys
from host_harness import (LAY, QY_NOTSUPPORTED, QY_OK, build_host_lib, build_host_program, clip, drive, filter_program, host_picture, i420_picture, load_host_lib, nals,
                          open_handle, preceded, session, try_open)

W, H, N = 208, 136, 17
BAD_VALUE = -2
T2 = dr.level_params(2)


class DnCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("w", "h", "thr", "weight", "has_hist", "hist_in", "hist_out")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_host_lib(build_host_lib("hip_stub_denoise.c"), call_log=str(tmp_path_factory.mktemp("stubdn") / "calls.log"))


@pytest.fixture(scope="module")
def plain():
    return load_host_lib(build_host_lib("hip_stub.c"))


def dn_calls(lib):
    buf = (DnCall * 4096)()
    n = lib.ks265_stub_denoise_calls(buf, 4096)
    return [(c.w, c.h, c.thr, c.weight, c.has_hist, c.hist_in, c.hist_out) for c in buf[:n]]


def noisy_clip(w, h, n, seed):
    """the harness's moving clip with noise in all three planes"""
    rng = np.random.default_rng(seed)
    return [np.clip(p.astype(np.int32) + np.rint(rng.normal(0, 3, p.shape)).astype(np.int32), 0, 255).astype(np.uint8) for p in clip(w, h, n, seed)]


# ------------------------------------------------------------------ the stand-in's filter

def stub_filter(lib, w, h, thr, wmax, cur, hist):
    n, nb = w * h * 3 // 2, ((w + 15) // 16) * ((h + 15) // 16)
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    pic, out, blocks = np.array(cur, np.uint8), np.full(n, 0x3C, np.uint8), np.full(2 * nb, -7, np.int32)
    hin = None if hist is None else np.array(hist, np.uint8)
    cfg = (C.c_int32 * 2)(thr, wmax)
    rc = lib.ks265_input_denoise(ctx, cfg, w, h, C.c_void_p(pic.ctypes.data), C.c_void_p(hin.ctypes.data if hin is not None else None), C.c_void_p(out.ctypes.data), C.c_void_p(blocks.ctypes.data))
    lib.ks265_destroy(ctx)
    assert rc == 0 and (hin is None or (hin == hist).all())
    return pic, out, blocks.reshape(nb, 2)


def test_stand_in_equals_the_reference(lib):
    from denoise_cases import PARAMS, SIZES, contents as _contents
    for w, h in SIZES:
        for name, (cur, hist) in _contents(w, h, seed=w + h).items():
            for thr, wmax in PARAMS:
                exp, eb = dr.filter_picture(cur, hist, w, h, thr, wmax)
                got, gh, gb = stub_filter(lib, w, h, thr, wmax, cur, hist)
                assert (gb == eb).all() and (got == exp).all() and (gh == exp).all(), (w, h, name, thr, wmax)
        got, gh, gb = stub_filter(lib, w, h, 10, 20, cur, None)
        assert (got == cur).all() and (gh == cur).all() and (gb == dr.filter_picture(cur, None, w, h, 10, 20)[1]).all()
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    for w, h, thr, wmax in ((20, 16, 10, 20), (16, 0, 10, 20), (16, 16, 0, 20), (16, 16, 65, 20), (16, 16, 10, 0), (16, 16, 10, 31)):
        assert lib.ks265_input_denoise_validate(ctx, (C.c_int32 * 2)(thr, wmax), w, h) == -4
    a = np.zeros(3 * 384 + 8, np.uint8)
    p = lambda off: C.c_void_p(a.ctypes.data + off)
    cfg = (C.c_int32 * 2)(10, 20)
    assert lib.ks265_input_denoise(ctx, cfg, 16, 16, p(0), p(384), p(384), None) == -3
    assert lib.ks265_input_denoise(ctx, cfg, 16, 16, p(0), p(384), p(392), None) == -3
    assert lib.ks265_input_denoise(ctx, cfg, 16, 16, p(0), p(0), p(768), None) == -3
    assert lib.ks265_input_denoise(ctx, cfg, 16, 16, p(0), None, None, None) == -3
    lib.ks265_destroy(ctx)


# ------------------------------------------------------------------ streams

CONFIGS = {"gop8": (b"default", ()), "ippp": (b"default", (("bframes", 0),)), "zerolatency": (b"zerolatency", ())}
_ref = {}


def reference(cfg):
    """(source clip, the plain handle's stream fed the reference-filtered clip)"""
    if cfg not in _ref:
        src = noisy_clip(W, H, N, 171)
        _ref[cfg] = (src, dr.filter_clip(src, W, H, *T2))
    return _ref[cfg]


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_way_in_gives_the_plain_handle_s_stream_of_filtered_pictures(lib, cfg):
    latency, params = CONFIGS[cfg]
    src, filt = reference(cfg)
    assert sum(int((a != b).sum()) for a, b in zip(src[1:], filt[1:])) > 10000, "level 2 does not filter this clip"
    lib.ks265_stub_denoise_reset()
    exp = session(lib, W, H, filt, ways="c", latency=latency, params=params)
    assert dn_calls(lib) == [], "a plain handle filters nothing"
    plain_src = session(lib, W, H, src, ways="c", latency=latency, params=params)
    assert plain_src != exp
    e = nals(exp)
    for ways in ("csa", "dn"):
        lib.ks265_stub_denoise_reset()
        got = session(lib, W, H, src, ways=ways, latency=latency, params=params + (("denoise", 2),))
        g = nals(got)
        assert len(g) == len(e) > N and all(a == b for a, b in zip(g, e)), (cfg, ways)
        calls = dn_calls(lib)
        assert len(calls) == N and all(c[:4] == (W, H, *T2) for c in calls)
        assert [c[4] for c in calls] == [0] + [1] * (N - 1), "only the first picture has no history"
        assert [c[6] for c in calls] == [t & 1 for t in range(N)] and [c[5] for c in calls] == [-1] + [(t - 1) & 1 for t in range(1, N)], "two buffers, ping-pong"


def scaled_session(lib, pictures, sw, sh, params=()):
    """a W x H handle fed sources of sw x sh through the scaled entry (filter 1); its stream"""
    hd = open_handle(lib, W, H, lanes=1, params=params)
    assert lib.ks265_enc_enable_device_input(hd) == QY_OK and lib.ks265_enc_enable_device_scale(hd, sw, sh) == QY_OK
    return drive(lib, hd, (i420_picture(lib, hd, a, sw, sh, t, scaled=(sw, sh, 1)) for t, a in enumerate(pictures)))


def test_scaled_way_in(lib):
    sw, sh, n = 312, 200, 9
    src = noisy_clip(sw, sh, n, 173)
    filt = dr.filter_clip([ys.scale_i420(p, sw, sh, W, H, 1) for p in src], W, H, *T2)
    lib.ks265_stub_denoise_reset()
    got = scaled_session(lib, src, sw, sh, params=(("denoise", 2),))
    calls = dn_calls(lib)
    assert [c[:5] for c in calls] == [(W, H, *T2, int(t > 0)) for t in range(n)]
    assert got == session(lib, W, H, filt, ways="c")


def test_two_lanes_restart_with_every_chunk(lib):
    """GOPs are dealt to lanes from a key period of 32 on (top_lanes_wanted): 40 pictures at -iper 32 are two chunks, on two lanes.  At -iper 8 a handle asked for two lanes
    runs one, and never restarts"""
    n, iper = 40, 32
    src = noisy_clip(W, H, n, 175)
    filt = dr.filter_clip(src, W, H, *T2, reset_at=(0, iper))
    assert not (filt[iper] != src[iper]).any() and (filt[iper + 1] != src[iper + 1]).any()
    lib.ks265_stub_denoise_reset()
    got = session(lib, W, H, src, ways="csa", lanes=2, params=(("iper", iper), ("denoise", 2)))
    calls = dn_calls(lib)
    assert [c[4] for c in calls] == [int(t % iper != 0) for t in range(n)], "every chunk's first picture has no history"
    assert len({c[6] for c in calls}) == 4 and all(c[5] != c[6] for c in calls), "two history buffers per lane"
    for t in range(1, n):
        if t % iper:
            assert calls[t][5] == calls[t - 1][6], t
    assert got == session(lib, W, H, filt, ways="c", lanes=2, params=(("iper", iper),))
    one = session(lib, W, H, src, ways="c", lanes=1, params=(("iper", iper), ("denoise", 2)))
    assert one != got, "one lane never restarts: the known difference between lane counts"
    unbroken = dr.filter_clip(src, W, H, *T2)
    assert one == session(lib, W, H, unbroken, ways="c", lanes=1, params=(("iper", iper),))
    lib.ks265_stub_denoise_reset()
    short = session(lib, W, H, src[:N], ways="csa", lanes=2, params=(("iper", 8), ("denoise", 2)))
    assert [c[4] for c in dn_calls(lib)] == [0] + [1] * (N - 1) and len({c[6] for c in dn_calls(lib)}) == 2
    assert short == session(lib, W, H, unbroken[:N], ways="c", lanes=2, params=(("iper", 8),))


def test_ragged_size_is_filtered_behind_the_pad(lib):
    w, h = 202, 134
    src = noisy_clip(w, h, 9, 177)
    filt = dr.filter_clip([pw.pad_i420(p, w, h) for p in src], W, H, *dr.level_params(3))
    lib.ks265_stub_denoise_reset()
    got = session(lib, w, h, src, ways="csadn", params=(("denoise", 3),))
    assert [c[:5] for c in dn_calls(lib)] == [(W, H, 16, 24, int(t > 0)) for t in range(9)]
    exp = session(lib, W, H, filt, ways="c")
    g, e = nals(got), nals(exp)
    assert len(g) == len(e) > 9 and all((a == b) == (t != ws.NAL_SPS) for (t, a), (_, b) in zip(g, e))
    assert ws.output_size(ws.stream_sps(got)) == (w, h)


def test_open_and_configuration(lib, plain):
    for params in ((("denoise", 1),), (("recur", 12),), (("denoise", 3), ("recur", 2.5))):
        hd, err = try_open(plain, W, H, lanes=1, params=params)
        assert not hd.value and err == QY_NOTSUPPORTED, params
    hd, err = try_open(plain, W, H, lanes=1)
    assert hd.value
    plain.QY265EncoderClose(hd)
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
    assert C.c_int.from_buffer(cfg, LAY["vpp_denoise"]).value == 0 and C.c_double.from_buffer(cfg, LAY["vpp_recur_filter"]).value == 0.0, "off by default"
    for k, v in (("denoise", "4"), ("denoise", "-1"), ("denoise", "x"), ("recur", "31"), ("recur", "30.5"), ("recur", "-1"), ("recur", "nan")):
        assert lib.QY265ConfigParse(cfg, k.encode(), v.encode()) == BAD_VALUE, (k, v)
    assert lib.QY265ConfigParse(cfg, b"denoise", b"3") == 0 and C.c_int.from_buffer(cfg, LAY["vpp_denoise"]).value == 3
    assert lib.QY265ConfigParse(cfg, b"recur", b"7.5") == 0 and C.c_double.from_buffer(cfg, LAY["vpp_recur_filter"]).value == 7.5
    # recur alone: thr 10, the weight as given; on top of a level: the level's thr
    src = noisy_clip(W, H, 3, 179)
    for params, want in (((("recur", 30),), (10, 30)), ((("recur", 0.2),), (10, 1)), ((("denoise", 1), ("recur", 7.5)), (6, 8)), ((("denoise", 1),), (6, 16)), ((("denoise", 3),), (16, 24))):
        lib.ks265_stub_denoise_reset()
        got = session(lib, W, H, src, ways="c", latency=b"zerolatency", params=params)
        assert [c[2:4] for c in dn_calls(lib)] == [want] * 3, params
        assert dr.level_params(*[dict(params).get(k, 0) for k in ("denoise", "recur")]) == want
        assert got == session(lib, W, H, dr.filter_clip(src, W, H, *want), ways="c", latency=b"zerolatency")
    # values outside the ranges written into the structure
    for off, ty, v in ((LAY["vpp_denoise"], C.c_int, 4), (LAY["vpp_denoise"], C.c_int, -1), (LAY["vpp_recur_filter"], C.c_double, 30.5), (LAY["vpp_recur_filter"], C.c_double, -2.0)):
        cfg = (C.c_uint8 * LAY["sizeof_config"])()
        assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
        for k, x in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34)):
            assert lib.QY265ConfigParse(cfg, k.encode(), str(x).encode()) == 0
        ty.from_buffer(cfg, off).value = v
        err = C.c_int(0)
        assert not lib.QY265EncoderOpen(cfg, C.byref(err)) and err.value == QY_NOTSUPPORTED, (off, v)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


def test_reconfig_leaves_the_filter_as_opened(lib):
    src = noisy_clip(W, H, 4, 181)
    hd = open_handle(lib, W, H, lanes=1, latency=b"zerolatency", params=(("denoise", 2),))
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"zerolatency") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34), ("denoise", 0)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    lib.QY265EncoderReconfig.restype = None
    lib.ks265_stub_denoise_reset()
    puts = [host_picture(lib, hd, p, W, H, t) for t, p in enumerate(src)]
    puts[2] = preceded(lambda: lib.QY265EncoderReconfig(hd, cfg), puts[2])
    drive(lib, hd, puts)
    assert [c[2:5] for c in dn_calls(lib)] == [(*T2, int(t > 0)) for t in range(4)]


def test_off_makes_no_call(lib):
    lib.ks265_stub_denoise_reset()
    before = sum(1 for _ in open(lib.call_log_path))
    for w, h, ways in ((W, H, "csadn"), (202, 134, "csa")):
        s = session(lib, w, h, clip(w, h, 9, 183), ways=ways)
        assert len(s) > 500
    new = open(lib.call_log_path).read().split("\n")[before:]
    assert new and not any("ks265_input_denoise" in ln for ln in new)
    assert dn_calls(lib) == []
    lib.ks265_stub_denoise_reset()
    session(lib, W, H, clip(W, H, 3, 185), ways="c", params=(("denoise", 1),))
    assert sum("ks265_input_denoise" in ln for ln in open(lib.call_log_path).read().split("\n")[before:]) == 3 == len(dn_calls(lib))


@pytest.fixture(scope="module")
def sanitized():
    """tests/input_filter_main.c + the host + the stand-in, built once with -fsanitize=address,undefined"""
    return build_host_program("input_filter_main.c", stub="hip_stub_denoise.c")


@pytest.mark.parametrize("latency", ["default", "zerolatency"])
def test_host_and_stand_in_under_the_sanitizers(sanitized, tmp_path, latency):
    out = str(tmp_path / "out.265")
    recs = filter_program(sanitized, 202, 134, 5, out, latency, "denoise=3")
    assert recs["denoise"] == [dict(w=208, h=136, thr=16, weight=24, has_hist=int(t > 0), hist_in=(t - 1) & 1 if t else -1, hist_out=t & 1) for t in range(5)]
    assert len(recs["pad"]) == 5 and not recs["enhance"] + recs["hdr"]
    sps = ws.stream_sps(open(out, "rb").read())
    assert ws.output_size(sps) == (202, 134) and (sps["width"], sps["height"]) == (208, 136)
