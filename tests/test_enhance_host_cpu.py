"""CPU: `vpp_edge` / `vpp_color` through the real encoder host, against the stand-in of the device library WITH the two entries (tests/hip_stub_enhance.c):
  * the stand-in's filter equals tests/enhance_ref.py byte for byte on the shapes, cfgs and contents of tests/enhance_cases.py (8x8, 72x24, 136x40), and refuses what the
    device library refuses;
  * at 208x136, 9 pictures, default GOP and zero latency: every NAL unit of an `edge=2 color=2` handle equals that of a plain handle fed the reference-enhanced pictures, for
    host pictures (contiguous, strided, an acquired slot) and "device" I420 / NV12 pictures; edge alone and colour alone likewise;
  * at 202x134 the filter sees 208x136, behind the pad;
  * `denoise=2` with `edge=2`: the stream is the plain handle's fed enhance(denoise(clip)) - the history stays unsharpened; the call log shows every enhance call behind a
    denoise call, its luma source the history buffer that call wrote, and not one ks265_memcpy_d2d_async more than the denoiser alone makes.  Edge alone: one copy per picture
    in front of the call; colour alone: none, and no luma source;
  * two GOP lanes (-iper 32 over 40 pictures) give the one-lane bytes: the filter has no state;
  * values outside 0 .. 3 are QY265_PARAM_BAD_VALUE in QY265ConfigParse and QY_NOTSUPPORTED at open when written into the structure; a handle with either field set on a
    stand-in without the entries (tests/hip_stub_denoise.c) is QY_NOTSUPPORTED; QY265EncoderReconfig leaves the filter as opened;
  * with both fields 0 the call log of an encode is line for line that of the same encode on the stand-in WITHOUT the entries (what the parent saw), thread numbers aside;
  * tests/input_filter_main.c, the host and the stand-in under -fsanitize=address,undefined as a program of its own: 5 pictures at 202x134, both latencies, with and without
    the denoiser."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import enhance_ref as er
import picture_window_ref as pw
import window_sps as ws
from enhance_cases import CFGS, SIZES, contents
from host_harness import (LAY, QY_NOTSUPPORTED, build_host_lib, build_host_program, drive, edgy_clip, en_calls, filter_program, host_picture, load_host_lib, logged, nals, open_handle,
                          preceded, same_calls, session, try_open)

W, H, N = 208, 136, 9
BAD_VALUE = -2
OFF_EDGE, OFF_COLOR = LAY["vpp_denoise"] + 4, LAY["vpp_denoise"] + 8     # int vpp_denoise, vpp_edge, vpp_color (include/ks265_enc.h)
E22 = er.level_params(2, 2)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_host_lib(build_host_lib("hip_stub_enhance.c"), call_log=str(tmp_path_factory.mktemp("stuben") / "calls.log"))


@pytest.fixture(scope="module")
def without(tmp_path_factory):
    """the stand-in without the two entries: the device library of the parent"""
    return load_host_lib(build_host_lib("hip_stub_denoise.c"), call_log=str(tmp_path_factory.mktemp("stubnoen") / "calls.log"))


def around_enhance(log):
    """per ks265_input_enhance line: (the line, the two lines in front of it and the one behind it ON ITS THREAD), each as a list of fields"""
    out = []
    for i, ln in enumerate(log):
        f = ln.split(" ")
        if f[1] == "ks265_input_enhance":
            mine = lambda rng: [log[k].split(" ") for k in rng if log[k].split(" ")[0] == f[0]]
            out.append((f, mine(range(i))[-2:], mine(range(i + 1, len(log)))[0]))
    return out


# ------------------------------------------------------------------ the stand-in's filter

def stub_enhance(lib, ctx, w, h, cfg, pic):
    buf = np.array(pic, np.uint8)
    src = buf[:w * h].copy()
    rc = lib.ks265_input_enhance(ctx, (C.c_int32 * 5)(*cfg), w, h, C.c_void_p(src.ctypes.data if cfg[0] else None), C.c_void_p(buf.ctypes.data))
    assert rc == 0 and (src == np.asarray(pic, np.uint8)[:w * h]).all()
    return buf


def test_stand_in_equals_the_reference(lib):
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    for w, h in SIZES:
        for name, pic in contents(w, h, seed=w + h).items():
            for cfg in CFGS:
                got = stub_enhance(lib, ctx, w, h, cfg, pic)
                assert (got == er.enhance_picture(pic, w, h, cfg)).all(), (w, h, name, cfg)
    for w, h, cfg in ((20, 16, E22), (16, 0, E22), (8200, 8, E22), (16, 16, (0, 0, 0, 0, 0)), (16, 16, (65, 0, 8, 0, 0)), (16, 16, (8, 17, 8, 0, 0)), (16, 16, (8, 0, 0, 0, 0)),
                      (16, 16, (8, 0, 65, 0, 0)), (16, 16, (8, 0, 8, 33, 0)), (16, 16, (0, 0, 0, 0, 33)), (16, 16, (-1, 0, 8, 0, 8))):
        assert lib.ks265_input_enhance_validate(ctx, (C.c_int32 * 5)(*cfg), w, h) == -4, (w, h, cfg)
    assert lib.ks265_input_enhance_validate(ctx, (C.c_int32 * 5)(0, 0, 0, 0, 8), 16, 16) == 0, "edge_limit is not judged when edge_gain is 0"
    a = np.zeros(1024, np.uint8)
    p = lambda off: C.c_void_p(a.ctypes.data + off)
    cfg = (C.c_int32 * 5)(*E22)
    assert lib.ks265_input_enhance(ctx, cfg, 16, 16, p(0), p(0)) == -3, "the luma source is the picture"
    assert lib.ks265_input_enhance(ctx, cfg, 16, 16, p(380), p(0)) == -3, "the luma source overlaps the picture's chroma"
    assert lib.ks265_input_enhance(ctx, cfg, 16, 16, None, p(0)) == -3, "no luma source"
    assert lib.ks265_input_enhance(ctx, cfg, 16, 16, p(384), None) == -3
    assert lib.ks265_input_enhance(ctx, (C.c_int32 * 5)(0, 0, 0, 0, 8), 16, 16, None, p(0)) == 0, "colour alone takes no luma source"
    lib.ks265_destroy(ctx)


# ------------------------------------------------------------------ streams

CONFIGS = {"gop8": b"default", "zerolatency": b"zerolatency"}
_src = {}


def source(w=W, h=H, n=N):
    if (w, h, n) not in _src:
        _src[(w, h, n)] = edgy_clip(w, h, n, 191)
    return _src[(w, h, n)]


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_way_in_gives_the_plain_handle_s_stream_of_enhanced_pictures(lib, cfg):
    latency = CONFIGS[cfg]
    src = source()
    enh = er.enhance_clip(src, W, H, E22)
    assert all((a[:W * H] != b[:W * H]).sum() > 500 and (a[W * H:] != b[W * H:]).sum() > 500 for a, b in zip(src, enh)), "level 2 / 2 does not change this clip"
    lib.ks265_stub_enhance_reset()
    exp = session(lib, W, H, enh, ways="c", latency=latency)
    assert en_calls(lib) == [], "a plain handle enhances nothing"
    assert session(lib, W, H, src, ways="c", latency=latency) != exp
    e = nals(exp)
    for ways in ("csa", "dn"):
        lib.ks265_stub_enhance_reset()
        got = session(lib, W, H, src, ways=ways, latency=latency, params=(("edge", 2), ("color", 2)))
        g = nals(got)
        assert len(g) == len(e) > N and all(a == b for a, b in zip(g, e)), (cfg, ways)
        assert en_calls(lib) == [(W, H, E22, 1, 0)] * N


@pytest.mark.parametrize("edge,color", [(1, 0), (3, 0), (0, 1), (0, 3), (3, 1)])
def test_levels_and_halves(lib, edge, color):
    src = source()[:4]
    cfg = er.level_params(edge, color)
    lib.ks265_stub_enhance_reset()
    (got, log) = logged(lib, lambda: session(lib, W, H, src, ways="csa", latency=b"zerolatency", params=(("edge", edge), ("color", color))))
    assert en_calls(lib) == [(W, H, cfg, int(edge > 0), 0)] * 4
    assert got == session(lib, W, H, er.enhance_clip(src, W, H, cfg), ways="c", latency=b"zerolatency")
    calls = around_enhance(log)
    assert len(calls) == 4 and all(f[-1] == str(int(edge > 0)) for f, _, _ in calls)
    for f, front, behind in calls:
        assert (front[-1][1] == "ks265_memcpy_d2d_async" and front[-1][2] == f[2]) == (edge > 0), "the luma copy goes in front of the launch, on its stream - with vpp_edge only"
        assert behind[1] == "ks265_event_record" and behind[2] == f[2], "ev_up is recorded again behind the filter"


def test_ragged_size_is_enhanced_behind_the_pad(lib):
    w, h = 202, 134
    src = source(w, h)
    cfg = er.level_params(3, 2)
    enh = er.enhance_clip([pw.pad_i420(p, w, h) for p in src], W, H, cfg)
    lib.ks265_stub_enhance_reset()
    got = session(lib, w, h, src, ways="csadn", params=(("edge", 3), ("color", 2)))
    assert en_calls(lib) == [(W, H, cfg, 1, 0)] * N
    exp = session(lib, W, H, enh, ways="c")
    g, e = nals(got), nals(exp)
    assert len(g) == len(e) > N and all((a == b) == (t != ws.NAL_SPS) for (t, a), (_, b) in zip(g, e))
    assert ws.output_size(ws.stream_sps(got)) == (w, h)


def test_behind_the_denoiser_the_history_stays_unsharpened(lib):
    rng = np.random.default_rng(193)
    src = [np.clip(p.astype(np.int32) + np.rint(rng.normal(0, 3, p.shape)).astype(np.int32), 0, 255).astype(np.uint8) for p in source()]
    t2 = dr.level_params(2)
    den = dr.filter_clip(src, W, H, *t2)
    assert sum(int((a != b).sum()) for a, b in zip(src[1:], den[1:])) > 5000, "level 2 does not filter this clip"
    cfg = er.level_params(2, 0)
    exp = session(lib, W, H, er.enhance_clip(den, W, H, cfg), ways="c")
    lib.ks265_stub_enhance_reset(); lib.ks265_stub_denoise_reset()
    _, log_dn = logged(lib, lambda: session(lib, W, H, src, ways="csa", params=(("denoise", 2),)))
    lib.ks265_stub_enhance_reset(); lib.ks265_stub_denoise_reset()
    got, log = logged(lib, lambda: session(lib, W, H, src, ways="csa", params=(("denoise", 2), ("edge", 2))))
    assert got == exp
    assert en_calls(lib) == [(W, H, cfg, 1, 1)] * N, "the luma source is a history buffer of the denoiser"
    calls = around_enhance(log)
    assert len(calls) == N
    for f, front, behind in calls:                                       # denoise, its event, enhance, its event: all on one stream
        assert [q[1] for q in front] == ["ks265_input_denoise", "ks265_event_record"] and behind[1] == "ks265_event_record" and {q[2] for q in front + [behind]} == {f[2]}
    count = lambda lg: sum(" ks265_memcpy_d2d_async " in ln for ln in lg)
    assert count(log) == count(log_dn), "no copy of the luma when the denoiser ran"
    # enhancing first and filtering then would be another stream
    assert got != session(lib, W, H, dr.filter_clip(er.enhance_clip(src, W, H, cfg), W, H, *t2), ways="c")


def test_two_lanes_give_the_one_lane_bytes(lib):
    n, iper = 40, 32
    src = edgy_clip(W, H, n, 195)
    params = (("iper", iper), ("edge", 2), ("color", 1))
    lib.ks265_stub_enhance_reset()
    two = session(lib, W, H, src, ways="csa", lanes=2, params=params)
    assert len(en_calls(lib)) == n
    one = session(lib, W, H, src, ways="c", lanes=1, params=params)
    assert two == one
    assert one == session(lib, W, H, er.enhance_clip(src, W, H, er.level_params(2, 1)), ways="c", lanes=1, params=(("iper", iper),))


def test_open_and_configuration(lib, without):
    for params in ((("edge", 1),), (("color", 3),), (("edge", 2), ("color", 2)), (("denoise", 2), ("edge", 1))):
        hd, err = try_open(without, W, H, lanes=1, params=params)
        assert not hd.value and err == QY_NOTSUPPORTED, params
    hd, err = try_open(without, W, H, lanes=1, params=(("denoise", 2),))
    assert hd.value
    without.QY265EncoderClose(hd)
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
    assert C.c_int.from_buffer(cfg, OFF_EDGE).value == 0 and C.c_int.from_buffer(cfg, OFF_COLOR).value == 0, "off by default"
    for k, v in (("edge", "4"), ("edge", "-1"), ("edge", "x"), ("color", "4"), ("color", "-1"), ("color", "")):
        assert lib.QY265ConfigParse(cfg, k.encode(), v.encode()) == BAD_VALUE, (k, v)
    assert lib.QY265ConfigParse(cfg, b"edge", b"3") == 0 and C.c_int.from_buffer(cfg, OFF_EDGE).value == 3 and C.c_int.from_buffer(cfg, OFF_COLOR).value == 0
    assert lib.QY265ConfigParse(cfg, b"color", b"1") == 0 and C.c_int.from_buffer(cfg, OFF_COLOR).value == 1 and C.c_int.from_buffer(cfg, LAY["vpp_denoise"]).value == 0
    for off, v in ((OFF_EDGE, 4), (OFF_EDGE, -1), (OFF_COLOR, 4), (OFF_COLOR, -3)):
        cfg = (C.c_uint8 * LAY["sizeof_config"])()
        assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
        for k, x in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34)):
            assert lib.QY265ConfigParse(cfg, k.encode(), str(x).encode()) == 0
        C.c_int.from_buffer(cfg, off).value = v
        err = C.c_int(0)
        assert not lib.QY265EncoderOpen(cfg, C.byref(err)) and err.value == QY_NOTSUPPORTED, (off, v)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


def test_open_names_the_resolved_parameters(lib, without, capfd):
    capfd.readouterr()
    lib.QY265EncoderClose(open_handle(lib, W, H, lanes=1, params=(("log", 0), ("edge", 3), ("color", 1))))
    out = capfd.readouterr().out
    assert out.count("enhancement on the way in") == 1 and "edge level 3 (gain 24/16, core 3, limit 24, over 8), colour level 1 (gain 8)" in out
    lib.QY265EncoderClose(open_handle(lib, W, H, lanes=1, params=(("log", 0),)))
    assert "enhancement" not in capfd.readouterr().out, "off: no log line"
    hd, err = try_open(without, W, H, lanes=1, params=(("log", 0), ("color", 2)))
    assert not hd.value and capfd.readouterr().out.count("has no ks265_input_enhance") == 1


def test_reconfig_leaves_the_filter_as_opened(lib):
    src = source()[:4]
    hd = open_handle(lib, W, H, lanes=1, latency=b"zerolatency", params=(("edge", 2), ("color", 2)))
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"zerolatency") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34), ("edge", 0), ("color", 3)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    lib.QY265EncoderReconfig.restype = None
    lib.ks265_stub_enhance_reset()
    puts = [host_picture(lib, hd, p, W, H, t) for t, p in enumerate(src)]
    puts[2] = preceded(lambda: lib.QY265EncoderReconfig(hd, cfg), puts[2])
    drive(lib, hd, puts)
    assert en_calls(lib) == [(W, H, E22, 1, 0)] * 4


def test_off_is_the_parent_s_call_log(lib, without):
    """both fields 0: the same calls, line for line, as on a device library that does not have the entries; the threads' interleaving aside (the lines are compared sorted)"""
    for w, h, ways, latency, params in ((W, H, "csadn", b"zerolatency", ()), (202, 134, "csa", b"default", ()), (W, H, "csa", b"default", (("denoise", 1),))):
        src = source(w, h, 5)
        lib.ks265_stub_enhance_reset()
        a, la = logged(lib, lambda: session(lib, w, h, src, ways=ways, latency=latency, params=params))
        b, lb = logged(without, lambda: session(without, w, h, src, ways=ways, latency=latency, params=params))
        assert a == b and len(a) > 500
        assert len(la) > 50 and not any("ks265_input_enhance" in ln for ln in la)
        assert same_calls(la) == same_calls(lb)
        assert en_calls(lib) == []


@pytest.fixture(scope="module")
def sanitized():
    """tests/input_filter_main.c + the host + the stand-in, built once with -fsanitize=address,undefined"""
    return build_host_program("input_filter_main.c", stub="hip_stub_enhance.c")


@pytest.mark.parametrize("denoise", [0, 1], ids=["alone", "behind_the_denoiser"])
@pytest.mark.parametrize("latency", ["default", "zerolatency"])
def test_host_and_stand_in_under_the_sanitizers(sanitized, tmp_path, latency, denoise):
    out = str(tmp_path / "out.265")
    recs = filter_program(sanitized, 202, 134, 5, out, latency, "edge=2", "color=3", *(["denoise=2"] if denoise else []))
    assert recs["enhance"] == [dict(w=208, h=136, edge_gain=16, edge_core=2, edge_limit=16, edge_over=4, color_gain=32, has_src=1, src_is_hist=denoise)] * 5
    assert len(recs["denoise"]) == 5 * denoise and not recs["hdr"]
    sps = ws.stream_sps(open(out, "rb").read())
    assert ws.output_size(sps) == (202, 134) and (sps["width"], sps["height"]) == (208, 136)
