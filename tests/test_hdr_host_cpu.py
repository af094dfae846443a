"""CPU: `vpp_hdr` through the real encoder host, against the stand-in of the device library WITH the three entries (tests/hip_stub_hdr.c):
  * the stand-in's filter equals tests/hdr_ref.py byte for byte on every size, cfg and content of tests/hdr_cases.py, and refuses what the device library refuses;
  * at 208x136, 9 pictures, default GOP and zero latency: every NAL unit of an `hdr=1` handle equals that of a plain handle fed the reference-filtered pictures, for host
    pictures (contiguous, strided, an acquired slot) and "device" I420 / NV12 pictures.  ON THE PARENT COMMIT THIS TEST FAILS: the field is ignored there (and `hdr` is no
    name QY265ConfigParse knows);
  * at 202x134 the filter sees 208x136, behind the pad;
  * `denoise=2 hdr=1 edge=2`: the stream is the plain handle's fed enhance(hdr(denoise(clip))); the call log pins denoise, hdr, the luma copy, enhance - each with its event
    behind it - on one stream, and the enhancement's luma source is the lane's plane, not the denoiser's history;
  * two GOP lanes give the one-lane bytes, each lane with a work buffer of its own;
  * QY265ConfigParse and QY265EncoderOpen refuse values outside the ranges; a stand-in without the entries (tests/hip_stub_enhance.c) refuses `hdr=1` with one log line;
    QY265EncoderReconfig leaves the filter as opened; one log line at open names the integers and the work buffer's bytes;
  * `vpp_hdr = 0` with junk in the other four fields: the call log is that of the same encode on the stand-in WITHOUT the entries, lines sorted, thread numbers aside;
  * the host's derived integers, read back through ks265_stub_hdr_calls, equal hdr_ref.params over a grid;
  * tests/input_filter_main.c, the host and the stand-in under -fsanitize=address,undefined as a program of its own: 5 pictures at 202x134, both latencies, alone and between the
    denoiser and the enhancement."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr
import enhance_ref as er
import hdr_ref as hr
import picture_window_ref as pw
import window_sps as ws
from hdr_cases import CFGS, SIZES, contents
from host_harness import (LAY, QY_NOTSUPPORTED, build_host_lib, build_host_program, drive, edgy_clip, en_calls, filter_program, host_picture, load_host_lib, logged, nals, open_handle,
                          preceded, same_calls, session, try_open)

W, H, N = 208, 136, 9
BAD_VALUE = -2
OFF_HDR, OFF_STRENGTH = LAY["vpp_denoise"] + 12, LAY["vpp_hdr_strength"]     # int vpp_denoise, vpp_edge, vpp_color, vpp_hdr; double vpp_hdr_strength; int vpp_hdr_iter;
OFF_ITER, OFF_SIGMA_S, OFF_SIGMA_R = OFF_STRENGTH + 8, OFF_STRENGTH + 16, OFF_STRENGTH + 24   # double vpp_hdr_sigma_s, vpp_hdr_sigma_r (include/ks265_enc.h)
DEF = hr.params(0, 0, 0, 0)
ON = (("hdr", 1),)


class HdrCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("w", "h", "gain", "iters", "slope")] + [("radius", C.c_int32 * 3), ("work_no", C.c_int32), ("work_ok", C.c_int32)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lb = load_host_lib(build_host_lib("hip_stub_hdr.c"), call_log=str(tmp_path_factory.mktemp("stubhdr") / "calls.log"))
    lb.ks265_input_hdr_work_bytes.restype = C.c_size_t
    return lb


@pytest.fixture(scope="module")
def without(tmp_path_factory):
    """the stand-in without the three entries: the device library of the parent"""
    return load_host_lib(build_host_lib("hip_stub_enhance.c"), call_log=str(tmp_path_factory.mktemp("stubnohdr") / "calls.log"))


def hdr_calls(lib):
    """(w, h, cfg as hdr_ref.params gives it, the work buffer's ordinal, its size was exactly ks265_input_hdr_work_bytes) per call"""
    buf = (HdrCall * 4096)()
    n = lib.ks265_stub_hdr_calls(buf, 4096)
    return [(c.w, c.h, (c.gain, c.iters, c.slope, tuple(c.radius[:c.iters])), c.work_no, c.work_ok) for c in buf[:n]]


def c_cfg(cfg):
    gain, iters, slope, radius = cfg
    return (C.c_int32 * 6)(gain, iters, slope, *(tuple(radius) + (0, 0, 0))[:3])


# ------------------------------------------------------------------ the stand-in's filter

def stub_hdr(lib, ctx, w, h, cfg, pic):
    buf = np.array(pic, np.uint8)
    nb = lib.ks265_input_hdr_work_bytes(w, h)
    assert nb == hr.work_bytes(w, h)
    work = np.zeros(nb, np.uint8)
    assert lib.ks265_input_hdr(ctx, c_cfg(cfg), w, h, C.c_void_p(buf.ctypes.data), C.c_void_p(work.ctypes.data), C.c_size_t(nb)) == 0
    return buf


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_stand_in_equals_the_reference(lib, size):
    w, h = size
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    for name, pic in contents(w, h, seed=w + h).items():
        for cfg in CFGS:
            assert (stub_hdr(lib, ctx, w, h, cfg, pic) == hr.hdr_picture(pic, w, h, cfg)).all(), (w, h, name, cfg)
    lib.ks265_destroy(ctx)


def test_stand_in_refuses_what_the_library_refuses(lib):
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    for w, h, cfg in ((20, 16, DEF), (16, 0, DEF), (8200, 8, DEF), (16, 16, (0, 3, 8, (484, 242, 121))), (16, 16, (81, 3, 8, (484, 242, 121))), (16, 16, (16, 1, 8, (484, 242, 121))),
                      (16, 16, (16, 4, 8, (484, 242, 121))), (16, 16, (16, 3, -1, (484, 242, 121))), (16, 16, (16, 3, 4097, (484, 242, 121))), (16, 16, (16, 3, 8, (2481, 242, 121))),
                      (16, 16, (16, 3, 8, (484, 242, 15))), (16, 16, (16, 2, 8, (484, 15, 121)))):
        assert lib.ks265_input_hdr_validate(ctx, c_cfg(cfg), w, h) == -4, (w, h, cfg)
    assert lib.ks265_input_hdr_validate(ctx, c_cfg((16, 2, 8, (484, 242, 0))), 16, 16) == 0, "the third radius is not judged at 2 iterations"
    assert lib.ks265_input_hdr_work_bytes(20, 16) == 0
    a = np.zeros(4096, np.uint8)
    p = lambda off: C.c_void_p(a.ctypes.data + off)
    nb = hr.work_bytes(16, 16)
    assert lib.ks265_input_hdr(ctx, c_cfg(DEF), 16, 16, p(0), p(384), C.c_size_t(nb - 1)) == -3, "a short work buffer"
    assert lib.ks265_input_hdr(ctx, c_cfg(DEF), 16, 16, p(0), p(380), C.c_size_t(nb)) == -3, "the work buffer overlaps the picture's chroma"
    assert lib.ks265_input_hdr(ctx, c_cfg(DEF), 16, 16, p(2000), p(1000), C.c_size_t(nb)) == -3, "the picture lies inside the work buffer"
    assert lib.ks265_input_hdr(ctx, c_cfg(DEF), 16, 16, p(0), None, C.c_size_t(nb)) == -3
    assert lib.ks265_input_hdr(ctx, c_cfg(DEF), 16, 16, None, p(384), C.c_size_t(nb)) == -3
    assert not a.any()
    lib.ks265_destroy(ctx)


# ------------------------------------------------------------------ streams

CONFIGS = {"gop8": b"default", "zerolatency": b"zerolatency"}
_src = {}


def source(w=W, h=H, n=N):
    if (w, h, n) not in _src:
        _src[(w, h, n)] = edgy_clip(w, h, n, 291)
    return _src[(w, h, n)]


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_way_in_gives_the_plain_handle_s_stream_of_filtered_pictures(lib, cfg):
    """fails on the parent commit, where vpp_hdr is accepted and ignored"""
    latency = CONFIGS[cfg]
    src = source()
    flt = hr.hdr_clip(src, W, H, DEF)
    assert all((a[:W * H] != b[:W * H]).sum() > 500 and (a[W * H:] == b[W * H:]).all() for a, b in zip(src, flt)), "the defaults do not change this clip"
    lib.ks265_stub_hdr_reset()
    exp = session(lib, W, H, flt, ways="c", latency=latency)
    assert hdr_calls(lib) == [], "a plain handle filters nothing"
    assert session(lib, W, H, src, ways="c", latency=latency) != exp
    e = nals(exp)
    for ways in ("csa", "dn"):
        lib.ks265_stub_hdr_reset()
        got = session(lib, W, H, src, ways=ways, latency=latency, params=ON)
        g = nals(got)
        assert len(g) == len(e) > N and all(a == b for a, b in zip(g, e)), (cfg, ways)
        assert hdr_calls(lib) == [(W, H, DEF, 0, 1)] * N


def test_named_parameters_reach_the_filter(lib):
    src = source()[:4]
    cfg = hr.params(2.5, 2, 60, 40)
    lib.ks265_stub_hdr_reset()
    got = session(lib, W, H, src, ways="csa", latency=b"zerolatency", params=ON + (("hdr-strength", 2.5), ("hdr-iter", 2), ("hdr-sigma-s", 60), ("hdr-sigma-r", 40)))
    assert hdr_calls(lib) == [(W, H, cfg, 0, 1)] * 4
    assert got == session(lib, W, H, hr.hdr_clip(src, W, H, cfg), ways="c", latency=b"zerolatency")


def test_ragged_size_is_filtered_behind_the_pad(lib):
    w, h = 202, 134
    src = source(w, h)
    flt = hr.hdr_clip([pw.pad_i420(p, w, h) for p in src], W, H, DEF)
    lib.ks265_stub_hdr_reset()
    got = session(lib, w, h, src, ways="csadn", params=ON)
    assert hdr_calls(lib) == [(W, H, DEF, 0, 1)] * N
    exp = session(lib, W, H, flt, ways="c")
    g, e = nals(got), nals(exp)
    assert len(g) == len(e) > N and all((a == b) == (t != ws.NAL_SPS) for (t, a), (_, b) in zip(g, e))
    assert ws.output_size(ws.stream_sps(got)) == (w, h)


def test_between_the_denoiser_and_the_enhancement(lib):
    rng = np.random.default_rng(293)
    src = [np.clip(p.astype(np.int32) + np.rint(rng.normal(0, 3, p.shape)).astype(np.int32), 0, 255).astype(np.uint8) for p in source()]
    t2, e2 = dr.level_params(2), er.level_params(2, 0)
    den = dr.filter_clip(src, W, H, *t2)
    exp = session(lib, W, H, er.enhance_clip(hr.hdr_clip(den, W, H, DEF), W, H, e2), ways="c")
    lib.ks265_stub_hdr_reset(); lib.ks265_stub_enhance_reset(); lib.ks265_stub_denoise_reset()
    got, log = logged(lib, lambda: session(lib, W, H, src, ways="csa", params=(("denoise", 2), ("hdr", 1), ("edge", 2))))
    assert got == exp
    assert hdr_calls(lib) == [(W, H, DEF, 0, 1)] * N
    assert en_calls(lib) == [(W, H, e2, 1, 0)] * N, "the enhancement's luma source is the lane's plane, not a history buffer of the denoiser"
    # the recursion never sees boosted samples: boosting in front of the denoiser would be another stream
    assert got != session(lib, W, H, er.enhance_clip(dr.filter_clip(hr.hdr_clip(src, W, H, DEF), W, H, *t2), W, H, e2), ways="c")
    rows = [ln.split(" ") for ln in log]
    at = [i for i, f in enumerate(rows) if f[1] == "ks265_input_denoise"]
    assert len(at) == N
    want = ["ks265_input_denoise", "ks265_event_record", "ks265_input_hdr", "ks265_event_record", "ks265_memcpy_d2d_async", "ks265_input_enhance", "ks265_event_record"]
    for i in at:
        mine = [f for f in rows[i:] if f[0] == rows[i][0]][:7]
        assert [f[1] for f in mine] == want and {f[2] for f in mine} == {rows[i][2]} and len({f[4] for f in mine if f[4] != "-"}) == 1, mine


def test_hdr_alone_records_its_event_behind_the_filter(lib):
    src = source()[:3]
    _, log = logged(lib, lambda: session(lib, W, H, src, ways="csa", latency=b"zerolatency", params=ON))
    rows = [ln.split(" ") for ln in log]
    at = [i for i, f in enumerate(rows) if f[1] == "ks265_input_hdr"]
    assert len(at) == 3 and all(f[5] == "3" for f in (rows[i] for i in at))
    for i in at:
        behind = [f for f in rows[i + 1:] if f[0] == rows[i][0]][0]
        assert behind[1] == "ks265_event_record" and behind[2] == rows[i][2]


def test_two_lanes_give_the_one_lane_bytes(lib):
    n, iper = 40, 32
    src = edgy_clip(W, H, n, 295)
    params = (("iper", iper),) + ON
    lib.ks265_stub_hdr_reset()
    two = session(lib, W, H, src, ways="csa", lanes=2, params=params)
    calls = hdr_calls(lib)
    assert len(calls) == n and {c[3] for c in calls} == {0, 1} and all(c[4] for c in calls), "a work buffer per lane"
    lib.ks265_stub_hdr_reset()
    one = session(lib, W, H, src, ways="c", lanes=1, params=params)
    assert {c[3] for c in hdr_calls(lib)} == {0}
    assert two == one
    assert one == session(lib, W, H, hr.hdr_clip(src, W, H, DEF), ways="c", lanes=1, params=(("iper", iper),))


def _fresh_cfg(lib):
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
    for k, x in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34), ("log", 1)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(x).encode()) == 0
    return cfg


def test_open_and_configuration(lib, without):
    for params in (ON, ON + (("hdr-iter", 2),), (("denoise", 2), ("hdr", 1)), (("hdr", 1), ("edge", 1))):
        hd, err = try_open(without, W, H, lanes=1, params=params)
        assert not hd.value and err == QY_NOTSUPPORTED, params
    hd, err = try_open(without, W, H, lanes=1, params=(("edge", 2), ("hdr-strength", 3)))
    assert hd.value, "vpp_hdr 0: the other fields are not looked at"
    without.QY265EncoderClose(hd)
    cfg = _fresh_cfg(lib)
    assert C.c_int.from_buffer(cfg, OFF_HDR).value == 0, "off by default"
    for k, v in (("hdr", "2"), ("hdr", "-1"), ("hdr", "x"), ("hdr-strength", "5.01"), ("hdr-strength", "-0.5"), ("hdr-strength", "nan"), ("hdr-iter", "1"), ("hdr-iter", "4"),
                 ("hdr-iter", "2.5"), ("hdr-iter", "-2"), ("hdr-sigma-s", "100.5"), ("hdr-sigma-s", "-1"), ("hdr-sigma-r", "101"), ("hdr-sigma-r", "-3"), ("hdr-sigma-r", "")):
        assert lib.QY265ConfigParse(cfg, k.encode(), v.encode()) == BAD_VALUE, (k, v)
    for k, v, off, ty in (("hdr", "1", OFF_HDR, C.c_int), ("hdr-strength", "0.75", OFF_STRENGTH, C.c_double), ("hdr-iter", "2", OFF_ITER, C.c_int), ("hdr-iter", "0", OFF_ITER, C.c_int),
                          ("hdr-sigma-s", "100", OFF_SIGMA_S, C.c_double), ("hdr-sigma-r", "0.01", OFF_SIGMA_R, C.c_double)):
        assert lib.QY265ConfigParse(cfg, k.encode(), v.encode()) == 0 and ty.from_buffer(cfg, off).value == float(v), (k, v)
    for off, ty, v in ((OFF_HDR, C.c_int, 2), (OFF_HDR, C.c_int, -1), (OFF_STRENGTH, C.c_double, 5.5), (OFF_STRENGTH, C.c_double, -1.0), (OFF_STRENGTH, C.c_double, float("nan")),
                       (OFF_ITER, C.c_int, 1), (OFF_ITER, C.c_int, 4), (OFF_SIGMA_S, C.c_double, 101.0), (OFF_SIGMA_S, C.c_double, -2.0), (OFF_SIGMA_R, C.c_double, 100.5),
                       (OFF_SIGMA_R, C.c_double, float("nan")), (OFF_STRENGTH, C.c_double, 0.01)):
        cfg = _fresh_cfg(lib)
        C.c_int.from_buffer(cfg, OFF_HDR).value = 1
        ty.from_buffer(cfg, off).value = v
        err = C.c_int(0)
        assert not lib.QY265EncoderOpen(cfg, C.byref(err)) and err.value == QY_NOTSUPPORTED, (off, v)      # (strength 0.01: a gain of 0, which the device library refuses)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


def test_open_names_the_resolved_parameters(lib, without, capfd):
    capfd.readouterr()
    lib.QY265EncoderClose(open_handle(lib, W, H, lanes=1, params=(("log", 0), ("hdr", 1), ("hdr-iter", 2), ("hdr-sigma-s", 100), ("hdr-sigma-r", 100), ("hdr-strength", 5))))
    out = capfd.readouterr().out
    assert out.count("local contrast on the way in") == 1
    assert "gain 80/16, 2 iterations, slope 6, radii 2479 / 1239 / 0 (1/16 sample), work buffer %d bytes" % hr.work_bytes(W, H) in out
    lib.QY265EncoderClose(open_handle(lib, W, H, lanes=1, params=(("log", 0),)))
    assert "local contrast" not in capfd.readouterr().out, "off: no log line"
    hd, err = try_open(without, W, H, lanes=1, params=(("log", 0), ("hdr", 1)))
    assert not hd.value and capfd.readouterr().out.count("has no ks265_input_hdr") == 1


def test_reconfig_leaves_the_filter_as_opened(lib):
    src = source()[:4]
    hd = open_handle(lib, W, H, lanes=1, latency=b"zerolatency", params=ON)
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"zerolatency") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34), ("hdr", 0), ("hdr-strength", 4)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    lib.QY265EncoderReconfig.restype = None
    lib.ks265_stub_hdr_reset()
    puts = [host_picture(lib, hd, p, W, H, t) for t, p in enumerate(src)]
    puts[2] = preceded(lambda: lib.QY265EncoderReconfig(hd, cfg), puts[2])
    drive(lib, hd, puts)
    assert hdr_calls(lib) == [(W, H, DEF, 0, 1)] * 4


def test_off_is_the_parent_s_call_log(lib, without):
    """vpp_hdr 0 and junk in the other four fields: the same calls, line for line, as on a device library that does not have the entries; the threads' interleaving aside.
    All three encodes at zero latency: with a GOP of B pictures the input slot - and so the event - a picture takes depends on whether the scheduler thread has freed one
    yet, and two runs of ONE library already differ in the events their lines name (about one run in fourteen here)"""
    junk = (("hdr-strength", 4.5), ("hdr-iter", 2), ("hdr-sigma-s", 77), ("hdr-sigma-r", 0.5))
    for w, h, ways, latency, params in ((W, H, "csadn", b"zerolatency", ()), (202, 134, "csa", b"zerolatency", ()), (W, H, "csa", b"zerolatency", (("denoise", 1), ("edge", 2)))):
        src = source(w, h, 5)
        lib.ks265_stub_hdr_reset()
        a, la = logged(lib, lambda: session(lib, w, h, src, ways=ways, latency=latency, params=params + junk))
        b, lb = logged(without, lambda: session(without, w, h, src, ways=ways, latency=latency, params=params))
        assert a == b and len(a) > 500
        assert len(la) > 50 and not any("ks265_input_hdr" in ln for ln in la)
        assert same_calls(la) == same_calls(lb)
        assert hdr_calls(lib) == []


def test_the_host_derives_the_reference_s_integers(lib):
    """one picture at 64x64 per point: what ks265_input_hdr was handed is hdr_ref.params of what QY265ConfigParse was handed"""
    pic = [contents(64, 64, 7)["ramp"]]
    grid = [(s, n, ss, sr) for s in (0.25, 1, 2.75, 5) for n in (2, 3) for ss in (1, 20, 63, 100) for sr in (1, 15, 100)]
    grid += [(0.5, 3, 100, 0.01), (0, 0, 0, 0), (0, 2, 0, 0), (3.3, 0, 0.4, 0), (1, 3, 0.1, 100), (4.97, 2, 99.9, 0.3)]
    for s, n, ss, sr in grid:
        lib.ks265_stub_hdr_reset()
        session(lib, 64, 64, pic, ways="c", latency=b"zerolatency", params=ON + (("hdr-strength", s), ("hdr-iter", n), ("hdr-sigma-s", ss), ("hdr-sigma-r", sr)))
        want = hr.params(s, n, ss, sr)
        assert hr.check_cfg(want, 64, 64)
        assert hdr_calls(lib) == [(64, 64, want, 0, 1)], (s, n, ss, sr)


@pytest.fixture(scope="module")
def sanitized():
    """tests/input_filter_main.c + the host + the stand-in, built once with -fsanitize=address,undefined"""
    return build_host_program("input_filter_main.c", stub="hip_stub_hdr.c")


@pytest.mark.parametrize("around", [0, 1], ids=["alone", "between_denoiser_and_enhancement"])
@pytest.mark.parametrize("latency", ["default", "zerolatency"])
def test_host_and_stand_in_under_the_sanitizers(sanitized, tmp_path, latency, around):
    """strength 2, 2 iterations, sigma_s 30, sigma_r at its default: the derived integers (32, 2, 13, 744 / 372), always the same work buffer of exactly
    ks265_input_hdr_work_bytes"""
    out = str(tmp_path / "out.265")
    recs = filter_program(sanitized, 202, 134, 5, out, latency, "hdr=1", "hdr-strength=2", "hdr-iter=2", "hdr-sigma-s=30", *(["denoise=2", "edge=2"] if around else []))
    assert len(recs["hdr"]) == 5
    for c in recs["hdr"]:
        assert (c["w"], c["h"], c["gain"], c["iters"], c["slope"], c["radius0"], c["radius1"], c["work_no"]) == (208, 136, 32, 2, 13, 744, 372, 0) and c["work_ok"], c
    assert len(recs["denoise"]) == len(recs["enhance"]) == 5 * around
    sps = ws.stream_sps(open(out, "rb").read())
    assert ws.output_size(sps) == (202, 134) and (sps["width"], sps["height"]) == (208, 136)
