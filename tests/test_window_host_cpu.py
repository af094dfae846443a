"""CPU: picture sizes that are no multiple of 8 through the real encoder host, against the stand-in of the device library WITH the three entries (tests/hip_stub_window.c),
at 202x134 (coded 208x136) and 128x72:
  * against the plain stand-in (tests/hip_stub.c: no ks265_input_pad) QY265EncoderOpen(202, 134) is QY_NOTSUPPORTED, as every such size was;
  * with the entries, on one and two GOP lanes, zero latency and the default GOP with B pictures: the SPS carries 208x136 and the window (0, 3, 0, 1); the stand-in saw one
    ks265_input_pad per picture with the source size and the pitches of what it was given - the staging picture for the three host ways in (contiguous, strided, acquired slot),
    the caller's own for a device picture; every NAL unit but the SPS equals that of a 208x136 handle fed tests/picture_window_ref.py's padded pictures; the -o pictures are
    202x134 and the crop of that handle's;
  * device I420 and NV12 pictures give the host pictures' stream;
  * odd sizes are refused; the scaled entry and an RGB device picture on a ragged handle are QY_NOTSUPPORTED and leave the handle usable;
  * at 1366x768 - large enough for the upload out of the caller's own memory, host-synchronous and (KS265_UPL_ORDER=0) on a stream of its own - the same holds;
  * `devrecon`: pictures fetched with ks265_enc_get_device_recon are 202x134, the crop of the coded handle's; every call's crop is issued behind a wait for the event recorded
    behind the previous call's conversion (the calls may name different streams and share the lane's scratch picture);
  * a `roi` map of the SOURCE picture's ceil(W / b) x ceil(H / b) elements is taken, from "device" and from host memory;
  * a 128x72 handle makes none of the new calls;
  * tests/input_filter_main.c, the host and the stand-in under -fsanitize=address,undefined as a program of its own: 5 pictures at 202x134, both latencies."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import picture_window_ref as pw
import window_sps as ws
from host_harness import (IN_I420, IN_NV12, IN_RGB, LAY, QY_NOTSUPPORTED, QY_OK, DevPicture, Nal, Picture, Roi, YUV, build_host_lib, build_host_program, clip,
                          filter_program, load_host_lib, nals, open_handle, session, try_open)

W, H, CW, CH, N = 202, 134, 208, 136, 17


class PadCall(C.Structure):
    _fields_ = [("format", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("cw", C.c_int32), ("ch", C.c_int32), ("pitch", C.c_int32 * 3)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_host_lib(build_host_lib("hip_stub_window.c"), call_log=str(tmp_path_factory.mktemp("stubwin") / "calls.log"))


@pytest.fixture(scope="module")
def plain():
    return load_host_lib(build_host_lib("hip_stub.c"))


def pad_calls(lib):
    buf = (PadCall * 4096)()
    n = lib.ks265_stub_pad_calls(buf, 4096)
    return [(c.format, c.w, c.h, c.cw, c.ch, tuple(c.pitch)) for c in buf[:n]]


def test_plain_stand_in_refuses_a_ragged_size(plain):
    hd, err = try_open(plain, W, H, lanes=1)
    assert not hd.value and err == QY_NOTSUPPORTED
    hd, err = try_open(plain, 128, 72, lanes=1)
    assert hd.value
    plain.QY265EncoderClose(hd)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("latency", [b"zerolatency", b"default"], ids=["zerolatency", "gop8"])
def test_ragged_handle_is_the_coded_handle_fed_padded_pictures(lib, tmp_path, lanes, latency):
    params = (("iper", 8),) if lanes == 2 else ()
    src = clip(W, H, N, 71)
    padded = [pw.pad_i420(p, W, H) for p in src]
    rec = (str(tmp_path / "rag.yuv"), str(tmp_path / "cod.yuv")) if lanes == 1 else (None, None)
    lib.ks265_stub_pad_reset()
    got = session(lib, W, H, src, ways="csa", lanes=lanes, latency=latency, params=params, recon=rec[0])
    calls = pad_calls(lib)
    assert calls == [(IN_I420, W, H, CW, CH, (W, W // 2, W // 2))] * N, "one pad per picture, from the staging picture"
    exp = session(lib, CW, CH, padded, ways="csa", lanes=lanes, latency=latency, params=params, recon=rec[1])
    assert pad_calls(lib) == calls, "the coded-size handle pads nothing"
    sps = ws.stream_sps(got)
    assert (sps["width"], sps["height"], sps["window"]) == (CW, CH, (0, 3, 0, 1)) and ws.output_size(sps) == (W, H)
    assert ws.stream_sps(exp)["flag"] == 0
    g, e = nals(got), nals(exp)
    assert len(g) == len(e) > N and [t for t, _ in g] == [t for t, _ in e]
    assert sum(t < 32 for t, _ in g) == N
    for (t, a), (_, b) in zip(g, e):
        assert (a == b) == (t != ws.NAL_SPS), t
    if rec[0]:
        r, c = np.fromfile(rec[0], np.uint8), np.fromfile(rec[1], np.uint8)
        assert r.size == N * W * H * 3 // 2 and c.size == N * CW * CH * 3 // 2
        r, c = r.reshape(N, -1), c.reshape(N, -1)
        for t in range(N):
            assert (r[t] == pw.crop_i420(c[t], CW, CH, W, H)).all(), t


def test_device_pictures_give_the_host_pictures_stream(lib):
    src = clip(W, H, 9, 73)
    lib.ks265_stub_pad_reset()
    host = session(lib, W, H, src, ways="c")
    assert len(pad_calls(lib)) == 9
    lib.ks265_stub_pad_reset()
    assert session(lib, W, H, src, ways="dn") == host
    calls = pad_calls(lib)
    assert calls[0] == (IN_I420, W, H, CW, CH, (W + 5, W // 2 + 5, W // 2 + 5)) and calls[1] == (IN_NV12, W, H, CW, CH, (W + 5, W + 5, 0)) and len(calls) == 9, "the caller's planes, where they lie"


def open_raw(lib, w, h):
    """QY265EncoderOpen with picWidth / picHeight written into the structure: QY265ConfigParse's own bounds are not in the way"""
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
    for k, v in (("fr", 50), ("rc", 0), ("qp", 34), ("threads", 4), ("log", 1)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0, k
    C.c_int.from_buffer(cfg, LAY["picWidth"]).value, C.c_int.from_buffer(cfg, LAY["picHeight"]).value = w, h
    err = C.c_int(0)
    return C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err))), err.value


def test_odd_sizes_are_refused(lib):
    for w, h in ((201, 134), (202, 133), (127, 72), (0, 72), (202, 0), (202, -2), (-202, 134), (8194, 72), (202, 8194), (1 << 30 | 2, 134)):
        hd, err = open_raw(lib, w, h)
        assert not hd.value and err == QY_NOTSUPPORTED, (w, h)
    assert lib.QY265ConfigParse((C.c_uint8 * LAY["sizeof_config"])(), b"wdt", b"0") != 0                  # (the parser's own bounds: 2 .. 8192)
    assert lib.QY265ConfigParse((C.c_uint8 * LAY["sizeof_config"])(), b"hgt", b"8194") != 0
    for w, h in ((2, 2), (10, 6), (8190, 2)):                           # tiny and thin even sizes open: the size rule asks for nothing but even, coded 8x8 / 16x8 / 8192x8
        hd, err = open_raw(lib, w, h)
        assert hd.value, (w, h, hex(err & 0xFFFFFFFF))
        lib.QY265EncoderClose(hd)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


def test_refusals_on_a_ragged_handle_leave_it_usable(lib):
    hd = open_handle(lib, W, H, lanes=1, latency=b"zerolatency")
    assert lib.ks265_enc_enable_device_input(hd) == QY_OK
    assert lib.ks265_enc_enable_device_scale(hd, 512, 512) == QY_NOTSUPPORTED
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()
    p = clip(W, H, 1, 75)[0]
    rgb = np.zeros((H, W, 3), np.uint8)
    before = sum(1 for _ in open(lib.call_log_path))
    d = DevPicture()
    d.format, d.device, d.pixel_step = IN_RGB, 0, 3
    for k in range(3):
        d.plane[k], d.pitch[k] = rgb.ctypes.data + k, 3 * W
    assert lib.ks265_enc_encode_device_frame(hd, C.byref(nal), C.byref(nn), C.byref(d), C.byref(outp)) == QY_NOTSUPPORTED and nn.value == 0
    d.format = 0x1000 | 1 << 8 | 1 << 5 | 10                            # P010
    assert lib.ks265_enc_encode_device_frame(hd, C.byref(nal), C.byref(nn), C.byref(d), C.byref(outp)) == QY_NOTSUPPORTED
    pl = [np.ascontiguousarray(q) for q in pw.planes(p, W, H)]
    d.format = IN_I420
    for k, q in enumerate(pl):
        d.plane[k], d.pitch[k] = q.ctypes.data, q.strides[0]
    for sw, sh in ((W, H), (CW, CH), (2 * CW, 2 * CH)):
        assert lib.ks265_enc_encode_device_frame_scaled(hd, C.byref(nal), C.byref(nn), C.byref(d), sw, sh, 1, C.byref(outp)) == QY_NOTSUPPORTED and nn.value == 0
    d.pitch[1] = W // 2 - 1                                             # a pitch below the row
    assert lib.ks265_enc_encode_device_frame(hd, C.byref(nal), C.byref(nn), C.byref(d), C.byref(outp)) == QY_NOTSUPPORTED
    d.pitch[1] = W // 2
    assert lib.QY265EncoderDelayedFrames(hd) == 0
    assert sum(1 for _ in open(lib.call_log_path)) == before, "a refused picture enqueued something"
    for _ in range(3):
        assert lib.ks265_enc_encode_device_frame(hd, C.byref(nal), C.byref(nn), C.byref(d), C.byref(outp)) == QY_OK and nn.value > 0
    lib.QY265EncoderClose(hd)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


@pytest.mark.parametrize("upl", [None, "0"], ids=["sync", "stream"])
def test_upload_out_of_the_callers_memory_is_padded_too(lib, upl):
    w, h, n = 1366, 768, 4
    cw, ch = pw.coded_size(w, h)
    src = clip(w, h, n, 81)
    old = os.environ.get("KS265_UPL_ORDER")
    if upl is not None:
        os.environ["KS265_UPL_ORDER"] = upl
    try:
        lib.ks265_stub_pad_reset()
        before = sum(1 for _ in open(lib.call_log_path))
        got = session(lib, w, h, src, ways="cs")
        assert pad_calls(lib) == [(IN_I420, w, h, cw, ch, (w, w // 2, w // 2))] * n
        new = open(lib.call_log_path).read().split("\n")[before:]
        assert sum("ks265_memcpy_h2d_sync" in ln for ln in new) == (3 * (n // 2) if upl is None else 0), "the contiguous pictures go up from where they lie, plane by plane"
        exp = session(lib, cw, ch, [pw.pad_i420(p, w, h) for p in src], ways="cs")
    finally:
        os.environ.pop("KS265_UPL_ORDER", None)
        if old is not None:
            os.environ["KS265_UPL_ORDER"] = old
    g, e = nals(got), nals(exp)
    assert len(g) == len(e) > n and all((a == b) == (t != ws.NAL_SPS) for (t, a), (_, b) in zip(g, e))
    assert ws.output_size(ws.stream_sps(got)) == (w, h)


def _fetch_all(lib, w, h, pictures):
    """a zero-latency handle with `devrecon`: every picture's reconstruction fetched as packed I420 right behind its call, each fetch naming another stream; (pictures, the
    call log's lines of every fetch)"""
    hd = open_handle(lib, w, h, lanes=1, latency=b"zerolatency", defaults=("devrecon",))
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
    yuv.iWidth, yuv.iHeight = w, h
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = w, w // 2, w // 2
    pic.yuv = C.pointer(yuv)
    out, logs = [], []
    for t, p in enumerate(pictures):
        for k, off in enumerate((0, w * h, w * h * 5 // 4)):
            yuv.pData[k] = C.cast(p.ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        assert lib.QY265EncoderEncodeFrame(hd, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == QY_OK
        assert lib.ks265_enc_device_recon_pending(hd) == 1
        dst = np.full(w * h * 3 // 2, 0xA5, np.uint8)
        d = DevPicture()
        d.format, d.device, d.stream = IN_I420, 0, 0x1000 * (t + 1)     # (the stand-in has no streams: the value only travels)
        d.plane[0], d.plane[1], d.plane[2] = dst.ctypes.data, dst.ctypes.data + w * h, dst.ctypes.data + w * h * 5 // 4
        d.pitch[0], d.pitch[1], d.pitch[2] = w, w // 2, w // 2
        before = sum(1 for _ in open(lib.call_log_path))
        assert lib.ks265_enc_get_device_recon(hd, C.byref(d), None) == QY_OK
        logs.append([ln.split(" ") for ln in open(lib.call_log_path).read().splitlines()[before:]])
        out.append(dst)
    lib.QY265EncoderClose(hd)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5
    return out, logs


def test_device_recon_is_the_window_and_its_scratch_picture_is_guarded(lib):
    src = clip(W, H, 4, 83)
    got, logs = _fetch_all(lib, W, H, src)
    exp, logs_c = _fetch_all(lib, CW, CH, [pw.pad_i420(p, W, H) for p in src])
    for a, b in zip(got, exp):
        assert (a == pw.crop_i420(b, CW, CH, W, H)).all()
    names = lambda log: [ln[1] for ln in log]
    assert all("ks265_output_crop" not in names(log) for log in logs_c), "the coded-size handle crops nothing"
    guard = None                                                        # the event recorded right behind the previous fetch's conversion
    for t, log in enumerate(logs):
        n = names(log)
        crop, conv = n.index("ks265_output_crop"), n.index("ks265_output_convert")
        assert crop < conv and n.count("ks265_output_crop") == n.count("ks265_output_convert") == 1
        waits = [ln[4] for ln in log[:crop] if ln[1] == "ks265_stream_wait_event"]
        if guard is not None:
            assert guard in waits, (t, guard, log)
        records = [ln[4] for ln in log[conv + 1:] if ln[1] == "ks265_event_record"]
        assert len(records) == 2, log                                   # the scratch picture's event and the slot's
        guard = records[0]
        # beside the crop, its wait and its event the fetch is the coded-size handle's, call for call
        rest = [x for x in n if x != "ks265_output_crop"]
        assert len(rest) - len(names(logs_c[t])) == (1 if t == 0 else 2), (rest, names(logs_c[t]))


def test_roi_maps_describe_the_source_picture(lib):
    hd = open_handle(lib, W, H, lanes=1, latency=b"zerolatency", roi=True)
    assert lib.ks265_enc_enable_device_input(hd) == QY_OK
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()
    pl = [np.ascontiguousarray(q) for q in pw.planes(clip(W, H, 1, 79)[0], W, H)]
    d = DevPicture()
    d.format = IN_I420
    for k, q in enumerate(pl):
        d.plane[k], d.pitch[k] = q.ctypes.data, q.strides[0]
    m = np.full(((H + 15) // 16, (W + 15) // 16), 4, np.int8)           # 9 x 13 blocks of 16: the last ones hang over 202 x 134
    for device in (0, -1):
        r = Roi()
        r.type, r.log2_block, r.device, r.data, r.pitch, r.stream = 0, 4, device, m.ctypes.data, m.strides[0], None
        before = sum(1 for _ in open(lib.call_log_path))
        assert lib.ks265_enc_set_next_roi(hd, C.byref(r)) == QY_OK
        assert lib.ks265_enc_encode_device_frame(hd, C.byref(nal), C.byref(nn), C.byref(d), C.byref(outp)) == QY_OK and nn.value > 0
        new = open(lib.call_log_path).read().split("\n")[before:]
        assert sum("ks265_roi_reduce" in ln for ln in new) == (1 if device == 0 else 0) and sum("ks265_input_pad" in ln for ln in new) == 1
    r.pitch = m.shape[1] - 1                                            # a pitch below the source picture's row of blocks
    assert lib.ks265_enc_set_next_roi(hd, C.byref(r)) == QY_NOTSUPPORTED
    lib.QY265EncoderClose(hd)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


def test_a_multiple_of_8_makes_no_new_call(lib):
    lib.ks265_stub_pad_reset()
    before = sum(1 for _ in open(lib.call_log_path))
    s = session(lib, 128, 72, clip(128, 72, 9, 77), ways="csad")
    assert len(s) > 500 and ws.stream_sps(s)["flag"] == 0
    new = open(lib.call_log_path).read().split("\n")[before:]
    assert new and not any(x in ln for ln in new for x in ("ks265_input_pad", "ks265_output_crop", "ks265_sse_window"))
    assert pad_calls(lib) == []


@pytest.fixture(scope="module")
def sanitized():
    """tests/input_filter_main.c + the host + the stand-in (which has none of the filters' entries), built with -fsanitize=address,undefined"""
    return build_host_program("input_filter_main.c", stub="hip_stub_window.c")


@pytest.mark.parametrize("latency", ["default", "zerolatency"])
def test_host_and_stand_in_under_the_sanitizers(sanitized, tmp_path, latency):
    rec, out = str(tmp_path / "rec.yuv"), str(tmp_path / "out.265")
    recs = filter_program(sanitized, W, H, 5, out, latency, "recon=" + rec)
    assert recs["pad"] == [dict(format=IN_I420, w=W, h=H, cw=CW, ch=CH, pitch0=W, pitch1=W // 2, pitch2=W // 2)] * 5 and not recs["denoise"] + recs["enhance"] + recs["hdr"]
    sps = ws.stream_sps(open(out, "rb").read())
    assert ws.output_size(sps) == (W, H) and (sps["width"], sps["height"]) == (CW, CH)
    assert os.path.getsize(rec) == 5 * W * H * 3 // 2
