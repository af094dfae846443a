"""CPU: pictures of the YUV family (KS265_IN_YUV, include/ks265_enc.h) through the real encoder host, against the stand-in of the device library WITH the family
(tests/hip_stub_yuv.c), 128x72:
  * a P010, an I210 and a YUYV clip through ks265_enc_encode_device_frame write, byte for byte, the stream of the same clip handed in as host I420 made by
    tests/yuv_hibit_ref.py - one and two GOP lanes;
  * the scaled entry takes a P010 source and equals reference-convert-then-yuv_scale_ref;
  * an odd pitch on a two-byte format, packed 4:4:4, depth 17 and depth 8 with msb are QY_NOTSUPPORTED, a pitch below the row QY_POINTER; each refusal shows no device call
    and leaves a pending ROI map pending;
  * a P010 clip makes the device-library calls an NV12 clip makes, entry by entry: the family adds none (tests/test_submit_order_cpu.py pins the scheduler's order as before);
  * the stand-in's conversion routine in a program of its own under -fsanitize=address,undefined, over ragged shapes in buffers of exactly their extent, equals the
    specification (no sanitizer touches anything loaded into Python)."""
from __future__ import annotations

import collections
import ctypes as C
import subprocess

import numpy as np
import pytest

import yuv_hibit_ref as yh
import yuv_scale_ref as ys
from host_harness import QY_NOTSUPPORTED, QY_OK, QY_POINTER, Nal, Picture, Roi, build_host_lib, build_host_program, dev_pic, device_picture, drive, host_picture, load_host_lib
from host_harness import open_handle as open_at

W, H, SW, SH, N = 128, 72, 256, 144, 17
P010, I210, YUYV8, NV12 = (yh.SEMI, yh.S420, 10, 1), (yh.PLANAR, yh.S422, 10, 0), (yh.YUYV, yh.S422, 8, 0), (yh.SEMI, yh.S420, 8, 0)
JUNK = dict(step=77, matrix=9, full_range=5)                            # pixel_step, matrix, full_range: ignored by the family


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_host_lib(build_host_lib("hip_stub_yuv.c"), call_log=str(tmp_path_factory.mktemp("stubyuv") / "calls.log"))


def open_handle(lib, params=(), lanes=1, roi=False):
    return open_at(lib, W, H, params=params, lanes=lanes, roi=roi)


def yuv_pic(bufs, offs, pitches, code, pts=0):
    return dev_pic(bufs, offs, pitches, code, pts, **JUNK)


def session(lib, pictures, lanes=1, scaled=None, params=()):
    """one handle fed `pictures`: flat uint8 arrays are host I420 pictures (QY265EncoderEncodeFrame), tuples (bufs, offs, pitches, code) pictures of the family in "device"
    memory (scaled=(sw, sh, filter): through the scaled entry).  The stream."""
    h = open_handle(lib, params=params, lanes=lanes)
    if any(isinstance(p, tuple) for p in pictures):
        assert lib.ks265_enc_enable_device_input(h) == QY_OK
    if scaled:
        assert lib.ks265_enc_enable_device_scale(h, scaled[0], scaled[1]) == QY_OK
    return drive(lib, h, (device_picture(lib, h, *p, pts=t, scaled=scaled, **JUNK) if isinstance(p, tuple) else host_picture(lib, h, p, W, H, t) for t, p in enumerate(pictures)))


def yuv_clip(fmt, w, h, n, seed, front=1, behind=3):
    """n moving pictures of the format as (bufs, offs, pitches, code) - off their buffers' starts, pitches above the row, stray bits beside the samples - and their planes"""
    layout, sub, depth, msb = fmt
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    pics, planes = [], []
    for t in range(n):
        full = []                                                       # Y, U, V at the luma grid in [0, 1): a moving pattern with a little noise
        for k, (a, b) in enumerate(((0.11, 0.07), (0.05, 0.13), (0.09, 0.03))):
            full.append(np.clip(0.5 + 0.4 * np.sin(a * (xx + 2 * t) + k) * np.cos(b * (yy + 3 * t)) + rng.random((h, w)) * 0.04, 0, 0.9999))
        c = [f if sub == yh.S444 else f[:, 0::2] if sub == yh.S422 else f[0::2, 0::2] for f in full[1:]]
        q = [np.floor(f * (1 << depth)).astype(np.int64) for f in (full[0], *c)]
        if layout == yh.PLANAR:
            stored = q
        elif layout == yh.SEMI:
            uv = np.empty((q[1].shape[0], 2 * q[1].shape[1]), np.int64)
            uv[:, 0::2], uv[:, 1::2] = q[1], q[2]
            stored = [q[0], uv]
        else:
            p = np.empty((h, 2 * w), np.int64)
            yo, uo, vo = (0, 1, 3) if layout == yh.YUYV else (1, 0, 2)
            p[:, yo::2], p[:, uo::4], p[:, vo::4] = q[0], q[1], q[2]
            stored = [p]
        out = []
        for s in stored:
            if 8 < depth < 16:
                junk = rng.integers(0, 1 << (16 - depth), s.shape)
                s = s << (16 - depth) | junk if msb else junk << depth | s
            out.append(s.astype(np.uint8 if depth == 8 else np.uint16))
        pics.append((*yh.lay_out(out, front, behind), yh.code(layout, sub, depth, msb)))
        planes.append(out)
    return pics, planes


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("fmt", [P010, I210, YUYV8], ids=["p010", "i210", "yuyv"])
def test_clip_writes_the_stream_of_its_reference_conversion(lib, fmt, lanes):
    params = (("iper", 8),) if lanes == 2 else ()
    pics, planes = yuv_clip(fmt, W, H, N, 51)
    host = [yh.to_i420(p, *fmt) for p in planes]
    got, exp = session(lib, pics, lanes, params=params), session(lib, host, lanes, params=params)
    assert len(got) > 1000 and got == exp
    if fmt[2] > 8 and lanes == 1:                                       # the comparison can tell roundings apart: the same clip truncated instead of rounded
        trunc = [np.concatenate([(yh.normalise(yh.split(p, fmt[0])[0], fmt[2], fmt[3]) >> (fmt[2] - 8)).astype(np.uint8).ravel(), h_[W * H:]]) for p, h_ in zip(planes, host)]
        assert session(lib, trunc, lanes, params=params) != exp


def test_scaled_entry_takes_p010(lib):
    pics, planes = yuv_clip(P010, SW, SH, 9, 53)
    host = [ys.scale_i420(yh.to_i420(p, *P010), SW, SH, W, H, 1) for p in planes]
    got, exp = session(lib, pics, scaled=(SW, SH, 1)), session(lib, host)
    assert len(got) > 1000 and got == exp
    host0 = [ys.scale_i420(yh.to_i420(p, *P010), SW, SH, W, H, 0) for p in planes[:3]]
    assert session(lib, pics[:3], scaled=(SW, SH, 0)) == session(lib, host0)


def _entries(lib, start):
    """entry -> calls, from line `start` of the call log on (the stand-ins below this one log their picture entries under the names they were included with)"""
    return collections.Counter(ln.split(" ")[1].replace("ks265_u8_", "ks265_") for ln in open(lib.call_log_path).read().splitlines()[start:] if " " in ln)


def test_the_family_adds_no_device_library_call(lib):
    counts = []
    for fmt in (NV12, P010, YUYV8):
        pics, _ = yuv_clip(fmt, W, H, 9, 55)
        if fmt == NV12:
            pics = [(*p[:3], 1) for p in pics]                          # KS265_IN_NV12 under its own code
        before = sum(1 for _ in open(lib.call_log_path))
        session(lib, pics)
        counts.append(_entries(lib, before))
    assert counts[0]["ks265_input_convert"] == 9 and counts[0] == counts[1] == counts[2]


def test_aliases_are_i420_and_nv12(lib):
    pics, planes = yuv_clip(NV12, W, H, 5, 57)
    host = [yh.to_i420(p, *NV12) for p in planes]
    assert session(lib, pics) == session(lib, host)                     # KS265_IN_YUV(1, 0, 8, 0)
    pics, planes = yuv_clip((yh.PLANAR, yh.S420, 8, 0), W, H, 5, 58)
    assert session(lib, pics) == session(lib, [yh.to_i420(p, yh.PLANAR, yh.S420, 8) for p in planes])


def test_refusals_enqueue_nothing_and_keep_the_map(lib):
    h = open_handle(lib, roi=True)
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), Picture()
    (bufs, offs, pitches, code), = yuv_clip(P010, W, H, 1, 59)[0]
    (pb, po, pp, pcode), = yuv_clip((yh.YUYV, yh.S422, 10, 1), W, H, 1, 60)[0]
    m = np.full(((H + 7) // 8, (W + 7) // 8), 3, np.int8)               # a map in "device" memory: its reduction shows in the call log
    r = Roi()
    r.type, r.log2_block, r.device, r.data, r.pitch, r.stream = 0, 3, 0, m.ctypes.data, m.strides[0], None
    assert lib.ks265_enc_set_next_roi(h, C.byref(r)) == QY_OK
    before = sum(1 for _ in open(lib.call_log_path))
    ok = lambda: yuv_pic(bufs, offs, pitches, code)
    bad = []
    p = ok(); p.pitch[0] = pitches[0] + 1; bad.append((p, QY_NOTSUPPORTED))               # an odd pitch on a two-byte format
    p = ok(); p.pitch[1] = pitches[1] + 1; bad.append((p, QY_NOTSUPPORTED))
    p = ok(); p.plane[1] = p.plane[1] + 1; bad.append((p, QY_NOTSUPPORTED))               # an odd address
    bad.append((yuv_pic(pb, po, pp, yh.code(yh.YUYV, yh.S444, 10, 1)), QY_NOTSUPPORTED))  # packed 4:4:4
    bad.append((yuv_pic(pb, po, pp, yh.code(yh.UYVY, yh.S420, 8, 0)), QY_NOTSUPPORTED))
    p = ok(); p.format = yh.code(yh.SEMI, yh.S420, 17, 1); bad.append((p, QY_NOTSUPPORTED))   # depth 17
    p = ok(); p.format = yh.code(yh.SEMI, yh.S420, 7, 0); bad.append((p, QY_NOTSUPPORTED))
    p = ok(); p.format = yh.code(yh.SEMI, yh.S420, 8, 1); bad.append((p, QY_NOTSUPPORTED))    # depth 8 with msb
    p = ok(); p.format = 0x1000; bad.append((p, QY_NOTSUPPORTED))
    p = ok(); p.format = 4095; bad.append((p, QY_NOTSUPPORTED))
    p = ok(); p.format = code | 0x400; bad.append((p, QY_NOTSUPPORTED))                   # another bit
    p = ok(); p.format = code | 0x2000; bad.append((p, QY_NOTSUPPORTED))
    p = ok(); p.format = yh.code(yh.SEMI, 3, 10, 1); bad.append((p, QY_NOTSUPPORTED))
    p = ok(); p.pitch[0] = 2 * W - 2; bad.append((p, QY_POINTER))                         # a buffer too short for its rows: the pitch below the row
    p = ok(); p.pitch[1] = 2 * W - 2; bad.append((p, QY_POINTER))
    p = ok(); p.plane[1] = None; bad.append((p, QY_POINTER))
    for p, want in bad:
        assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(p), C.byref(outp)) == want, hex(p.format)
        assert nn.value == 0 and lib.QY265EncoderDelayedFrames(h) == 0
    assert sum(1 for _ in open(lib.call_log_path)) == before, "a refused picture enqueued something"
    good = ok()
    for _ in range(2):
        assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(good), C.byref(outp)) == QY_OK
    new = open(lib.call_log_path).read().split("\n")[before:]
    assert sum("ks265_roi_reduce" in l for l in new) == 1, "the pending map went with the first picture that was taken"
    assert sum("ks265_input_convert" in l for l in new) == 2
    lib.QY265EncoderClose(h)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5


@pytest.fixture(scope="module")
def sanitized():
    return build_host_program("yuv_stub_main.c")


@pytest.mark.parametrize("layout,sub", yh.SHAPES, ids=[f"{yh.LAYOUT_NAMES[l]}{yh.SUB_NAMES[s]}" for l, s in yh.SHAPES])
def test_conversion_routine_under_the_sanitizers(sanitized, tmp_path, layout, sub):
    dst_f = str(tmp_path / "dst.bin")
    for w, h in ((8, 2), (24, 6), (520, 10)):
        for depth, msb in ((8, 0), (10, 0), (10, 1), (16, 0)):
            planes = yh.random_planes(np.random.default_rng(w + depth), layout, sub, depth, msb, w, h)
            for front, behind in ((0, 0), (1, 3)):
                bufs, offs, pitches = yh.lay_out(planes, front, behind)   # each buffer ends with its last row's last element
                args = []
                for k, b in enumerate(bufs):
                    f = str(tmp_path / f"p{k}.bin")
                    b.tofile(f)
                    args += [f, offs[k], pitches[k]]
                r = subprocess.run([sanitized, *[str(a) for a in (layout, sub, depth, msb, w, h, dst_f, *args)]], capture_output=True, text=True)
                assert r.returncode == 0, r.stderr[-2000:]
                assert (np.fromfile(dst_f, np.uint8) == yh.to_i420(planes, layout, sub, depth, msb)).all(), (w, h, depth, msb, front)
