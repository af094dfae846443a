"""CPU: `roi` (include/ks265_enc.h: a map of quantiser offsets per picture, from host or device memory) in the encoder host, against the stand-in of the device library
WITH the ROI entries (tests/hip_stub_roi.c), 128x72 and 200x136, a different map per display index so that a mix-up shows:
  * every picture's QP map (KS265_DUMP_QPMAP) is tests/roi_map_ref.py applied to the map handed in with that display index - default GOP, -bframes 0, -bframes 3, zero latency;
    pictures with and without a map mixed, a map set and withdrawn, a flush call in between, a key request in mid-stream; one and two GOP lanes give the same bytes;
  * with -rc 3 (cuTree) and with -aq 1 an all-zero map gives the maps and the stream of the run with no map ever set, and an integer constant c moves every CTU's delta by c
    wherever neither delta meets the +-12 clip;
  * with the switch off the scheduler thread's calls are the pinned ones (tests/golden/submit_order.json) - not one call added;
  * against the stand-in WITHOUT the entries (tests/hip_stub.c): one "unavailable" line, ks265_enc_set_next_roi is QY_NOTSUPPORTED, the stream is the plain one."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import roi_map_ref as R
from cutree_mirror import read_qpmap_dump
from host_harness import (LOG_CB, QY_NOTSUPPORTED, QY_OK, QY_POINTER, ROOT, Nal, Picture, Roi, YUV, build_host_lib, digest, load_host_lib, open_handle, scheduler_trace,
                          submit_order_cases)

REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")
SIZES = [(128, 72), (200, 136)]


@pytest.fixture(scope="module")
def roi_lib():
    return load_host_lib(build_host_lib("hip_stub_roi.c"))


@pytest.fixture(scope="module")
def plain_lib():
    return load_host_lib(build_host_lib("hip_stub.c"))


_CLIPS = {}


def clip(W, H):
    if (W, H) not in _CLIPS:
        _CLIPS[W, H] = np.random.default_rng(W).integers(0, 256, (13, W * H * 3 // 2), dtype=np.uint8)
    return _CLIPS[W, H]


def map_of(t: int, W: int, H: int):
    """the map of display index t: (array, log2_block, device) or None - int8 at 16 x 16 from host memory, a per-pixel float32 with a padded pitch from host memory, an int8 at
    8 x 8 from "device" memory (the stand-in's is the process's own), none"""
    rng = np.random.default_rng(1000 + t)
    kind = t % 4
    if kind == 3:
        return None
    lb = (4, 0, 3)[kind]
    rows, cols = R.map_shape(W, H, lb)
    if kind == 1:
        full = np.zeros((rows, cols + 3), np.float32)
        full[:, :cols] = (rng.standard_normal((rows, cols)) * 6 + (t % 7 - 3)).astype(np.float32)
        return full[:, :cols], lb, -1
    m = rng.integers(-11, 12, (rows, cols)).astype(np.int8)
    m[:, : cols // 2] += np.int8(t % 5 - 2)
    return m, lb, (0 if kind == 2 else -1)


def describe(m, lb, device):
    r = Roi()
    r.type, r.log2_block, r.device, r.data, r.pitch, r.stream = (R.INT8 if m.dtype == np.int8 else R.FLOAT32), lb, device, m.ctypes.data, m.strides[0], None
    return r


def run(lib, W, H, n, params=(), latency=b"default", env=None, roi=None, maps=map_of, dump=None, key_at=(), withdraw_at=(), flush_at=(), rc=0):
    """one session, maps(t, W, H) handed in with display index t.  Returns the stream and the log"""
    lines = []
    cb = LOG_CB(lambda m: lines.append(m.decode()))
    lib.QY265SetLogPrintf(cb)
    env = dict(env or {})
    if dump:
        if os.path.exists(dump):
            os.remove(dump)
        env["KS265_DUMP_QPMAP"] = str(dump)
    h = open_handle(lib, W, H, params=(("rc", rc), *params), latency=latency, env=env, roi=bool(roi))
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    bs = bytearray()
    src = clip(W, H)

    def collect():
        bs.extend(b"".join(C.string_at(nal[i].pPayload, nal[i].iSize) for i in range(nn.value) if nal[i].iSize > 0))

    for t in range(n):
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(src[t % len(src)].ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = 1000 + t
        m = maps(t, W, H) if maps else None
        if t in withdraw_at:                                                # another picture's map is set and withdrawn again: this picture goes in with its own (or none)
            other = map_of(4 * t + 1, W, H)
            assert lib.ks265_enc_set_next_roi(h, C.byref(describe(*other))) == QY_OK
            assert lib.ks265_enc_set_next_roi(h, None) == QY_OK
        if m is not None:
            keep = m[0]
            assert lib.ks265_enc_set_next_roi(h, C.byref(describe(*m))) == QY_OK
        if t in flush_at:                                                   # a flush call between the map and its picture does not consume the map
            assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == QY_OK
            collect()
        if t in key_at:
            lib.QY265EncoderKeyFrameRequest(h)
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == QY_OK
        collect()
        if m is not None:
            keep[:] = 99 if keep.dtype == np.int8 else np.float32("nan")   # the map is the caller's again once the call has returned (the stand-in runs everything inside the call)
    while lib.QY265EncoderDelayedFrames(h) > 0:
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == QY_OK
        collect()
    lib.QY265EncoderClose(h)
    lib.QY265SetLogPrintf(None)
    return bytes(bs), "".join(lines)


def expected(t, W, H, qp, maps=map_of, lo=0, hi=51):
    m = maps(t, W, H) if maps else None
    cols, rows = (W + 63) // 64, (H + 63) // 64
    rec = R.reduce(np.ascontiguousarray(m[0]), W, H, m[1]) if m is not None else None
    return R.ctu_map(rec, None, 0, 0, 4, cols, rows, qp, lo, hi)


def check_dump(dump, n, W, H, maps=map_of):
    got = read_qpmap_dump(str(dump))
    assert sorted(got) == list(range(n)), "one record per picture"
    flat = 0
    for d in range(n):
        kind, qp, qm = got[d]
        exp = expected(d, W, H, qp, maps)
        assert (qm == exp).all(), (d, kind, qp, qm.tolist(), exp.tolist())
        flat += int(qm.max() == qm.min())
    return got, flat


def decodes(tmp_path, bs, n, W, H):
    if not os.path.exists(REF_DEC):
        return
    (tmp_path / "d.265").write_bytes(bs)
    d = subprocess.run([REF_DEC, "-b", "d.265", "-o", "d.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
    assert os.path.getsize(tmp_path / "d.yuv") == n * W * H * 3 // 2


GOPS = {
    "default_gop": dict(params=(("iper", 32),)),
    "ippp": dict(params=(("iper", 32), ("bframes", 0))),
    "bframes3": dict(params=(("iper", 32), ("bframes", 3))),
    "zerolatency": dict(params=(("iper", 32), ("bframes", 0)), latency=b"zerolatency"),
}


@pytest.mark.parametrize("size", SIZES, ids=["128x72", "200x136"])
@pytest.mark.parametrize("gop", list(GOPS))
def test_every_pictures_map_is_the_spec_of_the_map_handed_in_with_it(roi_lib, tmp_path, gop, size):
    W, H = size
    n = 41
    kw = dict(GOPS[gop], env={"KS265_GOP_LANES": "1"})
    dump = tmp_path / "qp.bin"
    bs, log = run(roi_lib, W, H, n, roi=1, dump=dump, withdraw_at=(5, 7), flush_at=(10, 11), **kw)
    assert "unavailable" not in log
    got, flat = check_dump(dump, n, W, H)
    assert flat < n // 2, "the maps are not flat: the offsets reached the pictures"
    if gop in ("default_gop", "bframes3"):
        assert {k for k, _, _ in got.values()} == {"I", "P", "B"}
    decodes(tmp_path, bs, n, W, H)
    # a map moves the stream; the switch alone (no map ever set) costs cu_qp_delta's bits and gives flat maps
    none, _ = run(roi_lib, W, H, n, roi=1, maps=None, dump=dump, **kw)
    got0, flat0 = check_dump(dump, n, W, H, maps=None)
    assert flat0 == n and none != bs
    off, log_off = run(roi_lib, W, H, n, maps=None, dump=dump, **kw)
    assert not os.path.exists(dump) or os.path.getsize(dump) == 0, "switch off: no QP per CTU"
    assert off != none and "ROI" not in log_off


@pytest.mark.parametrize("size", SIZES, ids=["128x72", "200x136"])
def test_one_and_two_lanes_give_the_same_bytes(roi_lib, size):
    W, H = size
    kw = dict(n=100, params=(("iper", 32), ("bframes", 0)), roi=1)
    one, _ = run(roi_lib, W, H, env={"KS265_GOP_LANES": "1"}, **kw)
    two, log = run(roi_lib, W, H, env={"KS265_GOP_LANES": "2"}, **kw)
    assert "2 GOP lanes" in log and one == two and len(one) > 1000
    kw = dict(n=70, params=(("iper", 32),), roi=1)
    two, log = run(roi_lib, W, H, env={"KS265_GOP_LANES": "2"}, **kw)
    assert "2 GOP lanes" in log and run(roi_lib, W, H, env={"KS265_GOP_LANES": "1"}, **kw)[0] == two


@pytest.mark.parametrize("lanes", [1, 2])
def test_key_request_in_mid_stream(roi_lib, tmp_path, lanes):
    W, H, n = 200, 136, 50
    kw = dict(params=(("iper", 32), ("bframes", 0)), roi=1, key_at=(13,))
    if lanes == 1:
        dump = tmp_path / "qp.bin"
        bs, _ = run(roi_lib, W, H, n, env={"KS265_GOP_LANES": "1"}, dump=dump, **kw)
        got, _ = check_dump(dump, n, W, H)
        assert [d for d in got if got[d][0] == "I"] == [0, 13, 45]
        decodes(tmp_path, bs, n, W, H)
    else:
        assert run(roi_lib, W, H, n, env={"KS265_GOP_LANES": "2"}, **kw)[0] == run(roi_lib, W, H, n, env={"KS265_GOP_LANES": "1"}, **kw)[0]


def zero_map(t, W, H):
    rows, cols = R.map_shape(W, H, 4)
    return np.zeros((rows, cols), np.int8), 4, -1


CONST = 3


def const_map(t, W, H):
    rows, cols = R.map_shape(W, H, 2)
    return np.full((rows, cols), CONST, np.float32), 2, 0


BASES = {
    "cutree": dict(rc=3, params=(("crf", 30), ("bframes", 3), ("iper", 64))),
    "aq": dict(rc=0, params=(("aq", 1), ("aqs", 1.0), ("bframes", 3), ("iper", 64))),
}


@pytest.mark.parametrize("size", SIZES, ids=["128x72", "200x136"])
@pytest.mark.parametrize("base", list(BASES))
def test_on_top_of_the_cutree_and_aq_offsets(roi_lib, tmp_path, base, size):
    W, H = size
    n = 33
    kw = dict(BASES[base], env={"KS265_GOP_LANES": "1"})
    d0, d1, d2 = tmp_path / "none.bin", tmp_path / "zero.bin", tmp_path / "const.bin"
    never, log = run(roi_lib, W, H, n, roi=1, maps=None, dump=d0, **kw)
    assert ("cuTree over a lookahead" in log) == (base == "cutree")
    zero, _ = run(roi_lib, W, H, n, roi=1, maps=zero_map, dump=d1, **kw)
    assert zero == never, "an all-zero map: the stream of the run with no map ever set"
    g0, g1 = read_qpmap_dump(str(d0)), read_qpmap_dump(str(d1))
    assert sorted(g0) == sorted(g1) == list(range(n))
    assert all(g0[d][:2] == g1[d][:2] and (g0[d][2] == g1[d][2]).all() for d in range(n)), "and its maps"
    off, _ = run(roi_lib, W, H, n, maps=None, dump=tmp_path / "off.bin", **kw)
    goff = read_qpmap_dump(str(tmp_path / "off.bin"))
    assert all(goff[d][:2] == g0[d][:2] and (goff[d][2] == g0[d][2]).all() for d in range(n)), "the switch on, no map: the maps of the switch off (ks265_roi_ctu_map == the plain entries)"
    assert off == never, "and its stream"
    const, _ = run(roi_lib, W, H, n, roi=1, maps=const_map, dump=d2, **kw)
    g2 = read_qpmap_dump(str(d2))
    assert sorted(g2) == list(range(n))
    total = ok = spread = 0
    for d in range(n):
        (k0, q0, m0), (k2, q2, m2) = g0[d], g2[d]
        assert (k0, q0) == (k2, q2), "the caller's offsets do not reach the lookahead, the tree or the picture QPs"
        dl0, dl2 = m0.astype(int) - q0, m2.astype(int) - q2
        qual = (np.abs(dl0) < 12) & (np.abs(dl0 + CONST) <= 12)
        assert (dl2[qual] == dl0[qual] + CONST).all(), (d, dl0.tolist(), dl2.tolist())
        total += qual.size; ok += int(qual.sum()); spread = max(spread, int(dl0.max() - dl0.min()))
    assert ok >= 0.9 * total, f"{ok} of {total} CTUs away from the clip"
    assert spread >= 1, "the base offsets are not flat"
    decodes(tmp_path, const, n, W, H)


def test_refusals_leave_nothing_pending(roi_lib, tmp_path):
    W, H, n = 200, 136, 9
    dump = tmp_path / "qp.bin"
    good = map_of(0, W, H)

    lib = roi_lib
    # one handle, driven by hand: every refusal, then a picture - it must be coded without a map
    h = open_handle(lib, W, H, params=(("threads", 2), ("log", 3), ("bframes", 0)), latency=b"zerolatency", env={"KS265_DUMP_QPMAP": dump}, roi=True)
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    src = clip(W, H)
    m, lb, _ = good
    cases = []
    r = describe(m, lb, -1); r.log2_block = 7; cases.append((r, QY_NOTSUPPORTED))
    r = describe(m, lb, -1); r.type = 2; cases.append((r, QY_NOTSUPPORTED))
    r = describe(m, lb, -1); r.pitch = m.shape[1] - 1; cases.append((r, QY_NOTSUPPORTED))
    r = describe(m, lb, 1); cases.append((r, QY_NOTSUPPORTED))                           # another device
    r = describe(m, lb, -1); r.data = None; cases.append((r, QY_POINTER))
    r = describe(m, lb, 0); r.data = None; cases.append((r, QY_POINTER))
    for t, (r, code) in enumerate(cases):
        assert lib.ks265_enc_set_next_roi(h, C.byref(describe(*good))) == QY_OK            # something IS pending - the refusal clears it
        assert lib.ks265_enc_set_next_roi(h, C.byref(r)) == code, t
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(src[t].ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == QY_OK
    assert lib.ks265_enc_set_next_roi(None, None) == QY_POINTER
    lib.QY265EncoderClose(h)
    got = read_qpmap_dump(str(dump))
    assert sorted(got) == list(range(len(cases)))
    assert all(qm.max() == qm.min() == qp for _, qp, qm in got.values()), "every picture behind a refusal was coded without a map"


def test_switch_values_and_environment(roi_lib, tmp_path):
    for v, rc in ((0, 0), (1, 0), (2, -2), (-1, -2), (0, 0)):                  # QY265_PARAM_BAD_VALUE = -2
        assert roi_lib.ks265_enc_set_default(b"roi", C.c_int(v)) == rc, v
    W, H, n = 128, 72, 12
    kw = dict(params=(("iper", 32), ("bframes", 0)))
    dump = tmp_path / "qp.bin"
    run(roi_lib, W, H, n, env={"KS265_ROI": "1", "KS265_GOP_LANES": "1"}, dump=dump, **kw)
    check_dump(dump, n, W, H)
    plain = run(roi_lib, W, H, n, maps=None, **kw)[0]
    # the environment switches it off again: every map is refused, the stream is the plain one
    assert run(roi_lib, W, H, n, roi=1, maps=None, env={"KS265_ROI": "0"}, **kw)[0] == plain
    # refused at open, with one line, the switch then off: lanes on several GPUs
    env = {"KS265_GOP_LANES": "2", "KS265_GPUS": "2"}
    kw2 = dict(n=70, params=(("iper", 32), ("bframes", 0)), maps=None)
    bs, log = run(roi_lib, W, H, roi=1, env=env, **kw2)
    assert bs == run(roi_lib, W, H, env=env, **kw2)[0]
    assert log.count("ks265enc: ROI maps are unavailable: ") == 1 and "several GPUs" in log


@pytest.mark.parametrize("case", ["plain_ippp", "plain_hier8", "no_split_hier8"])
def test_switch_off_the_scheduler_threads_calls_are_the_pinned_ones(tmp_path, case):
    """the stand-in WITH the ROI entries, the switch off: the scheduler thread's calls to the device library are those tests/golden/submit_order.json pins - not one call added"""
    lib = build_host_lib("hip_stub_roi.c", ("KS265_STUB_SSIM",))
    c = submit_order_cases()[case]
    lines = scheduler_trace(lib, c, str(tmp_path / "calls.log"))
    assert len(lines) == c["lines"] and digest(lines) == c["sha256"]
    on = scheduler_trace(lib, dict(c, env=dict(c["env"], KS265_ROI=1)), str(tmp_path / "calls_on.log"))
    assert sum(ln.startswith("ks265_roi_ctu_map ") for ln in on) == c["n"], "and with it on: one map per picture"
    assert not any(ln.startswith(("ks265_aq_ctu_map ", "ks265_qoff_ctu_map ")) for ln in on)


def test_device_library_without_the_entries(plain_lib):
    assert hasattr(plain_lib, "ks265_enc_set_next_roi") and not hasattr(plain_lib, "ks265_roi_reduce")
    W, H = 128, 72
    for kw in (dict(n=40, params=(("iper", 32), ("bframes", 0))), dict(n=100, params=(("iper", 32), ("bframes", 0)), env={"KS265_GOP_LANES": "2"})):
        plain, log0 = run(plain_lib, W, H, maps=None, **kw)
        bs, log = run(plain_lib, W, H, roi=1, maps=None, **kw)
        assert bs == plain and len(plain) > 100
        assert log.count("ks265enc: ROI maps are unavailable: ") == 1 and "unavailable" not in log0
    lib = plain_lib
    h = open_handle(lib, W, H, params=(("log", 3),), roi=True)
    m = map_of(0, W, H)
    assert lib.ks265_enc_set_next_roi(h, C.byref(describe(*m))) == QY_NOTSUPPORTED
    assert lib.ks265_enc_set_next_roi(h, None) == QY_OK
    lib.QY265EncoderClose(h)
