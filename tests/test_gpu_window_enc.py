"""GPU: picture sizes that are no multiple of 8 through the encoder - the C API and Encoder - at 202x134, 480x270 and 854x480, 9 pictures, -rc 0, once with the default GOP and
once with zero latency:
  * the SPS carries the coded size and the conformance window of tests/picture_window_ref.py (854x480: 856x480 and (0, 1, 0, 0), what the reference's encoder writes);
  * every NAL unit but the SPS equals that of a coded-size handle fed the specification's padded clip: nothing downstream of the input slot moved;
  * the -o file holds W x H pictures, the crop of that handle's -o file; where the reference's decoder is staged (oracle/_ref/appdecoder) its output file equals it byte for byte;
  * Encoder: device I420 and NV12 pictures give the host pictures' stream; recon() as i420, and as rgb_planar float16, is the crop of the coded handle's reconstruction, then
    tests/yuv_output_ref.py / tests/yuv_float_ref.py; quality() is numpy's SSE and PSNR of source against cropped reconstruction, from the exact integer sums;
  * reconstructions fetched on TWO streams in turn, the first one busy, are the one-stream pictures (that the second stream's crop waits for the first one's conversion, which
    reads the lane's scratch picture, is pinned call by call in tests/test_window_host_cpu.py: streams that share a hardware queue run in turn anyway);
  * analysis=True and a roi= map at 202x134: arrays of the coded picture's ceil(H / 8) x ceil(W / 8) blocks, equal - like every NAL unit but the SPS - to those of the 208x136
    handle fed the padded clip and the same map;
  * every other format, and scale=, raises ValueError before anything is handed in."""
from __future__ import annotations

import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import picture_window_ref as pw  # noqa: E402
import window_sps as ws  # noqa: E402
import yuv_float_ref as fref  # noqa: E402
from test_gpu_device_input import REF_DEC, encode  # noqa: E402  (the C API session of the device-input tests)

N = 9
PARAMS = (("rc", 0), ("qp", 30), ("iper", 128))
KW = dict(fr=50, threads=8, psnr=1, **dict(PARAMS))
SIZES = [(202, 134), (480, 270), (854, 480)]
MODES = [b"default", b"zerolatency"]


def _clip(w, h, n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        y = np.clip(128 + 80 * np.sin(0.09 * (xx + 3 * t)) * np.cos(0.06 * (yy + 2 * t)) + rng.integers(0, 8, (h, w)), 0, 255).astype(np.uint8)
        u = np.clip(128 + 60 * np.sin(0.04 * (xx[::2, ::2] + yy[::2, ::2] + 2 * t)), 0, 255).astype(np.uint8)
        v = np.clip(128 + 60 * np.cos(0.07 * (xx[::2, ::2] - t)), 0, 255).astype(np.uint8)
        out.append(pw.pack([y, u, v]))
    return out


def _nals(stream: bytes):
    parts = stream.split(b"\x00\x00\x01")[1:]
    return [((p[0] >> 1) & 63, p.rstrip(b"\x00") if i + 1 < len(parts) else p) for i, p in enumerate(parts)]


_cache = {}


def _pair(w, h, mode, tmp):
    """the ragged handle fed the clip and the coded-size handle fed the padded clip, host input, both with -o: (clip, stream, -o pictures, coded stream, coded -o pictures)"""
    key = (w, h, mode)
    if key not in _cache:
        cw, ch = pw.coded_size(w, h)
        src = _clip(w, h, N, seed=w + h)
        padded = [pw.pad_i420(p, w, h) for p in src]
        fr, fc = tmp / f"r{w}{mode.decode()}.yuv", tmp / f"c{w}{mode.decode()}.yuv"
        got = encode(w, h, src, PARAMS, latency=mode, recon=fr)
        exp = encode(cw, ch, padded, PARAMS, latency=mode, recon=fc)
        _cache[key] = (src, got, np.fromfile(str(fr), np.uint8), exp, np.fromfile(str(fc), np.uint8))
    return _cache[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("window")


@pytest.mark.parametrize("mode", MODES, ids=["gop8", "zerolatency"])
@pytest.mark.parametrize("w,h", SIZES)
def test_stream_is_the_coded_handle_s_with_a_window(tmp, w, h, mode):
    cw, ch = pw.coded_size(w, h)
    src, got, rec, exp, rec_c = _pair(w, h, mode, tmp)
    sps = ws.stream_sps(got)
    assert (sps["width"], sps["height"], sps["window"]) == (cw, ch, pw.conf_window(w, h)) and ws.output_size(sps) == (w, h)
    if (w, h) == (854, 480):
        assert (cw, ch, sps["window"]) == (856, 480, (0, 1, 0, 0))       # the reference's own SPS for this size
    assert ws.stream_sps(exp)["flag"] == 0
    g, e = _nals(got), _nals(exp)
    assert len(g) == len(e) and [t for t, _ in g] == [t for t, _ in e] and sum(t < 32 for t, _ in g) == N
    for (t, a), (_, b) in zip(g, e):
        assert (a == b) == (t != ws.NAL_SPS), t
    assert rec.size == N * w * h * 3 // 2 and rec_c.size == N * cw * ch * 3 // 2
    rec, rec_c = rec.reshape(N, -1), rec_c.reshape(N, -1)
    for t in range(N):
        assert (rec[t] == pw.crop_i420(rec_c[t], cw, ch, w, h)).all(), t


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="the reference's decoder was not staged (oracle/_ref/appdecoder)")
@pytest.mark.parametrize("mode", MODES, ids=["gop8", "zerolatency"])
@pytest.mark.parametrize("w,h", SIZES)
def test_reference_decoder_writes_the_window(tmp, tmp_path, w, h, mode):
    _, got, rec, _, _ = _pair(w, h, mode, tmp)
    (tmp_path / "a.265").write_bytes(got)
    d = subprocess.run([REF_DEC, "-b", "a.265", "-o", "d.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
    dec = np.fromfile(str(tmp_path / "d.yuv"), np.uint8)
    assert dec.size == N * w * h * 3 // 2 and (dec == rec).all()


@pytest.mark.parametrize("mode", MODES, ids=["gop8", "zerolatency"])
@pytest.mark.parametrize("w,h", SIZES)
def test_encoder_recon_and_quality(tmp, w, h, mode):
    from ks265codec_amd.encoder import Encoder
    cw, ch = pw.coded_size(w, h)
    src, want, _, _, rec_c = _pair(w, h, mode, tmp)
    crop = [pw.crop_i420(p, cw, ch, w, h) for p in rec_c.reshape(N, -1)]
    dev = [torch.from_numpy(p).cuda().view(h * 3 // 2, w) for p in src]
    with Encoder(w, h, "slow", recon="i420", latency=mode.decode(), **KW) as enc:
        pics, bs = [], bytearray()
        for t in dev:
            bs += enc.encode(t, "i420")
            pics += enc.recon()
        bs += enc.flush()
        pics += enc.recon()
        q = enc.quality()
    assert bytes(bs) == want, "device I420 pictures give the host pictures' stream"
    assert sorted(p for p, _ in pics) == list(range(N))
    for poc, t in pics:
        assert t.shape == (h * 3 // 2, w) and t.dtype == torch.uint8
        assert (t.cpu().numpy().reshape(-1) == crop[poc]).all(), poc
    sse = np.sum([pw.sse3(a, b, w, h) for a, b in zip(src, crop)], axis=0).tolist()
    print("quality", q["sse"], q["psnr"], "numpy", sse)
    assert q["frames"] == N and q["sse"] == [float(s) for s in sse] and all(s > 0 for s in sse)
    for k, npx in enumerate((w * h, w * h // 4, w * h // 4)):
        assert abs(q["psnr"][k] - pw.psnr(sse[k], npx * N)) < 1e-9 and abs(q["psnr"][k] - 10.0 * math.log10(255.0 * 255.0 * npx * N / sse[k])) < 1e-9
    assert q["last"]["sse"] == [float(s) for s in pw.sse3(src[q["last"]["poc"]], crop[q["last"]["poc"]], w, h)]
    if mode != b"default":
        return
    # NV12 in, planar RGB as float16 out
    nv12 = []
    for p in src:
        y, u, v = pw.planes(p, w, h)
        uv = np.empty((h // 2, w), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = u, v
        nv12.append(torch.from_numpy(np.concatenate([y, uv])).cuda())
    with Encoder(w, h, "slow", recon="rgb_planar", recon_dtype=torch.float16, latency=mode.decode(), **KW) as enc:
        pics, bs = [], bytearray()
        for t in nv12:
            bs += enc.encode(t, "nv12")
            pics += enc.recon()
        bs += enc.flush()
        pics += enc.recon()
    assert bytes(bs) == want, "device NV12 pictures give the host pictures' stream"
    assert sorted(p for p, _ in pics) == list(range(N))
    for poc, t in pics:
        assert t.shape == (3, h, w) and t.dtype == torch.float16
        r, g, b = fref.i420_to_rgbf(crop[poc], w, h, fref.IN_RGB_F16)
        assert (t.cpu().numpy() == np.stack([r, g, b])).all(), poc


def test_other_formats_are_refused_before_anything_is_handed_in():
    from ks265codec_amd.encoder import Encoder
    w, h = 202, 134
    with pytest.raises(ValueError, match="scale"):
        Encoder(w, h, "slow", scale="bicubic", **KW)
    with Encoder(w, h, "slow", **KW) as enc:
        rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        for t, fmt, kw in ((rgb, "rgb", {}), (rgb.permute(2, 0, 1).contiguous(), "rgb_planar", {}), (rgb.float(), "rgb", {}),
                           ((torch.zeros((h, w), dtype=torch.int16, device="cuda"), torch.zeros((h // 2, w), dtype=torch.int16, device="cuda")), "nv12", dict(depth=10)),
                           ((torch.zeros((h, w), dtype=torch.uint8, device="cuda"),) * 3, "i444", {})):
            with pytest.raises(ValueError, match="i420 and nv12"):
                enc.encode(t, fmt, **kw)
        with pytest.raises(ValueError, match="picture"):
            enc.encode(torch.zeros((136 * 3 // 2, 208), dtype=torch.uint8, device="cuda"), "i420")          # the coded size is not the handle's size
        assert enc.lib.QY265EncoderDelayedFrames(enc.h) == 0
        y = torch.full((h, w), 90, dtype=torch.uint8, device="cuda")
        c = torch.full((h // 2, w // 2), 128, dtype=torch.uint8, device="cuda")
        bs = enc.encode((y, c, c), "i420") + enc.flush()                # planes with their own strides: the 8-bit 4:2:0 alias
        assert ws.output_size(ws.stream_sps(bs)) == (w, h)


def test_recon_fetched_on_two_streams(tmp):
    """successive ks265_enc_get_device_recon calls may name different streams; on a ragged handle they share the lane's scratch picture, which one event guards"""
    import ctypes as C
    from ks265codec_amd.encoder import Encoder, Picture, QY_OK, describe
    w, h, mode = 202, 134, b"default"
    cw, ch = pw.coded_size(w, h)
    src, want, _, _, rec_c = _pair(w, h, mode, tmp)
    crop = [pw.crop_i420(p, cw, ch, w, h) for p in rec_c.reshape(N, -1)]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    busy, busy_out = torch.rand((8192, 8192), device="cuda"), torch.empty((8192, 8192), device="cuda")
    held = []

    class TwoStreams(Encoder):
        def _fetch(self):
            out, info, k = [], Picture(), 0
            first = self.lib.ks265_enc_device_recon_pending(self.h) >= 2 and not held
            while self.lib.ks265_enc_device_recon_pending(self.h) > 0:
                st = (sa, sb)[k % 2]
                with torch.cuda.stream(st):
                    if first and k == 0:
                        for _ in range(8):                              # stream A: other work in front of its fetch, so that stream B's fetch is enqueued while A's has not run
                            torch.mm(busy, busy, out=busy_out)
                    t = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device="cuda")
                    assert self.lib.ks265_enc_get_device_recon(self.h, C.byref(describe(t, "i420")), C.addressof(info)) == QY_OK
                if first and k == 1:
                    held.append(True)
                out.append((info.poc, t))
                k += 1
            return out

    torch.cuda.synchronize()
    with TwoStreams(w, h, "slow", recon="i420", latency=mode.decode(), **KW) as enc:
        pics, bs = [], bytearray()
        for p in src:
            bs += enc.encode(torch.from_numpy(p).cuda().view(h * 3 // 2, w), "i420")
            pics += enc.recon()
        bs += enc.flush()
        pics += enc.recon()
        torch.cuda.synchronize()
    assert bytes(bs) == want and sorted(p for p, _ in pics) == list(range(N))
    for poc, t in pics:
        assert (t.cpu().numpy().reshape(-1) == crop[poc]).all(), poc
    assert held, "no call handed out two pictures"


def test_analysis_and_roi_describe_coded_and_source_picture():
    from ks265codec_amd.encoder import Encoder
    w, h, n = 202, 134, 5
    cw, ch = pw.coded_size(w, h)
    src = _clip(w, h, n, seed=91)
    padded = [pw.pad_i420(p, w, h) for p in src]
    ctu = np.array([[-6, 0, 4, 8], [3, -3, 6, 0], [5, 5, -4, 2]], np.int8)          # one offset per CTU, as blocks of 16: every block of a CTU equal, so the CTU's mean
    m = np.repeat(np.repeat(ctu, 4, axis=0), 4, axis=1)[:(h + 15) // 16, :(w + 15) // 16].copy()   # does not depend on how much of a block lies inside the picture
    assert m.shape == ((ch + 15) // 16, (cw + 15) // 16) == (9, 13)
    res = []
    for (ew, eh), clip_ in (((w, h), src), ((cw, ch), padded)):
        with Encoder(ew, eh, "slow", analysis=True, roi=True, **KW) as enc:
            bs, an = bytearray(), []
            for t, p in enumerate(clip_):
                bs += enc.encode(torch.from_numpy(p).cuda().view(eh * 3 // 2, ew), "i420", roi=torch.from_numpy(m).cuda() if t & 1 else m, roi_block=16)
                an += enc.analysis()
            bs += enc.flush()
            an += enc.analysis()
            with pytest.raises(ValueError, match="roi"):
                enc.encode(torch.from_numpy(clip_[0]).cuda().view(eh * 3 // 2, ew), "i420", roi=np.zeros((m.shape[0] + 1, m.shape[1]), np.int8), roi_block=16)
        res.append((bytes(bs), an))
    (got, a), (exp, b) = res
    g, e = _nals(got), _nals(exp)
    assert len(g) == len(e) and sum(t < 32 for t, _ in g) == n
    for (t, x), (_, y) in zip(g, e):
        assert (x == y) == (t != ws.NAL_SPS), t
    assert len(a) == len(b) == n and [x["poc"] for x in a] == [x["poc"] for x in b]
    for x, y in zip(a, b):
        assert x["mv"].shape == (2, 17, 26, 2) and x["cu"].shape == (5, 17, 26) and x["sse"].shape == (3, 17, 26) and x["qp"].shape == (3, 4)
        for k in ("mv", "ref", "cu", "qp", "sse"):
            assert torch.equal(x[k], y[k]), (x["poc"], k)
    qps = torch.stack([x["qp"] for x in a]).cpu().numpy()
    assert len(np.unique(qps[0])) > 1, "the map moved no CTU's QP"
