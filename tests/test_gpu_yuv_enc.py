"""GPU: pictures of the YUV family (KS265_IN_YUV, include/ks265_enc.h) through the encoder, 416x240 (the size of the device-input encode tests), 9 pictures:
  * a P010 clip u8 << 8 gives, byte for byte, the stream of the NV12 clip u8 - through ks265_enc_encode_device_frame, through Encoder.encode((y, uv), "nv12", depth=10) and
    with two GOP lanes;
  * an I422 clip whose chroma rows are the I420 clip's, each twice, gives the stream of the I420 clip (the (1, 1) filter of two equal rows is the row);
  * an I444 clip with the I420 clip's chroma replicated 2 x 2 gives the stream of the I420 clip, with one and two lanes.  (The co-sited (1, 2, 1) filter takes a replicated
    row C0 C0 C1 C1 .. at the even columns to (C[i - 1] + 3 C[i] + 2) >> 2, which is C[i] where neighbours differ by at most one code, as in this clip - the test asserts
    that of the clip.  With chroma that moves more the I444 clip gives the stream of the host pictures tests/yuv_hibit_ref.py makes of it, and not the I420 clip's.)
  * a 10-bit clip with every low bit in use - I010 through the scaler too - gives the stream of its reference conversion;
  * describe() writes the planes' own strides in bytes, picks the default alignment by layout, and refuses what the header refuses."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import yuv_hibit_ref as yh  # noqa: E402
import yuv_scale_ref as ys  # noqa: E402
from test_gpu_device_input import QY_OK, HostPicture, YUV, _clip, _nv12, _open  # noqa: E402  (the clip and the handle of the device-input tests)

W, H, N = 416, 240, 9
PARAMS = (("rc", 0), ("qp", 30), ("iper", 128))
LANES = dict(params=(("rc", 0), ("qp", 30), ("iper", 4), ("bframes", 0)), env={"KS265_GOP_LANES": "2"})


def _t(a: np.ndarray) -> torch.Tensor:
    """a plane on the GPU; uint16 travels as int16 (the same words)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def session(pictures, params=PARAMS, env=None, scaled=None):
    """pictures: numpy I420 frames (host input) or (planes, format name, depth, msb) (device input through describe(), torch's current stream); the stream's bytes"""
    from ks265codec_amd.encoder import Nal, describe, library
    lib = library()
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update({k: str(v) for k, v in (env or {}).items()})
    try:
        h = _open(lib, W, H, params)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    if any(not isinstance(p, np.ndarray) for p in pictures):
        assert lib.ks265_enc_enable_device_input(h) == QY_OK
    if scaled:
        assert lib.ks265_enc_enable_device_scale(h, scaled[0], scaled[1]) == QY_OK
    nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    bs = bytearray()

    def take():
        for i in range(nn.value):
            if nal[i].iSize > 0:
                bs.extend(C.string_at(nal[i].pPayload, nal[i].iSize))
    for t, p in enumerate(pictures):
        if isinstance(p, np.ndarray):
            for k, off in enumerate((0, W * H, W * H * 5 // 4)):
                yuv.pData[k] = C.cast(p.ctypes.data + off, C.POINTER(C.c_ubyte))
            pic.pts = t
            rc = lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.addressof(pic), C.addressof(outp), 0)
        else:
            dp = describe(p[0], p[1], depth=p[2], msb=p[3])
            dp.pts = t
            if scaled:
                rc = lib.ks265_enc_encode_device_frame_scaled(h, C.byref(nal), C.byref(nn), C.byref(dp), scaled[0], scaled[1], 1, C.addressof(outp))
            else:
                rc = lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(dp), C.addressof(outp))
        assert rc == QY_OK, (t, hex(rc & 0xFFFFFFFF))
        take()
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == QY_OK
        take()
    lib.QY265EncoderClose(h)
    return bytes(bs)


@pytest.fixture(scope="module")
def clip():
    return _clip(W, H, N, seed=23)                                      # N flat I420 frames


def _yuv(f):
    return f[:W * H].reshape(H, W), f[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), f[W * H * 5 // 4:].reshape(H // 2, W // 2)


def _p010(f):
    """(y, uv) of the frame as P010 words u8 << 8"""
    nv = _nv12(f, W, H).reshape(H * 3 // 2, W).astype(np.uint16) << 8
    return (_t(nv[:H]), _t(nv[H:]))


@pytest.fixture(scope="module")
def streams(clip):
    """the clip's stream from host pictures: one lane, two lanes"""
    one, two = session(list(clip)), session(list(clip), **LANES)
    assert len(one) > 1000 and len(two) > 1000 and one != two
    return one, two


def test_p010_clip_writes_the_stream_of_the_nv12_clip(clip, streams):
    nv12 = [((_t(_nv12(f, W, H).reshape(H * 3 // 2, W)[:H]), _t(_nv12(f, W, H).reshape(H * 3 // 2, W)[H:])), "nv12", None, None) for f in clip]
    assert session(nv12) == streams[0]                                  # the (y, uv) form of NV12 itself
    p010 = [(_p010(f), "nv12", 10, None) for f in clip]
    assert session(p010) == streams[0]
    assert session(p010, **LANES) == streams[1]


def test_p010_through_the_python_encoder(clip, streams):
    from ks265codec_amd.encoder import Encoder
    with Encoder(W, H, "slow", fr=50, threads=8, psnr=1, **dict(PARAMS)) as enc:
        got = b"".join(enc.encode(_p010(f), "nv12", depth=10) for f in clip) + enc.flush()
    assert got == streams[0]
    with Encoder(W, H, "slow", fr=50, threads=8, psnr=1, **dict(PARAMS)) as enc:                     # P016 and P012 read the same words
        got = b"".join(enc.encode(_p010(f), "nv12", depth=16 if t & 1 else 12) for t, f in enumerate(clip)) + enc.flush()
    assert got == streams[0]


def test_i422_of_doubled_rows_writes_the_stream_of_the_i420_clip(clip, streams):
    pics = []
    for f in clip:
        y, u, v = _yuv(f)
        pics.append(((_t(y), _t(np.repeat(u, 2, 0)), _t(np.repeat(v, 2, 0))), "i422", None, None))
    assert session(pics) == streams[0]
    assert session(pics, **LANES) == streams[1]
    yuyv = []
    for f in clip:                                                      # the same pictures packed: Y0 U Y1 V
        y, u, v = _yuv(f)
        p = np.empty((H, 2 * W), np.uint8)
        p[:, 0::2], p[:, 1::4], p[:, 3::4] = y, np.repeat(u, 2, 0), np.repeat(v, 2, 0)
        yuyv.append((_t(p), "yuyv", None, None))
    assert session(yuyv) == streams[0]


def test_i444_of_replicated_chroma_writes_the_stream_of_its_reference_conversion(clip, streams):
    rng = np.random.default_rng(44)
    for rough in (False, True):
        pics, host = [], []
        for f in clip:
            y, u, v = _yuv(f)
            if rough:                                                   # chroma that moves from sample to sample: the filter shows
                u, v = (np.clip(c.astype(np.int16) + rng.integers(-24, 25, c.shape), 0, 255).astype(np.uint8) for c in (u, v))
            planes = [y, np.repeat(np.repeat(u, 2, 0), 2, 1), np.repeat(np.repeat(v, 2, 0), 2, 1)]
            pics.append((tuple(_t(p) for p in planes), "i444", None, None))
            host.append(yh.to_i420(planes, yh.PLANAR, yh.S444, 8))
            assert (host[-1][:W * H] == f[:W * H]).all()
        if not rough:                                                   # the clip's own chroma moves by at most one code between neighbours: the filter gives it back,
            assert all((h == f).all() for h, f in zip(host, clip))      # and the I444 clip writes the stream of the I420 clip
            assert session(pics) == streams[0]
            assert session(pics, **LANES) == streams[1]
        else:
            want = session(host)
            assert len(want) > 1000 and want != streams[0]
            assert session(pics) == want


def test_ten_bit_clips_write_the_stream_of_their_reference_conversion(clip):
    rng = np.random.default_rng(10)
    pics, host = [], []
    for f in clip[:5]:
        y, u, v = _yuv(f)
        planes = [(p.astype(np.uint16) << 2 | rng.integers(0, 4, p.shape).astype(np.uint16)) | (rng.integers(0, 64, p.shape).astype(np.uint16) << 10) for p in (y, u, v)]
        pics.append((tuple(_t(p) for p in planes), "i420", 10, None))   # planar: the low bits by default; the high ones are stray
        host.append(yh.to_i420(planes, yh.PLANAR, yh.S420, 10, 0))
    want = session(host)
    assert len(want) > 1000 and session(pics) == want
    # a source of another size: I010 at 832x480 through the scaler
    SW, SH = 832, 480
    src = [rng.integers(0, 1024, s).astype(np.uint16) for s in ((SH, SW), (SH // 2, SW // 2), (SH // 2, SW // 2))]
    exp = ys.scale_i420(yh.to_i420(src, yh.PLANAR, yh.S420, 10, 0), SW, SH, W, H, 1)
    assert session([(tuple(_t(p) for p in src), "i420", 10, False)], scaled=(SW, SH)) == session([exp])


def test_describe_of_planes():
    from ks265codec_amd.encoder import IN_NV12, describe
    from ks265codec_amd import lib as kl
    big = torch.zeros((H + 4, W + 16), dtype=torch.int16, device="cuda")
    y, uv = big[2:2 + H, 8:8 + W], torch.zeros((H // 2, W), dtype=torch.int16, device="cuda")
    d = describe((y, uv), "nv12", depth=10)
    assert d.format == kl.IN_P010 and d.pitch[0] == 2 * (W + 16) and d.pitch[1] == 2 * W and d.plane[0] == big.data_ptr() + 2 * (2 * (W + 16) + 8) and d.plane[1] == uv.data_ptr()
    assert describe((y, uv), "nv12", depth=10, msb=False).format == kl.in_yuv(1, 0, 10, 0)
    assert describe((y, uv), "nv12", depth=16).format == kl.IN_P016
    c = torch.zeros((H // 2, W // 2), dtype=torch.int16, device="cuda")
    assert describe((y, c, c), "i420", depth=10).format == kl.IN_I010
    assert describe((y, torch.zeros((H, W // 2), dtype=torch.int16, device="cuda"), torch.zeros((H, W // 2), dtype=torch.int16, device="cuda")), "i422", depth=10).format == kl.IN_I210
    assert describe(torch.zeros((H, 2 * W), dtype=torch.int16, device="cuda"), "yuyv", depth=10).format == kl.IN_Y210
    y8 = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    assert describe((y8, torch.zeros((H // 2, W), dtype=torch.uint8, device="cuda")), "nv12").format == IN_NV12
    assert describe((y8, torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")), "nv24").format == kl.IN_NV24
    assert describe(torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda"), "uyvy").format == kl.IN_UYVY
    bad = [((y, uv), "nv12", {}),                                       # words without a depth
           ((y, uv), "nv12", dict(depth=8)), ((y, uv), "nv12", dict(depth=17)),
           ((y8, y8), "nv12", dict(depth=10)), ((y8, torch.zeros((H // 2, W), dtype=torch.uint8, device="cuda")), "nv12", dict(msb=True)),
           ((y, uv), "i420", dict(depth=10)), ((y, c, c), "nv12", dict(depth=10)), ((y, c, c), "i444", dict(depth=10)),
           ((y, uv.cpu()), "nv12", dict(depth=10)), ((y, uv.float()), "nv12", dict(depth=10)), ((y, uv[:, ::2]), "nv12", dict(depth=10)),
           (y, "i422", dict(depth=10)), ((y, uv), "yuyv", dict(depth=10)), (y8, "rgb_planar", dict(depth=8))]
    for t, fmt, kw in bad:
        with pytest.raises(ValueError):
            describe(t, fmt, **kw)
