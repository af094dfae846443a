"""GPU: pictures in device memory (ks265_enc_encode_device_frame, ks265codec_amd/csrc/input_convert.hip, ks265codec_amd/encoder.py).
  * the conversion kernel equals tests/yuv_convert_ref.py exactly, for every format, both matrices and both ranges, with pitches above the row and odd offsets;
  * host I420 and device I420 / NV12 / RGB(A) pictures give the same stream, byte for byte, in every GOP configuration;
  * the encoder reads in the caller's stream order and the caller's stream waits for the read (a reused tensor, no host synchronisation);
  * refused pictures (host memory, short buffers, short pitches, another device, a handle never enabled) launch nothing and leave the handle usable."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import yuv_convert_ref as ref  # noqa: E402
from host_harness import YUV  # noqa: E402  (YUV, HostPicture: the GPU modules that share this one's sessions import them from here too)
from host_harness import Picture as HostPicture  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")
QY_OK, QY_POINTER, QY_NOTSUPPORTED = 0, -0x7FFFFFFD, -0x7FFFFFFC


class InDesc(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


def _clip(W, H, n, seed=11):
    from ks265codec_amd.synth import make_clip
    return make_clip(W, H, n, seed=seed, abc=(37, 53, 19), pan=(5, 3))


def _rgb_of(clip_frame, W, H, t):
    """an RGB picture with structure in all three channels, derived from an I420 test picture"""
    y = clip_frame[:W * H].reshape(H, W).astype(np.int16)
    u = np.repeat(np.repeat(clip_frame[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), 2, 0), 2, 1).astype(np.int16)
    v = np.repeat(np.repeat(clip_frame[W * H * 5 // 4:].reshape(H // 2, W // 2), 2, 0), 2, 1).astype(np.int16)
    r = np.clip(y + 2 * (v - 128) + 7 * t, 0, 255).astype(np.uint8)
    g = np.clip(255 - y + (u - 128), 0, 255).astype(np.uint8)
    b = np.clip((y * 3) // 4 + 3 * (u - 128) - 5 * t, 0, 255).astype(np.uint8)
    r[:8, :64] = 255; g[:8, :64] = 0; b[:8, :64] = 0                                  # saturated primaries
    r[8:16, :64] = 0; g[8:16, :64] = 255; b[8:16, :64] = 0
    r[16:24, :64] = 0; g[16:24, :64] = 0; b[16:24, :64] = 255
    r[24:26, :] = g[24:26, :] = b[24:26, :] = np.linspace(0, 255, W).astype(np.uint8)   # a ramp
    return r, g, b


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nv12(frame, W, H):
    u = frame[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
    v = frame[W * H * 5 // 4:].reshape(H // 2, W // 2)
    uv = np.empty((H // 2, W), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return np.concatenate([frame[:W * H].reshape(H, W), uv])


# ------------------------------------------------------------------ the kernel alone

@pytest.fixture(scope="module")
def hip():
    from ks265codec_amd.lib import load_library
    lib = load_library()
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    yield lib, h
    lib.ks265_destroy(h)


def _convert(hip, desc: InDesc, W, H):
    lib, h = hip
    dst = torch.full((W * H * 3 // 2,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = lib.ks265_input_convert(h, C.byref(desc), C.c_void_p(dst.data_ptr()))
    assert rc == 0, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    return dst.cpu().numpy()


def _place(planes, rows_pitch, offset):
    """planes (list of 2-D uint8 arrays) into one device buffer at `offset`, each row `rows_pitch[k]` bytes apart; returns the buffer and the planes' addresses"""
    sizes = [p.shape[0] * rows_pitch[k] for k, p in enumerate(planes)]
    buf = np.full(offset + sum(sizes) + 64, 0x3C, np.uint8)
    addr, o = [], offset
    for k, p in enumerate(planes):
        view = buf[o:o + sizes[k]].reshape(p.shape[0], rows_pitch[k])
        view[:, :p.shape[1]] = p
        addr.append(o)
        o += sizes[k]
    d = _dev(buf)
    return d, [d.data_ptr() + a for a in addr]


LAYOUTS = [(0, 0), (3, 13), (1, 64)]          # (offset into the allocation, bytes of padding behind every row)


@pytest.mark.parametrize("W,H", [(416, 240), (1920, 1080), (3840, 2160)])
def test_yuv_formats_exact(hip, W, H):
    fr = _clip(W, H, 1, seed=W)[0]
    for off, pad in LAYOUTS:
        y = fr[:W * H].reshape(H, W); u = fr[W * H:W * H * 5 // 4].reshape(H // 2, W // 2); v = fr[W * H * 5 // 4:].reshape(H // 2, W // 2)
        d = InDesc(); d.format, d.width, d.height = 0, W, H
        buf, addr = _place([y, u, v], [W + pad, W // 2 + pad + 5, W // 2 + pad + 3], off)
        for k in range(3):
            d.plane[k] = addr[k]
        d.pitch[0], d.pitch[1], d.pitch[2] = W + pad, W // 2 + pad + 5, W // 2 + pad + 3
        assert (_convert(hip, d, W, H) == fr).all(), ("i420", off, pad)
        nv = _nv12(fr, W, H)
        d = InDesc(); d.format, d.width, d.height = 1, W, H
        buf, addr = _place([nv[:H], nv[H:]], [W + pad, W + pad + 7], off)
        d.plane[0], d.plane[1] = addr
        d.pitch[0], d.pitch[1] = W + pad, W + pad + 7
        assert (_convert(hip, d, W, H) == fr).all(), ("nv12", off, pad)


@pytest.mark.parametrize("W,H", [(416, 240), (1920, 1080), (3840, 2160)])
def test_rgb_formats_exact(hip, W, H):
    rng = np.random.default_rng(W)
    clip = _clip(W, H, 1, seed=H)
    r, g, b = _rgb_of(clip[0], W, H, 3)
    noise = rng.integers(0, 256, (3, H, W // 2), dtype=np.uint8)       # the right half: random pixels
    r[:, W // 2:], g[:, W // 2:], b[:, W // 2:] = noise
    for matrix in (ref.MATRIX_BT709, ref.MATRIX_BT601):
        for full in (0, 1):
            exp = ref.rgb_to_i420(r, g, b, matrix, bool(full))
            for off, pad in LAYOUTS:
                for name, step, order in (("rgb24", 3, (0, 1, 2)), ("rgba", 4, (0, 1, 2)), ("bgra", 4, (2, 1, 0)), ("planar", 1, None)):
                    d = InDesc(); d.format, d.width, d.height, d.pixel_step, d.matrix, d.full_range = 2, W, H, step, matrix, full
                    if order is None:
                        buf, addr = _place([r, g, b], [W + pad] * 3, off)
                        for k in range(3):
                            d.plane[k] = addr[k]
                    else:
                        px = np.full((H, W, step), 255, np.uint8)
                        for k in range(3):
                            px[:, :, order[k]] = (r, g, b)[k]
                        buf, addr = _place([px.reshape(H, W * step)], [W * step + pad], off)
                        for k in range(3):
                            d.plane[k] = addr[0] + order[k]
                    d.pitch[0] = (W * step if order is not None else W) + pad
                    got = _convert(hip, d, W, H)
                    assert (got == exp).all(), (name, matrix, full, off, pad, int((got != exp).sum()))


# small and ragged shapes: 8x2 (one thread), 24x6 and 200x134 (widths that are no multiple of 16: the 8-column kernel; H / 2 no multiple of the block's 4 rows), 1032x18 (129
# threads per row: a third block of which one thread works)
SMALL = [(8, 2), (24, 6), (200, 134), (1032, 18)]
SLACK = 256


def _convert_guarded(hip, desc: InDesc, W, H):
    """_convert into a destination SLACK bytes larger than the picture: the 0xA5 canary beyond W * H * 3 / 2 must be intact"""
    lib, h = hip
    n = W * H * 3 // 2
    dst = torch.full((n + SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = lib.ks265_input_convert(h, C.byref(desc), C.c_void_p(dst.data_ptr()))
    assert rc == 0, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    assert (out[n:] == 0xA5).all(), f"{int((out[n:] != 0xA5).sum())} bytes written beyond the picture"
    return out[:n]


@pytest.mark.parametrize("W,H", SMALL)
def test_yuv_formats_exact_at_small_and_ragged_shapes(hip, W, H):
    from adversarial_clips import FAMILIES, make_adversarial
    for kind in FAMILIES:
        fr = make_adversarial(kind, W, H, 2, seed=W)[1]
        for off, pad in LAYOUTS:
            y = fr[:W * H].reshape(H, W); u = fr[W * H:W * H * 5 // 4].reshape(H // 2, W // 2); v = fr[W * H * 5 // 4:].reshape(H // 2, W // 2)
            d = InDesc(); d.format, d.width, d.height = 0, W, H
            buf, addr = _place([y, u, v], [W + pad, W // 2 + pad + 5, W // 2 + pad + 3], off)
            for k in range(3):
                d.plane[k] = addr[k]
            d.pitch[0], d.pitch[1], d.pitch[2] = W + pad, W // 2 + pad + 5, W // 2 + pad + 3
            assert (_convert_guarded(hip, d, W, H) == fr).all(), (kind, "i420", off, pad)
            nv = _nv12(fr, W, H)
            d = InDesc(); d.format, d.width, d.height = 1, W, H
            buf, addr = _place([nv[:H], nv[H:]], [W + pad, W + pad + 7], off)
            d.plane[0], d.plane[1] = addr
            d.pitch[0], d.pitch[1] = W + pad, W + pad + 7
            assert (_convert_guarded(hip, d, W, H) == fr).all(), (kind, "nv12", off, pad)


def _rgb_inputs(W, H):
    """(name, R, G, B): the eight corners of the RGB cube in columns (saturated primaries, black, white) with rows alternating between a corner and its complement; the
    adversarial families' luma planes as the three channels"""
    from adversarial_clips import make_adversarial
    lum = lambda kind, t=0: np.ascontiguousarray(make_adversarial(kind, W, H, 2, seed=H)[t][:W * H].reshape(H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    corner = (xx + (yy & 1) * 7) & 7
    cube = [((corner >> b & 1) * 255).astype(np.uint8) for b in range(3)]
    return [("cube", *cube), ("cb1 / noise / bnoise", lum("cb1_flip"), lum("noise"), lum("bnoise_pan")), ("flat / edge / cb8", lum("flat_flip", 1), lum("edge_ramp"), lum("cb8_shift", 1)),
            ("noise", lum("noise"), lum("noise", 1), 255 - lum("noise"))]


@pytest.mark.parametrize("W,H", SMALL)
def test_rgb_formats_exact_at_small_and_ragged_shapes(hip, W, H):
    for label, r, g, b in _rgb_inputs(W, H):
        for matrix in (ref.MATRIX_BT709, ref.MATRIX_BT601):
            for full in (0, 1):
                exp = ref.rgb_to_i420(r, g, b, matrix, bool(full))
                for off, pad in LAYOUTS:
                    for name, step, order in (("rgb24", 3, (0, 1, 2)), ("rgba", 4, (0, 1, 2)), ("bgra", 4, (2, 1, 0)), ("planar", 1, None)):
                        d = InDesc(); d.format, d.width, d.height, d.pixel_step, d.matrix, d.full_range = 2, W, H, step, matrix, full
                        if order is None:
                            buf, addr = _place([r, g, b], [W + pad] * 3, off)
                            for k in range(3):
                                d.plane[k] = addr[k]
                        else:
                            px = np.full((H, W, step), 255, np.uint8)
                            for k in range(3):
                                px[:, :, order[k]] = (r, g, b)[k]
                            buf, addr = _place([px.reshape(H, W * step)], [W * step + pad], off)
                            for k in range(3):
                                d.plane[k] = addr[0] + order[k]
                        d.pitch[0] = (W * step if order is not None else W) + pad
                        got = _convert_guarded(hip, d, W, H)
                        assert (got == exp).all(), (label, name, matrix, full, off, pad, int((got != exp).sum()))


# ------------------------------------------------------------------ the encoder

def _open(lib, W, H, params, latency=b"default"):
    cfg = (C.c_uint8 * 4096)()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, latency) == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("threads", 8), ("psnr", 1), *params):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0, k
    err = C.c_int(0)
    h = lib.QY265EncoderOpen(cfg, C.byref(err))
    assert h, hex(err.value & 0xFFFFFFFF)
    return h


def encode(W, H, pictures, params=(), latency=b"default", env=None, recon=None, before=None):
    """pictures: numpy I420 frames (host input) or (format, tensor, matrix, full_range) (device input, torch's current stream); the stream's bytes"""
    from ks265codec_amd.encoder import Nal, describe, library
    lib = library()
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update({k: str(v) for k, v in (env or {}).items()})
    try:
        h = _open(lib, W, H, params, latency)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    if recon:
        assert lib.ks265_enc_set_recon_file(C.c_void_p(h), str(recon).encode()) == 0
    if any(not isinstance(p, np.ndarray) for p in pictures):
        assert lib.ks265_enc_enable_device_input(h) == QY_OK
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
        if before:
            before(t)
        if isinstance(p, np.ndarray):
            for k, off in enumerate((0, W * H, W * H * 5 // 4)):
                yuv.pData[k] = C.cast(p.ctypes.data + off, C.POINTER(C.c_ubyte))
            pic.pts = t
            rc = lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.addressof(pic), C.addressof(outp), 0)
        else:
            dp = describe(p[1], p[0], p[2], p[3])
            dp.pts = t
            rc = lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(dp), C.addressof(outp))
        assert rc == QY_OK, (t, hex(rc & 0xFFFFFFFF))
        take()
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == QY_OK
        take()
    lib.QY265EncoderClose(h)
    return bytes(bs)


def _md5(b):
    return hashlib.md5(b).hexdigest()


CONFIGS = {
    "ippp": dict(params=(("rc", 0), ("qp", 30), ("iper", 128), ("bframes", 0))),
    "default_gop": dict(params=(("rc", 0), ("qp", 30), ("iper", 128))),
    "crf_cutree_aq": dict(params=(("rc", 3), ("crf", 24), ("bframes", 3), ("iper", 128), ("aq", 1))),
    "two_lanes": dict(params=(("rc", 0), ("qp", 30), ("iper", 32), ("bframes", 0)), env={"KS265_GOP_LANES": "2"}),
    "zerolatency": dict(params=(("rc", 0), ("qp", 30), ("iper", 128), ("bframes", 0)), latency=b"zerolatency"),
}


@pytest.mark.parametrize("cfg,W,H,n", [(c, 416, 240, 70 if c == "two_lanes" else 26) for c in CONFIGS] + [("default_gop", 1920, 1080, 12), ("default_gop", 3840, 2160, 40)])
def test_device_input_writes_the_host_input_stream(cfg, W, H, n):
    clip = _clip(W, H, min(n, 12), seed=n + W)
    frames = [clip[t % len(clip)] for t in range(n)]
    kw = CONFIGS[cfg]
    host = encode(W, H, frames, **kw)
    assert len(host) > 1000
    dev_i420 = [("i420", _dev(f).view(H * 3 // 2, W), 0, 0) for f in clip]
    assert _md5(encode(W, H, [dev_i420[t % len(clip)] for t in range(n)], **kw)) == _md5(host), "device I420"
    dev_nv12 = [("nv12", _dev(_nv12(f, W, H)), 0, 0) for f in clip]
    assert _md5(encode(W, H, [dev_nv12[t % len(clip)] for t in range(n)], **kw)) == _md5(host), "device NV12"


def test_rgb_pictures_write_the_stream_of_their_reference_conversion(tmp_path):
    W, H, n = 416, 240, 14
    clip = _clip(W, H, n, seed=5)
    rgb = [_rgb_of(clip[t], W, H, t) for t in range(n)]
    kw = dict(params=(("rc", 0), ("qp", 27), ("iper", 128)))
    for matrix, full in ((ref.MATRIX_BT709, 0), (ref.MATRIX_BT601, 1)):
        host = encode(W, H, [ref.rgb_to_i420(*c, matrix, bool(full)) for c in rgb], recon=tmp_path / "host_rec.yuv", **kw)   # (the dump keeps key pictures on the main stream: both sides alike)
        rgba = [_dev(np.stack([*c, np.full_like(c[0], 255)], axis=2)) for c in rgb]
        bgra = [_dev(np.stack([c[2], c[1], c[0], np.full_like(c[0], 9)], axis=2)) for c in rgb]
        planar = [_dev(np.stack(c)) for c in rgb]
        rec = tmp_path / f"rec{matrix}.yuv"
        a = encode(W, H, [("rgba", x, matrix, full) for x in rgba], recon=rec, **kw)
        assert _md5(a) == _md5(host), "RGBA"
        assert _md5(encode(W, H, [("bgra", x, matrix, full) for x in bgra], **kw)) == _md5(host), "BGRA"
        assert _md5(encode(W, H, [("rgb_planar", x, matrix, full) for x in planar], **kw)) == _md5(host), "planar RGB"
        if os.path.exists(REF_DEC):
            bsf, dec = tmp_path / f"a{matrix}.265", tmp_path / f"dec{matrix}.yuv"
            bsf.write_bytes(a)
            d = subprocess.run([REF_DEC, "-b", str(bsf), "-o", str(dec), "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
            assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
            assert np.fromfile(dec, np.uint8).tobytes() == rec.read_bytes()


def test_reads_in_the_callers_stream_order():
    """each picture made by torch ops on a non-default stream into ONE reused tensor, encoded, and at once overwritten on that stream - no host synchronisation"""
    from ks265codec_amd.encoder import Encoder
    W, H, n = 416, 240, 20
    clip = _clip(W, H, n, seed=9)
    rgb = [_rgb_of(clip[t], W, H, t) for t in range(n)]
    host = encode(W, H, [ref.rgb_to_i420(*c) for c in rgb], params=(("rc", 0), ("qp", 27), ("iper", 128), ("bframes", 0)))
    src = [_dev(np.stack([*c, np.zeros_like(c[0])], axis=2)).to(torch.int16) for c in rgb]   # made on the default stream
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    buf = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    work = torch.empty((H, W, 4), dtype=torch.int16, device="cuda")
    out = bytearray()
    enc = Encoder(W, H, "slow", rc=0, qp=27, iper=128, bframes=0, threads=8, fr=50)
    with torch.cuda.stream(s):
        for t in range(n):
            torch.mul(src[t], 3, out=work)                    # a few kernels of the caller's own on its stream
            work.sub_(src[t]).sub_(src[t]).add_(1).sub_(1)
            buf.copy_(work)
            out += enc.encode(buf, "rgba")
            buf.fill_(0x77)                                   # overwritten at once, on the same stream
            work.fill_(0)
        out += enc.flush()
    enc.close()
    torch.cuda.synchronize()
    assert _md5(bytes(out)) == _md5(host)


def test_wrapper_equals_the_c_api():
    from ks265codec_amd.encoder import Encoder
    W, H, n = 416, 240, 12
    clip = _clip(W, H, n, seed=3)
    tens = [_dev(_nv12(f, W, H)) for f in clip]
    c_api = encode(W, H, [("nv12", x, 0, 0) for x in tens], params=(("rc", 0), ("qp", 27), ("iper", 128)))
    with Encoder(W, H, "slow", rc=0, qp=27, iper=128, threads=8, fr=50, psnr=1) as enc:
        out = b"".join(enc.encode(x, "nv12") for x in tens) + enc.flush()
    assert out == c_api == encode(W, H, list(clip), params=(("rc", 0), ("qp", 27), ("iper", 128)))


def test_refused_pictures_launch_nothing_and_leave_the_handle_usable():
    from ks265codec_amd.encoder import DevPicture, Nal, describe, library
    from ks265codec_amd.lib import load_library
    lib, hl = library(), load_library()
    W, H, n = 416, 240, 8
    clip = _clip(W, H, n, seed=4)
    tens = [_dev(_nv12(f, W, H)) for f in clip]
    params = (("rc", 0), ("qp", 30), ("iper", 128), ("bframes", 0))
    nal, nn, outp = C.POINTER(Nal)(), C.c_int(0), HostPicture()

    h = _open(lib, W, H, params)                                          # never enabled
    assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(describe(tens[0], "nv12")), C.addressof(outp)) == QY_NOTSUPPORTED
    lib.QY265EncoderClose(h)

    ctx = C.c_void_p()
    assert hl.ks265_create(C.byref(ctx), 0) == 0
    pitch = 4096                                                           # allocations of whole pages: their ends are where the test puts them
    short, ok_y, ok_uv = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for p, nb in ((short, pitch * (H - 1)), (ok_y, pitch * H), (ok_uv, pitch * H // 2)):
        assert hl.ks265_dev_malloc(ctx, C.byref(p), C.c_size_t(nb)) == 0
        assert hl.ks265_memset_async(ctx, p, 128, C.c_size_t(nb)) == 0
    assert hl.ks265_synchronize(ctx) == 0
    host_buf = np.zeros(W * H * 3 // 2, np.uint8)

    def pic(y, uv, py=pitch, device=0):
        d = DevPicture(); d.format, d.device = 1, device
        d.plane[0], d.plane[1], d.pitch[0], d.pitch[1] = y, uv, py, pitch
        d.stream = torch.cuda.current_stream().cuda_stream
        return d
    refusals = [
        (pic(host_buf.ctypes.data, host_buf.ctypes.data + W * H, W), QY_POINTER),          # host memory
        (pic(short.value, ok_uv.value), QY_POINTER),                                     # one row short of pitch x height
        (pic(ok_y.value, ok_uv.value, py=W - 1), QY_POINTER),                            # pitch below the row
        (pic(ok_y.value, ok_uv.value, device=1), QY_NOTSUPPORTED),                       # another device ordinal
    ]
    h = _open(lib, W, H, params)
    assert lib.ks265_enc_enable_device_input(h) == QY_OK
    bs = bytearray()
    for t in range(n):
        for d, want in refusals:
            assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(d), C.addressof(outp)) == want
        if t == 1:                                                        # the extent exactly at the end of its allocations is taken (and encoded)
            d = pic(ok_y.value, ok_uv.value)
        else:
            d = describe(tens[t], "nv12")
        d.pts = t
        assert lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(d), C.addressof(outp)) == QY_OK
        if t == 0:
            assert lib.ks265_enc_enable_device_input(h) == QY_NOTSUPPORTED  # after the first picture
        bs += b"".join(C.string_at(nal[i].pPayload, nal[i].iSize) for i in range(nn.value))
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == QY_OK
        bs += b"".join(C.string_at(nal[i].pPayload, nal[i].iSize) for i in range(nn.value))
    lib.QY265EncoderClose(h)
    for p in (short, ok_y, ok_uv):
        hl.ks265_dev_free(ctx, p)
    hl.ks265_destroy(ctx)
    grey = np.full(W * H * 3 // 2, 128, np.uint8)
    assert bytes(bs) == encode(W, H, [clip[0], grey] + list(clip[2:]), params=params), "the refusals left the stream as it is without them"
