"""GPU: local contrast on the way in (ks265codec_amd/csrc/input_hdr.hip, `vpp_hdr` of include/ks265_enc.h) against tests/hdr_ref.py.
  * ks265_input_hdr, byte for byte, on every size x cfg x content of tests/hdr_cases.py - the defaults, the corners of every range, the three quoted parameter sets; 8x8
    where every window is cut by the picture, the enhancement's sizes, 1288 samples along either axis (interior tiles with both halos in neighbours), 8192 along either axis.
    Chroma is untouched, guard bytes around the picture and the work buffer stay;
  * refusals enqueue nothing - a sentinel-filled picture and work buffer are unchanged: a bad cfg, a bad size, a misaligned, short or overlapping work buffer, host pointers,
    a pointer whose extent leaves its allocation;
  * end to end, 9 pictures, default GOP, at 208x136 and 202x134 (filtered at 208x136, behind the pad): the stream of Encoder(..., hdr=True) is that of a plain handle fed the
    reference-filtered pictures, through the C API with host pictures as well;
  * scaled input (scale="bicubic" from 416x272) and a float32 RGB input in front of the filter equal convert-then-reference-filter."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import hdr_ref as hr  # noqa: E402
from hdr_cases import CFGS, SIZES, contents as _contents  # noqa: E402
import picture_window_ref as pw  # noqa: E402
import window_sps as ws  # noqa: E402
import yuv_float_ref as fref  # noqa: E402
import yuv_scale_ref as ys  # noqa: E402

SLACK = 256
KS265_POINTER, KS265_NOTSUPPORTED = -3, -4
DEF = hr.params(0, 0, 0, 0)


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


def _guarded(n: int, a=None):
    """a device buffer with 0xA5 guards around n bytes (those of `a`, else 0x3C); (buffer, the view of the bytes)"""
    buf = torch.full((n + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[SLACK:SLACK + n] = torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else 0x3C
    return buf, buf[SLACK:SLACK + n]


def _guards_ok(buf, n):
    b = buf.cpu().numpy()
    return (b[:SLACK] == 0xA5).all() and (b[SLACK + n:] == 0xA5).all()


@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_equals_the_reference(ks, w, h):
    n, nb = w * h * 3 // 2, ks.input_hdr_work_bytes(w, h)
    assert nb == hr.work_bytes(w, h)
    wb, work = _guarded(nb)
    changed = 0
    for name, pic in _contents(w, h, seed=w + h).items():
        for cfg in CFGS:
            exp = hr.hdr_picture(pic, w, h, cfg)
            pb, p = _guarded(n, pic)
            ks.input_hdr(cfg, w, h, p, work)
            ks.sync()
            got = p.cpu().numpy()
            assert _guards_ok(pb, n), "bytes written outside the picture"
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (name, cfg, bad.size, "differ, first at", bad[:8], "got", got[bad[:8]], "expected", exp[bad[:8]], "source", pic[bad[:8]])
            assert (got[w * h:] == pic[w * h:]).all(), "chroma"
            changed += int((exp != pic).sum())
    assert _guards_ok(wb, nb), "bytes written outside the work buffer"
    assert changed > 0, "the cases changed nothing: the filter was not exercised"


def test_refusals_enqueue_nothing(ks):
    w, h = 32, 16
    npx, n, nb = w * h, w * h * 3 // 2, hr.work_bytes(w, h)
    a = torch.full((n + nb + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    pic, work = a[:n], a[n:n + nb]
    host = np.zeros(n + nb, np.uint8)
    assert ks.input_hdr_validate(DEF, w, h) == 0 and ks.input_hdr_validate((16, 2, 8, (484, 242, 99999)), w, h) == 0, "the third radius is not judged at 2 iterations"
    assert ks.input_hdr_work_bytes(20, 16) == 0 and ks.input_hdr_work_bytes(8200, 8) == 0
    r3 = (484, 242, 121)
    bad = [(20, 16, DEF), (32, 12, DEF), (0, 16, DEF), (32, -8, DEF), (8200, 16, DEF), (w, h, (0, 3, 8, r3)), (w, h, (81, 3, 8, r3)), (w, h, (16, 1, 8, r3)), (w, h, (16, 4, 8, r3)),
           (w, h, (16, 3, -1, r3)), (w, h, (16, 3, 4097, r3)), (w, h, (16, 3, 8, (15, 242, 121))), (w, h, (16, 3, 8, (484, 2481, 121))), (w, h, (16, 3, 8, (484, 242, 0))),
           (w, h, (16, 2, 8, (484, -16, 121)))]
    for tw, th, cfg in bad:
        assert ks.input_hdr_validate(cfg, tw, th) == KS265_NOTSUPPORTED, (tw, th, cfg)
        assert ks.input_hdr_rc(cfg, tw, th, pic, work) == KS265_NOTSUPPORTED, (tw, th, cfg)
    assert ks.input_hdr_rc(DEF, w, h, pic, work, nb - 1) == KS265_POINTER, "a work buffer one byte short"
    assert ks.input_hdr_rc(DEF, w, h, pic, a[n - 64:n - 64 + nb]) == KS265_POINTER, "the work buffer overlaps the picture's chroma"
    assert ks.input_hdr_rc(DEF, w, h, a[n + 128:2 * n + 128], work) == KS265_POINTER, "the picture lies inside the work buffer"
    assert ks.input_hdr_rc(DEF, w, h, pic, 0, nb) == KS265_POINTER, "no work buffer"
    assert ks.input_hdr_rc(DEF, w, h, 0, work) == KS265_POINTER, "no picture"
    assert ks.input_hdr_rc(DEF, w, h, host.ctypes.data, work) == KS265_POINTER, "a host picture"
    assert ks.input_hdr_rc(DEF, w, h, pic, host.ctypes.data + n, nb) == KS265_POINTER, "a host work buffer"
    own = []                                                              # allocations of their own (a tensor is a piece of a larger block of torch's allocator)
    for nbytes in (n, nb):
        q = C.c_void_p()
        assert ks.lib.ks265_dev_malloc(ks.h, C.byref(q), C.c_size_t(nbytes)) == 0
        own.append(q)
    assert ks.input_hdr_rc(DEF, w, h, pic, own[1].value + 4, nb) == KS265_POINTER, "a work buffer that begins inside its allocation and ends 4 bytes behind it"
    assert ks.input_hdr_rc(DEF, w, h, own[0].value + 4, work) == KS265_POINTER, "a picture that begins inside its allocation and ends 4 bytes behind it"
    for q in own:
        ks.lib.ks265_dev_free(ks.h, q)
    assert ks.input_hdr_rc(DEF, w, h, pic, a[n + 2:n + 2 + nb]) == KS265_NOTSUPPORTED, "a work buffer at an odd address"
    assert ks.input_hdr_rc(DEF, w, h, a[1:n + 1], a[n + 4:n + 4 + nb]) == KS265_NOTSUPPORTED, "a picture at an odd address"
    ks.sync()
    assert (a.cpu().numpy() == 0x5A).all(), "a refused call wrote something"
    assert ks.input_hdr_rc(DEF, w, h, pic, work) == 0
    ks.sync()
    got = a.cpu().numpy()
    assert (got[:n] == 0x5A).all() and (got[n + nb:] == 0x5A).all(), "a flat picture is unchanged, and nothing behind the work buffer is written"


# ------------------------------------------------------------------ through the encoder

N = 9
KW = dict(fr=50, threads=8, psnr=1, rc=0, qp=30, iper=128)
CPARAMS = (("rc", 0), ("qp", 30), ("iper", 128))


def _clip(w, h, n, seed):
    """moving smooth texture under a hard-edged box and a dark bar"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        y = np.clip(128 + 70 * np.sin(0.09 * (xx + 3 * t)) * np.cos(0.06 * (yy + 2 * t)) + rng.normal(0, 2, (h, w)), 0, 255).astype(np.uint8)
        y[20 + t:60 + t, 30 + 3 * t:90 + 3 * t] = 210
        y[h - 30:h - 26, :] = 25
        u = np.clip(128 + 90 * np.sin(0.04 * (xx[::2, ::2] + yy[::2, ::2] + 2 * t)), 0, 255).astype(np.uint8)
        v = np.clip(128 + 127 * np.cos(0.07 * (xx[::2, ::2] - t)), 0, 255).astype(np.uint8)
        out.append(pw.pack([y, u, v]))
    return out


def _nals(stream: bytes):
    parts = stream.split(b"\x00\x00\x01")[1:]
    return [((p[0] >> 1) & 63, p.rstrip(b"\x00") if i + 1 < len(parts) else p) for i, p in enumerate(parts)]


def _same_but_sps(got, exp, ragged):
    g, e = _nals(got), _nals(exp)
    assert len(g) == len(e) and [t for t, _ in g] == [t for t, _ in e] and sum(t < 32 for t, _ in g) == N
    for (t, a), (_, b) in zip(g, e):
        assert (a == b) == (not ragged or t != ws.NAL_SPS), t


def _stream(w, h, pictures, fmt="i420", shape=None, **extra):
    from ks265codec_amd.encoder import Encoder
    with Encoder(w, h, "slow", **extra, **KW) as enc:
        out = b"".join(enc.encode(p if torch.is_tensor(p) else torch.from_numpy(p).cuda().view(*shape), fmt) for p in pictures) + enc.flush()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("w,h", [(208, 136), (202, 134)])
def test_encoder_is_the_plain_handle_fed_filtered_pictures(w, h):
    from test_gpu_device_input import encode
    cw, ch = pw.coded_size(w, h)
    ragged = (w, h) != (cw, ch)
    src = _clip(w, h, N, seed=w)
    coded = [pw.pad_i420(p, w, h) for p in src] if ragged else src
    flt = hr.hdr_clip(coded, cw, ch, DEF)
    assert all((a != b).sum() > 1000 for a, b in zip(flt, coded)), "the clip is not changed at the defaults"
    exp = _stream(cw, ch, flt, shape=(ch * 3 // 2, cw))
    _same_but_sps(_stream(w, h, src, shape=(h * 3 // 2, w), hdr=True), exp, ragged)
    strong = dict(hdr=True, hdr_strength=2.5, hdr_iter=2, hdr_sigma_s=60, hdr_sigma_r=40)
    _same_but_sps(_stream(w, h, src, shape=(h * 3 // 2, w), **strong), _stream(cw, ch, hr.hdr_clip(coded, cw, ch, hr.params(2.5, 2, 60, 40)), shape=(ch * 3 // 2, cw)), ragged)
    _same_but_sps(encode(w, h, src, CPARAMS + (("hdr", 1),)), encode(cw, ch, flt, CPARAMS), ragged)        # host pictures through the C API
    assert encode(w, h, src, CPARAMS) != encode(w, h, src, CPARAMS + (("hdr", 1),)), "off is another stream"


def test_scaled_input_then_filtered():
    w, h, sw, sh = 208, 136, 416, 272
    src = _clip(sw, sh, N, seed=7)
    want = hr.hdr_clip([ys.scale_i420(p, sw, sh, w, h, ys.CATMULL_ROM) for p in src], w, h, DEF)
    got = _stream(w, h, src, shape=(sh * 3 // 2, sw), scale="bicubic", scale_from=(sw, sh), hdr=True)
    assert len(got) > 1000 and got == _stream(w, h, want, shape=(h * 3 // 2, w))


def test_float_rgb_input_then_filtered():
    w, h = 208, 136
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = []
    for t in range(N):
        base = 0.5 + 0.3 * np.sin(0.08 * (xx + 3 * t)) * np.cos(0.05 * (yy + t))
        p = np.stack([base, 0.8 * base + 0.1, 1.0 - base]).astype(np.float32) + rng.random((3, h, w), dtype=np.float32) * 0.02
        p[:, 30:70, 40 + 2 * t:100 + 2 * t] = 0.9
        rgb.append(np.clip(p, 0, 1).astype(np.float32))
    want = hr.hdr_clip([fref.rgbf_to_i420(*p) for p in rgb], w, h, DEF)
    got = _stream(w, h, [torch.from_numpy(p).cuda() for p in rgb], fmt="rgb_planar", hdr=True)
    assert len(got) > 1000 and got == _stream(w, h, want, shape=(h * 3 // 2, w))
