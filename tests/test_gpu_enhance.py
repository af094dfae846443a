"""GPU: edge and colour enhancement on the way in (ks265codec_amd/csrc/input_enhance.hip, `vpp_edge` / `vpp_color` of include/ks265_enc.h) against tests/enhance_ref.py.
  * ks265_input_enhance, byte for byte, on the case list of tests/enhance_cases.py - every pair of levels, edge-only and colour-only among them, and the corners of the
    parameter ranges - at 8x8 (a partial tile where every neighbourhood clamps), 72x24 (one 64x16 tile plus 8-column and 8-row remainders, chroma rows of 36 bytes) and 136x40
    (interior tile seams both ways).  Guard bytes around the picture and the luma source stay; the luma source is the same bytes afterwards; a gain of 0 leaves its planes;
  * one 512x512 picture whose chroma planes hold all 65 536 (u, v) pairs, at the three colour gains;
  * refusals enqueue nothing - a canary-filled destination is unchanged: sizes outside the rule, every cfg value outside its range, both gains 0, a luma source that overlaps
    the picture or is missing, host pointers, odd addresses;
  * end to end, 9 pictures, default GOP, at 208x136 and 202x134 (enhanced at 208x136, behind the pad): the stream, the `devrecon` pictures and the `analysis` arrays of
    Encoder(..., edge=2, color=2) are those of a plain handle fed the reference-enhanced pictures; `ks265enc -edge 2 -color 2` writes the same stream;
  * scaled input (scale="bicubic" from 416x272) with edge=1 equals scale-then-reference-enhance."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import enhance_ref as er  # noqa: E402
from enhance_cases import CFGS, SIZES, contents as _contents  # noqa: E402
import picture_window_ref as pw  # noqa: E402
import window_sps as ws  # noqa: E402
import yuv_scale_ref as ys  # noqa: E402

SLACK = 256
KS265_POINTER, KS265_NOTSUPPORTED = -3, -4


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


def _guarded(a: np.ndarray):
    """a device buffer with 0xA5 guards around the bytes of `a`; (buffer, the view of the bytes)"""
    buf = torch.full((a.size + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[SLACK:SLACK + a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return buf, buf[SLACK:SLACK + a.size]


def _guards_ok(buf, n):
    b = buf.cpu().numpy()
    return (b[:SLACK] == 0xA5).all() and (b[SLACK + n:] == 0xA5).all()


def _run(ks, w, h, cfg, pic):
    """one call: the picture as numpy, guards checked"""
    n = w * h * 3 // 2
    pb, p = _guarded(pic)
    sb, s = _guarded(pic[:w * h]) if cfg[0] else (None, None)
    ks.input_enhance(cfg, w, h, s, p)
    ks.sync()
    assert _guards_ok(pb, n), "bytes written outside the picture"
    if sb is not None:
        assert _guards_ok(sb, w * h) and (s.cpu().numpy() == pic[:w * h]).all(), "the luma source changed"
    return p.cpu().numpy()


@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_equals_the_reference(ks, w, h):
    changed = [0, 0]
    for name, pic in _contents(w, h, seed=w + h).items():
        for cfg in CFGS:
            exp = er.enhance_picture(pic, w, h, cfg)
            got = _run(ks, w, h, cfg, pic)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (name, cfg, "differs at", bad[:8], "got", got[bad[:8]], "expected", exp[bad[:8]], "source", pic[bad[:8]])
            if not cfg[0]:
                assert (got[:w * h] == pic[:w * h]).all()
            if not cfg[4]:
                assert (got[w * h:] == pic[w * h:]).all()
            changed[0] += int((exp[:w * h] != pic[:w * h]).sum()); changed[1] += int((exp[w * h:] != pic[w * h:]).sum())
    assert min(changed) > 0, "the cases changed nothing: the filter was not exercised"


def test_all_chroma_pairs(ks):
    w = h = 512
    rng = np.random.default_rng(5)
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    pic = np.concatenate([rng.integers(0, 256, w * h), u.ravel(), v.ravel()]).astype(np.uint8)
    for cfg in (er.level_params(0, 1), er.level_params(0, 2), er.level_params(2, 3)):
        got = _run(ks, w, h, cfg, pic)
        assert (got == er.enhance_picture(pic, w, h, cfg)).all(), cfg


def test_refusals_enqueue_nothing(ks):
    w, h = 32, 16
    npx, n = w * h, w * h * 3 // 2
    a = torch.full((2 * n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    pic, src = a[:n], a[n:n + npx]
    host = np.zeros(n, np.uint8)
    ok = er.level_params(2, 2)
    assert ks.input_enhance_validate(ok, w, h) == 0 and ks.input_enhance_validate((0, 99, 99, 0, 8), w, h) == KS265_NOTSUPPORTED
    assert ks.input_enhance_validate((0, 0, 99, 0, 8), w, h) == 0, "edge_limit is not judged when edge_gain is 0"
    bad = [(20, 16, ok), (32, 12, ok), (0, 16, ok), (32, -8, ok), (8200, 16, ok), (w, h, (0, 0, 0, 0, 0)), (w, h, (65, 2, 8, 2, 0)), (w, h, (-1, 2, 8, 2, 8)), (w, h, (8, 17, 8, 2, 0)),
           (w, h, (8, -1, 8, 2, 0)), (w, h, (8, 2, 0, 2, 0)), (w, h, (8, 2, 65, 2, 0)), (w, h, (8, 2, 8, 33, 0)), (w, h, (8, 2, 8, -1, 0)), (w, h, (0, 0, 0, 0, 33)), (w, h, (8, 2, 8, 2, -1))]
    for tw, th, cfg in bad:
        assert ks.input_enhance_validate(cfg, tw, th) == KS265_NOTSUPPORTED, (tw, th, cfg)
        assert ks.input_enhance_rc(cfg, tw, th, src, pic) == KS265_NOTSUPPORTED, (tw, th, cfg)
    assert ks.input_enhance_rc(ok, w, h, pic[:npx], pic) == KS265_POINTER, "the luma source is the picture's luma"
    assert ks.input_enhance_rc(ok, w, h, a[n - 64:n - 64 + npx], pic) == KS265_POINTER, "the luma source overlaps the picture's chroma"
    assert ks.input_enhance_rc(ok, w, h, None, pic) == KS265_POINTER, "no luma source"
    assert ks.input_enhance_rc(ok, w, h, src, 0) == KS265_POINTER, "no picture"
    assert ks.input_enhance_rc(ok, w, h, src, host.ctypes.data) == KS265_POINTER, "a host picture"
    assert ks.input_enhance_rc(ok, w, h, host.ctypes.data, pic) == KS265_POINTER, "a host luma source"
    assert ks.input_enhance_rc(ok, w, h, src, a[1:n + 1]) == KS265_NOTSUPPORTED, "a picture at an odd address"
    assert ks.input_enhance_rc(ok, w, h, a[n + 2:n + 2 + npx], pic) == KS265_NOTSUPPORTED, "a luma source at an odd address"
    ks.sync()
    assert (a.cpu().numpy() == 0x5A).all(), "a refused call wrote something"
    assert ks.input_enhance_rc(er.level_params(0, 2), w, h, None, pic) == 0, "colour alone takes no luma source"
    ks.sync()
    got = a.cpu().numpy()
    assert (got[:npx] == 0x5A).all() and (got[n:] == 0x5A).all() and (got[npx:n] == er.enhance_chroma(np.full(1, 0x5A), np.full(1, 0x5A), 16)[0][0]).all()


# ------------------------------------------------------------------ through the encoder

N = 9
KW = dict(fr=50, threads=8, psnr=1, rc=0, qp=30, iper=128)
CPARAMS = (("rc", 0), ("qp", 30), ("iper", 128))
E22 = er.level_params(2, 2)


def _clip(w, h, n, seed):
    """moving smooth texture under a hard-edged box, a dark bar, saturated chroma patches"""
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


def _session(w, h, clip_, **extra):
    """(stream, {poc: reconstruction}, [analysis dicts as numpy, coding order])"""
    from ks265codec_amd.encoder import Encoder
    with Encoder(w, h, "slow", recon="i420", analysis=True, **extra, **KW) as enc:
        bs, pics, ans = bytearray(), [], []
        for p in clip_:
            bs += enc.encode(torch.from_numpy(p).cuda().view(h * 3 // 2, w), "i420")
            pics += enc.recon(); ans += enc.analysis()
        bs += enc.flush()
        pics += enc.recon(); ans += enc.analysis()
    torch.cuda.synchronize()
    return bytes(bs), {poc: t.cpu().numpy().reshape(-1) for poc, t in pics}, [{k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in a.items()} for a in ans]


@pytest.mark.parametrize("w,h", [(208, 136), (202, 134)])
def test_encoder_is_the_plain_handle_fed_enhanced_pictures(tmp_path, w, h):
    from ks265codec_amd import stream
    from test_gpu_device_input import encode
    cw, ch = pw.coded_size(w, h)
    ragged = (w, h) != (cw, ch)
    src = _clip(w, h, N, seed=w)
    coded = [pw.pad_i420(p, w, h) for p in src] if ragged else src
    enh = er.enhance_clip(coded, cw, ch, E22)
    assert all((a != b).sum() > 1000 for a, b in zip(enh, coded)), "the clip is not changed at level 2 / 2"
    exp, rb, ab = _session(cw, ch, enh)
    got, ra, aa = _session(w, h, src, edge=2, color=2)
    _same_but_sps(got, exp, ragged)
    assert sorted(ra) == sorted(rb) == list(range(N)) and len(aa) == len(ab) == N
    for poc in ra:
        assert (ra[poc] == (pw.crop_i420(rb[poc], cw, ch, w, h) if ragged else rb[poc])).all(), poc
    for x, y in zip(aa, ab):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
    _same_but_sps(encode(w, h, src, CPARAMS + (("edge", 2), ("color", 2))), encode(cw, ch, enh, CPARAMS), ragged)        # host pictures through the C API
    assert encode(w, h, src, CPARAMS) != encode(w, h, src, CPARAMS + (("edge", 2),)), "off is another stream"
    # the CLI
    stream.build()
    cli = {}
    for name, (ew, eh, pics, extra) in {"on": (w, h, src, ["-edge", "2", "-color", "2"]), "plain": (cw, ch, enh, [])}.items():
        yuv, out = tmp_path / (name + ".yuv"), tmp_path / (name + ".265")
        np.concatenate(pics).tofile(yuv)
        r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(ew), "-hgt", str(eh), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "30", "-iper", "128", "-threads", "8",
                            "-psnr", "1", *extra, "-b", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Total Frames: %d" % N in r.stdout, r.stdout[-500:] + r.stderr[-500:]
        cli[name] = open(out, "rb").read()
    _same_but_sps(cli["on"], cli["plain"], ragged)


def test_scaled_input_then_enhanced():
    from ks265codec_amd.encoder import Encoder
    w, h, sw, sh = 208, 136, 416, 272
    src = _clip(sw, sh, N, seed=7)
    cfg = er.level_params(1, 0)
    want = er.enhance_clip([ys.scale_i420(p, sw, sh, w, h, ys.CATMULL_ROM) for p in src], w, h, cfg)
    res = []
    for (ew, eh), clip_, extra in (((sw, sh), src, dict(scale="bicubic", scale_from=(sw, sh), edge=1)), ((w, h), want, {})):
        with Encoder(w, h, "slow", **extra, **KW) as enc:
            res.append(b"".join(enc.encode(torch.from_numpy(p).cuda().view(eh * 3 // 2, ew), "i420") for p in clip_) + enc.flush())
    assert len(res[1]) > 1000 and res[0] == res[1]
