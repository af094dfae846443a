"""GPU: the temporal denoiser on the way in (ks265codec_amd/csrc/input_denoise.hip, `vpp_denoise` / `vpp_recur_filter` of include/ks265_enc.h) against tests/denoise_ref.py.
  * ks265_input_denoise, byte for byte in the picture, in dev_hist_out and in dev_blocks (vectors, gate and SAD: a wrong vector shows as such, not as a wrong blend), at 16x16
    (one candidate), 24x40 (every block partial), 104x72 and 152x40 (two whole 64x16 work-group tiles and a partial one in each direction); contents: a noisy displaced copy,
    independent noise (gated), a flat picture and ramps (ties), 0 / 255 extremes, and the panning clip as a chain of 4 pictures with the kernel's own output as the next
    history; the three levels, weight 1 and 30, thr 1 and 64.  Guard bytes around all three pictures stay; the history-in is the same bytes afterwards;
  * refusals enqueue nothing: 20x16, thr 0, weight 31, aliased pictures, a host pointer, an odd address;
  * end to end, 17 pictures, default GOP, at 208x136 and 202x134 (filtered at 208x136, behind the pad): the stream of Encoder(..., denoise=2) is that of a plain handle fed the
    reference-filtered pictures - for device I420, an NV12 pair, a uint8 RGB tensor (208x136: a ragged handle takes no RGB) and host pictures through the C API, and with roi=
    and recon= switched on, where the reconstructions are equal too."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import denoise_ref as dr  # noqa: E402
from denoise_cases import PARAMS, SIZES, contents as _contents  # noqa: E402
import picture_window_ref as pw  # noqa: E402
import window_sps as ws  # noqa: E402
import yuv_convert_ref as cref  # noqa: E402

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


def _run(ks, w, h, thr, wmax, cur, hist):
    """one call: (picture, history out, blocks) as numpy, guards checked"""
    n = w * h * 3 // 2
    nb = ((w + 15) // 16) * ((h + 15) // 16)
    pb, pic = _guarded(cur)
    ob, out = _guarded(np.full(n, 0x3C, np.uint8))
    hb, hin = _guarded(hist) if hist is not None else (None, None)
    blocks = torch.full((2 * nb + 8,), -7, dtype=torch.int32, device="cuda")
    ks.input_denoise(thr, wmax, w, h, pic, hin, out, blocks[:2 * nb])
    ks.sync()
    assert _guards_ok(pb, n) and _guards_ok(ob, n), "bytes written outside a picture"
    if hb is not None:
        assert _guards_ok(hb, n) and (hin.cpu().numpy() == hist).all(), "the history-in changed"
    bl = blocks.cpu().numpy()
    assert (bl[2 * nb:] == -7).all(), "words written behind the block words"
    return pic.cpu().numpy(), out.cpu().numpy(), bl[:2 * nb].reshape(nb, 2)


def _check(ks, w, h, thr, wmax, cur, hist, what):
    exp, eb = dr.filter_picture(cur, hist, w, h, thr, wmax)
    got, gh, gb = _run(ks, w, h, thr, wmax, cur, hist)
    bad = np.nonzero((gb != eb).any(axis=1))[0]
    assert bad.size == 0, (what, thr, wmax, "block", int(bad[0]), "got", [dr.vectors(gb[bad[:1]]), int(gb[bad[0], 1])], "expected", [dr.vectors(eb[bad[:1]]), int(eb[bad[0], 1])])
    assert (got == exp).all(), (what, thr, wmax, "picture differs at", np.nonzero(got != exp)[0][:8])
    assert (gh == exp).all(), (what, thr, wmax, "history out differs at", np.nonzero(gh != exp)[0][:8])
    return got, eb


@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_equals_the_reference(ks, w, h):
    moved = 0
    for name, (cur, hist) in _contents(w, h, seed=w + h).items():
        for thr, wmax in PARAMS:
            got, eb = _check(ks, w, h, thr, wmax, cur, hist, name)
            dx, dy, gated = dr.vectors(eb)
            moved += int(((dx != 0) | (dy != 0)).sum())
            if name in ("flat", "ramp_x"):                               # every row alike: the tie rule keeps dy = 0
                assert (dy == 0).all() and (name != "flat" or (dx == 0).all())
        got, eb = _check(ks, w, h, 10, 20, cur, None, name + " without a history")
        assert (got == cur).all() and (eb[:, 0] == (8 | 8 << 8 | 1 << 16)).all() and (eb[:, 1] == 0).all()
    assert moved > 0 or (w, h) == (16, 16), "no content moved a block: the search was not exercised"


@pytest.mark.parametrize("w,h", SIZES)
def test_chain_of_four_with_the_kernels_own_history(ks, w, h):
    _, noisy = dr.synthetic_clip(w, h, 4, seed=w)
    for thr, wmax in PARAMS[:5]:
        exp = dr.filter_clip(noisy, w, h, thr, wmax)
        hist, blended = None, 0
        for t, p in enumerate(noisy):
            got, gh, gb = _run(ks, w, h, thr, wmax, p, hist)
            assert (got == exp[t]).all() and (gh == exp[t]).all(), (thr, wmax, t)
            blended += int((got != p).sum())
            hist = gh
        if w >= 104 and thr >= 10 and wmax >= 16:                        # (at 16x16 the pan cannot be followed: (0, 0) is the only candidate and the gate closes; weight 1 moves no sample below thr 32)
            assert blended > 0, (thr, wmax, "the chain never blended a sample")


def test_refusals_enqueue_nothing(ks):
    w, h = 32, 16
    n = w * h * 3 // 2
    a = torch.full((3 * n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    pic, hin, hout = a[:n], a[n:2 * n], a[2 * n:3 * n]
    host = np.zeros(n, np.uint8)
    assert ks.input_denoise_validate(10, 20, w, h) == 0
    for tw, th, thr, wmax in ((20, 16, 10, 20), (32, 12, 10, 20), (0, 16, 10, 20), (32, -8, 10, 20), (8200, 16, 10, 20), (w, h, 0, 20), (w, h, 65, 20), (w, h, 10, 0), (w, h, 10, 31)):
        assert ks.input_denoise_validate(thr, wmax, tw, th) == KS265_NOTSUPPORTED, (tw, th, thr, wmax)
        assert ks.input_denoise_rc(thr, wmax, tw, th, pic, hin, hout) == KS265_NOTSUPPORTED, (tw, th, thr, wmax)
    assert ks.input_denoise_rc(10, 20, w, h, pic, hin, hin) == KS265_POINTER, "history out = history in"
    assert ks.input_denoise_rc(10, 20, w, h, pic, hin, a[n + 64:2 * n + 64]) == KS265_POINTER, "history out overlaps history in"
    assert ks.input_denoise_rc(10, 20, w, h, pic, pic, hout) == KS265_POINTER, "history in = the picture"
    assert ks.input_denoise_rc(10, 20, w, h, pic, None, pic) == KS265_POINTER, "history out = the picture"
    assert ks.input_denoise_rc(10, 20, w, h, host.ctypes.data, hin, hout) == KS265_POINTER, "a host picture"
    assert ks.input_denoise_rc(10, 20, w, h, pic, host.ctypes.data, hout) == KS265_POINTER, "a host history"
    assert ks.input_denoise_rc(10, 20, w, h, pic, hin, 0) == KS265_POINTER, "no history out"
    assert ks.input_denoise_rc(10, 20, w, h, a[1:n + 1], hin, hout) == KS265_NOTSUPPORTED, "a picture at an odd address"
    ks.sync()
    assert (a.cpu().numpy() == 0x5A).all(), "a refused call wrote something"


# ------------------------------------------------------------------ through the encoder

N = 17
KW = dict(fr=50, threads=8, psnr=1, rc=0, qp=30, iper=128)
CPARAMS = (("rc", 0), ("qp", 30), ("iper", 128))


def _clip(w, h, n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        y = np.clip(128 + 80 * np.sin(0.09 * (xx + 3 * t)) * np.cos(0.06 * (yy + 2 * t)) + rng.normal(0, 3, (h, w)), 0, 255).astype(np.uint8)
        u = np.clip(128 + 60 * np.sin(0.04 * (xx[::2, ::2] + yy[::2, ::2] + 2 * t)) + rng.normal(0, 2, (h // 2, w // 2)), 0, 255).astype(np.uint8)
        v = np.clip(128 + 60 * np.cos(0.07 * (xx[::2, ::2] - t)) + rng.normal(0, 2, (h // 2, w // 2)), 0, 255).astype(np.uint8)
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


_cache = {}


def _case(w, h):
    """(source clip, the reference-filtered coded-size clip, the plain coded-size handle's stream fed that clip)"""
    from test_gpu_device_input import encode
    if (w, h) not in _cache:
        cw, ch = pw.coded_size(w, h)
        src = _clip(w, h, N, seed=w)
        coded = [pw.pad_i420(p, w, h) for p in src] if (cw, ch) != (w, h) else src
        filt = dr.filter_clip(coded, cw, ch, *dr.level_params(2))
        assert sum(int((a != b).sum()) for a, b in zip(filt[1:], coded[1:])) > 1000, "the clip is not filtered at level 2"
        _cache[(w, h)] = (src, filt, encode(cw, ch, filt, CPARAMS))
    return _cache[(w, h)]


@pytest.mark.parametrize("w,h", [(208, 136), (202, 134)])
def test_encoder_stream_is_the_plain_handle_s_fed_filtered_pictures(w, h):
    from ks265codec_amd.encoder import Encoder
    from test_gpu_device_input import encode
    ragged = (w, h) != pw.coded_size(w, h)
    src, filt, want = _case(w, h)
    _same_but_sps(encode(w, h, src, CPARAMS + (("denoise", 2),)), want, ragged)                      # host pictures through the C API
    with Encoder(w, h, "slow", denoise=2, **KW) as enc:                                              # device I420
        bs = b"".join(enc.encode(torch.from_numpy(p).cuda().view(h * 3 // 2, w), "i420") for p in src) + enc.flush()
    _same_but_sps(bs, want, ragged)
    with Encoder(w, h, "slow", denoise=2, **KW) as enc:                                              # an NV12 pair
        bs = bytearray()
        for p in src:
            y, u, v = pw.planes(p, w, h)
            uv = np.empty((h // 2, w), np.uint8)
            uv[:, 0::2], uv[:, 1::2] = u, v
            bs += enc.encode((torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(uv).cuda()), "nv12")
        bs += enc.flush()
    _same_but_sps(bytes(bs), want, ragged)
    with Encoder(w, h, "slow", recur=20, **KW) as enc:                                               # recur alone at 20 = level 2's (10, 20)
        bs = b"".join(enc.encode(torch.from_numpy(p).cuda().view(h * 3 // 2, w), "i420") for p in src) + enc.flush()
    _same_but_sps(bs, want, ragged)
    with Encoder(w, h, "slow", **KW) as enc:                                                         # off: the plain stream of the unfiltered clip
        off = b"".join(enc.encode(torch.from_numpy(p).cuda().view(h * 3 // 2, w), "i420") for p in src) + enc.flush()
    assert off == encode(w, h, src, CPARAMS) and off != bs


def test_encoder_rgb_tensor():
    from ks265codec_amd.encoder import Encoder
    from test_gpu_device_input import _rgb_of, encode
    w, h = 208, 136
    src, _, _ = _case(w, h)
    rgb = [_rgb_of(p, w, h, t) for t, p in enumerate(src)]
    filt = dr.filter_clip([cref.rgb_to_i420(*c) for c in rgb], w, h, *dr.level_params(2))
    want = encode(w, h, filt, CPARAMS)
    with Encoder(w, h, "slow", denoise=2, **KW) as enc:
        bs = b"".join(enc.encode(torch.from_numpy(np.stack(c, axis=2)).cuda(), "rgb") for c in rgb) + enc.flush()
    assert bs == want


@pytest.mark.parametrize("w,h", [(208, 136), (202, 134)])
def test_encoder_with_roi_and_recon(w, h):
    from ks265codec_amd.encoder import Encoder
    cw, ch = pw.coded_size(w, h)
    ragged = (w, h) != (cw, ch)
    src, filt, _ = _case(w, h)
    ctu = np.array([[-6, 0, 4, 8], [3, -3, 6, 0], [5, 5, -4, 2]], np.int8)          # one offset per CTU, as blocks of 16: every block of a CTU equal, so the CTU's mean
    m = np.repeat(np.repeat(ctu, 4, axis=0), 4, axis=1)[:(h + 15) // 16, :(w + 15) // 16].copy()   # does not depend on how much of a block lies inside the picture
    res = []
    for (ew, eh), clip_, extra in (((w, h), src, dict(denoise=2)), ((cw, ch), filt, {})):
        with Encoder(ew, eh, "slow", roi=True, recon="i420", **extra, **KW) as enc:
            bs, pics = bytearray(), []
            for t, p in enumerate(clip_):
                bs += enc.encode(torch.from_numpy(p).cuda().view(eh * 3 // 2, ew), "i420", roi=m, roi_block=16)
                pics += enc.recon()
            bs += enc.flush()
            pics += enc.recon()
        res.append((bytes(bs), {poc: t.cpu().numpy().reshape(-1) for poc, t in pics}))
    (got, ra), (exp, rb) = res
    _same_but_sps(got, exp, ragged)
    assert sorted(ra) == sorted(rb) == list(range(N))
    for poc in ra:
        assert (ra[poc] == (pw.crop_i420(rb[poc], cw, ch, w, h) if ragged else rb[poc])).all(), poc
