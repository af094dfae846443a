"""GPU: overlays on the way in (ks265codec_amd/csrc/input_overlay.hip, ks265_enc_set_overlay of include/ks265_enc.h) against tests/overlay_ref.py.  The kernel is held to the
reference on the WHOLE slot - every byte outside the rectangles is compared as well - with guard bytes around the slot:
  * pictures 72x40, 200x136 and coded 856x480 with the window 854x480; rectangles 2x2 at (0, 0), x = 2, 6, 14, 62 (and 510) with w = 8 - cells and work-groups straddled -,
    negative x and y, past the right and bottom edges, wholly outside (nothing changes);
  * RGBA, BGRA, RGB24 without alpha, planar uint8 at odd addresses with padded pitches, HWC4 float16 / bfloat16 / float32 with NaN, negative values and values above 1;
    both matrices and both ranges; eight mutually overlapping overlays of mixed formats; two runs from the same input are identical;
  * refusals enqueue nothing;
  * end to end at 200x136 over 6 pictures through Encoder: the stream and the recon= pictures are those of a plain handle fed the pre-blended pictures - with a device overlay
    that is rewritten on the caller's stream right after each encode() returns (a different caption per picture), a static logo in another slot, and forced_only."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import overlay_ref as ovr  # noqa: E402
import yuv_float_ref as yf  # noqa: E402

SLACK = 256
KS265_POINTER, KS265_NOTSUPPORTED = -3, -4
IN_RGB = 2
SIZES = [(72, 40, 72, 40), (200, 136, 200, 136), (856, 480, 854, 480)]
MODES = [(m, fr) for m in (0, 1) for fr in (False, True)]
_FMT = {torch.uint8: IN_RGB, torch.float16: yf.IN_RGB_F16, torch.bfloat16: yf.IN_RGB_BF16, torch.float32: yf.IN_RGB_F32}


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


def _codes(t: torch.Tensor) -> np.ndarray:
    """a (h, w) view of samples -> codes"""
    if t.dtype == torch.uint8:
        return ovr.codes(t.cpu().numpy())
    if t.dtype == torch.bfloat16:
        return ovr.codes(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), yf.IN_RGB_BF16)
    return ovr.codes(t.cpu().numpy(), _FMT[t.dtype])


class Ov:
    """an overlay as four (h, w) channel views of ONE device tensor (alpha None: opaque) with a common row and column stride: its descriptor tuple and its reference"""

    def __init__(self, chans, x, y, opacity=256, matrix=0, full=False):
        self.chans, self.x, self.y, self.opacity, self.matrix, self.full = chans, x, y, opacity, matrix, full

    def desc(self):
        r = self.chans[0]
        es = r.element_size()
        h, w = r.shape
        assert all(c is None or (c.stride() == r.stride() and c.shape == r.shape) for c in self.chans)
        a = self.chans[3]
        return (_FMT[r.dtype], w, h, [c.data_ptr() for c in self.chans[:3]], a.data_ptr() if a is not None else None, r.stride(0) * es, r.stride(1) * es,
                self.x, self.y, self.opacity, self.matrix, self.full)

    def ref(self):
        r, g, b, a = (None if c is None else _codes(c) for c in self.chans)
        return ovr.overlay(r, g, b, a, self.x, self.y, self.opacity, self.matrix, self.full)


def _hwc(t, order, alpha=True):
    """channel views of an (h, w, n) tensor; order: the element of R, G, B (and alpha: element 3)"""
    return [t[:, :, order[0]], t[:, :, order[1]], t[:, :, order[2]], t[:, :, 3] if alpha else None]


def _rgba8(seed, w, h):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)).cuda()


def _floats(seed, w, h, dtype):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.2, 1.2, (h, w, 4)).astype(np.float32)
    v[rng.uniform(size=v.shape) < 0.02] = np.nan
    v[rng.uniform(size=v.shape) < 0.02] = 7.5
    v[rng.uniform(size=v.shape) < 0.02] = -3.0
    v[0, 0] = (np.inf, -np.inf, 1.0, 0.5)
    return torch.from_numpy(v).cuda().to(dtype)


def _picture(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, w * h * 3 // 2, dtype=np.uint8)


def _run(ks, size, pic, ovs):
    """one call onto a guarded copy of the picture; the slot as numpy"""
    W, H, ww, wh = size
    n = W * H * 3 // 2
    buf = torch.full((n + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[SLACK:SLACK + n] = torch.from_numpy(pic).cuda()
    ks.input_overlay([o.desc() for o in ovs], W, H, buf[SLACK:SLACK + n], ww, wh)
    ks.sync()
    b = buf.cpu().numpy()
    assert (b[:SLACK] == 0xA5).all() and (b[SLACK + n:] == 0xA5).all(), "bytes written outside the picture"
    return b[SLACK:SLACK + n]


def _check(ks, size, pic, ovs, what):
    W, H, ww, wh = size
    exp = ovr.blend(pic, W, H, [o.ref() for o in ovs], ww, wh)
    got = _run(ks, size, pic, ovs)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, size, "differs at", bad[:8], "got", got[bad[:8]], "expected", exp[bad[:8]], "picture", pic[bad[:8]])
    return exp


@pytest.mark.parametrize("size", SIZES)
def test_rectangles(ks, size):
    W, H, ww, wh = size
    pic = _picture(W, W, H)
    small, big = _rgba8(1, 8, 4), _rgba8(2, 24, 16)
    changed = 0
    cases = [("2x2", _rgba8(3, 2, 2), 0, 0)] + [("w8 at %d" % x, small, x, 6) for x in (2, 6, 14, 62, 510) if x < W] + [
        ("negative", big, -10, -6), ("negative x", big, -22, 8), ("right", big, ww - 10, 4), ("bottom", big, 30, wh - 6), ("corner", big, ww - 2, wh - 2), ("coded edge", big, W - 8, H - 8)]
    for what, t, x, y in cases:
        exp = _check(ks, size, pic, [Ov(_hwc(t, (0, 1, 2)), x, y, 230)], what)
        changed += int((exp != pic).sum())
        if what != "coded edge" or (ww, wh) == (W, H):
            assert (exp != pic).any(), what
    assert changed > 0
    for what, x, y in (("right of", ww, 0), ("left of", -24, 0), ("below", 0, wh), ("above", 8, -16), ("far", 16384, -16384)):
        assert (_check(ks, size, pic, [Ov(_hwc(big, (0, 1, 2)), x, y)], what) == pic).all(), what
    if (ww, wh) != (W, H):                                               # the padding keeps its bytes
        got = _run(ks, size, pic, [Ov(_hwc(_rgba8(4, 64, 32), (0, 1, 2)), ww - 32, wh - 16)])
        assert (got[:W * H].reshape(H, W)[:, ww:] == pic[:W * H].reshape(H, W)[:, ww:]).all()


@pytest.mark.parametrize("matrix,full", MODES)
def test_formats(ks, matrix, full):
    size = SIZES[1]
    W, H = size[:2]
    pic = _picture(9, W, H)
    w, h = 40, 24
    t = _rgba8(5, w, h)
    kw = dict(matrix=matrix, full=full)
    _check(ks, size, pic, [Ov(_hwc(t, (0, 1, 2)), 16, 8, 256, **kw)], "rgba")
    _check(ks, size, pic, [Ov(_hwc(t, (0, 1, 2)), 18, 8, 200, **kw)], "rgba, cells straddled")
    _check(ks, size, pic, [Ov(_hwc(t, (2, 1, 0)), 16, 8, 256, **kw)], "bgra")
    _check(ks, size, pic, [Ov(_hwc(t[2:, 1:w - 1], (0, 1, 2)), 0, 0, 256, **kw)], "rgba, a view at an odd pixel with a padded pitch")
    rgb = t[:, :, :3].contiguous()
    exp = _check(ks, size, pic, [Ov(_hwc(rgb, (0, 1, 2), alpha=False), 16, 8, 256, **kw)], "rgb24")
    import yuv_convert_ref as yc
    own = yc.rgb_to_i420(*(rgb[:, :, k].cpu().numpy() for k in range(3)), matrix, full)
    assert (exp[:W * H].reshape(H, W)[8:8 + h, 16:16 + w] == own[:w * h].reshape(h, w)).all(), "an opaque overlay is the conversion of its RGB"
    _check(ks, size, pic, [Ov(_hwc(rgb, (0, 1, 2), alpha=False), 16, 8, 100, **kw)], "rgb24 at opacity 100")
    planar = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (4, h, w + 7), dtype=np.uint8)).cuda()
    _check(ks, size, pic, [Ov([planar[k][:, 1:1 + w] for k in range(4)], 26, 30, 256, **kw)], "planar at odd addresses, padded pitch")
    _check(ks, size, pic, [Ov([planar[k][:, 1:1 + w] for k in range(3)] + [None], 26, 30, 256, **kw)], "planar without alpha")
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        f = _floats(7, w, h, dt)
        _check(ks, size, pic, [Ov(_hwc(f, (0, 1, 2)), 16, 8, 256, **kw)], dt)
        _check(ks, size, pic, [Ov(_hwc(f, (2, 1, 0)), -6, 120, 77, **kw)], (dt, "bgra, clipped"))
        _check(ks, size, pic, [Ov(_hwc(f[:, :, :3].contiguous(), (0, 1, 2), alpha=False), 50, 8, 256, **kw)], (dt, "hwc3"))
    f32 = (t.to(torch.float32) / 255).contiguous()
    assert (_run(ks, size, pic, [Ov(_hwc(f32, (0, 1, 2)), 16, 8, 99, **kw)]) == _run(ks, size, pic, [Ov(_hwc(t, (0, 1, 2)), 16, 8, 99, **kw)])).all(), "float32 u8 / 255 is the u8 overlay"


@pytest.mark.parametrize("size", SIZES[:2])
def test_eight_overlapping(ks, size):
    W, H = size[:2]
    pic = _picture(11, W, H)
    dts = [torch.uint8, torch.float16, torch.uint8, torch.bfloat16, torch.float32, torch.uint8, torch.uint8, torch.float16]
    ovs = []
    for k, dt in enumerate(dts):
        w, h = 24 + 4 * k, 16 + 2 * (k % 3)
        t = _rgba8(20 + k, w, h) if dt == torch.uint8 else _floats(20 + k, w, h, dt)
        ovs.append(Ov(_hwc(t, (0, 1, 2) if k % 2 else (2, 1, 0)), 4 * k - 6, 2 * k - 2, 256 - 20 * k, k & 1, bool(k & 2)))
    exp = _check(ks, size, pic, ovs, "eight")
    assert (exp != ovr.blend(pic, W, H, [o.ref() for o in ovs[::-1]])).any(), "the order matters on this case"
    assert (_run(ks, size, pic, ovs) == _run(ks, size, pic, ovs)).all(), "two runs from the same input differ"


def test_refusals_enqueue_nothing(ks):
    W, H = 72, 40
    n = W * H * 3 // 2
    pic = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    t = _rgba8(1, 24, 16)
    ok = Ov(_hwc(t, (0, 1, 2)), 8, 4).desc()

    def alt(**kw):
        names = ("fmt", "w", "h", "planes", "alpha", "pitch", "step", "x", "y", "opacity", "matrix", "full")
        d = dict(zip(names, ok)); d.update(kw)
        return tuple(d[k] for k in names)
    assert ks.input_overlay_validate([ok], W, H) == 0
    bad = [alt(w=23), alt(h=15), alt(w=0), alt(h=8194), alt(x=7), alt(y=-3), alt(x=16386), alt(opacity=257), alt(opacity=-1), alt(fmt=0), alt(fmt=1), alt(fmt=19), alt(step=0),
           alt(step=17), alt(matrix=2), alt(fmt=yf.IN_RGB_F32, step=6), alt(fmt=yf.IN_RGB_F16, alpha=ok[4] - 2, step=8)]
    for d in bad:
        assert ks.input_overlay_validate([d], W, H) == KS265_NOTSUPPORTED, d
        assert ks.input_overlay_rc([ok, d], W, H, pic[:n]) == KS265_NOTSUPPORTED, d
    for cw, ch, ww, wh in ((70, 40, 70, 40), (72, 36, 72, 36), (72, 40, 74, 40), (72, 40, 71, 40), (72, 40, 72, 0), (8200, 40, 72, 40)):
        assert ks.input_overlay_rc([ok], cw, ch, pic[:n], ww, wh) == KS265_NOTSUPPORTED, (cw, ch, ww, wh)
    assert ks.input_overlay_rc([ok] * 9, W, H, pic[:n]) == KS265_NOTSUPPORTED and ks.input_overlay_rc([ok], W, H, pic[:n], n=0) == KS265_NOTSUPPORTED
    assert ks.input_overlay_rc([ok], W, H, pic[1:n + 1]) == KS265_NOTSUPPORTED, "a picture at an odd address"
    # extents: allocations of whole pages, their ends are where the test puts them - a 32x32 RGBA overlay fills 4096 bytes, a 128x64 picture 12288
    import ctypes as C
    raw, rawpic = C.c_void_p(), C.c_void_p()
    assert ks.lib.ks265_dev_malloc(ks.h, C.byref(raw), C.c_size_t(4096)) == 0 and ks.lib.ks265_dev_malloc(ks.h, C.byref(rawpic), C.c_size_t(12288)) == 0
    assert ks.lib.ks265_memset_async(ks.h, raw, 0x33, C.c_size_t(4096)) == 0 and ks.lib.ks265_memset_async(ks.h, rawpic, 0x5A, C.c_size_t(12288)) == 0
    ks.sync()
    ok = (IN_RGB, 32, 32, [raw.value + k for k in range(3)], raw.value + 3, 128, 4, 8, 4, 256, 0, False)
    assert ks.input_overlay_validate([ok], 128, 64) == 0, "an extent that ends where its allocation ends"
    host = np.zeros(4096, np.uint8)
    for d, what in ((alt(h=34), "rows past the allocation"), (alt(w=34, pitch=136), "a pitch past the allocation"), (alt(pitch=124), "a pitch below the row"),
                    (alt(planes=[host.ctypes.data + k for k in range(3)], alpha=host.ctypes.data + 3), "host memory"), (alt(alpha=host.ctypes.data + 3), "alpha in host memory"),
                    (alt(alpha=ok[4] + 4), "alpha's extent past the allocation"), (alt(planes=[0, ok[3][1], ok[3][2]]), "a NULL channel")):
        assert ks.input_overlay_validate([d], 128, 64) == KS265_POINTER, what
        assert ks.input_overlay_rc([ok, d], 128, 64, rawpic.value) == KS265_POINTER, what
    assert ks.input_overlay_rc([ok], 128, 64, 0) == KS265_POINTER and ks.input_overlay_rc([ok], 128, 64, host.ctypes.data) == KS265_POINTER
    assert ks.input_overlay_rc([ok], 128, 64, rawpic.value + 16) == KS265_POINTER, "a picture past its allocation"
    ks.sync()
    back = torch.empty(12288, dtype=torch.uint8, device="cuda")
    assert ks.lib.ks265_memcpy_d2d_async(ks.h, C.c_void_p(back.data_ptr()), rawpic, C.c_size_t(12288)) == 0
    ks.sync()
    assert (back.cpu().numpy() == 0x5A).all(), "a refused call wrote something"
    assert ks.input_overlay_rc([ok], 128, 64, rawpic.value) == 0, "the picture's extent ends where its allocation ends"
    ks.sync()
    ks.lib.ks265_dev_free(ks.h, raw); ks.lib.ks265_dev_free(ks.h, rawpic)
    ok = Ov(_hwc(t, (0, 1, 2)), 8, 4).desc()
    assert (pic.cpu().numpy() == 0x5A).all(), "a refused call wrote something"
    assert ks.input_overlay_rc([ok], W, H, pic[:n]) == 0
    ks.sync()
    assert (pic[:n].cpu().numpy() == ovr.blend(np.full(n, 0x5A, np.uint8), W, H, [Ov(_hwc(t, (0, 1, 2)), 8, 4).ref()])).all() and (pic[n:].cpu().numpy() == 0x5A).all()


# ------------------------------------------------------------------ through the encoder

N = 6
EW, EH = 200, 136
KW = dict(fr=50, threads=8, psnr=1, rc=0, qp=30, iper=128)


def _clip(n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:EH, 0:EW]
    out = []
    for t in range(n):
        y = np.clip(128 + 70 * np.sin(0.09 * (xx + 3 * t)) * np.cos(0.06 * (yy + 2 * t)) + rng.normal(0, 2, (EH, EW)), 0, 255).astype(np.uint8)
        u = np.clip(128 + 90 * np.sin(0.04 * (xx[::2, ::2] + yy[::2, ::2] + 2 * t)), 0, 255).astype(np.uint8)
        v = np.clip(128 + 100 * np.cos(0.07 * (xx[::2, ::2] - t)), 0, 255).astype(np.uint8)
        out.append(np.concatenate([y.ravel(), u.ravel(), v.ravel()]))
    return out


def _session(clip_, setup=None, after=None):
    """(stream, {poc: reconstruction}); setup(enc) before the first picture, after(enc, k) right after encode() of picture k returned"""
    from ks265codec_amd.encoder import Encoder
    with Encoder(EW, EH, "slow", recon="i420", **KW) as enc:
        if setup:
            setup(enc)
        bs, pics = bytearray(), []
        for k, p in enumerate(clip_):
            bs += enc.encode(torch.from_numpy(p).cuda().view(EH * 3 // 2, EW), "i420")
            if after:
                after(enc, k)
            pics += enc.recon()
        bs += enc.flush()
        pics += enc.recon()
    torch.cuda.synchronize()
    return bytes(bs), {poc: t.cpu().numpy().reshape(-1) for poc, t in pics}


def test_encoder_is_the_plain_handle_fed_blended_pictures():
    src = _clip(N, 3)
    logo = _rgba8(31, 48, 24)
    captions = [_floats(40 + k, 96, 16, torch.float16) for k in range(N)]
    for c in captions:
        c[:, :, 3] = torch.rand((16, 96), device="cuda").to(torch.float16)
    live = captions[0].clone()                                           # the device overlay that is rewritten between pictures

    def setup(enc):
        enc.set_overlay(0, logo, x=EW - 40, y=-4, opacity=0.75, format="bgra", matrix=1, full_range=True)     # clipped at the right and the top
        enc.set_overlay(3, live, x=52, y=EH - 20, format="rgba")

    def after(enc, k):                                                   # on torch's current stream, right behind the encode() call that read it
        if k + 1 < N:
            live.copy_(captions[k + 1])
    want = []
    for k, p in enumerate(src):
        a = Ov(_hwc(logo, (2, 1, 0)), EW - 40, -4, 192, 1, True).ref()
        b = Ov(_hwc(captions[k], (0, 1, 2)), 52, EH - 20, 256).ref()
        want.append(ovr.blend(p, EW, EH, [a, None, None, b]))
    assert all((a != b).sum() > 500 for a, b in zip(want, src))
    exp, rb = _session(want)
    got, ra = _session(src, setup, after)
    assert len(exp) > 1000 and got == exp
    assert sorted(ra) == sorted(rb) == list(range(N)) and all((ra[p] == rb[p]).all() for p in ra), "recon= shows the overlay"
    plain, rp = _session(src)
    assert plain != got and any((rp[p] != ra[p]).any() for p in rp)

    # replaced and cleared between pictures; forced_only is never drawn for device pictures
    def setup2(enc):
        enc.set_overlay(1, logo, x=10, y=10, forced_only=True)

    def after2(enc, k):
        if k == 1:
            enc.set_overlay(0, logo, x=20, y=30)
        if k == 3:
            enc.set_overlay(0, None)
    want2 = [ovr.blend(p, EW, EH, [Ov(_hwc(logo, (0, 1, 2)), 20, 30).ref()]) if k in (2, 3) else p for k, p in enumerate(src)]
    assert _session(src, setup2, after2)[0] == _session(want2)[0]
