"""GPU: tone mapping on the way in (ks265_input_tonemap, ks265codec_amd/csrc/input_tonemap.hip) against tests/tonemap_ref.py, byte for byte:
  * P010, I010, P012 and P016 at 8x2 (one cell, both clamps in it), 24x6, 72x34 (a partial work-group in both directions) and 520x4 (the 512-column boundary between
    waves), limited and full range, the three curves, peaks 1000 and 4000, on random words over the whole word range (stray bits included), the grey ramp and saturated
    BT.2020 primaries; the planes one element into their allocations with pitches three elements above the row and poisoned padding, every row ending where the next bytes
    are a guard value; 0xA5 guards on both sides of the destination stay, the source is the same bytes afterwards; both table placements (global memory, LDS);
  * refusals enqueue nothing: an 8-bit format, 4:2:2, an odd pitch, a host pointer, a short buffer, a misaligned destination, configurations out of range;
  * through Encoder at 64x48 over 4 pictures: P010 tensors with tonemap="bt2390" give the stream of the reference-mapped pictures handed to a twin handle as 8-bit "i420",
    recon= hands back the same pictures and quality() counts the error against the MAPPED picture; the same with scale= from 128x96."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import tonemap_ref as tm  # noqa: E402
import yuv_hibit_ref as yh  # noqa: E402
import yuv_scale_ref as ys  # noqa: E402
from ks265codec_amd.lib import InDesc  # noqa: E402

SLACK = 256
KS265_POINTER, KS265_NOTSUPPORTED = -3, -4
FORMATS = {"P010": (yh.SEMI, 10, 1), "I010": (yh.PLANAR, 10, 0), "P012": (yh.SEMI, 12, 1), "P016": (yh.SEMI, 16, 1)}
SHAPES = [(8, 2), (24, 6), (72, 34), (520, 4)]
SETTINGS = [(curve, full, peak) for curve in tm.CURVES.values() for full in (False, True) for peak in (1000.0, 4000.0)]


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


@pytest.fixture(scope="module")
def plans(ks):
    """one plan per setting, shared by the tests"""
    made = {s: ks.tonemap_plan_create(s[0], s[2], 203.0, s[1]) for s in SETTINGS}
    yield made
    ks.sync()
    for p in made.values():
        ks.tonemap_plan_destroy(p)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _desc(code, W, H, ptrs, pitches) -> InDesc:
    d = InDesc()
    d.format, d.width, d.height = code, W, H
    d.pixel_step, d.matrix, d.full_range = 77, 9, 5                      # ignored: the range is the plan's
    for k, p in enumerate(ptrs):
        d.plane[k], d.pitch[k] = p, pitches[k]
    return d


def _map(ks, plan, desc, W, H, want=0):
    """ks265_input_tonemap into a destination with SLACK bytes of 0xA5 on both sides; the picture (or, for a refusal, None after checking that nothing was written)"""
    n = W * H * 3 // 2
    dst = torch.full((n + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = ks.input_tonemap_rc(plan, desc, dst.data_ptr() + SLACK)
    assert rc == want, (rc, ks.lib.ks265_last_error(ks.h))
    ks.sync()
    out = dst.cpu().numpy()
    assert (out[:SLACK] == 0xA5).all() and (out[SLACK + n:] == 0xA5).all(), "bytes written outside the picture"
    if want:
        assert (out == 0xA5).all(), "a refused picture enqueued something"
        return None
    return out[SLACK:SLACK + n]


def _contents(name, W, H, seed, full):
    layout, depth, msb = FORMATS[name]
    rnd = yh.random_planes(np.random.default_rng(seed), layout, yh.S420, depth, msb, W, H)
    top = 0xFFFF
    for p in rnd:                                                      # the extremes next to each other at the picture's left edge and at its end
        p[0, :4] = (top, top, 0, top)
        p[-1, -4:] = (0, top, top, top)
    out = [("random", W, H, rnd), ("primaries", W, H, tm.primaries(depth, layout, msb, W, H, full))]
    if (W, H) == SHAPES[0] and depth <= 12:                            # every luma code once under neutral chroma: a picture of 32 columns
        ramp = tm.grey_ramp(depth, layout, msb)
        out.append(("ramp", ramp[0].shape[1], ramp[0].shape[0], ramp))
    return out


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_kernel_equals_the_specification(ks, plans, name, W, H):
    layout, depth, msb = FORMATS[name]
    code = yh.code(layout, yh.S420, depth, msb)
    for k, (curve, full, peak) in enumerate(SETTINGS):
        for what, w, h, planes in _contents(name, W, H, 7 * W + k, full):
            exp = tm.to_i420(planes, layout, depth, msb, curve, peak, 203.0, full)
            bufs, offs, pitches = yh.lay_out(planes, 1, 3)
            devs = [_dev(b) for b in bufs]
            desc = _desc(code, w, h, [d.data_ptr() + o for d, o in zip(devs, offs)], pitches)
            assert ks.input_tonemap_validate(plans[curve, full, peak], desc) == 0
            for where in (0, 1):
                ks.tonemap_plan_tables(plans[curve, full, peak], where)
                got = _map(ks, plans[curve, full, peak], desc, w, h)
                assert (got == exp).all(), (what, curve, full, peak, where, int((got != exp).sum()), np.flatnonzero(got != exp)[:8])
            assert all((d.cpu().numpy() == b).all() for d, b in zip(devs, bufs)), "the source changed"


def test_planes_at_their_allocations_starts(ks, plans):
    """pitch = row, 16-byte aligned runs: the wide loads"""
    W, H = 72, 34
    for name in sorted(FORMATS):
        layout, depth, msb = FORMATS[name]
        planes = yh.random_planes(np.random.default_rng(depth + layout), layout, yh.S420, depth, msb, W, H)
        bufs, offs, pitches = yh.lay_out(planes, 0, 0)
        devs = [_dev(b) for b in bufs]
        got = _map(ks, plans[tm.BT2390, False, 1000.0], _desc(yh.code(layout, yh.S420, depth, msb), W, H, [d.data_ptr() for d in devs], pitches), W, H)
        assert (got == tm.to_i420(planes, layout, depth, msb)).all(), name


def test_refusals_enqueue_nothing(ks, plans):
    W, H = 8, 2
    plan = plans[tm.BT2390, False, 1000.0]
    layout, depth, msb = FORMATS["P010"]
    planes = yh.random_planes(np.random.default_rng(5), layout, yh.S420, depth, msb, W, H)
    bufs, offs, pitches = yh.lay_out(planes, 0, 4)
    devs = [_dev(b) for b in bufs]
    ptrs = [d.data_ptr() for d in devs]
    ok = lambda code=yh.code(layout, yh.S420, depth, msb): _desc(code, W, H, ptrs, pitches)
    assert _map(ks, plan, ok(), W, H) is not None
    bad = [(ok(c), KS265_NOTSUPPORTED) for c in (0, 1, 2, 16, yh.code(1, 0, 8), yh.code(0, 0, 8), yh.code(0, 0, 9), yh.code(1, 1, 10, 1), yh.code(0, 1, 10), yh.code(1, 2, 10, 1),
                                                 yh.code(2, 1, 10, 1), yh.code(1, 0, 17, 1), yh.code(1, 0, 10, 1) | 0x2000, -1)]
    x = ok(); x.pitch[0] = pitches[0] + 1; bad.append((x, KS265_NOTSUPPORTED))                       # an odd pitch, an odd address
    x = ok(); x.pitch[1] = pitches[1] + 1; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.plane[1] = ptrs[1] + 1; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.width = 12; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.height = 3; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.pitch[0] = 2 * W - 2; bad.append((x, KS265_POINTER))                                  # a pitch below the row
    x = ok(); x.plane[1] = None; bad.append((x, KS265_POINTER))
    host = [np.zeros(b.size, np.uint8) for b in bufs]
    bad.append((_desc(yh.code(layout, yh.S420, depth, msb), W, H, [b.ctypes.data for b in host], pitches), KS265_POINTER))   # host memory
    for x, want in bad:
        assert ks.input_tonemap_validate(plan, x) == want, hex(x.format & 0xFFFFFFFF)
        _map(ks, plan, x, W, H, want)
    # a plane one element short: a page of its own, the plane's last row ends with it - and then begins one element later
    page = C.c_void_p()
    assert ks.lib.ks265_dev_malloc(ks.h, C.byref(page), C.c_size_t(4096)) == 0
    assert ks.lib.ks265_memset_async(ks.h, page, 0, C.c_size_t(4096)) == 0
    ks.sync()
    rows = [(H, 2 * W), (H // 2, 2 * W)]
    for k in range(2):
        pl = [page.value + 256 * j for j in range(2)]
        pl[k] = page.value + 4096 - (64 * (rows[k][0] - 1) + rows[k][1])
        assert _map(ks, plan, _desc(yh.NAMED["P010"], W, H, pl, [64, 64]), W, H) is not None
        pl[k] += 2
        _map(ks, plan, _desc(yh.NAMED["P010"], W, H, pl, [64, 64]), W, H, KS265_POINTER)
    # the destination: misaligned, NULL, and one that ends 8 bytes behind its allocation
    n = W * H * 3 // 2
    dst = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ks.input_tonemap_rc(plan, ok(), dst.data_ptr() + 4) == KS265_NOTSUPPORTED
    assert ks.input_tonemap_rc(plan, ok(), 0) == KS265_POINTER
    assert ks.input_tonemap_rc(plan, ok(), page.value + 4096 - 16) == KS265_POINTER
    assert ks.input_tonemap_rc(plan, ok(), page.value + 4096 - 32) == 0
    ks.sync()
    assert ks.lib.ks265_dev_free(ks.h, page) == 0
    ks.sync()
    assert (dst.cpu().numpy() == 0xA5).all()
    # configurations
    for cfg in ((3, 1000.0, 203.0), (0, 99.0, 80.0), (0, 10001.0, 203.0), (0, 1000.0, 79.0), (0, 1000.0, 1001.0), (0, 150.0, 203.0)):
        assert ks.tonemap_plan_create_rc(*cfg) == (KS265_NOTSUPPORTED, None)
    assert ks.tonemap_plan_create_rc(0, 1000.0, 203.0, False, transfer=18)[0] == KS265_NOTSUPPORTED


# ------------------------------------------------------------------ through the encoder

N, EW, EH = 4, 64, 48
KW = dict(fr=50, threads=8, psnr=1, rc=0, qp=30, iper=128)


def _hdr_clip(w, h, n, seed):
    """P010 pictures (y, uv) with structure that moves"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        y = np.clip((0.1 + 0.6 * ((xx + 3 * t) % w) / w + 0.1 * np.sin(0.2 * (yy + t))) * 1023 + rng.integers(0, 16, (h, w)), 0, 1023).astype(np.int64)
        u = np.clip((0.5 + 0.3 * np.sin(0.1 * (xx[::2, ::2] + t))) * 1023, 0, 1023).astype(np.int64)
        v = np.clip((0.5 + 0.3 * np.cos(0.13 * (yy[::2, ::2] + 2 * t))) * 1023, 0, 1023).astype(np.int64)
        c = np.empty((h // 2, w), np.uint16)
        c[:, 0::2], c[:, 1::2] = (u << 6).astype(np.uint16), (v << 6).astype(np.uint16)
        out.append([(y << 6).astype(np.uint16), c])
    return out


def _session(pictures, feed, **more):
    """(stream, {poc: reconstruction}, quality) of an EW x EH handle; feed(enc, picture) -> bytes"""
    from ks265codec_amd.encoder import Encoder
    with Encoder(EW, EH, "slow", recon="i420", **KW, **more) as enc:
        bs, pics = bytearray(), []
        for p in pictures:
            bs += feed(enc, p)
            pics += enc.recon()
        bs += enc.flush()
        pics += enc.recon()
        q = enc.quality()
    torch.cuda.synchronize()
    return bytes(bs), {poc: t.cpu().numpy().reshape(-1) for poc, t in pics}, q


def _p010(enc, planes):
    return enc.encode(tuple(torch.from_numpy(p.view(np.int16)).cuda() for p in planes), "nv12", depth=10)


@pytest.mark.parametrize("scaled", [False, True], ids=["same_size", "scale"])
def test_encoder_is_the_plain_handle_fed_mapped_pictures(scaled):
    sw, sh = (128, 96) if scaled else (EW, EH)
    src = _hdr_clip(sw, sh, N, 21)
    mapped = [tm.to_i420(p, yh.SEMI, 10, 1) for p in src]
    more = dict(scale="bicubic", scale_from=(sw, sh)) if scaled else {}
    exp, rb, _ = _session(mapped, lambda enc, p: enc.encode(torch.from_numpy(p).cuda().view(sh * 3 // 2, sw), "i420"), **more)
    got, ra, q = _session(src, _p010, tonemap="bt2390", **more)
    assert len(exp) > 300 and got == exp
    assert sorted(ra) == sorted(rb) == list(range(N)) and all((ra[p] == rb[p]).all() for p in ra)
    # -psnr counts the error against the mapped picture (behind the scaler where there is one)
    slot = [ys.scale_i420(m, sw, sh, EW, EH, 1) for m in mapped] if scaled else mapped
    n = EW * EH
    sse = [sum(int(((ra[p][a:b].astype(np.int64) - slot[p][a:b]) ** 2).sum()) for p in ra) for a, b in ((0, n), (n, n + n // 4), (n + n // 4, n * 3 // 2))]
    assert q["frames"] == N and [int(v) for v in q["sse"]] == sse
    plain, _, _ = _session(src, _p010, **more)
    assert plain != got                                                  # (without tonemap=: the pictures are only rounded)


def test_encoder_refuses_what_the_library_refuses():
    from ks265codec_amd.encoder import Encoder, EncoderError
    with pytest.raises(ValueError):
        Encoder(EW, EH, "slow", tonemap="hlg", **KW)
    with pytest.raises(ValueError):
        Encoder(EW, EH, "slow", tonemap="clip", tonemap_peak=50.0, **KW)
    with pytest.raises(ValueError):
        Encoder(100, 50, "slow", tonemap="clip", **KW)
    with pytest.raises(ValueError):
        Encoder(EW, EH, "slow", tonemap_peak=4000.0, **KW)
    src = _hdr_clip(EW, EH, 1, 22)[0]
    with Encoder(EW, EH, "slow", tonemap="reinhard", tonemap_peak=4000.0, **KW) as enc:
        p210 = (torch.zeros((EH, EW), dtype=torch.int16, device="cuda"), torch.zeros((EH, EW), dtype=torch.int16, device="cuda"))
        with pytest.raises(EncoderError):
            enc.encode(p210, "nv16", depth=10)
        assert len(_p010(enc, src) + enc.flush()) > 100                  # and the handle goes on
