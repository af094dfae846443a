"""GPU: the YUV family of the device input (ks265_input_convert with KS265_IN_YUV(layout, sub, depth, msb), ks265codec_amd/csrc/input_yuv.hip) against tests/yuv_hibit_ref.py,
byte for byte:
  * every valid (layout, subsampling) at depths 8, 10, 12, 16 and both alignments, at 8x2 (one thread), 24x6 (width no multiple of 16), 520x10 (a second block in x, a fifth
    chroma row = a second block in y) and 1040x6 (a third block); each once with the planes at their allocations' starts and pitch = row, and once with the planes one element
    in and pitch = row + 2 elements (the element path; every row ends where the next buffer bytes are a guard value); 0xA5 guards on both sides of the destination stay, the
    source is the same bytes afterwards;
  * all 65 536 word patterns as luma and as chroma of a 256x256 picture: depth 10 with msb 0 and 1, depth 16, semi-planar 4:2:2 and packed YUYV;
  * a P010 source through ks265_input_scale (64x48 -> 32x24, both filters) equals convert-then-scale of the specifications;
  * refusals enqueue nothing: invalid codes, odd pitches and addresses, a plane one byte short, host memory."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import yuv_hibit_ref as yh  # noqa: E402
import yuv_scale_ref as ys  # noqa: E402
from ks265codec_amd.lib import InDesc  # noqa: E402

SLACK = 256
KS265_POINTER, KS265_NOTSUPPORTED = -3, -4
SHAPES = [(8, 2), (24, 6), (520, 10), (1040, 6)]
DEPTHS = [(8, 0), (10, 0), (10, 1), (12, 0), (12, 1), (16, 0), (16, 1)]
PLACES = [(0, 0), (1, 2)]                     # (elements in front of each plane, elements behind every row)
IDS = [f"{yh.LAYOUT_NAMES[l]}{yh.SUB_NAMES[s]}" for l, s in yh.SHAPES]


@pytest.fixture(scope="module")
def hip():
    from ks265codec_amd.lib import load_library
    lib = load_library()
    lib.ks265_last_error.restype = C.c_char_p
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    yield lib, h
    lib.ks265_destroy(h)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _desc(code, W, H, ptrs, pitches) -> InDesc:
    d = InDesc()
    d.format, d.width, d.height = code, W, H
    d.pixel_step, d.matrix, d.full_range = 77, 9, 5                      # ignored by the family
    for k, p in enumerate(ptrs):
        d.plane[k], d.pitch[k] = p, pitches[k]
    return d


def _convert(hip, desc, W, H, want=0):
    """ks265_input_convert into a destination with SLACK bytes of 0xA5 on both sides; the picture (or, for a refusal, None after checking that nothing was written)"""
    lib, h = hip
    n = W * H * 3 // 2
    dst = torch.full((n + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = lib.ks265_input_convert(h, C.byref(desc), C.c_void_p(dst.data_ptr() + SLACK))
    assert rc == want, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    assert (out[:SLACK] == 0xA5).all() and (out[SLACK + n:] == 0xA5).all(), "bytes written outside the picture"
    if want:
        assert (out == 0xA5).all(), "a refused picture enqueued something"
        return None
    return out[SLACK:SLACK + n]


def _run(hip, planes, fmt, W, H, front, behind):
    bufs, offs, pitches = yh.lay_out(planes, front, behind)
    devs = [_dev(b) for b in bufs]
    got = _convert(hip, _desc(yh.code(*fmt), W, H, [d.data_ptr() + o for d, o in zip(devs, offs)], pitches), W, H)
    assert all((d.cpu().numpy() == b).all() for d, b in zip(devs, bufs)), "the source changed"
    return got


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("layout,sub", yh.SHAPES, ids=IDS)
def test_every_format_equals_the_specification(hip, layout, sub, W, H):
    for depth, msb in DEPTHS:
        planes = yh.random_planes(np.random.default_rng(W + depth + msb), layout, sub, depth, msb, W, H)
        top = 0xFF if depth == 8 else 0xFFFF
        for p in planes:                                               # the extremes next to each other at the picture's left edge and at its end
            p[0, :4] = (top, top, 0, top)
            p[-1, -4:] = (0, top, top, top)
        exp = yh.to_i420(planes, layout, sub, depth, msb)
        for front, behind in PLACES:
            got = _run(hip, planes, (layout, sub, depth, msb), W, H, front, behind)
            assert (got == exp).all(), (depth, msb, front, behind, int((got != exp).sum()), np.flatnonzero(got != exp)[:8])


@pytest.mark.parametrize("depth,msb", [(10, 0), (10, 1), (16, 0)])
@pytest.mark.parametrize("layout", [yh.SEMI, yh.YUYV], ids=["semi422", "yuyv"])
def test_all_65536_word_patterns(hip, layout, depth, msb):
    W = H = 256
    i = np.arange(65536, dtype=np.uint32)
    a, b = i.astype(np.uint16).reshape(H, W), ((i * 40503 + 12345) & 0xFFFF).astype(np.uint16).reshape(H, W)
    assert len(np.unique(b)) == 65536
    if layout == yh.SEMI:
        planes = [a, b]                                                 # luma: every pattern; U and V together: every pattern
    else:
        p = np.empty((H, 2 * W), np.uint16)
        p[:, 0::2], p[:, 1::2] = a, b
        planes = [p]
    exp = yh.to_i420(planes, layout, yh.S422, depth, msb)
    got = _run(hip, planes, (layout, yh.S422, depth, msb), W, H, 0, 0)
    assert (got == exp).all(), int((got != exp).sum())


@pytest.mark.parametrize("filt", [0, 1])
def test_p010_through_the_scaler(hip, filt):
    lib, h = hip
    SW, SH, DW, DH = 64, 48, 32, 24
    fmt = (yh.SEMI, yh.S420, 10, 1)
    planes = yh.random_planes(np.random.default_rng(64 + filt), *fmt, SW, SH)
    exp = ys.scale_i420(yh.to_i420(planes, *fmt), SW, SH, DW, DH, filt)
    bufs, offs, pitches = yh.lay_out(planes, 1, 2)
    devs = [_dev(b) for b in bufs]
    plan = C.c_void_p()
    assert lib.ks265_scale_plan_create(h, SW, SH, DW, DH, filt, C.byref(plan)) == 0
    scratch = torch.zeros(SW * SH * 3 // 2, dtype=torch.uint8, device="cuda")
    dst = torch.full((DW * DH * 3 // 2 + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    desc = _desc(yh.code(*fmt), SW, SH, [d.data_ptr() + o for d, o in zip(devs, offs)], pitches)
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert lib.ks265_input_scale_validate(h, plan, C.byref(desc)) == 0
    assert lib.ks265_input_scale(h, plan, C.byref(desc), None, C.c_void_p(dst.data_ptr() + SLACK)) == KS265_POINTER      # the family needs the scratch picture
    rc = lib.ks265_input_scale(h, plan, C.byref(desc), C.c_void_p(scratch.data_ptr()), C.c_void_p(dst.data_ptr() + SLACK))
    assert rc == 0, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    assert lib.ks265_scale_plan_destroy(h, plan) == 0
    assert (out[:SLACK] == 0xA5).all() and (out[-SLACK:] == 0xA5).all()
    assert (out[SLACK:-SLACK] == exp).all()
    assert (scratch.cpu().numpy() == yh.to_i420(planes, *fmt)).all()


def test_aliases_go_the_way_of_i420_and_nv12(hip):
    W, H = 24, 6
    for layout, own in ((yh.PLANAR, 0), (yh.SEMI, 1)):
        planes = yh.random_planes(np.random.default_rng(layout), layout, yh.S420, 8, 0, W, H)
        bufs, offs, pitches = yh.lay_out(planes, 1, 2)
        devs = [_dev(b) for b in bufs]
        ptrs = [d.data_ptr() + o for d, o in zip(devs, offs)]
        a, b = _convert(hip, _desc(yh.code(layout, yh.S420, 8), W, H, ptrs, pitches), W, H), _convert(hip, _desc(own, W, H, ptrs, pitches), W, H)
        assert (a == b).all() and (a == yh.to_i420(planes, layout, yh.S420, 8)).all()


def test_refusals_enqueue_nothing(hip):
    lib, h = hip
    W, H = 8, 2
    fmt = (yh.SEMI, yh.S422, 10, 1)                                     # P210
    planes = yh.random_planes(np.random.default_rng(5), *fmt, W, H)
    bufs, offs, pitches = yh.lay_out(planes, 0, 4)
    devs = [_dev(b) for b in bufs]
    ptrs = [d.data_ptr() for d in devs]
    ok = lambda code=yh.code(*fmt): _desc(code, W, H, ptrs, pitches)
    assert _convert(hip, ok(), W, H) is not None
    bad = []
    for code in (3, 7, 15, 19, 4095, 0x1000, yh.code(1, 1, 7), yh.code(1, 1, 17, 1), yh.code(1, 1, 8, 1), yh.code(2, 0, 8), yh.code(2, 2, 10, 1), yh.code(3, 2, 8), yh.code(3, 0, 16),
                 yh.code(1, 3, 10, 1), yh.code(*fmt) | 0x400, yh.code(*fmt) | 0x800, yh.code(*fmt) | 0x2000, yh.code(*fmt) | 1 << 16, yh.code(*fmt) | -(1 << 31), -1):
        bad.append((ok(code), KS265_NOTSUPPORTED))
    x = ok(); x.pitch[0] = pitches[0] + 1; bad.append((x, KS265_NOTSUPPORTED))                       # odd pitches and addresses of a two-byte format
    x = ok(); x.pitch[1] = pitches[1] + 1; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.plane[0] = ptrs[0] + 1; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.plane[1] = ptrs[1] + 1; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.width = 12; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.height = 3; bad.append((x, KS265_NOTSUPPORTED))
    x = ok(); x.pitch[0] = 2 * W - 2; bad.append((x, KS265_POINTER))                                  # a pitch below the row
    x = ok(); x.pitch[1] = 2 * W - 2; bad.append((x, KS265_POINTER))
    x = ok(); x.plane[1] = None; bad.append((x, KS265_POINTER))
    host = [np.zeros(b.size, np.uint8) for b in bufs]
    bad.append((_desc(yh.code(*fmt), W, H, [b.ctypes.data for b in host], pitches), KS265_POINTER))   # host memory
    for x, want in bad:
        assert lib.ks265_input_validate(h, C.byref(x)) == want, hex(x.format & 0xFFFFFFFF)
        _convert(hip, x, W, H, want)
    # a plane one byte short: a page of its own, the plane's last row ends with it - and then begins one byte later (8-bit formats: any address is allowed)
    page = C.c_void_p()
    assert lib.ks265_dev_malloc(h, C.byref(page), C.c_size_t(4096)) == 0
    assert lib.ks265_memset_async(h, page, 0, C.c_size_t(4096)) == 0 and lib.ks265_synchronize(h) == 0
    for code, rows, step in ((yh.NAMED["NV16"], [(H, W), (H, W)], 1), (yh.NAMED["I444"], [(H, W), (H, W), (H, W)], 1), (yh.NAMED["UYVY"], [(H, 2 * W)], 1),
                             (yh.NAMED["P010"], [(H, 2 * W), (H // 2, 2 * W)], 2)):              # (rows, bytes per row); P010: one element short
        for k in range(len(rows)):
            pl = [page.value + 256 * j for j in range(len(rows))]
            pt = [64] * len(rows)
            pl[k] = page.value + 4096 - (64 * (rows[k][0] - 1) + rows[k][1])
            assert _convert(hip, _desc(code, W, H, pl, pt), W, H) is not None
            pl[k] += step
            _convert(hip, _desc(code, W, H, pl, pt), W, H, KS265_POINTER)
    assert lib.ks265_dev_free(h, page) == 0
