"""GPU: the kernels of ragged picture sizes (ks265codec_amd/csrc/picture_window.hip) against tests/picture_window_ref.py, byte for byte:
  * ks265_input_pad: I420 and NV12 at 2x2 (one thread), 6x6, 10x2, 250x130 (6 columns and 6 rows of padding), 854x480 (columns only, rows at odd addresses), 480x270 (rows
    only) and 4098x2 (a second block in x); pitches = row, row + 1, row + 13; every plane at an odd address inside a larger allocation whose other bytes hold 0xA5 (the source is
    the same bytes afterwards); 0xA5 on both sides of the destination stays;
  * ks265_output_crop the same way back, the destination at an odd address;
  * ks265_sse_window behind ks265_sse_picture on random picture pairs: the window's sums, exact;
  * refusals enqueue nothing: host memory and a short buffer are KS265_POINTER, a pitch below the row and sizes / formats outside the rules KS265_NOTSUPPORTED."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import picture_window_ref as pw  # noqa: E402
from ks265codec_amd.lib import IN_I420, IN_NV12, InDesc  # noqa: E402

SLACK = 256
KS265_POINTER, KS265_NOTSUPPORTED = -3, -4
SIZES = [(2, 2), (6, 6), (10, 2), (250, 130), (854, 480), (480, 270), (4098, 2)]
EXTRA = [0, 1, 13]                            # bytes behind every row


@pytest.fixture(scope="module")
def hip():
    from ks265codec_amd.lib import load_library
    lib = load_library()
    lib.ks265_last_error.restype = C.c_char_p
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    yield lib, h
    lib.ks265_destroy(h)


def _wait_torch(hip):
    lib, h = hip
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0


def _lay_out(planes, front, extra):
    """every plane in a buffer of its own: `front` guard bytes, rows of row + extra bytes (the last row ends with its own bytes... and then SLACK guard bytes), all guards 0xA5"""
    bufs, offs, pitches = [], [], []
    for p in planes:
        rows, rb = p.shape
        pitch = rb + extra
        buf = np.full(front + pitch * (rows - 1) + rb + SLACK, 0xA5, np.uint8)
        for r in range(rows):
            buf[front + r * pitch: front + r * pitch + rb] = p[r]
        bufs.append(buf); offs.append(front); pitches.append(pitch)
    return bufs, offs, pitches


def _desc(fmt, w, h, ptrs, pitches) -> InDesc:
    d = InDesc()
    d.format, d.width, d.height = fmt, w, h
    for k, p in enumerate(ptrs):
        d.plane[k], d.pitch[k] = p, pitches[k]
    return d


def _pad(hip, desc, cw, ch, want=0):
    lib, h = hip
    n = cw * ch * 3 // 2
    dst = torch.full((n + 2 * SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    _wait_torch(hip)
    rc = lib.ks265_input_pad(h, C.byref(desc), cw, ch, C.c_void_p(dst.data_ptr() + SLACK))
    assert rc == want, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    assert (out[:SLACK] == 0xA5).all() and (out[SLACK + n:] == 0xA5).all(), "bytes written outside the picture"
    if want:
        assert (out == 0xA5).all(), "a refused picture enqueued something"
        return None
    return out[SLACK:SLACK + n]


def _source(rng, w, h, nv12):
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u, v = (rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8) for _ in range(2))
    y[0, :2] = (255, 0); y[-1, -2:] = (0, 255); u[-1, -1] = 255; v[-1, -1] = 0          # the extremes in the replicated corner
    if not nv12:
        return [y, u, v], [y, u, v]
    uv = np.empty((h // 2, w), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return [y, uv], [y, u, v]


@pytest.mark.parametrize("nv12", [False, True], ids=["i420", "nv12"])
@pytest.mark.parametrize("w,h", SIZES)
def test_pad_equals_the_specification(hip, w, h, nv12):
    cw, ch = pw.coded_size(w, h)
    stored, yuv = _source(np.random.default_rng(w * 7 + h + nv12), w, h, nv12)
    exp = pw.pad_planes(yuv, w, h)
    for extra in EXTRA:
        for front in (0, 3):
            bufs, offs, pitches = _lay_out(stored, front, extra)
            devs = [torch.from_numpy(b).cuda() for b in bufs]
            desc = _desc(IN_NV12 if nv12 else IN_I420, w, h, [d.data_ptr() + o for d, o in zip(devs, offs)], pitches)
            assert hip[0].ks265_input_pad_validate(hip[1], C.byref(desc), cw, ch) == 0
            got = _pad(hip, desc, cw, ch)
            assert all((d.cpu().numpy() == b).all() for d, b in zip(devs, bufs)), "the source changed"
            assert (got == exp).all(), (extra, front, int((got != exp).sum()), np.flatnonzero(got != exp)[:8])


def _crop(hip, src, cw, ch, w, h, front, want=0):
    lib, hd = hip
    n = w * h * 3 // 2
    dst = torch.full((front + n + SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    _wait_torch(hip)
    rc = lib.ks265_output_crop(hd, C.c_void_p(src.data_ptr()), cw, ch, w, h, C.c_void_p(dst.data_ptr() + front))
    assert rc == want, (rc, lib.ks265_last_error(hd))
    assert lib.ks265_synchronize(hd) == 0
    out = dst.cpu().numpy()
    assert (out[:front] == 0xA5).all() and (out[front + n:] == 0xA5).all(), "bytes written outside the picture"
    if want:
        assert (out == 0xA5).all()
        return None
    return out[front:front + n]


@pytest.mark.parametrize("w,h", SIZES)
def test_crop_equals_the_specification(hip, w, h):
    cw, ch = pw.coded_size(w, h)
    pic = np.random.default_rng(w + 31 * h).integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8)
    src = torch.from_numpy(pic).cuda()
    exp = pw.crop_i420(pic, cw, ch, w, h)
    for front in (0, 1, 16):
        got = _crop(hip, src, cw, ch, w, h, front)
        assert (got == exp).all(), (front, int((got != exp).sum()))
    assert (src.cpu().numpy() == pic).all()


def test_pad_then_crop_is_the_source(hip):
    w, h = 250, 130
    cw, ch = pw.coded_size(w, h)
    pic = np.random.default_rng(9).integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    d = torch.from_numpy(pic).cuda()
    p = d.data_ptr()
    padded = _pad(hip, _desc(IN_I420, w, h, [p, p + w * h, p + w * h * 5 // 4], [w, w // 2, w // 2]), cw, ch)
    assert (_crop(hip, torch.from_numpy(padded.copy()).cuda(), cw, ch, w, h, 0) == pic).all()


@pytest.mark.parametrize("w,h", [(58, 34), (250, 130), (854, 480), (480, 270)])
def test_sse_window_is_exact(w, h):
    from ks265codec_amd.lib import KsContext, KsFrame
    from ks265codec_amd.synth import lambda_q4
    cw, ch = pw.coded_size(w, h)
    rng = np.random.default_rng(w + h)
    ks = KsContext(0)
    fr = KsFrame(ks, cw, ch, 27, lambda_q4(27))
    lib = ks.lib
    try:
        for trial in range(2):
            a = rng.integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8)
            b = a.copy() if trial else rng.integers(0, 256, cw * ch * 3 // 2, dtype=np.uint8)
            if trial:                                                   # equal inside the window, different outside it: the window's sums are zero
                for p, s in zip(pw.planes(b, cw, ch), (1, 2, 2)):
                    p[:, w // s:] ^= 0xFF
                    p[h // s:, :] ^= 0x55
            pa, pb = fr.new_pic(), fr.new_pic()
            da, db = ks.dev(a), ks.dev(b)                               # alive across the calls
            ks._chk(lib.ks265_load_i420(fr.h, C.c_void_p(da.data_ptr()), pa.c()))
            ks._chk(lib.ks265_load_i420(fr.h, C.c_void_p(db.data_ptr()), pb.c()))
            out = ks.zeros(24)
            ks._chk(lib.ks265_sse_picture(fr.h, pa.c(), pb.c(), C.c_void_p(out.data_ptr())))
            whole = ks.host(out, np.uint64).tolist()
            assert whole == pw.sse3(a, b, cw, ch)
            ks._chk(lib.ks265_sse_window(ks.h, fr.h, pa.c(), pb.c(), w, h, C.c_void_p(out.data_ptr())))
            got = ks.host(out, np.uint64).tolist()
            assert got == pw.sse_window(a, b, cw, ch, w, h), (trial, got)
            if trial:
                assert got == [0, 0, 0]
            # the frame's own size: nothing to take out
            ks._chk(lib.ks265_sse_window(ks.h, fr.h, pa.c(), pb.c(), cw, ch, C.c_void_p(out.data_ptr())))
            assert ks.host(out, np.uint64).tolist() == got
            assert lib.ks265_sse_window(ks.h, fr.h, pa.c(), pb.c(), w - 8, h, C.c_void_p(out.data_ptr())) == KS265_NOTSUPPORTED
    finally:
        fr.close(); ks.close()


def test_refusals_enqueue_nothing(hip):
    lib, hd = hip
    w, h = 10, 6
    cw, ch = pw.coded_size(w, h)
    stored, _ = _source(np.random.default_rng(4), w, h, False)
    bufs, offs, pitches = _lay_out(stored, 0, 2)
    devs = [torch.from_numpy(b).cuda() for b in bufs]
    ptrs = [d.data_ptr() for d in devs]
    ok = lambda: _desc(IN_I420, w, h, ptrs, pitches)
    assert _pad(hip, ok(), cw, ch) is not None
    bad = []
    host = [np.zeros(b.size, np.uint8) for b in bufs]
    bad.append((_desc(IN_I420, w, h, [b.ctypes.data for b in host], pitches), cw, ch, KS265_POINTER))          # host memory
    x = ok(); x.plane[2] = None; bad.append((x, cw, ch, KS265_POINTER))
    for k, row in enumerate((w, w // 2, w // 2)):                                                             # a pitch below the row
        x = ok(); x.pitch[k] = row - 1; bad.append((x, cw, ch, KS265_NOTSUPPORTED))
    x = ok(); x.format = 2; bad.append((x, cw, ch, KS265_NOTSUPPORTED))                                        # RGB
    x = ok(); x.format = 0x1000 | 10; bad.append((x, cw, ch, KS265_NOTSUPPORTED))                              # 10 bits
    x = ok(); x.width = 9; bad.append((x, cw, ch, KS265_NOTSUPPORTED))
    x = ok(); x.height = 5; bad.append((x, cw, ch, KS265_NOTSUPPORTED))
    bad.append((ok(), cw + 8, ch, KS265_NOTSUPPORTED))                                                        # more than the rounding
    bad.append((ok(), cw, ch + 8, KS265_NOTSUPPORTED))
    bad.append((ok(), 12, ch, KS265_NOTSUPPORTED))
    bad.append((ok(), 8, ch, KS265_NOTSUPPORTED))                                                             # below the source
    for x, a, b, want in bad:
        assert lib.ks265_input_pad_validate(hd, C.byref(x), a, b) == want
        n = cw * ch * 3 // 2
        dst = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        _wait_torch(hip)
        assert lib.ks265_input_pad(hd, C.byref(x), a, b, C.c_void_p(dst.data_ptr())) == want
        assert lib.ks265_synchronize(hd) == 0
        assert (dst.cpu().numpy() == 0xA5).all(), "a refused picture enqueued something"
    # a short buffer: a page of its own, the plane's last row ends with it - and then begins one byte later
    page = C.c_void_p()
    assert lib.ks265_dev_malloc(hd, C.byref(page), C.c_size_t(4096)) == 0
    assert lib.ks265_memset_async(hd, page, 0, C.c_size_t(4096)) == 0 and lib.ks265_synchronize(hd) == 0
    for fmt, rows in ((IN_I420, [(h, w), (h // 2, w // 2), (h // 2, w // 2)]), (IN_NV12, [(h, w), (h // 2, w)])):
        for k in range(len(rows)):
            pl = [page.value + 512 * j for j in range(len(rows))]
            pt = [64] * len(rows)
            pl[k] = page.value + 4096 - (64 * (rows[k][0] - 1) + rows[k][1])
            assert _pad(hip, _desc(fmt, w, h, pl, pt), cw, ch) is not None
            pl[k] += 1
            assert lib.ks265_input_pad_validate(hd, C.byref(_desc(fmt, w, h, pl, pt)), cw, ch) == KS265_POINTER
            _pad(hip, _desc(fmt, w, h, pl, pt), cw, ch, KS265_POINTER)
    # the destination: it ends with the page, then one byte later; not 16-byte aligned
    n = cw * ch * 3 // 2
    _wait_torch(hip)
    assert lib.ks265_input_pad(hd, C.byref(ok()), cw, ch, C.c_void_p(page.value + 4096 - n)) == 0
    assert lib.ks265_input_pad(hd, C.byref(ok()), cw, ch, C.c_void_p(page.value + 4096 - n + 16)) == KS265_POINTER
    assert lib.ks265_input_pad(hd, C.byref(ok()), cw, ch, C.c_void_p(page.value + 8)) == KS265_NOTSUPPORTED
    # crop: a source and a destination that end with the page, then 8 / 1 bytes later; host memory; sizes outside the rules
    m = w * h * 3 // 2
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.full((m,), 0xA5, dtype=torch.uint8, device="cuda")
    _crop(hip, src, cw, ch, w, h, 0)
    _crop(hip, src, cw, ch, w - 1, h, 0, KS265_NOTSUPPORTED)
    _crop(hip, src, cw, ch, w - 8, h, 0, KS265_NOTSUPPORTED)
    _wait_torch(hip)
    crop = lambda s, d: lib.ks265_output_crop(hd, C.c_void_p(s), cw, ch, w, h, C.c_void_p(d))
    assert crop(page.value + 4096 - n, dst.data_ptr()) == 0
    assert lib.ks265_synchronize(hd) == 0
    dst.fill_(0xA5)
    _wait_torch(hip)
    assert crop(page.value + 4096 - n + 8, dst.data_ptr()) == KS265_POINTER
    assert crop(np.zeros(n, np.uint8).ctypes.data & ~7, dst.data_ptr()) == KS265_POINTER
    assert lib.ks265_synchronize(hd) == 0 and (dst.cpu().numpy() == 0xA5).all()
    assert crop(src.data_ptr(), page.value + 4096 - m) == 0
    assert crop(src.data_ptr(), page.value + 4096 - m + 1) == KS265_POINTER
    assert lib.ks265_synchronize(hd) == 0
    assert lib.ks265_dev_free(hd, page) == 0
