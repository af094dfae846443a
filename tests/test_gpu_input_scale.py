"""GPU: the device-input scaler alone (ks265_input_scale, ks265codec_amd/csrc/input_scale.hip) against tests/yuv_scale_ref.py, byte for byte:
  * exact 2:1, odd ratios with a ragged last tile, ratio 8, up-scaling, identity (also equal to ks265_input_convert), a long row;
  * both filters; I420 with three pitches, NV12, RGBA, BGR24, planar RGB; base addresses at 16-, 8-, 4- and 1-byte alignment; random, all 0, all 255, a 0 / 255 checkerboard;
  * the destination sits between two canaries, the padding behind every source row holds a canary value (read as samples it would show in the output);
  * refusals return the documented code and leave the destination untouched."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import yuv_convert_ref as cref  # noqa: E402
import yuv_scale_ref as ys  # noqa: E402

KS265_POINTER, KS265_NOTSUPPORTED = -3, -4
GUARD = 256
CASES = [(128, 96, 64, 48), (200, 136, 128, 72), (512, 256, 64, 32), (64, 64, 104, 88), (64, 64, 64, 64), (4096, 16, 2048, 8)]
FORMATS = ["i420_p0", "i420_p1", "i420_p2", "nv12", "rgba", "bgr24", "planar"]
OFFSETS = [0, 8, 4, 1]
CONTENTS = ["random", "zeros", "ones", "checker"]
I420_PADS = {"i420_p0": (0, 0, 0), "i420_p1": (16, 8, 24), "i420_p2": (13, 5, 3)}      # bytes behind every row of Y, U, V


class InDesc(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


@pytest.fixture(scope="module")
def hip():
    from ks265codec_amd.lib import load_library
    lib = load_library()
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    yield lib, h
    lib.ks265_destroy(h)


def _plane(kind, h, w, rng):
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "ones":
        return np.full((h, w), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def _place(planes, pitches, offset):
    """2-D uint8 planes into one device buffer from `offset` on, rows `pitches[k]` bytes apart, the padding and the rest 0x3C; the buffer and the planes' addresses"""
    sizes = [p.shape[0] * pitches[k] for k, p in enumerate(planes)]
    buf = np.full(offset + sum(sizes) + 64, 0x3C, np.uint8)
    addr, o = [], offset
    for k, p in enumerate(planes):
        buf[o:o + sizes[k]].reshape(p.shape[0], pitches[k])[:, :p.shape[1]] = p
        addr.append(o)
        o += sizes[k]
    d = torch.from_numpy(buf).cuda()
    assert d.data_ptr() % 16 == 0
    return d, [d.data_ptr() + a for a in addr]


def _source(fmt, content, sw, sh, offset, seed):
    """(descriptor, the device buffer that backs it, the packed I420 picture the scaler is to see at the source's size)"""
    rng = np.random.default_rng(seed)
    d = InDesc()
    d.width, d.height = sw, sh
    if fmt in I420_PADS or fmt == "nv12":
        y, u, v = _plane(content, sh, sw, rng), _plane(content, sh // 2, sw // 2, rng), _plane(content, sh // 2, sw // 2, rng)
        if content == "checker":
            v = 255 - v
        i420 = np.concatenate([y.ravel(), u.ravel(), v.ravel()])
        if fmt == "nv12":
            uv = np.empty((sh // 2, sw), np.uint8)
            uv[:, 0::2], uv[:, 1::2] = u, v
            pit = [sw + 9, sw + 7]
            buf, addr = _place([y, uv], pit, offset)
            d.format = 1
        else:
            pads = I420_PADS[fmt]
            pit = [sw + pads[0], sw // 2 + pads[1], sw // 2 + pads[2]]
            buf, addr = _place([y, u, v], pit, offset)
            d.format = 0
        for k, a in enumerate(addr):
            d.plane[k], d.pitch[k] = a, pit[k]
        return d, buf, i420
    r, g, b = (_plane(content, sh, sw, rng) for _ in range(3))
    if content == "checker":
        g = 255 - g
    d.format, d.matrix, d.full_range = 2, cref.MATRIX_BT709, 0
    if fmt == "planar":
        buf, addr = _place([r, g, b], [sw + 5] * 3, offset)
        for k in range(3):
            d.plane[k] = addr[k]
        d.pitch[0], d.pixel_step = sw + 5, 1
    else:
        step, order = (4, (0, 1, 2)) if fmt == "rgba" else (3, (2, 1, 0))
        px = np.full((sh, sw, step), 0x77, np.uint8)
        for k in range(3):
            px[:, :, order[k]] = (r, g, b)[k]
        buf, addr = _place([px.reshape(sh, sw * step)], [sw * step + 6], offset)
        for k in range(3):
            d.plane[k] = addr[0] + order[k]
        d.pitch[0], d.pixel_step = sw * step + 6, step
    return d, buf, cref.rgb_to_i420(r, g, b, cref.MATRIX_BT709, False)


def _plan(hip, sw, sh, dw, dh, filt):
    lib, h = hip
    plan = C.c_void_p()
    rc = lib.ks265_scale_plan_create(h, sw, sh, dw, dh, filt, C.byref(plan))
    return rc, plan


def _run(hip, plan, desc, sw, sh, dw, dh, scratch=True):
    """ks265_input_scale into a guarded destination: (return code, the picture, whether both canaries are intact)"""
    lib, h = hip
    n = dw * dh * 3 // 2
    dst = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    scr = torch.empty(sw * sh * 3 // 2, dtype=torch.uint8, device="cuda") if scratch else None
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = lib.ks265_input_scale(h, plan, C.byref(desc), C.c_void_p(scr.data_ptr() if scratch else None), C.c_void_p(dst.data_ptr() + GUARD))
    assert lib.ks265_synchronize(h) == 0
    out = dst.cpu().numpy()
    return rc, out[GUARD:GUARD + n], bool((out[:GUARD] == 0xA5).all() and (out[GUARD + n:] == 0xA5).all())


@pytest.mark.parametrize("filt", [ys.TRIANGLE, ys.CATMULL_ROM])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_scaler_equals_the_spec(hip, case, filt):
    lib, h = hip
    sw, sh, dw, dh = case
    rc, plan = _plan(hip, sw, sh, dw, dh, filt)
    assert rc == 0, lib.ks265_last_error(h)
    expected = {}
    try:
        for content in CONTENTS:
            for fmt in FORMATS:
                for off in OFFSETS:
                    seed = CONTENTS.index(content) * 10 + (0 if fmt in I420_PADS or fmt == "nv12" else 1)
                    desc, buf, i420 = _source(fmt, content, sw, sh, off, seed)
                    if seed not in expected:                        # one reference per content and colour path, shared by every layout
                        expected[seed] = ys.scale_i420(i420, sw, sh, dw, dh, filt)
                    rc, got, intact = _run(hip, plan, desc, sw, sh, dw, dh)
                    assert rc == 0, (fmt, content, off, lib.ks265_last_error(h))
                    assert intact, (fmt, content, off, "bytes written outside the destination")
                    bad = np.flatnonzero(got != expected[seed])
                    assert bad.size == 0, (fmt, content, off, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), expected[seed][bad[:8]].tolist())
                    if (sw, sh) == (dw, dh) and off == 0:            # identity: ks265_input_convert alone
                        ref = torch.full((dw * dh * 3 // 2,), 0xA5, dtype=torch.uint8, device="cuda")
                        assert lib.ks265_input_convert(h, C.byref(desc), C.c_void_p(ref.data_ptr())) == 0
                        assert lib.ks265_synchronize(h) == 0
                        assert (ref.cpu().numpy() == got).all(), (fmt, content)
    finally:
        assert lib.ks265_scale_plan_destroy(h, plan) == 0


def test_refusals_leave_the_destination_untouched(hip):
    lib, h = hip
    for bad in [(520, 64, 64, 64), (64, 520, 64, 64), (64, 64, 520, 64), (128, 97, 64, 48), (132, 96, 64, 48), (128, 96, 60, 48), (128, 96, 64, 44), (8200, 96, 4096, 48)]:
        rc, plan = _plan(hip, *bad, ys.CATMULL_ROM)                 # a ratio above 8, an odd height, widths and heights that are no multiples of 8, a size above 8192
        assert rc == KS265_NOTSUPPORTED and not plan.value, bad
    assert _plan(hip, 128, 96, 64, 48, 2)[0] == KS265_NOTSUPPORTED   # no such filter
    sw, sh, dw, dh = 128, 96, 64, 48
    rc, plan = _plan(hip, sw, sh, dw, dh, ys.CATMULL_ROM)
    assert rc == 0
    good, buf, _ = _source("i420_p1", "random", sw, sh, 0, 1)
    rgb, rgb_buf, _ = _source("rgba", "random", sw, sh, 0, 1)

    def refused(desc, code, scratch=True):
        rc, got, intact = _run(hip, plan, desc, sw, sh, dw, dh, scratch)
        assert rc == code, (rc, code, lib.ks265_last_error(h))
        assert intact and (got == 0xA5).all()
        assert lib.ks265_input_scale_validate(h, plan, C.byref(desc)) == (0 if not scratch else code)

    short = C.c_void_p()                                             # one row short of pitch x height
    assert lib.ks265_dev_malloc(h, C.byref(short), C.c_size_t(good.pitch[0] * (sh - 1))) == 0
    d = InDesc.from_buffer_copy(good); d.plane[0] = short.value
    refused(d, KS265_POINTER)
    host = np.zeros(sw * sh * 2, np.uint8)                           # host memory
    d = InDesc.from_buffer_copy(good); d.plane[0] = host.ctypes.data
    refused(d, KS265_POINTER)
    d = InDesc.from_buffer_copy(good); d.pitch[1] = sw // 2 - 1     # a pitch below the row
    refused(d, KS265_POINTER)
    d = InDesc.from_buffer_copy(good); d.plane[2] = None
    refused(d, KS265_POINTER)
    d = InDesc.from_buffer_copy(good); d.height = sh - 2             # not the plan's size
    refused(d, KS265_NOTSUPPORTED)
    d = InDesc.from_buffer_copy(good); d.format = 3
    refused(d, KS265_NOTSUPPORTED)
    refused(rgb, KS265_POINTER, scratch=False)                       # an RGB source without the scratch picture (the source itself validates)
    n = dw * dh * 3 // 2
    dst = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.ks265_input_scale(h, plan, C.byref(good), None, C.c_void_p(dst.data_ptr() + 8)) == KS265_NOTSUPPORTED    # a destination off its 16 bytes
    assert lib.ks265_input_scale(h, plan, C.byref(good), None, C.c_void_p(host.ctypes.data)) in (KS265_POINTER, KS265_NOTSUPPORTED)
    assert lib.ks265_input_scale(h, plan, C.byref(good), None, None) == KS265_POINTER
    assert lib.ks265_synchronize(h) == 0 and (dst.cpu().numpy() == 0xA5).all()
    rc, got, intact = _run(hip, plan, good, sw, sh, dw, dh, scratch=False)      # after all of it the plan still works, and I420 needs no scratch
    assert rc == 0 and intact and (got == ys.scale_i420(_source("i420_p1", "random", sw, sh, 0, 1)[2], sw, sh, dw, dh, ys.CATMULL_ROM)).all()
    assert lib.ks265_dev_free(h, short) == 0
    assert lib.ks265_scale_plan_destroy(h, plan) == 0
