"""GPU: reconstructed pictures in device memory (`devrecon`: ks265_enc_get_device_recon, ks265codec_amd/csrc/output_convert.hip, Encoder.recon()).
  * the conversion kernel equals tests/yuv_output_ref.py byte for byte - every format, both matrices, both ranges, pitches above the row and odd offsets - and writes nothing
    outside the rows (a canary in the padding, before the picture and behind it);
  * refused destinations (host memory, one byte short, a pitch below the row, no allocation at all) launch nothing and leave context and handle usable;
  * the encoder with the switch writes the stream it writes without it; the fetched reconstructions are the -o dump's pictures (and the reference decoder's, where it is
    staged), I420 exactly and RGBA / NV12 as the specification converts them; every picture is fetched exactly once;
  * fetches run in the caller's stream order (one reused tensor on a side stream, overwritten at once, no host synchronisation) through more pictures than the pool has slots;
  * Encoder.recon() equals the C API, and order="display" yields 0, 1, 2, ... without gaps."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import yuv_output_ref as ref  # noqa: E402
from test_gpu_device_input import CONFIGS, REF_DEC, YUV, HostPicture, InDesc, _clip, _open  # noqa: E402

QY_OK, QY_FAIL, QY_POINTER, QY_NOTSUPPORTED = 0, -0x7FFFFFFF, -0x7FFFFFFD, -0x7FFFFFFC
KS265_POINTER = -3
CANARY, SLACK = 0x3C, 256
LAYOUTS = [(0, 0), (3, 13), (1, 64)]          # (offset into the allocation, bytes of padding behind every row)
# 8x2: one thread, every chroma clamp at once; 24x6 and 200x134: widths that are no multiple of 16, H / 2 no multiple of the block's 4 rows; 1032x18: 129 threads per row - a
# third block of which one thread works; 416x240
SHAPES = [(8, 2), (24, 6), (200, 134), (1032, 18), (416, 240)]
MODES = [(m, f) for m in (ref.MATRIX_BT709, ref.MATRIX_BT601) for f in (0, 1)]


@pytest.fixture(scope="module")
def hip():
    from ks265codec_amd.lib import load_library
    lib = load_library()
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    yield lib, h
    lib.ks265_destroy(h)


def _pictures(W, H):
    """(name, packed I420): the second picture of every adversarial family, and one with U = V = 128"""
    from adversarial_clips import FAMILIES, make_adversarial
    out = [(kind, np.ascontiguousarray(make_adversarial(kind, W, H, 2, seed=W)[1])) for kind in FAMILIES]
    gray = out[3][1].copy()                                        # the noise family's luma
    gray[W * H:] = 128
    return out + [("gray", gray)]


def _convert_into(hip, src_dev, W, H, fmt, planes, pitches, offset, step=0, order=None, matrix=0, full=0):
    """planes: the expected 2-D uint8 arrays (rows of bytes) in the order they lie in the destination buffer.  The destination is a canary-filled allocation with the planes at
    `offset`, row k of plane p `pitches[p]` bytes apart, SLACK bytes behind the last row.  Returns (bytes the kernel left, bytes expected): equal = right values in every row
    and not one byte written anywhere else"""
    lib, h = hip
    sizes = [p.shape[0] * pitches[k] for k, p in enumerate(planes)]
    total = offset + sum(sizes) + SLACK
    want = np.full(total, CANARY, np.uint8)
    addr, o = [], offset
    for k, p in enumerate(planes):
        want[o:o + sizes[k]].reshape(p.shape[0], pitches[k])[:, :p.shape[1]] = p
        addr.append(o)
        o += sizes[k]
    dst = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    d = InDesc()
    d.format, d.width, d.height, d.pixel_step, d.matrix, d.full_range = fmt, W, H, step, matrix, full
    base = dst.data_ptr()
    if fmt == 2 and order is not None:                              # interleaved pixels: one plane of bytes, the channel pointers inside its first pixel
        for k in range(3):
            d.plane[k] = base + addr[0] + order[k]
        d.pitch[0] = pitches[0]
    else:
        for k in range(len(planes)):
            d.plane[k] = base + addr[k]
            d.pitch[k] = pitches[k]
    assert lib.ks265_wait_external(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    rc = lib.ks265_output_convert(h, C.c_void_p(src_dev.data_ptr()), C.byref(d))
    assert rc == 0, (rc, lib.ks265_last_error(h))
    assert lib.ks265_synchronize(h) == 0
    return dst.cpu().numpy(), want


def _same(got, want, what):
    assert (got == want).all(), (*what, int((got != want).sum()), np.flatnonzero(got != want)[:4].tolist())


@pytest.mark.parametrize("W,H", SHAPES)
def test_yuv_formats_exact_and_nothing_else_written(hip, W, H):
    for name, pic in _pictures(W, H):
        src = torch.from_numpy(pic).cuda()
        y, u, v = ref.planes(pic, W, H)
        nv = ref.i420_to_nv12(pic, W, H)
        for off, pad in LAYOUTS:
            _same(*_convert_into(hip, src, W, H, 0, [y, u, v], [W + pad, W // 2 + pad + 5, W // 2 + pad + 3], off), (name, "i420", off, pad))
            _same(*_convert_into(hip, src, W, H, 1, [nv[:H], nv[H:]], [W + pad, W + pad + 7], off), (name, "nv12", off, pad))


@pytest.mark.parametrize("W,H", SHAPES)
def test_rgb_formats_exact_and_nothing_else_written(hip, W, H):
    for name, pic in _pictures(W, H):
        src = torch.from_numpy(pic).cuda()
        for matrix, full in MODES:
            r, g, b = ref.i420_to_rgb(pic, W, H, matrix, bool(full))                # once per picture and mode, shared by every layout
            if name == "gray":
                assert (r == g).all() and (g == b).all()
            for fmt, step, order in (("rgb24", 3, (0, 1, 2)), ("rgba", 4, (0, 1, 2)), ("bgra", 4, (2, 1, 0)), ("planar", 1, None)):
                if order is not None:
                    px = np.full((H, W, step), 255, np.uint8)                   # the fourth byte of a four-byte pixel: 255
                    for k in range(3):
                        px[:, :, order[k]] = (r, g, b)[k]
                    planes = [px.reshape(H, W * step)]
                for off, pad in LAYOUTS:
                    if order is None:
                        got, want = _convert_into(hip, src, W, H, 2, [r, g, b], [W + pad] * 3, off, 1, None, matrix, full)
                    else:
                        got, want = _convert_into(hip, src, W, H, 2, planes, [W * step + pad], off, step, order, matrix, full)
                    _same(got, want, (name, fmt, matrix, full, off, pad))


def test_an_unaligned_source_picture(hip):
    """the packed source at an odd address (the encoder's own slots are aligned; the entry point asks for nothing)"""
    W, H = 200, 134
    name, pic = _pictures(W, H)[3]
    hold = torch.zeros(W * H * 3 // 2 + 8, dtype=torch.uint8, device="cuda")
    for shift in (1, 4):
        src = hold[shift:shift + W * H * 3 // 2]
        src.copy_(torch.from_numpy(pic))
        r, g, b = ref.i420_to_rgb(pic, W, H)
        px = np.stack([r, g, b, np.full_like(r, 255)], axis=2).reshape(H, W * 4)
        _same(*_convert_into(hip, src, W, H, 2, [px], [W * 4], 0, 4, (0, 1, 2)), ("rgba", shift))
        nv = ref.i420_to_nv12(pic, W, H)
        _same(*_convert_into(hip, src, W, H, 1, [nv[:H], nv[H:]], [W, W], 0), ("nv12", shift))


@pytest.mark.parametrize("W,H", [(10, 2), (22, 6), (206, 10), (1030, 4)])
def test_widths_that_are_only_even(hip, W, H):
    """the entry point asks for even sizes and no more: the thread at the right edge owns a run of 2, 4 or 6 columns (the encoder itself codes multiples of 8)"""
    for name, pic in _pictures(W, H)[2:5]:
        src = torch.from_numpy(pic).cuda()
        y, u, v = ref.planes(pic, W, H)
        nv = ref.i420_to_nv12(pic, W, H)
        r, g, b = ref.i420_to_rgb(pic, W, H, ref.MATRIX_BT601, False)
        for off, pad in LAYOUTS:
            _same(*_convert_into(hip, src, W, H, 0, [y, u, v], [W + pad, W // 2 + pad + 5, W // 2 + pad + 3], off), (name, "i420", off, pad))
            _same(*_convert_into(hip, src, W, H, 1, [nv[:H], nv[H:]], [W + pad, W + pad + 7], off), (name, "nv12", off, pad))
            _same(*_convert_into(hip, src, W, H, 2, [r, g, b], [W + pad] * 3, off, 1, None, ref.MATRIX_BT601, 0), (name, "planar", off, pad))
            for step in (3, 4):
                px = np.full((H, W, step), 255, np.uint8)
                px[:, :, 2], px[:, :, 1], px[:, :, 0] = r, g, b
                _same(*_convert_into(hip, src, W, H, 2, [px.reshape(H, W * step)], [W * step + pad], off, step, (2, 1, 0), ref.MATRIX_BT601, 0), (name, step, off, pad))


def _nv12_desc(y, uv, pitch_y, pitch_uv, W, H):
    d = InDesc()
    d.format, d.width, d.height = 1, W, H
    d.plane[0], d.plane[1], d.pitch[0], d.pitch[1] = y, uv, pitch_y, pitch_uv
    return d


def test_kernel_refusals_launch_nothing(hip):
    lib, h = hip
    W, H = 416, 240
    src = torch.full((W * H * 3 // 2,), 77, dtype=torch.uint8, device="cuda")
    pitch = 4096                                                           # allocations of whole pages: their ends are where the test puts them
    y_mem, ok_uv = C.c_void_p(), C.c_void_p()
    for p, nb in ((y_mem, pitch * H), (ok_uv, pitch * H // 2)):
        assert lib.ks265_dev_malloc(h, C.byref(p), C.c_size_t(nb)) == 0
        assert lib.ks265_memset_async(h, p, CANARY, C.c_size_t(nb)) == 0
    assert lib.ks265_synchronize(h) == 0
    ok_y = y_mem.value + pitch - W                                         # the last row ends with the allocation
    host_buf = np.zeros(W * H * 3 // 2, np.uint8)
    for d, why in ((_nv12_desc(host_buf.ctypes.data, host_buf.ctypes.data + W * H, W, W, W, H), "host memory"),
                   (_nv12_desc(ok_y + 1, ok_uv.value, pitch, pitch, W, H), "one byte short"),
                   (_nv12_desc(ok_y, ok_uv.value, W - 1, pitch, W, H), "pitch below the row"),
                   (_nv12_desc(0x1000, ok_uv.value, pitch, pitch, W, H), "no allocation")):
        assert lib.ks265_output_validate(h, C.byref(d)) == KS265_POINTER, why
        assert lib.ks265_output_convert(h, C.c_void_p(src.data_ptr()), C.byref(d)) == KS265_POINTER, why
    back = np.empty(pitch * H // 2, np.uint8)
    assert lib.ks265_memcpy_d2h_async(h, C.c_void_p(back.ctypes.data), ok_uv, C.c_size_t(back.size)) == 0 and lib.ks265_synchronize(h) == 0
    assert (back == CANARY).all(), "nothing was launched"
    d = _nv12_desc(ok_y, ok_uv.value, pitch, pitch, W, H)                # the extent that ends exactly at the end of its allocation is taken
    assert lib.ks265_output_convert(h, C.c_void_p(src.data_ptr()), C.byref(d)) == 0 and lib.ks265_synchronize(h) == 0
    assert lib.ks265_memcpy_d2h_async(h, C.c_void_p(back.ctypes.data), ok_uv, C.c_size_t(back.size)) == 0 and lib.ks265_synchronize(h) == 0
    rows = back.reshape(H // 2, pitch)
    assert (rows[:, :W] == 77).all() and (rows[:, W:] == CANARY).all()
    for p in (y_mem, ok_uv):
        lib.ks265_dev_free(h, p)


# ------------------------------------------------------------------ the encoder

def session(W, H, frames, params=(), latency=b"default", env=None, devrecon=0, recon_file=None, fetch=None, refusals=None):
    """one encoder session over host I420 frames.  fetch(k, call) (k: the picture's number in hand-out order, call: the API call's) -> None (leave the k-th handed-out picture where it is: it and what follows it in this call are released by the
    next call) or (format name, tensor, matrix, full_range): ks265_enc_get_device_recon into it, on torch's current stream.  Returns the stream, and the (poc, slice type, pts,
    k) of the fetched pictures.  refusals: DevPictures that must be refused with the given code before the first fetch"""
    from ks265codec_amd.encoder import Nal, Picture, describe, library
    lib = library()
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update({k: str(v) for k, v in (env or {}).items()})
    assert lib.ks265_enc_set_default(b"devrecon", C.c_int(devrecon)) == 0
    try:
        h = _open(lib, W, H, params, latency)
    finally:
        lib.ks265_enc_set_default(b"devrecon", C.c_int(0))
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    if recon_file:
        assert lib.ks265_enc_set_recon_file(C.c_void_p(h), str(recon_file).encode()) == 0
    nal, nn, pic, outp, yuv, info = C.POINTER(Nal)(), C.c_int(0), HostPicture(), HostPicture(), YUV(), Picture()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    bs, fetched, handed, calls = bytearray(), [], [0], [0]

    def take():
        vcl = [nal[i].pts for i in range(nn.value) if nal[i].iSize > 0 and nal[i].naltype < 32]
        bs.extend(b"".join(C.string_at(nal[i].pPayload, nal[i].iSize) for i in range(nn.value) if nal[i].iSize > 0))
        p = lib.ks265_enc_device_recon_pending(h)
        assert p == (len(vcl) if devrecon else 0), "one pending reconstruction per picture the call handed out"
        for j in range(p):
            k = handed[0] + j
            want = fetch(k, calls[0]) if fetch else None
            if want is None:
                break
            name, t, matrix, full = want
            d = describe(t, name, matrix, full)
            if refusals and not fetched:
                for bad, code in refusals:
                    bad.stream = d.stream
                    assert lib.ks265_enc_get_device_recon(h, C.byref(bad), C.addressof(info)) == code
                    assert lib.ks265_enc_device_recon_pending(h) == p, "a refused destination leaves the picture pending"
            assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.addressof(info)) == QY_OK
            assert lib.ks265_enc_device_recon_pending(h) == p - j - 1, "pending counts down"
            assert info.pts == vcl[j], "in the order of the call's NAL units"
            fetched.append((info.poc, info.iSliceType, info.pts, k))
        else:
            if p:
                assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.addressof(info)) == QY_FAIL, "nothing pending any more"
        handed[0] += p
        calls[0] += 1

    for t, f in enumerate(frames):
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(f.ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        rc = lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.addressof(pic), C.addressof(outp), 0)
        assert rc == QY_OK, (t, hex(rc & 0xFFFFFFFF))
        take()
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.addressof(outp), 0) == QY_OK
        take()
    lib.QY265EncoderClose(h)
    return bytes(bs), fetched


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_reconstructions_are_the_decoders_pictures(cfg, tmp_path):
    W, H, n = 416, 240, 70 if cfg == "two_lanes" else 26
    fsz = W * H * 3 // 2
    clip = _clip(W, H, min(n, 12), seed=n + W)
    frames = [clip[t % len(clip)] for t in range(n)]
    kw = CONFIGS[cfg]
    plain, none = session(W, H, frames, **kw)
    assert len(plain) > 1000 and not none
    dumped, _ = session(W, H, frames, recon_file=tmp_path / "rec.yuv", **kw)          # a separate run: the -o dump (one lane, key pictures on the main stream)
    assert dumped == plain
    rec = np.fromfile(str(tmp_path / "rec.yuv"), np.uint8).reshape(-1, fsz)
    assert len(rec) == n
    # every picture as I420; the first fetch after four refused destinations
    from ks265codec_amd.encoder import DevPicture

    def bad(y, uv, pitch):
        d = DevPicture()
        d.format, d.device = 1, 0
        d.plane[0], d.plane[1], d.pitch[0], d.pitch[1] = y, uv, pitch, pitch
        return d
    from ks265codec_amd.lib import load_library
    hl, ctx, pitch = load_library(), C.c_void_p(), 4096                   # allocations of whole pages: their ends are where the test puts them
    assert hl.ks265_create(C.byref(ctx), 0) == 0
    y_mem, uv_mem = C.c_void_p(), C.c_void_p()
    assert hl.ks265_dev_malloc(ctx, C.byref(y_mem), C.c_size_t(pitch * H)) == 0 and hl.ks265_dev_malloc(ctx, C.byref(uv_mem), C.c_size_t(pitch * H // 2)) == 0
    ok_y = y_mem.value + pitch - W                                         # the last row ends with the allocation
    host_buf = np.zeros(fsz, np.uint8)
    refusals = [(bad(host_buf.ctypes.data, host_buf.ctypes.data + W * H, W), QY_POINTER),     # host memory
                (bad(ok_y + 1, uv_mem.value, pitch), QY_POINTER),                            # one byte short
                (bad(ok_y, uv_mem.value, W - 1), QY_POINTER),                                # a pitch below the row
                (bad(0x1000, uv_mem.value, pitch), QY_POINTER)]                              # on no allocation
    out = torch.full((n, H * 3 // 2, W), 0xEE, dtype=torch.uint8, device="cuda")
    bs, got = session(W, H, frames, devrecon=1, fetch=lambda k, call: ("i420", out[k], 0, 0), refusals=refusals, **kw)
    for m in (y_mem, uv_mem):
        hl.ks265_dev_free(ctx, m)
    hl.ks265_destroy(ctx)
    assert bs == plain, "the stream with the switch is the stream without it"
    assert sorted(g[0] for g in got) == list(range(n)), "every picture fetched exactly once"
    assert all(pts == poc for poc, _, pts, _ in got)
    pics = out.cpu().numpy().reshape(n, fsz)
    for poc, _, _, k in got:
        assert (pics[k] == rec[poc]).all(), (cfg, poc)
    if os.path.exists(REF_DEC):
        (tmp_path / "a.265").write_bytes(bs)
        d = subprocess.run([REF_DEC, "-b", "a.265", "-o", "dec.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
        assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
        dec = np.fromfile(str(tmp_path / "dec.yuv"), np.uint8).reshape(-1, fsz)
        assert len(dec) == n and all((pics[k] == dec[poc]).all() for poc, _, _, k in got)
    # RGBA (BT.601, full range) and NV12 in turn
    rgba = torch.full((n, H, W, 4), 0xEE, dtype=torch.uint8, device="cuda")
    nv12 = torch.full((n, H * 3 // 2, W), 0xEE, dtype=torch.uint8, device="cuda")
    bs, got = session(W, H, frames, devrecon=1, fetch=lambda k, call: ("rgba", rgba[k], ref.MATRIX_BT601, 1) if k % 2 else ("nv12", nv12[k], 0, 0), **kw)
    assert bs == plain and sorted(g[0] for g in got) == list(range(n))
    rgba_h, nv12_h = rgba.cpu().numpy(), nv12.cpu().numpy()
    for poc, _, _, k in got:
        if k % 2:
            r, g, b = ref.i420_to_rgb(rec[poc], W, H, ref.MATRIX_BT601, True)
            assert (rgba_h[k] == np.stack([r, g, b, np.full_like(r, 255)], axis=2)).all(), (cfg, poc, "rgba")
        else:
            assert (nv12_h[k] == ref.i420_to_nv12(rec[poc], W, H)).all(), (cfg, poc, "nv12")


def test_stream_order_and_slot_reuse(tmp_path):
    """300 IPPP pictures - more than any pool at this size (the ring: 128 pictures) - each fetched into ONE reused tensor on a side stream, copied at once into its row of the
    result on that stream and overwritten; no host synchronisation until the end.  Then only every third call's pictures are fetched: the rest goes back unfetched, nothing stalls."""
    W, H, n = 416, 240, 300
    fsz = W * H * 3 // 2
    clip = _clip(W, H, 12, seed=21)
    frames = [clip[t % 12] for t in range(n)]
    kw = dict(params=(("rc", 0), ("qp", 30), ("iper", 128), ("bframes", 0)))
    plain, _ = session(W, H, frames, recon_file=tmp_path / "rec.yuv", **kw)
    rec = np.fromfile(str(tmp_path / "rec.yuv"), np.uint8).reshape(n, fsz)
    result = torch.zeros((n, H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    buf = torch.empty((H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    last = [-1]

    def fetch(k, call):
        if last[0] >= 0:                                               # the picture fetched before this one: out of the reused tensor, which is overwritten at once
            result[last[0]].copy_(buf)
            buf.fill_(0x77)
        last[0] = k
        return ("i420", buf, 0, 0)
    with torch.cuda.stream(s):
        bs, got = session(W, H, frames, devrecon=1, fetch=fetch, **kw)
        result[last[0]].copy_(buf)
    torch.cuda.synchronize()
    assert bs == plain and [g[0] for g in got] == list(range(n))
    assert (result.cpu().numpy().reshape(n, fsz) == rec).all()
    # the pictures of every third call only (the list is a queue: what a call leaves unfetched goes back with the next call)
    third = torch.zeros((n, H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    bs, got = session(W, H, frames, devrecon=1, fetch=lambda k, call: ("i420", third[k], 0, 0) if call % 3 == 0 else None, **kw)
    assert bs == plain and 0 < len(got) < n
    th = third.cpu().numpy().reshape(n, fsz)
    assert all((th[k] == rec[poc]).all() for poc, _, _, k in got)


def test_switch_off_means_not_supported():
    from ks265codec_amd.encoder import DevPicture, library
    lib = library()
    h = _open(lib, 416, 240, (("rc", 0), ("qp", 30)))
    d = DevPicture()
    assert lib.ks265_enc_get_device_recon(h, C.byref(d), None) == QY_NOTSUPPORTED and lib.ks265_enc_device_recon_pending(h) == 0
    lib.QY265EncoderClose(h)
    for v, rc in ((2, -2), (-1, -2), (0, 0)):
        assert lib.ks265_enc_set_default(b"devrecon", C.c_int(v)) == rc


def test_wrapper_equals_the_c_api_and_display_order_has_no_gaps():
    from ks265codec_amd.encoder import Encoder
    W, H, n = 416, 240, 21
    fsz = W * H * 3 // 2
    clip = _clip(W, H, n, seed=3)
    params = (("rc", 0), ("qp", 27), ("iper", 128))
    out = torch.zeros((n, H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    c_api, got = session(W, H, list(clip), params=params, devrecon=1, fetch=lambda k, call: ("i420", out[k], 0, 0))
    by_poc = {poc: out[k].cpu().numpy() for poc, _, _, k in got}
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda().view(H * 3 // 2, W) for f in clip]
    for order in ("coding", "display"):
        seen, bs = [], bytearray()
        with Encoder(W, H, "slow", rc=0, qp=27, iper=128, threads=8, fr=50, psnr=1, recon="i420") as enc:
            for x in dev:
                bs += enc.encode(x, "i420")
                seen += enc.recon(order)
            bs += enc.flush()
            seen += enc.recon(order)
            assert enc.recon(order) == []
        assert bytes(bs) == c_api
        assert sorted(p for p, _ in seen) == list(range(n))
        if order == "display":
            assert [p for p, _ in seen] == list(range(n))
        else:
            assert [p for p, _ in seen] == [g[0] for g in got] and [p for p, _ in seen] != list(range(n))
        assert all((t.cpu().numpy() == by_poc[p]).all() for p, t in seen)
    # another format, matrix and range: one key picture
    with Encoder(W, H, "slow", rc=0, qp=27, iper=128, threads=8, fr=50, recon="i420") as enc:
        enc.encode(dev[0], "i420")
        enc.flush()
        (poc, first), = enc.recon()
    with Encoder(W, H, "slow", rc=0, qp=27, iper=128, threads=8, fr=50, recon="bgra", recon_matrix=1, recon_full_range=True) as enc:
        enc.encode(dev[0], "i420")
        enc.flush()
        (poc, pix), = enc.recon()
    r, g, b = ref.i420_to_rgb(first.cpu().numpy().ravel(), W, H, 1, True)
    assert poc == 0 and pix.shape == (H, W, 4) and (pix.cpu().numpy() == np.stack([b, g, r, np.full_like(r, 255)], axis=2)).all()
