"""GPU: Encoder(scale=...) - device pictures of another size scaled into the encoder's input on the GPU (ks265_enc_encode_device_frame_scaled).
  * 17 RGBA tensors of 256x144 into a 128x72 encoder, default GOP: the stream is, byte for byte, that of a handle fed the I420 tensors tests/yuv_scale_ref.py makes of them;
    it decodes with the reference decoder (where present) to the pictures recon="i420" hands out;
  * the ordering contract: the source tensor is overwritten on the same stream right after every encode(), with no synchronise, and the bytes still match;
  * the ladder: two handles of different sizes fed the same tensor in one loop;
  * without scale= the ValueError still comes; sizes outside the rules are refused and the handle goes on."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import yuv_convert_ref as cref  # noqa: E402
import yuv_scale_ref as ys  # noqa: E402
from test_gpu_device_input import REF_DEC, _clip, _rgb_of  # noqa: E402

SW, SH, W, H, N = 256, 144, 128, 72, 17
PARAMS = dict(rc=0, qp=30, threads=8, fr=50)


@pytest.fixture(scope="module")
def rgba():
    """the 17 source pictures as (SH, SW, 4) uint8 arrays, and their planes"""
    clip = _clip(SW, SH, N, seed=9)
    out = []
    for t in range(N):
        r, g, b = _rgb_of(clip[t], SW, SH, t)
        px = np.full((SH, SW, 4), 255, np.uint8)
        px[:, :, 0], px[:, :, 1], px[:, :, 2] = r, g, b
        out.append(px)
    return out


@pytest.fixture(scope="module")
def prescaled(rgba):
    """what the specification makes of them, per (filter, size): packed I420 pictures"""
    cache = {}

    def get(filt, w, h):
        if (filt, w, h) not in cache:
            cache[filt, w, h] = [ys.scale_rgb(p[:, :, 0], p[:, :, 1], p[:, :, 2], w, h, filt, cref.MATRIX_BT709, False) for p in rgba]
        return cache[filt, w, h]
    return get


def encode_all(enc, tensors, fmt, scribble=False, recon=False):
    bs, rec = bytearray(), {}
    with enc:
        for t in tensors:
            src = t.clone() if scribble else t
            bs += enc.encode(src, fmt)
            if scribble:
                src.fill_(77)                                          # same stream, right behind the call, no synchronise: ordered behind the encoder's read
            if recon:
                rec.update(enc.recon())
        bs += enc.flush()
        if recon:
            rec.update(enc.recon())
    torch.cuda.synchronize()
    return bytes(bs), {p: t_.cpu().numpy().reshape(-1) for p, t_ in rec.items()}


@pytest.mark.parametrize("scale,filt", [("bicubic", ys.CATMULL_ROM), ("bilinear", ys.TRIANGLE)])
def test_scaled_stream_equals_prescaled_stream(tmp_path, rgba, prescaled, scale, filt):
    from ks265codec_amd.encoder import Encoder
    dev = [torch.from_numpy(p).cuda() for p in rgba]
    pre = [torch.from_numpy(p).cuda().view(H * 3 // 2, W) for p in prescaled(filt, W, H)]
    exp, rec = encode_all(Encoder(W, H, "slow", recon="i420", **PARAMS), pre, "i420", recon=True)
    got, _ = encode_all(Encoder(W, H, "slow", scale=scale, scale_from=(SW, SH), **PARAMS), dev, "rgba", scribble=True)
    assert len(exp) > 1000 and got == exp, "the scaled handle's bytes are those of the handle fed the specification's pictures (sources overwritten right after every encode())"
    calm, _ = encode_all(Encoder(W, H, "slow", scale=scale, **PARAMS), dev, "rgba")          # scale_from left to its default
    assert calm == exp
    other, _ = encode_all(Encoder(W, H, "slow", **PARAMS), [torch.from_numpy(p).cuda().view(H * 3 // 2, W) for p in prescaled(1 - filt, W, H)], "i420")
    assert other != exp, "the comparison tells the filters apart"
    if filt == ys.CATMULL_ROM and os.path.exists(REF_DEC):
        (tmp_path / "a.265").write_bytes(got)
        d = subprocess.run([REF_DEC, "-b", "a.265", "-o", "dec.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
        assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
        dec = np.fromfile(str(tmp_path / "dec.yuv"), np.uint8).reshape(-1, W * H * 3 // 2)
        assert len(dec) == N and sorted(rec) == list(range(N)) and all((dec[p] == rec[p]).all() for p in range(N))


def test_ladder_two_handles_one_tensor(rgba, prescaled):
    from ks265codec_amd.encoder import Encoder
    sizes = [(128, 72), (64, 40)]
    encs = [Encoder(w, h, "slow", scale="bicubic", scale_from=(SW, SH), **PARAMS) for w, h in sizes]
    out = [bytearray() for _ in sizes]
    frame = torch.empty((SH, SW, 4), dtype=torch.uint8, device="cuda")
    for p in rgba:
        frame.copy_(torch.from_numpy(p), non_blocking=False)           # ONE tensor, refilled for every picture on torch's current stream
        for k, e in enumerate(encs):
            out[k] += e.encode(frame, "rgba")
    for k, e in enumerate(encs):
        out[k] += e.flush()
        e.close()
    for k, (w, h) in enumerate(sizes):
        pre = [torch.from_numpy(p).cuda().view(h * 3 // 2, w) for p in prescaled(ys.CATMULL_ROM, w, h)]
        exp, _ = encode_all(Encoder(w, h, "slow", **PARAMS), pre, "i420")
        assert bytes(out[k]) == exp, (w, h)


def test_without_scale_the_value_error_stays_and_bad_sizes_are_refused(rgba):
    from ks265codec_amd.encoder import Encoder, EncoderError, QY_NOTSUPPORTED
    t = torch.from_numpy(rgba[0]).cuda()
    with Encoder(W, H, "slow", **PARAMS) as enc:
        with pytest.raises(ValueError, match=f"picture {SW}x{SH}, encoder {W}x{H}"):
            enc.encode(t, "rgba")
    with pytest.raises(ValueError):
        Encoder(W, H, "slow", scale="lanczos", **PARAMS)
    with pytest.raises(ValueError):
        Encoder(W, H, "slow", scale_from=(SW, SH), **PARAMS)
    with pytest.raises(EncoderError):
        Encoder(W, H, "slow", scale="bicubic", scale_from=(W * 16, H), **PARAMS)
    with Encoder(W, H, "slow", scale="bicubic", scale_from=(SW, SH), **PARAMS) as enc:
        for bad in [(SH, SW + 8, 4), (SH + 2, SW, 4), (SH, SW - 4, 4), (SH - 1, SW, 4), (8, 8, 4)]:      # above the maximum; no multiple of 8; an odd height; a ratio above 8
            with pytest.raises(EncoderError) as ei:
                enc.encode(torch.zeros(bad, dtype=torch.uint8, device="cuda"), "rgba")
            assert ei.value.rc == QY_NOTSUPPORTED
        assert enc.lib.QY265EncoderDelayedFrames(enc.h) == 0
        bs = enc.encode(t, "rgba") + enc.encode(t[: SH // 2, : SW // 2], "rgba") + enc.flush()       # a strided view of another size: its own plan
        assert len(bs) > 100
