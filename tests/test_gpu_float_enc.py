"""GPU: float tensors through ks265codec_amd.encoder.Encoder (KS265_IN_RGB_F16 / _BF16 / _F32 from describe() down to the kernels), 416x240:
  * float32 pictures u8 / 255, planar and RGBA, write the stream of the uint8 tensors, byte for byte;
  * a bfloat16 HWC clip writes the stream of host I420 pictures made by tests/yuv_float_ref.py;
  * recon_dtype=torch.float16 returns the uint8 reconstruction of a second handle / 255, rounded to float16;
  * describe() takes strides in elements and writes bytes (a crop of a larger float tensor), and refuses float64, float I420 and CPU tensors;
  * a float picture of another size goes through scale="bicubic"."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import yuv_float_ref as fref  # noqa: E402
from test_gpu_device_input import _clip, _rgb_of, encode  # noqa: E402  (the clip, its RGB pictures and the C API session of the device-input tests)

W, H, N = 416, 240, 5
KW = dict(rc=0, qp=27, iper=128, threads=8, fr=50, psnr=1)


@pytest.fixture(scope="module")
def rgb():
    clip = _clip(W, H, N, seed=7)
    return [np.stack(_rgb_of(clip[t], W, H, t)) for t in range(N)]           # (3, H, W) uint8


def _over255(t):
    """uint8 GPU tensor -> float32 GPU tensor t / 255, divided on the host: correctly rounded there (torch's GPU kernel multiplies by the rounded 1 / 255)"""
    return (t.cpu().float() / 255).cuda()


def _stream(pictures, fmt, **kw):
    from ks265codec_amd.encoder import Encoder
    with Encoder(W, H, "slow", **{**KW, **kw}) as enc:
        return b"".join(enc.encode(p, fmt) for p in pictures) + enc.flush()


def test_float32_pictures_write_the_uint8_stream(rgb):
    planar = [torch.from_numpy(p).cuda() for p in rgb]
    rgba = [torch.cat([p.permute(1, 2, 0), torch.full((H, W, 1), 255, dtype=torch.uint8, device="cuda")], dim=2).contiguous() for p in planar]
    want = _stream(planar, "rgb_planar")
    assert len(want) > 1000 and _stream(rgba, "rgba") == want
    assert _stream([_over255(p) for p in planar], "rgb_planar") == want
    assert _stream([_over255(p) for p in rgba], "rgba") == want


def test_bfloat16_hwc_clip_writes_the_stream_of_its_reference_conversion(rgb):
    rng = np.random.default_rng(2)
    x = [(_over255(torch.from_numpy(p).cuda()) + torch.from_numpy(rng.random((3, H, W), dtype=np.float32) * 0.01).cuda()).to(torch.bfloat16) for p in rgb]
    hwc = [t.permute(1, 2, 0).contiguous() for t in x]
    host = [fref.rgbf_to_i420(*fref.bf16_to_f32(t.view(torch.int16).cpu().numpy().view(np.uint16))) for t in x]
    want = encode(W, H, host, params=(("rc", 0), ("qp", 27), ("iper", 128)))
    assert len(want) > 1000 and _stream(hwc, "rgb") == want
    assert _stream([t.flip(2) for t in hwc], "bgr") == want                 # (flip makes a new contiguous tensor: B, G, R)


def test_float16_reconstructions_are_the_uint8_ones_over_255(rgb):
    from ks265codec_amd.encoder import Encoder
    pics = [torch.from_numpy(p).cuda() for p in rgb]
    got, ref = [], []
    for out, kw in ((got, dict(recon_dtype=torch.float16)), (ref, {})):
        with Encoder(W, H, "slow", recon="rgb_planar", **KW, **kw) as enc:
            for p in pics:
                enc.encode(p, "rgb_planar")
                out += enc.recon()
            enc.flush()
            out += enc.recon()
    assert len(got) == len(ref) == N and [p for p, _ in got] == [p for p, _ in ref]
    for (_, a), (_, b) in zip(got, ref):
        assert a.dtype == torch.float16 and a.shape == (3, H, W) and b.dtype == torch.uint8
        assert torch.equal(a, _over255(b).to(torch.float16))
    one = []
    for kw in (dict(recon_dtype=torch.float32), dict(recon_dtype=torch.uint8)):              # a four-element pixel: B, G, R and 1.0
        with Encoder(W, H, "slow", recon="bgra", **KW, **kw) as enc:
            enc.encode(pics[0], "rgb_planar")
            out = enc.recon()
            enc.flush()
            one.append((out + enc.recon())[0][1])
    t, b = one
    assert t.dtype == torch.float32 and b.dtype == torch.uint8 and t.shape == b.shape == (H, W, 4)
    assert torch.equal(t[:, :, 3], torch.ones(H, W, device="cuda")) and torch.equal(t[:, :, :3] * 255, b[:, :, :3].float())


def test_recon_dtype_is_refused_where_it_means_nothing():
    from ks265codec_amd.encoder import Encoder
    for kw in (dict(recon="i420", recon_dtype=torch.float16), dict(recon="nv12", recon_dtype=torch.float32), dict(recon_dtype=torch.bfloat16),
               dict(recon="rgb", recon_dtype=torch.float64)):
        with pytest.raises(ValueError):
            Encoder(W, H, "slow", **KW, **kw)


def test_describe_takes_strides_in_elements_and_writes_bytes(rgb):
    from ks265codec_amd.encoder import IN_RGB_BF16, IN_RGB_F16, IN_RGB_F32, describe
    big = torch.zeros((3, H + 10, W + 24), dtype=torch.float32, device="cuda")
    crop = big[:, 4:4 + H, 8:8 + W]
    crop.copy_(_over255(torch.from_numpy(rgb[0]).cuda()))
    d = describe(crop, "rgb_planar")
    assert d.format == IN_RGB_F32 and d.pixel_step == 4 and d.pitch[0] == 4 * (W + 24)
    assert [d.plane[k] for k in range(3)] == [big.data_ptr() + 4 * (k * (H + 10) * (W + 24) + 4 * (W + 24) + 8) for k in range(3)]
    hwc = torch.zeros((H + 2, W + 6, 4), dtype=torch.float16, device="cuda")
    v = hwc[1:1 + H, 3:3 + W]
    d = describe(v, "bgra")
    assert d.format == IN_RGB_F16 and d.pixel_step == 8 and d.pitch[0] == 2 * 4 * (W + 6)
    assert [d.plane[k] - v.data_ptr() for k in range(3)] == [4, 2, 0]
    assert describe(torch.zeros((H, W, 3), dtype=torch.bfloat16, device="cuda"), "rgb").format == IN_RGB_BF16
    # the crop codes as the picture it shows
    want = _stream([torch.from_numpy(rgb[0]).cuda()], "rgb_planar")
    assert _stream([crop], "rgb_planar") == want
    for bad, fmt in ((torch.zeros((3, H, W), dtype=torch.float64, device="cuda"), "rgb_planar"), (torch.zeros((H * 3 // 2, W), dtype=torch.float32, device="cuda"), "i420"),
                     (torch.zeros((H * 3 // 2, W), dtype=torch.float16, device="cuda"), "nv12"), (torch.zeros((3, H, W), dtype=torch.float32), "rgb_planar"),
                     (torch.zeros((3, H, W), dtype=torch.int8, device="cuda"), "rgb_planar")):
        with pytest.raises(ValueError):
            describe(bad, fmt)


def test_scaled_float_picture(rgb):
    SW, SH = 832, 480
    u8 = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (SH, SW, 4), dtype=np.uint8)).cuda()
    want = _stream([u8], "rgba", scale="bicubic")
    assert len(want) > 100
    assert _stream([_over255(u8)], "rgba", scale="bicubic") == want
    assert len(_stream([_over255(u8).to(torch.float16)], "rgba", scale="bicubic")) > 100
