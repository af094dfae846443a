"""CPU: `ks265enc -ssim 1` on the encoder host linked against the device library's CPU stand-in (tests/hip_stub.c), which has no ks265_ssim_picture - the host reaches the fused
SSIM pass as a weak symbol, so the library still loads (RTLD_NOW), the encoder works, writes the stream it writes without -ssim, says once that SSIM is unavailable and prints
`bitrate, psnr:` but no ` ssim:` line.  (The guard of the weak-symbol path: the GPU side of -ssim is tests/test_gpu_ssim.py.)"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from host_harness import build_host_cli, build_host_lib, load_host_lib

W, H, N = 128, 72, 9


@pytest.fixture(scope="module")
def stub_cli(tmp_path_factory):
    """a directory with the command line on the stand-in (as ks265enc) and a clip"""
    d = tmp_path_factory.mktemp("stubssim")
    os.symlink(build_host_cli(), d / "ks265enc")
    np.random.default_rng(11).integers(0, 256, (N, W * H * 3 // 2), dtype=np.uint8).tofile(str(d / "in.yuv"))
    return d


def _run(d, name, *extra):
    out = str(d / (name + ".265"))
    r = subprocess.run([str(d / "ks265enc"), "-i", str(d / "in.yuv"), "-wdt", str(W), "-hgt", str(H), "-fr", "25", "-frms", str(N), "-preset", "medium", "-rc", "0", "-qp", "34",
                        "-bframes", "0", "-threads", "3", "-psnr", "1", "-b", out, *extra], capture_output=True, text=True, timeout=120)
    return r, open(out, "rb").read() if os.path.exists(out) else b""


def test_host_library_loads_now():
    lib = load_host_lib(build_host_lib("hip_stub.c"), mode=os.RTLD_NOW)
    assert hasattr(lib, "ks265_enc_get_quality") and not hasattr(lib, "ks265_ssim_picture")


def test_ssim_flag_without_the_device_pass(stub_cli):
    plain, bs0 = _run(stub_cli, "plain")
    ssim, bs1 = _run(stub_cli, "ssim", "-ssim", "1")
    assert plain.returncode == 0 and ssim.returncode == 0, ssim.stdout[-600:] + ssim.stderr[-600:]
    assert len(bs0) > 100 and bs0 == bs1, "-ssim leaves the stream as it is"
    assert "bitrate, psnr:" in ssim.stdout and " ssim:" not in ssim.stdout
    assert ssim.stdout.count("SSIM is unavailable") == 1 and "SSIM is unavailable" not in plain.stdout
    assert f"Total Frames: {N}," in ssim.stdout and "H265 encoder passed!!!" in ssim.stdout
    assert [ln for ln in ssim.stdout.splitlines() if ln.startswith("bitrate, psnr:")] == [ln for ln in plain.stdout.splitlines() if ln.startswith("bitrate, psnr:")]
