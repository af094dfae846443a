"""CPU: the encoder host linked against the device library's CPU stand-in (tests/hip_stub.c), which has no conversion entry points - the host reaches them as weak symbols, so the
library still loads (RTLD_NOW), device input is QY_NOTSUPPORTED and host input writes the stream it wrote without the device-input calls."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from host_harness import ROOT, build_host_lib

_DRIVER = r"""
import ctypes as C, hashlib, json, os, sys
import numpy as np
ROOT, probe = sys.argv[1], int(sys.argv[2])
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ks265codec_amd.encoder import DevPicture, Nal, QY_NOTSUPPORTED
from host_harness import LAY, YUV, Picture
lib = C.CDLL(os.environ["KS265_STUB_LIB"], mode=os.RTLD_NOW); lib.QY265EncoderOpen.restype = C.c_void_p
W, H, N = 128, 72, 9
clip = np.random.default_rng(5).integers(0, 256, (N, W * H * 3 // 2), dtype=np.uint8)
cfg = (C.c_uint8 * LAY["sizeof_config"])()
assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34), ("iper", 32), ("bframes", 0), ("threads", 3), ("log", 3)):
    assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
err = C.c_int(0)
h = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err))); assert h.value, hex(err.value & 0xFFFFFFFF)
nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
codes = []
if probe:
    codes.append(lib.ks265_enc_enable_device_input(h))
    dp = DevPicture(); dp.format = 0; dp.plane[0] = dp.plane[1] = dp.plane[2] = clip[0].ctypes.data; dp.pitch[0] = W; dp.pitch[1] = dp.pitch[2] = W // 2
    codes.append(lib.ks265_enc_encode_device_frame(h, C.byref(nal), C.byref(nn), C.byref(dp), C.byref(outp)))
yuv.iWidth, yuv.iHeight = W, H
yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
pic.yuv = C.pointer(yuv)
md = hashlib.md5()
def take():
    for i in range(nn.value):
        if nal[i].iSize > 0: md.update(C.string_at(nal[i].pPayload, nal[i].iSize))
for t in range(N):
    for k, off in enumerate((0, W * H, W * H * 5 // 4)): yuv.pData[k] = C.cast(clip[t].ctypes.data + off, C.POINTER(C.c_ubyte))
    pic.pts = t
    assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == 0
    take()
while lib.QY265EncoderDelayedFrames(h):
    assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
    take()
lib.QY265EncoderClose(h)
print(json.dumps({"md5": md.hexdigest(), "codes": codes, "notsupported": QY_NOTSUPPORTED}))
"""


@pytest.fixture(scope="module")
def stub_lib():
    return build_host_lib("hip_stub.c")


def _run(stub_lib, probe):
    r = subprocess.run([sys.executable, "-c", _DRIVER, ROOT, str(probe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, KS265_STUB_LIB=stub_lib))
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-1200:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_device_input_is_not_supported_without_the_conversion(stub_lib):
    a = _run(stub_lib, probe=1)
    assert a["codes"] == [a["notsupported"], a["notsupported"]]
    b = _run(stub_lib, probe=0)
    assert a["md5"] == b["md5"], "host input after the refused device-input calls writes the stream it writes without them"
