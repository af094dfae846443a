"""CPU: the encoder option sao-ref (QY265ConfigParse) - 1 = the reference's SAO decision (what sao 3 by name selects), 2 = with its merge candidates (ks265_frame_cfg.sao = 3) -
on the encoder host linked against the device library's CPU stand-in (tests/hip_stub.c)."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from host_harness import LAY, ROOT, build_host_lib, load_host_lib

_DRIVER = r"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "tests"))
from host_harness import LAY, YUV, Nal, Picture
lib = C.CDLL(os.environ["KS265_STUB_LIB"]); lib.QY265EncoderOpen.restype = C.c_void_p
W, H, N = 128, 72, 6
clip = np.random.default_rng(5).integers(0, 256, (N, W * H * 3 // 2), dtype=np.uint8)
cfg = (C.c_uint8 * LAY["sizeof_config"])()
assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34), ("iper", 32), ("bframes", 0), ("threads", 3), ("log", 0), ("sao-ref", 2)):
    assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
err = C.c_int(0)
h = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err))); assert h.value, hex(err.value & 0xFFFFFFFF)
nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
yuv.iWidth, yuv.iHeight = W, H
yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
pic.yuv = C.pointer(yuv)
vcl = 0
def take():
    global vcl
    vcl += sum(1 for i in range(nn.value) if nal[i].iSize > 0 and nal[i].naltype < 32)
for t in range(N):
    for k, off in enumerate((0, W * H, W * H * 5 // 4)): yuv.pData[k] = C.cast(clip[t].ctypes.data + off, C.POINTER(C.c_ubyte))
    pic.pts = t
    assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == 0
    take()
while lib.QY265EncoderDelayedFrames(h):
    assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
    take()
lib.QY265EncoderClose(h)
print(json.dumps({"vcl": vcl}))
"""


@pytest.fixture(scope="module")
def stub_lib():
    return build_host_lib("hip_stub.c")


def test_sao_ref_is_parsed_and_sao_is_parsed_as_before(stub_lib):
    lib = load_host_lib(stub_lib)
    gold = LAY
    buf = (C.c_uint8 * gold["sizeof_config"])()

    def sao(): return C.c_int32.from_buffer(buf, gold["sao"]).value
    assert lib.QY265ConfigDefaultPreset(buf, b"slow", None, b"default") == 0 and sao() == 4
    assert lib.QY265ConfigParse(buf, b"sao-ref", b"0") == 0 and sao() == 4            # 0 leaves sao alone
    assert lib.QY265ConfigParse(buf, b"sao-ref", b"1") == 0 and sao() == 5
    assert lib.QY265ConfigParse(buf, b"sao-ref", b"0") == 0 and sao() == 5
    assert lib.QY265ConfigParse(buf, b"sao-ref", b"2") == 0 and sao() == 6
    for bad in (b"3", b"-1", b"x", b"", b"1.5", b"2x"):
        assert lib.QY265ConfigParse(buf, b"sao-ref", bad) == -2 and sao() == 6, bad   # QY265_PARAM_BAD_VALUE, nothing stored
    for v, stored in ((0, 0), (1, 1), (2, 2), (3, 5), (4, 4)):
        assert lib.QY265ConfigParse(buf, b"sao", str(v).encode()) == 0 and sao() == stored
    assert lib.QY265ConfigParse(buf, b"sao", b"5") == -2 and lib.QY265ConfigParse(buf, b"sao", b"6") == -2 and sao() == 4


def test_an_encoder_with_sao_ref_2_codes_pictures(stub_lib, tmp_path):
    log = tmp_path / "tools.log"
    r = subprocess.run([sys.executable, "-c", _DRIVER, ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, KS265_STUB_LIB=stub_lib, KS265_STUB_TOOLS_LOG=str(log)))
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-1200:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["vcl"] == 6
    assert "the reference's decision with merge candidates" in r.stderr + r.stdout            # the open-time log line names the mode
    lines = [l.split() for l in open(log).read().splitlines()]
    assert lines and all(l[3] == "3" for l in lines), lines                                   # the frame objects were made for, and run, ks265_frame_cfg.sao = 3
