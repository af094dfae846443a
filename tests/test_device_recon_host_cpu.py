"""CPU: `devrecon` (include/ks265_enc.h: reconstructed pictures handed out in device memory) in the encoder host, 128x72.
  * against the stand-in of the device library WITHOUT the way back (tests/hip_stub.c) the host loads, says once that device reconstruction is unavailable,
    ks265_enc_get_device_recon is QY_NOTSUPPORTED and the stream is the plain one;
  * against the stand-in WITH it (tests/hip_stub_recon.c): one and two lanes, zero latency, the default GOP - the stream is unchanged, every handed-out picture is fetchable
    once, in the order of the call's NAL units, with the stand-in's picture (the -o dump of a separate run); what is not fetched is released by the next call; a close with
    pending pictures leaves nothing of the stand-in's alive; with the switch off the scheduler thread's calls are the pinned ones (tests/golden/submit_order.json);
  * the bookkeeping unit alone (ks265codec_amd/host/ks265_recon.h) under the sanitizers: tests/recon_pool_main.c, a stand-alone program run as a child process."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from host_harness import (CLIP, LOG_CB, SESSIONS, QY_FAIL, QY_NOTSUPPORTED, QY_OK, QY_POINTER, DevPicture, Nal, Picture, YUV, build_host_lib, build_host_program, digest, load_host_lib, open_handle,
                          scheduler_trace, submit_order_cases)

W, H = 128, 72
FSZ = W * H * 3 // 2


@pytest.fixture(scope="module")
def recon_lib():
    return load_host_lib(build_host_lib("hip_stub_recon.c"))


@pytest.fixture(scope="module")
def plain_lib():
    return load_host_lib(build_host_lib("hip_stub.c"))


def run(lib, n, params=(), latency=b"default", env=None, devrecon=None, dump=None, fetch=lambda k, t: True, close_early=False, bad_first=False):
    """one session.  Returns the stream, the log, and per call the list of fetched (poc, slice type, pts, I420 picture or None when `fetch` left it), plus the counts of
    ks265_enc_device_recon_pending seen before the call's first fetch"""
    lines = []
    cb = LOG_CB(lambda m: lines.append(m.decode()))
    lib.QY265SetLogPrintf(cb)
    h = open_handle(lib, W, H, params=params, latency=latency, env=env, defaults=("devrecon",) if devrecon else ())
    if dump:
        assert lib.ks265_enc_set_recon_file(h, str(dump).encode()) == 0
    nal, nn, pic, outp, yuv, info = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV(), Picture()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    bs, calls, pend = bytearray(), [], []
    dst = np.zeros(FSZ, np.uint8)

    def collect():
        vcl = [nal[i].pts for i in range(nn.value) if nal[i].naltype < 32 and nal[i].iSize > 0]
        bs.extend(b"".join(C.string_at(nal[i].pPayload, nal[i].iSize) for i in range(nn.value) if nal[i].iSize > 0))
        p = lib.ks265_enc_device_recon_pending(h)
        pend.append((p, len(vcl)))
        got = []
        for k in range(p):
            if not fetch(len(calls), k):
                break
            d = DevPicture()
            d.format, d.device = 0, 0
            d.plane[0], d.plane[1], d.plane[2] = dst.ctypes.data, dst.ctypes.data + W * H, dst.ctypes.data + W * H * 5 // 4
            d.pitch[0], d.pitch[1], d.pitch[2] = W, W // 2, W // 2
            if bad_first and not calls and k == 0:                           # a refused destination: the picture stays pending, the handle usable
                d.pitch[0] = W - 1
                assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.byref(info)) == QY_POINTER
                assert lib.ks265_enc_device_recon_pending(h) == p
                d.pitch[0] = W
            dst[:] = 0x5A
            assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.byref(info)) == QY_OK
            assert lib.ks265_enc_device_recon_pending(h) == p - k - 1
            got.append((info.poc, info.iSliceType, info.pts, dst.copy()))
        if got and len(got) == p:
            d = DevPicture()
            assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.byref(info)) == QY_FAIL, "nothing pending"
        calls.append((vcl, got))

    for t in range(n):
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(CLIP[t % len(CLIP)].ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = 1000 + t
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == QY_OK
        collect()
        if close_early and t == n - 1:
            break
    else:
        while lib.QY265EncoderDelayedFrames(h) > 0:
            assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == QY_OK
            collect()
    lanes = lib.ks265_enc_lanes(h)
    lib.QY265EncoderClose(h)
    lib.QY265SetLogPrintf(None)
    return bytes(bs), "".join(lines), calls, pend, lanes


@pytest.mark.parametrize("name", list(SESSIONS))
def test_every_picture_is_fetchable_once_in_nal_order(recon_lib, tmp_path, name):
    kw = SESSIONS[name]
    n = kw["n"]
    plain, log0, calls0, pend0, lanes0 = run(recon_lib, **kw)
    assert "device reconstruction" not in log0
    assert all(p[0] == 0 for p in pend0) and not any(got for _, got in calls0), "switch off: nothing is handed out"
    dump_kw = dict(kw, env={"KS265_GOP_LANES": "1"})                          # the -o dump is one lane's; lanes leave the stream (and so the pictures) as they are
    dumped, _, _, _, _ = run(recon_lib, dump=tmp_path / "rec.yuv", **dump_kw)
    rec = np.fromfile(str(tmp_path / "rec.yuv"), np.uint8).reshape(-1, FSZ)
    assert len(rec) == n
    bs, log, calls, pend, lanes = run(recon_lib, devrecon=1, bad_first=True, **kw)
    assert bs == plain and lanes == lanes0 == (2 if name == "two_lanes" else 1), "the stream (and the lanes) with the switch are those without it"
    assert log.count("ks265enc: device reconstruction: a pool of ") == 1 and "unavailable" not in log
    seen = []
    for (vcl, got), (p, nv) in zip(calls, pend):
        assert p == nv == len(got), "one reconstruction per picture the call handed out"
        assert [g[2] for g in got] == vcl, "in the order of the call's NAL units (pts)"
        for poc, st, pts, pix in got:
            assert pts == 1000 + poc and st in (0, 1, 2)
            # (the stand-in stamps a picture's first two luma rows with its frame object's state: a key picture on the key pictures' own stream - which the -o dump
            #  switches off - carries another stamp there than on the main stream; the run below compares those rows too)
            assert (pix[2 * W:] == rec[poc][2 * W:]).all(), (name, poc)
            seen.append(poc)
    assert sorted(seen) == list(range(n)), "every picture exactly once"
    if name == "zerolatency":
        assert all(p == 1 for p, _ in pend)
    if name == "default_gop":
        assert seen != sorted(seen), "coding order, not display order"
    assert len({rec[i].tobytes() for i in range(n)}) == n, "the stand-in's pictures differ: every slot held its own"
    if name != "two_lanes":
        # key pictures on the main stream, as in the dump's run: every byte of every picture, the stamped rows included.  (Not with two lanes: there the stand-in's second GOP
        # meets a frame object that has coded no P picture yet, and is stamped otherwise than in the dump's one lane.)
        same = dict(kw, env=dict(kw.get("env", {}), KS265_NO_KEY_OVERLAP="1"))
        bs2, _, calls2, _, _ = run(recon_lib, devrecon=1, **same)
        assert bs2 == dumped
        got2 = {poc: pix for _, got in calls2 for poc, _, _, pix in got}
        assert sorted(got2) == list(range(n)) and all((got2[i] == rec[i]).all() for i in range(n))


def test_unfetched_pictures_are_released_by_the_next_call(recon_lib):
    """300 pictures through a pool of 128 (the ring at this size) while only every third hand-out is fetched, and in some calls none: nothing stalls, the stream stays"""
    kw = dict(n=300, params=(("iper", 128), ("bframes", 0)))
    plain = run(recon_lib, **kw)[0]
    bs, log, calls, pend, _ = run(recon_lib, devrecon=1, fetch=lambda call, k: call % 3 == 0, **kw)
    assert bs == plain
    assert "a pool of 128 packed" in log
    assert sum(p for p, _ in pend) == 300 and sum(len(g) for _, g in calls) < 150
    for (vcl, got), (p, nv) in zip(calls, pend):
        assert p == nv, "what a call reports as pending is what IT handed out: the previous call's leftovers are gone"


def test_close_with_pending_pictures_leaves_nothing_alive(recon_lib):
    for kw in (SESSIONS["ippp"], SESSIONS["two_lanes"]):
        _, _, calls, pend, _ = run(recon_lib, devrecon=1, fetch=lambda call, k: False, close_early=True, **kw)
        assert sum(p for p, _ in pend) > 0
        assert [recon_lib.ks265_stub_live(k) for k in range(5)] == [0] * 5, "contexts, frame objects, events, device and pinned blocks"


def test_switch_values_and_environment(recon_lib):
    for v, rc in ((0, 0), (1, 0), (2, -2), (-1, -2), (0, 0)):                  # QY265_PARAM_BAD_VALUE = -2
        assert recon_lib.ks265_enc_set_default(b"devrecon", C.c_int(v)) == rc, v
    kw = SESSIONS["ippp"]
    _, log, calls, pend, _ = run(recon_lib, env={"KS265_DEVRECON": "1"}, **kw)
    assert sum(p for p, _ in pend) == kw["n"] and "a pool of" in log
    _, log, calls, pend, _ = run(recon_lib, devrecon=1, env={"KS265_DEVRECON": "0"}, **kw)
    assert sum(p for p, _ in pend) == 0 and "device reconstruction" not in log
    # refused at open, with a line, the switch then off: the graph experiment; lanes on several GPUs
    for env, why in (({"KS265_GRAPH": "1"}, "KS265_GRAPH"), ({"KS265_GOP_LANES": "2", "KS265_GPUS": "2"}, "several GPUs")):
        plain = run(recon_lib, env=env, **kw)[0]
        bs, log, calls, pend, _ = run(recon_lib, devrecon=1, env=env, **kw)
        assert bs == plain and sum(p for p, _ in pend) == 0
        assert log.count("ks265enc: device reconstruction is unavailable: ") == 1 and why in log


def test_device_library_without_the_way_back(plain_lib):
    assert hasattr(plain_lib, "ks265_enc_get_device_recon") and not hasattr(plain_lib, "ks265_output_convert")
    for name in ("ippp", "two_lanes"):
        kw = SESSIONS[name]
        plain, log0, _, _, _ = run(plain_lib, **kw)
        bs, log, calls, pend, _ = run(plain_lib, devrecon=1, fetch=lambda call, k: False, **kw)
        assert bs == plain and len(plain) > 100 and all(p == 0 for p, _ in pend)
        assert log.count("ks265enc: device reconstruction is unavailable: ") == 1 and "unavailable" not in log0
    # ks265_enc_get_device_recon on such a handle
    lib = plain_lib
    h = open_handle(lib, W, H, params=(("log", 3),), defaults=("devrecon",))
    d, info = DevPicture(), Picture()
    assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.byref(info)) == QY_NOTSUPPORTED
    assert lib.ks265_enc_device_recon_pending(h) == 0
    lib.QY265EncoderClose(h)


@pytest.mark.parametrize("case", ["plain_ippp", "plain_hier8", "no_split_hier8"])
def test_switch_off_the_scheduler_threads_calls_are_the_pinned_ones(tmp_path, case):
    """the stand-in WITH the way back, the switch off: the scheduler thread's calls to the device library are those tests/golden/submit_order.json pins - not one call added"""
    lib = build_host_lib("hip_stub_recon.c", ("KS265_STUB_SSIM",))
    c = submit_order_cases()[case]
    lines = scheduler_trace(lib, c, str(tmp_path / "calls.log"))
    assert len(lines) == c["lines"] and digest(lines) == c["sha256"]
    on = scheduler_trace(lib, dict(c, env=dict(c["env"], KS265_DEVRECON=1)), str(tmp_path / "calls_on.log"))
    assert len(on) > c["lines"] and sum(ln.startswith("ks265_store_i420 ") for ln in on) == c["n"], "and with it on: one pack per picture"


def test_bookkeeping_unit_under_the_sanitizers():
    """ks265_recon.h driven alone by a stand-alone program built with -fsanitize=address,undefined, as a child process"""
    exe = build_host_program("recon_pool_main.c")
    for seed in (1, 2, 3):
        r = subprocess.run([exe, str(seed), "60000"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-400:] + r.stderr[-2000:]
        takes, outs, fetches, releases, refusals = (int(x) for x in r.stdout.split()[1:])
        assert min(takes, outs, fetches, releases, refusals) > 1000, "every kind of step ran"
