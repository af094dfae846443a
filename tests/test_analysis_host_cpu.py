"""CPU: `analysis` (include/ks265_enc.h: motion, modes, QP and block error of every picture fetched as arrays in device memory) in the encoder host, 128x72.
  * against the stand-in of the device library WITHOUT the entries (tests/hip_stub.c) the host says once that the analysis is unavailable, ks265_enc_get_device_analysis is
    QY_NOTSUPPORTED and the stream is the plain one;
  * against the stand-in WITH them (tests/hip_stub_analysis.c, which records what the host passed for each picture): one and two lanes, zero latency, the default GOP,
    -bframes 3, IPPP - the stream is unchanged; pending counts equal the call's VCL NAL units; every picture is fetchable exactly once, in NAL order, and its block is ITS
    block (the stand-in's stamp of the source picture); info matches pOutpic / the reconstruction's info; the picture's QP and the lists' POC deltas are the GOP plan's;
    unfetched slots are released by the next call; a close with pending pictures leaves nothing alive; devrecon + analysis together with interleaved fetches; analysis alone
    allocates no reconstruction memory;
  * the shared bookkeeping with two fetch cursors (ks265codec_amd/host/ks265_recon.h) under the sanitizers: tests/analysis_list_main.c, a stand-alone program run as a child."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import host_harness
from host_harness import (CLIP, LOG_CB, QY_FAIL, QY_NOTSUPPORTED, QY_OK, QY_POINTER, DevPicture, Nal, Picture, YUV, build_host_lib, build_host_program, digest, load_host_lib,
                          open_handle, scheduler_trace, submit_order_cases)

W, H = 128, 72
FSZ = W * H * 3 // 2
W8, H8, CC, CR = W // 8, H // 8, (W + 63) // 64, (H + 63) // 64
MAGIC = 0x414E4C59


class AnField(C.Structure):
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_int), ("plane", C.c_longlong)]


class DevAnalysis(C.Structure):
    _fields_ = [("device", C.c_int), ("stream", C.c_void_p), ("mv", AnField), ("ref", AnField), ("cu", AnField), ("qp", AnField), ("sse", AnField)]


@pytest.fixture(scope="module")
def an_lib():
    return load_host_lib(build_host_lib("hip_stub_analysis.c"))


@pytest.fixture(scope="module")
def plain_lib():
    return load_host_lib(build_host_lib("hip_stub.c"))


class Arrays:
    """the caller's five arrays (host memory: the stand-in's device) with padded pitches, and their descriptor"""

    def __init__(self):
        self.mv = np.zeros((2, H8, W8 + 3, 2), np.int16)
        self.ref = np.zeros((2, H8, W8 + 5), np.int8)
        self.cu = np.zeros((5, H8, W8 + 1), np.uint8)
        self.qp = np.zeros((CR, CC + 7), np.int8)
        self.sse = np.zeros((3, H8, W8 + 2), np.int32)

    def desc(self, wanted=("mv", "ref", "cu", "qp", "sse")):
        d = DevAnalysis()
        d.device = 0
        for n in wanted:
            a = getattr(self, n)
            setattr(d, n, AnField(a.ctypes.data, a.strides[0] if n == "qp" else a.strides[1], 0 if n == "qp" else a.strides[0]))
        return d

    def fill(self, v):
        for n in ("mv", "ref", "cu", "qp", "sse"):
            getattr(self, n).view(np.uint8)[...] = v                      # every byte

    def fields(self):
        """what the stand-in's export lays out: (picture QP, has_map, list deltas [2][4], the source picture's first eight luma bytes)"""
        assert int(self.sse[0, 0, 0]) == MAGIC and not self.cu[:, :, :W8].any() and not self.ref[:, 1:, :W8].any() and not self.ref[:, 0, 4:W8].any()
        assert (self.qp[:, CC:] == 0x5A).all() and (self.ref[:, :, W8:] == 0x5A).all() and (self.sse[:, :, W8:] == 0x5A5A5A5A).all() and (self.mv[:, :, W8:] == 0x5A5A).all(), "behind a pitch"
        has_map = int(self.sse[0, 0, 1])
        qp = self.qp[:, :CC].reshape(-1)
        assert (qp[1:] == qp[1]).all() if qp.size > 1 else True
        return int(qp[-1]), has_map, self.ref[:, 0, :4].astype(int).tolist(), self.mv[0, 0, :2].copy().view(np.uint8).tobytes()


def run(lib, n, params=(), latency=b"default", env=None, analysis=None, devrecon=None, fetch=lambda call, k: True, order="an_first", close_early=False, bad_first=False, wanted=None):
    """one session.  Per call: (pts of its VCL NAL units, fetched analyses [(poc, slice type, pts, fields)], fetched reconstruction infos [(poc, slice type, pts)], pOutpic's
    (poc, slice type, pts)); per call the pending counts (analyses, reconstructions, VCL NAL units); device blocks alive right after the open"""
    lines = []
    cb = LOG_CB(lambda m: lines.append(m.decode()))
    lib.QY265SetLogPrintf(cb)
    h = open_handle(lib, W, H, params=params, latency=latency, env=env, defaults=[name for name, v in (("analysis", analysis), ("devrecon", devrecon)) if v])
    live_dev = lib.ks265_stub_live(3) if hasattr(lib, "ks265_stub_live") else -1
    nal, nn, pic, outp, yuv, info = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV(), Picture()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    bs, calls, pend = bytearray(), [], []
    arr, dst = Arrays(), np.zeros(FSZ, np.uint8)

    def fetch_an(p, k, first):
        d = arr.desc(wanted or ("mv", "ref", "cu", "qp", "sse"))
        if bad_first and first and k == 0:                                   # a refused field: the picture stays pending, the handle usable
            d.ref.pitch = W8 - 1
            assert lib.ks265_enc_get_device_analysis(h, C.byref(d), C.byref(info)) == QY_POINTER
            assert lib.ks265_enc_get_device_analysis(h, C.byref(DevAnalysis()), C.byref(info)) == QY_POINTER      # no field wanted
            d.device = 1
            assert lib.ks265_enc_get_device_analysis(h, C.byref(d), C.byref(info)) == QY_NOTSUPPORTED            # another GPU's memory
            assert lib.ks265_enc_device_analysis_pending(h) == p
            d = arr.desc()
        arr.fill(0x5A)
        assert lib.ks265_enc_get_device_analysis(h, C.byref(d), C.byref(info)) == QY_OK
        assert lib.ks265_enc_device_analysis_pending(h) == p - k - 1
        return (info.poc, info.iSliceType, info.pts, arr.fields() if not wanted else None)

    def fetch_rec(p, k):
        d = DevPicture()
        d.format, d.device = 0, 0
        d.plane[0], d.plane[1], d.plane[2] = dst.ctypes.data, dst.ctypes.data + W * H, dst.ctypes.data + W * H * 5 // 4
        d.pitch[0], d.pitch[1], d.pitch[2] = W, W // 2, W // 2
        assert lib.ks265_enc_get_device_recon(h, C.byref(d), C.byref(info)) == QY_OK
        assert lib.ks265_enc_device_recon_pending(h) == p - k - 1
        return (info.poc, info.iSliceType, info.pts)

    def collect():
        vcl = [nal[i].pts for i in range(nn.value) if nal[i].naltype < 32 and nal[i].iSize > 0]
        bs.extend(b"".join(C.string_at(nal[i].pPayload, nal[i].iSize) for i in range(nn.value) if nal[i].iSize > 0))
        pa, pr = lib.ks265_enc_device_analysis_pending(h), lib.ks265_enc_device_recon_pending(h)
        pend.append((pa, pr, len(vcl)))
        na = sum(1 for k in range(pa) if fetch(len(calls), k))
        got_an, got_rec = [], []
        if order == "an_first":
            got_an = [fetch_an(pa, k, not calls) for k in range(na)]
            got_rec = [fetch_rec(pr, k) for k in range(pr)]
        elif order == "rec_first":
            got_rec = [fetch_rec(pr, k) for k in range(pr)]
            got_an = [fetch_an(pa, k, not calls) for k in range(na)]
        else:                                                                # interleaved, the reconstructions one ahead; then whatever is left of either
            for k in range(max(na, pr)):
                if k < pr:
                    got_rec.append(fetch_rec(pr, k))
                if k < na:
                    got_an.append(fetch_an(pa, k, not calls))
                assert lib.ks265_enc_device_recon_pending(h) == pr - len(got_rec) and lib.ks265_enc_device_analysis_pending(h) == pa - len(got_an)
        if pa and len(got_an) == pa:
            assert lib.ks265_enc_get_device_analysis(h, C.byref(arr.desc()), C.byref(info)) == QY_FAIL, "nothing pending"
        calls.append((vcl, got_an, got_rec, (outp.poc, outp.iSliceType, outp.pts)))

    t = 0
    while t < n or (close_early and not pend[-1][0] and t < 50 * n):        # close_early: closed while something IS pending, however far the output lags behind the input
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(CLIP[t % len(CLIP)].ctypes.data + off, C.POINTER(C.c_ubyte))
        pic.pts = 1000 + t
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == QY_OK
        collect()
        t += 1
    if not close_early:
        while lib.QY265EncoderDelayedFrames(h) > 0:
            assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == QY_OK
            collect()
    lanes = lib.ks265_enc_lanes(h)
    lib.QY265EncoderClose(h)
    lib.QY265SetLogPrintf(None)
    return bytes(bs), "".join(lines), calls, pend, lanes, live_dev


SESSIONS = dict(host_harness.SESSIONS, bframes3=dict(n=40, params=(("iper", 32), ("bframes", 3))))


def check_plan(name, st, qp, has_map, deltas):
    """what the GOP plan says of a picture of slice type st: -rc 0 without -aq passes no QP map; a key picture has no lists; IPPP predicts from the picture before (and,
    with more references, from the ones before that, nearest first); a B picture has a past picture in list 0 and a future one in list 1"""
    l0, l1 = deltas
    assert not has_map and 0 <= qp <= 51
    if st == 2:
        assert l0 == [0, 0, 0, 0] and l1 == [0, 0, 0, 0], "a key picture has no lists"
        assert qp == 34
        return
    n0 = [d for d in l0 if d]
    assert l0[0] < 0 and n0 == l0[:len(n0)] and all(a > b for a, b in zip(n0, n0[1:])), ("list 0: past pictures, nearest first", l0)
    if name in ("ippp", "two_lanes", "zerolatency"):
        assert st == 1 and l0[0] == -1 and l1 == [0, 0, 0, 0]
    if st == 1:
        assert l1 == [0, 0, 0, 0]
    if st == 0:
        n1 = [d for d in l1 if d]
        assert l1[0] > 0 and n1 == l1[:len(n1)] and all(d > 0 for d in n1), ("list 1 of a B picture: future pictures", l1)
        assert max(max(n1), -min(n0)) <= (4 if name == "bframes3" else 8)


@pytest.mark.parametrize("name", list(SESSIONS))
def test_every_analysis_is_fetchable_once_in_nal_order(an_lib, name):
    kw = SESSIONS[name]
    n = kw["n"]
    plain, log0, calls0, pend0, lanes0, live0 = run(an_lib, **kw)
    assert "analysis" not in log0 and all(p[0] == 0 and p[1] == 0 for p in pend0) and not any(c[1] for c in calls0), "switch off: nothing is handed out"
    bs, log, calls, pend, lanes, live1 = run(an_lib, analysis=1, bad_first=True, **kw)
    assert bs == plain and lanes == lanes0 == (2 if name == "two_lanes" else 1), "the stream (and the lanes) with the switch are those without it"
    assert log.count("ks265enc: analysis: a pool of ") == 1 and "unavailable" not in log and "device reconstruction" not in log      # (one lane of a handle speaks)
    slots = int(re.search(r"analysis: a pool of (\d+) blocks of 256 bytes", log).group(1))
    assert live1 - live0 == slots * lanes, "analysis alone: one block per slot and no reconstruction memory"
    seen, kinds = [], set()
    for (vcl, got, rec, outp), (pa, pr, nv) in zip(calls, pend):
        assert pa == nv == len(got) and pr == 0 and not rec, "one analysis per picture the call handed out; no reconstructions without devrecon"
        assert [g[2] for g in got] == vcl, "in the order of the call's NAL units (pts)"
        for poc, st, pts, (qp, has_map, deltas, stamp) in got:
            assert pts == 1000 + poc and st in (0, 1, 2)
            assert stamp == CLIP[poc % len(CLIP)][:8].tobytes(), (name, poc, "the block is another picture's")
            check_plan(name, st, qp, has_map, deltas)
            seen.append(poc); kinds.add(st)
        if got:
            assert got[-1][:3] == outp, "info of the call's last picture is pOutpic's"
    assert sorted(seen) == list(range(n)), "every picture exactly once"
    assert kinds == ({0, 1, 2} if name in ("default_gop", "bframes3") else {1, 2}) or (name == "default_gop" and kinds == {0, 2})
    if name == "zerolatency":
        assert all(p[0] == 1 for p in pend)
    if name in ("default_gop", "bframes3"):
        assert seen != sorted(seen), "coding order, not display order"


@pytest.mark.parametrize("order", ["an_first", "rec_first", "interleaved"])
@pytest.mark.parametrize("name", ["default_gop", "two_lanes"])
def test_devrecon_and_analysis_together(an_lib, name, order):
    kw = SESSIONS[name]
    plain = run(an_lib, **kw)[0]
    only_rec = run(an_lib, devrecon=1, **kw)
    bs, log, calls, pend, lanes, live = run(an_lib, analysis=1, devrecon=1, order=order, fetch=lambda call, k: k % 2 == 0, **kw)       # the first half of every call's analyses, rounded up
    assert bs == plain
    assert log.count("ks265enc: analysis: a pool of ") == 1 and log.count("ks265enc: device reconstruction: a pool of ") == 1 and "the slots of the device reconstruction's pool" in log
    slots = [int(x) for x in re.findall(r"analysis: a pool of (\d+) blocks", log)]
    assert slots == [int(x) for x in re.findall(r"device reconstruction: a pool of (\d+) packed", only_rec[1])], "the pool's size is devrecon's"
    assert live - only_rec[5] == slots[0] * lanes, "one analysis block per slot on top of devrecon's memory"
    for (vcl, got, rec, outp), (pa, pr, nv) in zip(calls, pend):
        assert pa == pr == nv == len(rec) and [r[2] for r in rec] == vcl, "the reconstructions, all fetched, in NAL order"
        assert [g[:3] for g in got] == rec[:len(got)], "an analysis's info is its reconstruction's"
        for poc, st, pts, (qp, has_map, deltas, stamp) in got:
            assert stamp == CLIP[poc % len(CLIP)][:8].tobytes()
    assert sum(len(c[2]) for c in calls) == kw["n"] and [len(c[1]) for c in calls] == [(p[0] + 1) // 2 for p in pend] and any(c[1] for c in calls)


def test_unfetched_analyses_are_released_by_the_next_call(an_lib):
    """300 pictures through a pool of 128 (the ring at this size) while at most half of every call's analyses are fetched (none of a call that hands out one picture) -
    however the output bunches up, more pictures stay unfetched than the pool has slots: nothing stalls, the stream stays"""
    kw = dict(n=300, params=(("iper", 128), ("bframes", 0)))
    plain = run(an_lib, **kw)[0]
    bs, log, calls, pend, _, _ = run(an_lib, analysis=1, fetch=lambda call, k: k % 2 == 1, **kw)
    assert bs == plain and "a pool of 128 blocks" in log
    assert sum(p[0] for p in pend) == 300 and [len(c[1]) for c in calls] == [p[0] // 2 for p in pend] and sum(p[0] - p[0] // 2 for p in pend) > 128
    for (vcl, got, _, _), (pa, _, nv) in zip(calls, pend):
        assert pa == nv, "what a call reports as pending is what IT handed out: the previous call's leftovers are gone"


def test_a_subset_of_fields(an_lib):
    kw = SESSIONS["ippp"]
    _, _, calls, pend, _, _ = run(an_lib, analysis=1, wanted=("qp",), **kw)
    assert sum(len(c[1]) for c in calls) == kw["n"]


def test_close_with_pending_analyses_leaves_nothing_alive(an_lib):
    for kw, both in ((SESSIONS["ippp"], 0), (SESSIONS["two_lanes"], 1)):
        _, _, calls, pend, _, _ = run(an_lib, analysis=1, devrecon=both or None, fetch=lambda call, k: False, close_early=True, **kw)
        assert sum(p[0] for p in pend) > 0
        assert [an_lib.ks265_stub_live(k) for k in range(5)] == [0] * 5, "contexts, frame objects, events, device and pinned blocks"


def test_switch_values_and_environment(an_lib):
    for v, rc in ((0, 0), (1, 0), (2, -2), (-1, -2), (0, 0)):                  # QY265_PARAM_BAD_VALUE = -2
        assert an_lib.ks265_enc_set_default(b"analysis", C.c_int(v)) == rc, v
    kw = SESSIONS["ippp"]
    _, log, calls, pend, _, _ = run(an_lib, env={"KS265_ANALYSIS": "1"}, **kw)
    assert sum(p[0] for p in pend) == kw["n"] and "analysis: a pool of" in log
    _, log, calls, pend, _, _ = run(an_lib, analysis=1, env={"KS265_ANALYSIS": "0"}, **kw)
    assert sum(p[0] for p in pend) == 0 and "analysis" not in log
    # refused at open, with a line, the switch then off: the graph experiment; lanes on several GPUs
    for env, why in (({"KS265_GRAPH": "1"}, "KS265_GRAPH"), ({"KS265_GOP_LANES": "2", "KS265_GPUS": "2"}, "several GPUs")):
        plain = run(an_lib, env=env, **kw)[0]
        bs, log, calls, pend, _, _ = run(an_lib, analysis=1, env=env, **kw)
        assert bs == plain and sum(p[0] for p in pend) == 0
        assert log.count("ks265enc: analysis is unavailable: ") == 1 and why in log


def test_device_library_without_the_entries(plain_lib):
    assert hasattr(plain_lib, "ks265_enc_get_device_analysis") and not hasattr(plain_lib, "ks265_analysis_pack")
    for name in ("ippp", "two_lanes"):
        kw = SESSIONS[name]
        plain, log0, _, _, _, _ = run(plain_lib, **kw)
        bs, log, calls, pend, _, _ = run(plain_lib, analysis=1, fetch=lambda call, k: False, **kw)
        assert bs == plain and len(plain) > 100 and all(p[0] == 0 for p in pend)
        assert log.count("ks265enc: analysis is unavailable: ") == 1 and "unavailable" not in log0
    lib = plain_lib
    h = open_handle(lib, W, H, params=(("log", 3),), defaults=("analysis",))
    assert lib.ks265_enc_get_device_analysis(h, C.byref(Arrays().desc()), C.byref(Picture())) == QY_NOTSUPPORTED
    assert lib.ks265_enc_device_analysis_pending(h) == 0
    lib.QY265EncoderClose(h)


@pytest.mark.parametrize("case", ["plain_ippp", "plain_hier8", "no_split_hier8"])
def test_switch_off_the_scheduler_threads_calls_are_the_pinned_ones(tmp_path, case):
    """the stand-in WITH the entries, the switch off: the scheduler thread's calls to the device library are those tests/golden/submit_order.json pins - not one call added;
    with it on: one pack per picture, and one record of the slot's ev_packed behind it"""
    lib = build_host_lib("hip_stub_analysis.c", ("KS265_STUB_SSIM",))
    c = submit_order_cases()[case]
    lines = scheduler_trace(lib, c, str(tmp_path / "calls.log"))
    assert len(lines) == c["lines"] and digest(lines) == c["sha256"]
    on = scheduler_trace(lib, dict(c, env=dict(c["env"], KS265_ANALYSIS=1)), str(tmp_path / "calls_on.log"))
    packs = [i for i, ln in enumerate(on) if ln.startswith("ks265_analysis_pack_on ")]
    assert len(packs) == c["n"] and len(on) == c["lines"] + 2 * c["n"], "one pack and one event record per picture, nothing else"
    assert all(on[i + 1].startswith("ks265_event_record ") for i in packs)
    both = scheduler_trace(lib, dict(c, env=dict(c["env"], KS265_ANALYSIS=1, KS265_DEVRECON=1)), str(tmp_path / "calls_both.log"))
    assert len(both) == c["lines"] + 3 * c["n"], "both switches: two packs, ONE record of ev_packed"


def test_bookkeeping_with_two_cursors_under_the_sanitizers():
    """ks265_recon.h with both fetch cursors driven alone by a stand-alone program built with -fsanitize=address,undefined, as a child process"""
    exe = build_host_program("analysis_list_main.c")
    for seed in (1, 2, 3):
        r = subprocess.run([exe, str(seed), "60000"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-400:] + r.stderr[-2000:]
        assert min(int(x) for x in r.stdout.split()[1:]) > 1000, "every kind of step ran"
