"""GPU: the C host (libks265enc.so: SDK-compatible API over the HIP path + bitstream writer) and its CLI.
  * `ks265enc -preset slow -rc 0 -qp 27 -bframes 0` on the clip of stream case ippp_416x240_umh writes byte for byte the stream that the
    reference decoder verified (tests/golden/stream_md5.json) - the C host, the Python test mirror and the oracle agree;
  * the API with the SDK's default GOP (hierarchical B, 8) and with -bframes 3: call sequence of the SDK's own callers, NAL bookkeeping,
    delayed-frame accounting; the streams are left in gpurun_out/ so that the builder container can decode them with appdecoder."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from host_harness import LAY, YUV, Nal, Picture
from stream_cases import CASES

pytestmark = pytest.mark.gpu
# torch carries its own copy of the HIP runtime: let it load first, so that the other GPU test modules of the same pytest process (which use
# torch for device memory) are not handed the system copy that libks265enc.so -> libks265hip.so would otherwise pull in
import torch  # noqa: E402
torch.cuda.is_available()
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "stream_md5.json")))
OUT = os.path.join(ROOT, "gpurun_out")


def _clip(name, n):
    from ks265codec_amd.synth import make_clip
    W, H = CASES[name][0], CASES[name][1]
    return make_clip(W, H, n, seed=len(name) * 7 + W, abc=(17, 23, 9))


def test_cli_stream_equals_decoder_verified_fixture(tmp_path):
    from ks265codec_amd import stream
    stream.build()
    name = "enc_ippp_416x240_umh"                      # what the C host runs: sign-data hiding, pre-search candidates, merge pass, CTU rows as WPP substreams (the skip pass acts on B pictures only)
    clip = _clip(name, 4)
    yuv, out = tmp_path / "in.yuv", tmp_path / "out.265"
    clip.tofile(yuv)
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", "416", "-hgt", "240", "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "27", "-iper", "128", "-bframes", "0",
                        "-threads", "3", "-psnr", "2", "-b", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    assert "H265 encoder passed!!!" in r.stdout and "Total Frames: 4" in r.stdout and "bitrate, psnr:" in r.stdout, r.stdout
    bs = open(out, "rb").read()
    assert hashlib.md5(bs).hexdigest() == GOLD[name]["stream_md5"], f"CLI stream differs from the decoder-verified fixture ({len(bs)} vs {GOLD[name]['stream_bytes']} bytes)"


@pytest.mark.parametrize("W,H,n,iper", [(416, 240, 230, 32), (200, 136, 150, 48)])
def test_gop_lanes_write_the_one_lane_stream(tmp_path, W, H, n, iper):
    """GOP lanes (closed GOPs coded concurrently on one GPU, ks265_enc.c): 2 and 3 lanes write byte for byte what one lane writes - GOP order kept,
    the last (short) GOP and the flush included"""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    stream.build()
    clip = make_clip(W, H, 23, seed=77, abc=(17, 23, 9))
    yuv = tmp_path / "in.yuv"
    with open(yuv, "wb") as f:
        for t in range(n):
            f.write(clip[t % 23].tobytes())
    md5 = {}
    for lanes in (1, 2, 3):
        out = tmp_path / f"l{lanes}.265"
        r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "30", "-iper", str(iper), "-bframes", "0",
                            "-threads", "6", "-psnr", "1", "-b", str(out)], capture_output=True, text=True, env=dict(os.environ, KS265_GOP_LANES=str(lanes)))
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
        assert f"Total Frames: {n}" in r.stdout and "H265 encoder passed!!!" in r.stdout, r.stdout[-400:]
        assert ("GOP lanes" in (r.stdout + r.stderr)) == (lanes > 1), r.stdout[:600] + r.stderr[:600]      # switched on by KS265_GOP_LANES only
        md5[lanes] = hashlib.md5(open(out, "rb").read()).hexdigest()
    assert md5[1] == md5[2] == md5[3], md5
    # the same lanes reached through the device list (one handle, N GPUs: KS265_DEVICES / ks265enc -gpus N); this box has one GPU, so the list names it twice
    out = tmp_path / "dev.265"
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "30", "-iper", str(iper), "-bframes", "0",
                        "-threads", "6", "-psnr", "1", "-b", str(out)], capture_output=True, text=True, env=dict(os.environ, KS265_DEVICES="0,0"))
    assert r.returncode == 0 and "2 GOP lanes on 2 GPU(s)" in (r.stdout + r.stderr), r.stdout[-400:] + r.stderr[-400:]
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == md5[1]
    if os.path.exists(REF_DEC):
        d = subprocess.run([REF_DEC, "-b", str(tmp_path / "l2.265"), "-o", str(tmp_path / "d.yuv"), "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
        assert d.returncode == 0 and os.path.getsize(tmp_path / "d.yuv") == n * W * H * 3 // 2, d.stdout[-300:] + d.stderr[-300:]


_LANES_DRIVER = r"""
import ctypes as C, hashlib, json, os, sys
import torch; torch.cuda.is_available()
sys.path.insert(0, sys.argv[1])
from ks265codec_amd import stream
from ks265codec_amd.synth import make_clip
W, H, N, iper = 416, 240, int(sys.argv[2]), int(sys.argv[3])
LAY = json.load(open(os.path.join(sys.argv[1], "tests", "golden", "qy265_layout.json")))
lib = C.CDLL(stream.build()); lib.QY265EncoderOpen.restype = C.c_void_p
class YUV(C.Structure): _fields_ = [("iWidth", C.c_int), ("iHeight", C.c_int), ("pData", C.POINTER(C.c_ubyte) * 3), ("iStride", C.c_int * 3)]
class Picture(C.Structure): _fields_ = [("iSliceType", C.c_int), ("poc", C.c_int), ("pts", C.c_longlong), ("dts", C.c_longlong), ("yuv", C.POINTER(YUV))]
class Nal(C.Structure): _fields_ = [("naltype", C.c_int), ("tid", C.c_int), ("iSize", C.c_int), ("pts", C.c_longlong), ("pPayload", C.POINTER(C.c_ubyte))]
clip = make_clip(W, H, 7, seed=3, abc=(17, 23, 9))
cfg = (C.c_uint8 * LAY["sizeof_config"])()
assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, b"default") == 0
for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 34), ("iper", iper), ("bframes", int(os.environ.get("KS_TEST_BFRAMES", "0"))), ("threads", 6), ("psnr", 0), ("log", 3)):
    assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
err = C.c_int(0)
h = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err))); assert h.value
nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
yuv.iWidth, yuv.iHeight = W, H
yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
pic.yuv = C.pointer(yuv)
md, pts, pocs = hashlib.md5(), [], []
def take():
    for i in range(nn.value):
        md.update(C.string_at(nal[i].pPayload, nal[i].iSize))
        if nal[i].naltype < 32: pts.append(nal[i].pts)
    if nn.value: pocs.append(outp.poc)
for t in range(N):
    fr = clip[t % 7]
    for k, off in enumerate((0, W * H, W * H * 5 // 4)): yuv.pData[k] = C.cast(fr.ctypes.data + off, C.POINTER(C.c_ubyte))
    pic.pts = t
    assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == 0
    take()
while lib.QY265EncoderDelayedFrames(h):
    assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
    take()
lanes = lib.ks265_enc_lanes(h)
lib.QY265EncoderClose(h)
if int(os.environ.get("KS_TEST_BFRAMES", "0")) == 0:
    assert pts == list(range(N)), "pictures must leave in stream order"
    assert pocs == sorted(pocs) and pocs[-1] == N - 1, pocs[-5:]
else:
    assert sorted(pts) == list(range(N))
print(json.dumps({"md5": md.hexdigest(), "lanes": lanes}))
"""


def test_pyramid_gops_run_on_two_lanes_by_default(tmp_path):
    """round 5: the SDK's default GOP (hierarchical B, 8, slice-type decision) and -bframes 3 open two GOP lanes on one GPU by themselves; the stream is the one-lane stream
    (KS265_GOP_LANES=1), the reference decoder takes it, -bframes 0 stays on one lane"""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    stream.build()
    W, H, n, iper = 416, 240, 210, 48
    clip = make_clip(W, H, 23, seed=78, abc=(17, 23, 9))
    yuv = tmp_path / "in.yuv"
    with open(yuv, "wb") as f:
        for t in range(n):
            f.write(clip[t % 23].tobytes())
    env0 = {k: v for k, v in os.environ.items() if k != "KS265_GOP_LANES"}
    for extra, tag in (([], "default"), (["-bframes", "3"], "b3")):
        md5 = {}
        for lanes in (None, 1):
            out = tmp_path / f"{tag}_{lanes}.265"
            r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "30", "-iper", str(iper), *extra,
                                "-threads", "6", "-psnr", "1", "-b", str(out)], capture_output=True, text=True, env=dict(env0, **({"KS265_GOP_LANES": "1"} if lanes else {})))
            assert r.returncode == 0 and f"Total Frames: {n}" in r.stdout and "H265 encoder passed!!!" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
            assert ("2 GOP lanes" in (r.stdout + r.stderr)) == (lanes is None), r.stdout[:600] + r.stderr[:600]
            md5[lanes] = hashlib.md5(open(out, "rb").read()).hexdigest()
        assert md5[None] == md5[1], (tag, md5)
        if os.path.exists(REF_DEC):
            d = subprocess.run([REF_DEC, "-b", str(tmp_path / f"{tag}_None.265"), "-o", str(tmp_path / "d.yuv"), "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
            assert d.returncode == 0 and os.path.getsize(tmp_path / "d.yuv") == n * W * H * 3 // 2, d.stdout[-300:] + d.stderr[-300:]
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "30", "-iper", str(iper), "-bframes", "0",
                        "-threads", "6", "-frms", "60", "-b", str(tmp_path / "p.265")], capture_output=True, text=True, env=env0)
    assert r.returncode == 0 and "GOP lanes" not in (r.stdout + r.stderr)


@pytest.mark.parametrize("n,iper", [(1500, 300), (700, 64)])
def test_gop_lanes_under_a_fast_caller(tmp_path, n, iper):
    """the caller feeds as fast as the API takes pictures (no file read in between): with GOPs longer than a lane's ring the lanes fill up completely, input
    waits for older GOPs to leave, the scheduler threads wait for ring space - and the stream still is the one-lane stream.  Each run is a process of its
    own under a hard time limit: a dead-lock shows as a failure, not as a hung test session."""
    res = {}
    for lanes in (1, 2, 3):
        r = subprocess.run([sys.executable, "-c", _LANES_DRIVER, ROOT, str(n), str(iper)], capture_output=True, text=True, timeout=120, env=dict(os.environ, KS265_GOP_LANES=str(lanes)))
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        res[lanes] = json.loads(r.stdout.strip().splitlines()[-1])
        assert res[lanes]["lanes"] == lanes
    assert res[1]["md5"] == res[2]["md5"] == res[3]["md5"], res
    # KS265_GRAPH=1 (opt-in since round 4): P pictures are replayed as captured graphs from the ninth picture on (ks265_capture_begin / ks265_graph_launch): same stream as the launch-by-launch path
    r = subprocess.run([sys.executable, "-c", _LANES_DRIVER, ROOT, str(n), str(iper)], capture_output=True, text=True, timeout=120, env=dict(os.environ, KS265_GOP_LANES="1", KS265_GRAPH="1"))
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["md5"] == res[1]["md5"], "graph replay and plain launches disagree"


@pytest.mark.parametrize("bframes", [-1, 3])
def test_b_pictures_replayed_as_graphs(bframes):
    """hierarchical-B 8 and P + 3 B: with KS265_GRAPH=1, from the ninth picture on P and B pictures are replayed as captured graphs (one per rotation of the buffers involved);
    the stream equals the launch-by-launch one"""
    md5 = {}
    for tag, env in (("graph", {"KS265_GRAPH": "1"}), ("plain", {})):
        r = subprocess.run([sys.executable, "-c", _LANES_DRIVER, ROOT, "170", "64"], capture_output=True, text=True, timeout=120, env=dict(os.environ, KS_TEST_BFRAMES=str(bframes), **env))
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        md5[tag] = json.loads(r.stdout.strip().splitlines()[-1])["md5"]
    assert md5["graph"] == md5["plain"], md5


def test_graph_replay_at_2160p_beside_the_callers_uploads(tmp_path):
    """KS265_GRAPH=1 at the bench's size with the default GOP (two lanes, lookahead): pictures this large used to go up by a host-synchronous copy from the CALLING thread, which fails
    while a lane's thread has a capture open (end of round 6: 2 of 6 runs passed) - with graphs the input now takes the copying path; three runs, each == the launch-by-launch stream"""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    stream.build()
    W, H, n = 3840, 2160, 40
    make_clip(W, H, n, seed=7, abc=(67, 91, 33), pan=(8, 5)).tofile(tmp_path / "in.yuv")
    md5 = []
    for env in ({}, {"KS265_GRAPH": "1"}, {"KS265_GRAPH": "1"}, {"KS265_GRAPH": "1"}):
        r = subprocess.run([stream.CLI, "-i", str(tmp_path / "in.yuv"), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-rc", "0", "-preset", "slow", "-qp", "27", "-iper", "128", "-threads", "8",
                            "-psnr", "1", "-b", str(tmp_path / "o.265")], capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, (env, r.stdout[-500:] + r.stderr[-500:])
        md5.append(hashlib.md5(open(tmp_path / "o.265", "rb").read()).hexdigest())
    assert len(set(md5)) == 1, md5


@pytest.mark.parametrize("bframes,iper,n", [(-1, 64, 100), (-1, 20, 70), (3, 48, 110)])
def test_anchor_lane_writes_the_same_stream(bframes, iper, n):
    """round 5: a pyramid's anchor P pictures run on a stream, frame object and DPB slots of their own, beside the B pictures of the mini-GOP behind them; with the lane
    switched off (everything but key pictures on the main stream) the stream is the same - long intra period (key pictures on their stream) and short (on the main stream)"""
    md5 = {}
    for tag, env in (("lane", {"KS265_ANCHOR_LANE": "1"}), ("main", {})):
        r = subprocess.run([sys.executable, "-c", _LANES_DRIVER, ROOT, str(n), str(iper)], capture_output=True, text=True, timeout=120, env=dict(os.environ, KS_TEST_BFRAMES=str(bframes), **env))
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        md5[tag] = json.loads(r.stdout.strip().splitlines()[-1])["md5"]
    assert md5["lane"] == md5["main"], md5


@pytest.mark.parametrize("bframes,tag", [(-1, "hier8"), (3, "b3"), (0, "ippp_ref3")])
def test_api_call_sequence(bframes, tag):
    from ks265codec_amd import stream
    assert C.sizeof(YUV) == LAY["sizeof_yuv"] and C.sizeof(Picture) == LAY["sizeof_picture"] and C.sizeof(Nal) == LAY["sizeof_nal"]
    lib = C.CDLL(stream.build())
    lib.QY265EncoderOpen.restype = C.c_void_p
    W, H, N = 416, 240, 21
    clip = _clip("hierb4_416x240", N)
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
    for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 27), ("iper", 16), ("bframes", bframes), ("threads", 4), ("psnr", 1)):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
    if tag == "ippp_ref3":
        assert lib.QY265ConfigParse(cfg, b"ref", b"3") == 0
    err = C.c_int(0)
    h = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err)))
    assert h.value, hex(err.value & 0xFFFFFFFF)
    nal, nn = C.POINTER(Nal)(), C.c_int(0)
    pic, outp, yuv = Picture(), Picture(), YUV()
    yuv.iWidth, yuv.iHeight = W, H
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
    pic.yuv = C.pointer(yuv)
    bs, types, max_delay = bytearray(), [], 0
    for t in range(N):
        fr = clip[t].copy()
        base = fr.ctypes.data
        for k, off in enumerate((0, W * H, W * H * 5 // 4)):
            yuv.pData[k] = C.cast(base + off, C.POINTER(C.c_ubyte))
        pic.pts = t
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == 0
        fr[:] = 0                                           # the library copied the picture: the caller's buffer is free again
        for i in range(nn.value):
            bs += C.string_at(nal[i].pPayload, nal[i].iSize); types.append(nal[i].naltype)
        max_delay = max(max_delay, lib.QY265EncoderDelayedFrames(h))
    while lib.QY265EncoderDelayedFrames(h):
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
        for i in range(nn.value):
            bs += C.string_at(nal[i].pPayload, nal[i].iSize); types.append(nal[i].naltype)
    lib.QY265EncoderClose(h)
    vcl = [t for t in types if t < 32]
    assert len(vcl) == N, (len(vcl), types)
    assert types[:4] == [32, 33, 34, 19] and vcl.count(19) == 2          # key pictures at 0 and 16, parameter sets in front of each
    assert types.count(32) == 2 and types.count(33) == 2 and types.count(34) == 2
    if bframes != 0:
        assert vcl.count(0) > 0 and max_delay >= 2                        # non-reference B pictures exist, output lags input
    starts = [i for i in range(len(bs) - 4) if bs[i:i + 4] == b"\x00\x00\x00\x01"]
    assert len(starts) == len(types)
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, f"api_{tag}.265"), "wb").write(bs)
    clip.tofile(os.path.join(OUT, f"api_{tag}_src.yuv"))


REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")          # staged by __graft_entry__.build() in the builder container; travels with the snapshot


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="the reference's decoder was not staged (oracle/_ref/appdecoder)")
@pytest.mark.parametrize("W,H,n,opts", [
    (1280, 720, 25, ["-preset", "veryfast", "-qp", "32", "-iper", "16"]),                      # the SDK's default GOP: hierarchical B of 8, two closed GOPs
    (1920, 1080, 10, ["-preset", "slow", "-qp", "27", "-bframes", "0", "-iper", "128"]),       # config 2's tools: UMH, three list-0 pictures
    (1920, 1088, 9, ["-preset", "medium", "-qp", "30", "-bframes", "3", "-iper", "128"]),      # a pyramid of 4 (round 4, as in the reference): anchors, a reference B between them, non-reference B pictures; the flush ends on P + plain B
    (3840, 2160, 6, ["-preset", "slow", "-qp", "27", "-iper", "128"]),                         # the bench workload (config 3)
    (1920, 1080, 8, ["-preset", "veryslow", "-qp", "27", "-bframes", "0", "-ref", "1", "-iper", "128"]),   # config 5's tools on P pictures: -part 1 (two prediction units, four TUs), -subme 2 by Hadamard
    (3840, 2160, 4, ["-preset", "veryslow", "-qp", "27", "-bframes", "0", "-ref", "1", "-iper", "128"]),
])
def test_reference_decoder_reproduces_the_gpu_reconstruction(tmp_path, W, H, n, opts):
    """the conformance contract end to end ON THIS BOX: what the MI355X reconstructed (ks265enc -o) is byte for byte what the reference's
    own decoder makes of the stream the host wrote (ks265enc -b) - at the sizes the bench runs, not only at the fixture sizes"""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    stream.build()
    clip = make_clip(W, H, n, seed=W + n, abc=(37, 53, 19), pan=(5, 3))
    yuv, out, rec, dec = tmp_path / "in.yuv", tmp_path / "out.265", tmp_path / "rec.yuv", tmp_path / "dec.yuv"
    clip.tofile(yuv)
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-rc", "0", *opts, "-threads", "8", "-psnr", "1", "-b", str(out), "-o", str(rec)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    d = subprocess.run([REF_DEC, "-b", str(out), "-o", str(dec), "-threads", "4"], capture_output=True, text=True, cwd=tmp_path)
    assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
    a, b = np.fromfile(rec, np.uint8), np.fromfile(dec, np.uint8)
    assert a.size == b.size == n * W * H * 3 // 2, (a.size, b.size)
    fsz = W * H * 3 // 2
    bad = [t for t in range(n) if not (a[t * fsz:(t + 1) * fsz] == b[t * fsz:(t + 1) * fsz]).all()]
    assert not bad, f"pictures {bad} decode differently from the encoder's reconstruction"
    src = clip.reshape(n, -1)[:, :W * H].astype(np.int64)
    mse = float(((src - a.reshape(n, -1)[:, :W * H].astype(np.int64)) ** 2).mean())
    m = [ln for ln in r.stdout.splitlines() if ln.startswith("bitrate, psnr:")]
    assert m and abs(float(m[0].split()[3]) - 10 * np.log10(255.0 ** 2 / mse)) < 0.02, (m, mse)      # the PSNR the encoder prints is that of this reconstruction


def test_strong_scaling_job_is_rank_count_invariant(tmp_path):
    """bench.py --scaling strong: ONE fixed job split GOP by GOP over the ranks; the gathered stream of a 2-rank run (both ranks on this box's
    one GPU, host-side gloo collectives) is byte for byte the 1-rank stream"""
    import sys
    env = dict(os.environ, KS265_BENCH_BACKEND="gloo", KS265_BENCH_ONE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    common = ["--scaling", "strong", "--job-frames", "24", "--iper", "8", "--width", "640", "--height", "368", "--warmup", "2", "--host-threads", "4"]
    o1, o2 = tmp_path / "w1.265", tmp_path / "w2.265"
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *common, "--out", str(o1)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r1.returncode == 0, r1.stdout[-500:] + r1.stderr[-800:]
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29677",
                         os.path.join(ROOT, "bench.py"), "--gpus", "2", *common, "--out", str(o2)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r2.returncode == 0, r2.stdout[-500:] + r2.stderr[-800:]
    l1 = json.loads([ln for ln in r1.stdout.splitlines() if ln.startswith("{")][-1])
    l2 = json.loads([ln for ln in r2.stdout.splitlines() if ln.startswith("{")][-1])
    assert l1["scaling"] == l2["scaling"] == "strong" and l2["n_gpus"] == 2
    assert l1["config"]["job"]["frames"] == l2["config"]["job"]["frames"] == 24
    assert open(o1, "rb").read() == open(o2, "rb").read()
    if os.path.exists(REF_DEC):
        d = subprocess.run([REF_DEC, "-b", str(o2), "-o", str(tmp_path / "d.yuv"), "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
        assert "decoder passed" in d.stdout and os.path.getsize(tmp_path / "d.yuv") == 24 * 640 * 368 * 3 // 2


@pytest.mark.parametrize("W,H,n", [(3840, 2160, 3), (1920, 1080, 12)])
def test_encoder_reconstruction_equals_the_oracle_pipeline(tmp_path, W, H, n):
    """what the C host makes the MI355X reconstruct (ks265enc -o: its own tool dict, QP ladder and lambda tables) is picture for picture what the oracle pipeline
    computes with the same settings - at the bench size (3 pictures: the launch-by-launch path) and at 1080p over 12 pictures (from the ninth on P pictures are replayed
    as captured graphs).  VERDICT r2 2: the encoder itself against the oracle, not only against the decoder."""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip, lambda_q4
    from oracle_lib import OraclePipeline
    from test_gpu_configs import ENCODER_TOOLS
    from stream_cases import HOST_IPPP_CASCADE
    stream.build()
    clip = make_clip(W, H, n, seed=W + n, abc=(67, 91, 33) if W >= 3000 else (37, 53, 19), pan=(8, 5) if W >= 3000 else (5, 3))
    yuv, out, rec = tmp_path / "in.yuv", tmp_path / "out.265", tmp_path / "rec.yuv"
    clip.tofile(yuv)
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-rc", "0", "-preset", "slow", "-qp", "27", "-bframes", "0", "-ref", "1", "-iper", "128",
                        "-threads", "8", "-psnr", "1", "-b", str(out), "-o", str(rec)], capture_output=True, text=True)
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    a = np.fromfile(rec, np.uint8)
    fsz = W * H * 3 // 2
    assert a.size == n * fsz
    o = OraclePipeline(W, H, 27, lambda_q4(27), me_method=2, me_hex_thr=16, **ENCODER_TOOLS)     # -preset slow: UMH with the HEX shortcut below 16 SAD / sample
    ref = None
    for t in range(n):
        q = 27 if t == 0 else 28 + HOST_IPPP_CASCADE[t & 3]           # the host's ladder: I = Q, P = Q + 1 + the IPPP cascade
        o.set_qp(q, lambda_q4(q, inter=t > 0))
        ref = o.encode(clip[t], "I" if t == 0 else "P", ref, None)
        want = o.store(ref)
        assert (a[t * fsz:(t + 1) * fsz] == want).all(), f"picture {t}: the encoder's reconstruction differs from the oracle pipeline's"


def test_scene_cut_lookahead(tmp_path):
    """-lookahead N (the lookahead's frame-cost kernels composed in the host): two unrelated scenes of 12 pictures each - the first picture of the second
    scene becomes a key picture, nothing else does, and without the option the stream has its one key picture; the stream still decodes to the encoder's reconstruction"""
    import re
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    stream.build()
    W, H, n = 832, 480, 24
    clip = np.concatenate([make_clip(W, H, 12, seed=5, abc=(37, 53, 19), pan=(5, 3)), make_clip(W, H, 12, seed=99, abc=(11, 17, 7), pan=(2, 4))])
    yuv = tmp_path / "in.yuv"
    clip.tofile(yuv)
    kinds = {}
    for tag, extra in (("plain", []), ("la", ["-lookahead", "8"])):
        out, rec = tmp_path / f"{tag}.265", tmp_path / f"{tag}.yuv"
        r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-rc", "0", "-preset", "slow", "-qp", "30", "-bframes", "0", "-iper", "128",
                            "-threads", "8", "-psnr", "2", "-b", str(out), "-o", str(rec), *extra], capture_output=True, text=True)
        assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
        per = sorted((int(a), b, int(c)) for a, b, c in re.findall(r"^(\d+)\t([IPB])\t(\d+)\t", r.stdout, re.M))
        assert len(per) == n
        kinds[tag] = [k for _, k, _ in per]
        if tag == "la" and os.path.exists(REF_DEC):
            dec = tmp_path / "dec.yuv"
            d = subprocess.run([REF_DEC, "-b", str(out), "-o", str(dec), "-threads", "4"], capture_output=True, text=True, cwd=tmp_path)
            assert "decoder passed" in d.stdout, d.stdout[-400:]
            assert (np.fromfile(rec, np.uint8) == np.fromfile(dec, np.uint8)).all()
    assert kinds["plain"] == ["I"] + ["P"] * (n - 1)
    assert kinds["la"] == ["I"] + ["P"] * 11 + ["I"] + ["P"] * 11, kinds["la"]


def test_slice_type_decision_on_the_gpu(tmp_path):
    """-lookahead N with the default (hierarchical) GOP: every block of 8 pictures is coded as 8 or as 4 + 4 from the frame costs at both distances (the reference's adaptive
    BiPredFrames).  On the bench-style clip (squares in front of a pan of (8, 5): at 8 pictures' distance the edge of the search window) every block becomes 4 + 4, as in
    the reference's own stream of this clip; without the option the anchors stay 8 apart; both streams decode to the encoder's reconstruction (profiles/r03_minigop.txt is this run)"""
    import re
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    stream.build()
    W, H, n = 832, 480, 41
    yuv = tmp_path / "in.yuv"
    make_clip(W, H, n, seed=7, abc=(37, 53, 19), pan=(8, 5)).tofile(yuv)
    order = {}
    for tag, extra in (("plain", ["-lookahead", "0"]), ("la", ["-lookahead", "8"]), ("auto", [])):      # round 4: without the option the decision runs by itself (grid pictures only)
        out, rec = tmp_path / f"{tag}.265", tmp_path / f"{tag}.yuv"
        r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-rc", "0", "-preset", "slow", "-qp", "27", "-iper", "128",
                            "-threads", "8", "-psnr", "2", "-b", str(out), "-o", str(rec), *extra], capture_output=True, text=True)
        assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
        order[tag] = [(int(a), b) for a, b in re.findall(r"^(\d+)\t([IPB])\t\d+\t", r.stdout, re.M)]
        assert sorted(a for a, _ in order[tag]) == list(range(n))
        if tag != "plain":
            m = re.search(r"lookahead: (\d+) scene cuts, (\d+) blocks of 8 pictures coded as 4 \+ 4", r.stdout)
            assert m and int(m.group(1)) == 0 and int(m.group(2)) == 5, r.stdout[-600:]
        if os.path.exists(REF_DEC):
            dec = tmp_path / "dec.yuv"
            d = subprocess.run([REF_DEC, "-b", str(out), "-o", str(dec), "-threads", "4"], capture_output=True, text=True, cwd=tmp_path)
            assert "decoder passed" in d.stdout, d.stdout[-400:]
            assert (np.fromfile(rec, np.uint8) == np.fromfile(dec, np.uint8)).all()
    assert [a for a, k in order["plain"] if k == "P"] == [8, 16, 24, 32, 40]
    assert [a for a, k in order["la"] if k == "P"] == list(range(4, 41, 4)), order["la"][:20]
    assert order["auto"] == order["la"] and (tmp_path / "auto.265").read_bytes() == (tmp_path / "la.265").read_bytes()


def test_zero_copy_input_on_the_gpu():
    """ks265_enc_acquire_input: pictures produced straight into the encoder's pinned input buffers give the stream of the copying path, byte for byte"""
    from ks265codec_amd import stream
    lib = C.CDLL(stream.build())
    lib.QY265EncoderOpen.restype = C.c_void_p
    W, H, N = 416, 240, 14
    clip = _clip("hierb4_416x240", N)

    def encode(zero_copy):
        cfg = (C.c_uint8 * LAY["sizeof_config"])()
        assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
        for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 27), ("iper", 128), ("bframes", 0), ("threads", 4), ("psnr", 1)):
            assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
        err = C.c_int(0)
        h = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err)))
        assert h.value, hex(err.value & 0xFFFFFFFF)
        nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
        pic.yuv = C.pointer(yuv)
        bs, used = bytearray(), 0
        for t in range(N):
            if zero_copy and lib.ks265_enc_acquire_input(h, C.byref(yuv)) == 0:
                C.memmove(yuv.pData[0], clip[t].ctypes.data, W * H * 3 // 2); used += 1
            else:
                yuv.iWidth, yuv.iHeight = W, H
                yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
                for k, off in enumerate((0, W * H, W * H * 5 // 4)):
                    yuv.pData[k] = C.cast(clip[t].ctypes.data + off, C.POINTER(C.c_ubyte))
            pic.pts = t
            assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == 0
            for i in range(nn.value):
                bs += C.string_at(nal[i].pPayload, nal[i].iSize)
        while lib.QY265EncoderDelayedFrames(h):
            assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
            for i in range(nn.value):
                bs += C.string_at(nal[i].pPayload, nal[i].iSize)
        lib.QY265EncoderClose(h)
        return bytes(bs), used

    a, _ = encode(False)
    b, used = encode(True)
    assert used == N and a == b


@pytest.mark.parametrize("bframes", [0, -1])
def test_input_straight_from_the_callers_buffers_on_the_gpu(bframes):
    """round 6: pictures of 1 MB and more are uploaded by DMA from the CALLER's planes (pinned in place once, remembered by address) - no copy into the encoder's pinned memory first.
    The upload has finished when QY265EncoderEncodeFrame returns: a caller that refills ONE buffer for every picture (the SDK's own demo callers, encoderwrapper.c:367-379) and scribbles
    over it right after the call gets the stream of the copying path (KS265_INPUT_COPY=1), byte for byte; so do distinct buffers, and buffers the caller keeps (KS265_INPUT_HOLD=1)"""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    lib = C.CDLL(stream.build())
    lib.QY265EncoderOpen.restype = C.c_void_p
    W, H, N = 1920, 1080, 19
    clip = make_clip(W, H, N, seed=5, abc=(37, 53, 19), pan=(5, 3))

    def encode(one_buffer, **env):
        old = {k: os.environ.get(k) for k in ("KS265_INPUT_COPY", "KS265_INPUT_HOLD")}
        for k in old:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            cfg = (C.c_uint8 * LAY["sizeof_config"])()
            assert lib.QY265ConfigDefaultPreset(cfg, b"slow", None, b"default") == 0
            for k, v in (("wdt", W), ("hgt", H), ("fr", 50), ("rc", 0), ("qp", 30), ("iper", 128), ("bframes", bframes), ("threads", 8), ("psnr", 1)):
                assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0
            err = C.c_int(0)
            h = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err)))
            assert h.value, hex(err.value & 0xFFFFFFFF)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        nal, nn, pic, outp, yuv = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture(), YUV()
        pic.yuv = C.pointer(yuv)
        yuv.iWidth, yuv.iHeight = W, H
        yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = W, W // 2, W // 2
        one = np.zeros(W * H * 3 // 2, np.uint8)
        bs = bytearray()
        for t in range(N):
            src = clip[t]
            if one_buffer:
                one[:] = clip[t]; src = one
            for k, off in enumerate((0, W * H, W * H * 5 // 4)):
                yuv.pData[k] = C.cast(src.ctypes.data + off, C.POINTER(C.c_ubyte))
            pic.pts = t
            assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == 0
            if one_buffer:
                one[:] = 0x5A                                         # the buffer is the caller's again
            for i in range(nn.value):
                bs += C.string_at(nal[i].pPayload, nal[i].iSize)
        while lib.QY265EncoderDelayedFrames(h):
            assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
            for i in range(nn.value):
                bs += C.string_at(nal[i].pPayload, nal[i].iSize)
        lib.QY265EncoderClose(h)
        return bytes(bs)

    ref = encode(False, KS265_INPUT_COPY=1)
    assert len(ref) > 10000
    assert encode(True) == ref, "one refilled buffer"
    assert encode(False) == ref, "distinct buffers"
    assert encode(False, KS265_INPUT_HOLD=1) == ref, "buffers the caller keeps"
    assert encode(True, KS265_INPUT_COPY=1) == ref


def test_b_spread_runs_hip_code_on_one_device(tmp_path):
    """bench.py --b-spread - the one path with a collective (config 5: the anchor chain rotates over the ranks, every reconstructed anchor is broadcast, the B pictures are spread) -
    with two ranks on ONE MI355X (KS265_BENCH_ONE_DEVICE=1, host-side gloo broadcast): the sharding logic that the gloo CPU tests pin (tests/test_distributed_cpu.py) has run the HIP
    pixel path once, and rank 0 prints a well-formed line.  The 8-GPU RCCL run itself is the driver's."""
    port = 29600 + os.getpid() % 200
    env = dict(os.environ, KS265_BENCH_ONE_DEVICE="1", KS265_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "bench.py"), "--gpus", "2", "--b-spread", "--bframes", "3", "--width", "1280", "--height", "720", "--steps", "16", "--warmup", "4", "--no-cpu-baseline", "--clip-frames", "9"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-1500:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and "anchor chain rotating" in line["config"]["sharding"], line["config"]
