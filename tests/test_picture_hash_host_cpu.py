"""CPU: the `hash` switch of the encoder host (decoded picture hash SEI messages) on the host linked against the device library's CPU stand-in with the two hash
entries (tests/hip_stub_hash.c), 128x72.
  * every picture of every kind of GOP is followed, directly, by exactly one suffix SEI NAL unit whose values are tests/picture_hash_ref.py's on the picture's reconstruction
    (the -o dump, matched by display index); where oracle/_ref/appdecoder is staged it decodes the stream with the messages to the pictures of the stream without them
    (the stand-in does not encode, so the decoder's pictures are not its reconstruction: the values against the decoder's output are checked on the GPU);
  * the stream minus its type-40 NAL units is the stream without the switch, for -rc 0 and for -rc 2 (no controller counts the messages);
  * GOP lanes leave the bytes as they are; the switch's values and where it comes from (ks265_enc_set_default, KS265_HASH, -hash); the API's extra QY265Nal;
  * against the stand-in WITHOUT the entries (tests/hip_stub.c) the host library still loads, says once that the picture hash is unavailable and writes the plain stream."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import picture_hash_ref as ph
from host_harness import ROOT, Nal, Picture, build_host_cli, build_host_lib, load_host_lib, open_handle, packed_yuv

REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")
W, H, N = 128, 72, 17
FSZ = W * H * 3 // 2
GOPS = {"ippp": ("-bframes", "0"), "pyramid": (), "gpb": ("-gpb", "1"), "zerolatency": ("-latency", "zerolatency")}


def _cli(d, stub):
    """a directory with the command line on the stand-in (as ks265enc) and a clip"""
    os.symlink(build_host_cli(stub), d / "ks265enc")
    np.random.default_rng(11).integers(0, 256, (64, FSZ), dtype=np.uint8).tofile(str(d / "in.yuv"))
    return d


@pytest.fixture(scope="module")
def stub_cli(tmp_path_factory):
    return _cli(tmp_path_factory.mktemp("stubhash"), "hip_stub_hash.c")


@pytest.fixture(scope="module")
def plain_cli(tmp_path_factory):
    return _cli(tmp_path_factory.mktemp("stubnohash"), "hip_stub.c")


_runs = {}


def _run(d, *opts, n=N, dump=False, env=None, ok=True):
    """(stdout, stream, reconstruction or None) of one CLI run; equal runs are made once"""
    key = (str(d), opts, n, dump, tuple(sorted((env or {}).items())))
    if key not in _runs:
        tag = f"r{len(_runs)}"
        out, rec = d / f"{tag}.265", d / f"{tag}.yuv"
        r = subprocess.run([str(d / "ks265enc"), "-i", str(d / "in.yuv"), "-wdt", str(W), "-hgt", str(H), "-fr", "25", "-frms", str(n), "-preset", "medium", "-qp", "34",
                            "-threads", "3", "-psnr", "1", "-b", str(out), *(("-o", str(rec)) if dump else ()), *opts],
                           capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
        if ok:
            assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-800:] + r.stderr[-800:]
        _runs[key] = (r.stdout + r.stderr, out.read_bytes() if out.exists() else b"", np.fromfile(str(rec), np.uint8).reshape(-1, FSZ) if dump and rec.exists() else None, r.returncode)
    return _runs[key]


def _check_messages(stream, hash_switch, pictures_of, n=N):
    """one message per picture, directly behind it (sei_hashes refuses any other place), of the switch's type, with the specification's values on pictures_of[display index]"""
    pics, stripped = ph.sei_hashes(stream)
    assert len(pics) == n and sorted(p["disp"] for p in pics) == list(range(n))
    for p in pics:
        assert len(p["hashes"]) == 1, p
        t, vals = p["hashes"][0]
        assert t == hash_switch - 1
        assert vals == ph.expected(pictures_of[p["disp"]], W, H, t), (p["disp"], p["slice_type"])
    return pics, stripped


@pytest.mark.parametrize("hash_switch", [2, 3], ids=["crc", "checksum"])
@pytest.mark.parametrize("gop", list(GOPS))
def test_messages_against_the_specification(stub_cli, gop, hash_switch):
    _, plain, rec0, _ = _run(stub_cli, "-rc", "0", *GOPS[gop], "-hash", "0", dump=True)
    _, bs, rec, _ = _run(stub_cli, "-rc", "0", *GOPS[gop], "-hash", str(hash_switch), dump=True)
    assert (rec == rec0).all() and len(rec) == N
    pics, stripped = _check_messages(bs, hash_switch, rec)
    assert stripped == plain and len(bs) == len(plain) + N * (16 if hash_switch == 2 else 22)        # (these pictures' values need no emulation prevention ... or the run says so)
    assert {p["slice_type"] for p in pics} == ({"I", "P"} if gop in ("ippp", "zerolatency") else {"I", "P", "B"})
    if os.path.exists(REF_DEC):
        # The stand-in does not encode: its records are made up and its "reconstruction" is the source with a stamp, so the reference's decoder turns the stream into OTHER
        # pictures than the -o dump (measured: every value differs) and the messages cannot be held to its output here - that check needs the real pixel path and is in
        # tests/test_gpu_picture_hash.py.  What holds on this host: the decoder takes the stream with the messages and decodes exactly the pictures of the stream without them.
        dec = {}
        for tag, data in (("with", bs), ("without", plain)):
            (stub_cli / "d.265").write_bytes(data)
            d = subprocess.run([REF_DEC, "-b", "d.265", "-o", "d.yuv", "-threads", "2"], capture_output=True, text=True, cwd=stub_cli, timeout=120)
            assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
            dec[tag] = np.fromfile(str(stub_cli / "d.yuv"), np.uint8)
        assert len(dec["with"]) == N * FSZ and (dec["with"] == dec["without"]).all()


@pytest.mark.parametrize("hash_switch", [2, 3], ids=["crc", "checksum"])
@pytest.mark.parametrize("gop", list(GOPS))
@pytest.mark.parametrize("rc", ["0", "2"])
def test_stream_minus_the_messages_is_the_plain_stream(stub_cli, gop, hash_switch, rc):
    """no -o here: the key pictures' and the anchors' streams and the split pipeline, which a run with the reconstruction dump does not use"""
    opts = ("-rc", rc, "-br", "300", *GOPS[gop])
    out0, plain, _, _ = _run(stub_cli, *opts, "-hash", "0")
    out1, bs, _, _ = _run(stub_cli, *opts, "-hash", str(hash_switch))
    pics, stripped = ph.sei_hashes(bs)
    assert stripped == plain and [len(p["hashes"]) for p in pics] == [1] * N and not any(p["hashes"] for p in ph.sei_hashes(plain)[0])
    # the bitrate line counts the messages: bytes x 8 x 25 / N / 1000
    kbps = lambda o: float([ln for ln in o.splitlines() if ln.startswith("bitrate, psnr:")][0].split()[2])
    assert abs(kbps(out1) - len(bs) * 8 * 25 / N / 1000) < 1e-3 and abs(kbps(out0) - len(plain) * 8 * 25 / N / 1000) < 1e-3


@pytest.mark.parametrize("hash_switch", [2, 3], ids=["crc", "checksum"])
def test_gop_lanes_give_the_same_bytes(stub_cli, hash_switch):
    outs = {lanes: _run(stub_cli, "-rc", "0", "-iper", "32", "-bframes", "0", "-hash", str(hash_switch), n=64, env={"KS265_GOP_LANES": str(lanes)}) for lanes in (1, 2)}
    assert "GOP lanes" in outs[2][0] and "GOP lanes" not in outs[1][0], "the switch does not force one lane"
    assert outs[1][1] == outs[2][1]
    pics, stripped = ph.sei_hashes(outs[2][1])
    assert [len(p["hashes"]) for p in pics] == [1] * 64 and sorted(p["disp"] for p in pics) == list(range(64))
    assert stripped == _run(stub_cli, "-rc", "0", "-iper", "32", "-bframes", "0", "-hash", "0", n=64, env={"KS265_GOP_LANES": "2"})[1]
    assert len({tuple(p["hashes"][0][1]) for p in pics}) == 64, "64 different pictures: every message travelled with its own"


def test_graph_path(stub_cli):
    """KS265_GRAPH=1: the hash pass is part of the captured picture, the copy home is behind its launch"""
    env = {"KS265_GRAPH": "1", "KS265_GOP_LANES": "1"}
    _, plain, _, _ = _run(stub_cli, "-rc", "0", "-bframes", "0", "-hash", "0", n=40, env=env)
    _, bs, _, _ = _run(stub_cli, "-rc", "0", "-bframes", "0", "-hash", "3", n=40, env=env)
    _, nograph, _, _ = _run(stub_cli, "-rc", "0", "-bframes", "0", "-hash", "3", n=40, env={"KS265_GOP_LANES": "1"})
    assert ph.sei_hashes(bs)[1] == plain and bs == nograph


@pytest.mark.parametrize("value", ["1", "4", "-1"])
def test_other_values_are_rejected(stub_cli, value):
    out, bs, _, rc = _run(stub_cli, "-rc", "0", "-hash", value, ok=False)
    assert rc == 2 and "bad value for -hash" in out and bs == b""


def test_set_default_values():
    lib = load_host_lib(build_host_lib("hip_stub_hash.c"), mode=os.RTLD_NOW)
    assert hasattr(lib, "ks265_picture_hash") and hasattr(lib, "ks265_write_picture_hash_sei")
    for v, rc in ((0, 0), (2, 0), (3, 0), (1, -2), (4, -2), (-1, -2), (0, 0)):                       # QY265_PARAM_BAD_VALUE = -2; MD5 (1) stays with -md5
        assert lib.ks265_enc_set_default(b"hash", C.c_int(v)) == rc, v


def test_environment_overrides_the_default(stub_cli):
    base = ("-rc", "0", "-bframes", "0")
    by_flag = _run(stub_cli, *base, "-hash", "2")[1]
    assert _run(stub_cli, *base, env={"KS265_HASH": "2"})[1] == by_flag
    assert _run(stub_cli, *base, "-hash", "3", env={"KS265_HASH": "2"})[1] == by_flag
    assert _run(stub_cli, *base, "-hash", "3", env={"KS265_HASH": "0"})[1] == _run(stub_cli, *base, "-hash", "0")[1]


def test_device_library_without_the_entry(plain_cli):
    lib = load_host_lib(build_host_lib("hip_stub.c"), mode=os.RTLD_NOW)
    assert hasattr(lib, "ks265_enc_set_default") and not hasattr(lib, "ks265_picture_hash")
    for gop in ((), ("-bframes", "0")):                                  # (the default GOP runs two lanes: one line per handle all the same)
        out0, plain, _, _ = _run(plain_cli, "-rc", "0", *gop, "-hash", "0", n=64, env={"KS265_GOP_LANES": "2"} if not gop else None)
        out1, bs, _, _ = _run(plain_cli, "-rc", "0", *gop, "-hash", "2", n=64, env={"KS265_GOP_LANES": "2"} if not gop else None)
        assert len(plain) > 100 and bs == plain
        assert out1.count("ks265enc: picture hash is unavailable: ") == 1 and "picture hash is unavailable" not in out0


# ---------------------------------------------------------------- the API: one more QY265Nal per picture
class _Stats(C.Structure):
    _fields_ = [("frames", C.c_long), ("bytes", C.c_longlong), ("rest", C.c_uint8 * 1024)]


def test_api_hands_the_message_out_as_a_nal_of_its_own(stub_cli):
    lib = load_host_lib(build_host_lib("hip_stub_hash.c"))
    clip = np.fromfile(str(stub_cli / "in.yuv"), np.uint8).reshape(-1, FSZ)[:N].copy()
    h = open_handle(lib, W, H, params=(("threads", 3), ("log", 3)), defaults={"hash": 2})
    nal, nn, pic, outp = C.POINTER(Nal)(), C.c_int(0), Picture(), Picture()
    got = []                                                             # (naltype, pts, bytes) in output order

    def take():
        got.extend((nal[i].naltype, nal[i].pts, C.string_at(nal[i].pPayload, nal[i].iSize)) for i in range(nn.value) if nal[i].iSize > 0)

    for t in range(N):
        yuv = packed_yuv(clip[t], W, H)
        pic.yuv, pic.pts = C.pointer(yuv), 1000 + t
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0) == 0
        take()
    while lib.QY265EncoderDelayedFrames(h) > 0:
        assert lib.QY265EncoderEncodeFrame(h, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == 0
        take()
    st = _Stats()
    assert lib.ks265_enc_get_stats(h, C.byref(st)) == 0
    lib.QY265EncoderClose(h)
    slices = [i for i, g in enumerate(got) if g[0] < 32]
    assert len(slices) == N and sorted(got[i][1] for i in slices) == [1000 + t for t in range(N)]
    for i in slices:                                                     # behind every picture its message: an entry of its own, type 40, the picture's pts
        assert got[i + 1][0] == 40 and got[i + 1][1] == got[i][1] and got[i + 1][2][:6] == bytes.fromhex("000000015001")
    assert [g[0] for g in got].count(40) == N
    bs = b"".join(g[2] for g in got)
    assert st.frames == N and st.bytes == len(bs), "the bytes statistic counts the messages"
    pics, _ = ph.sei_hashes(bs)
    assert [len(p["hashes"]) for p in pics] == [1] * N and all(p["hashes"][0][0] == 1 for p in pics)
