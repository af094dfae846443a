"""CPU: generalised-B anchors (`gpb`, include/ks265_enc.h) in the encoder host, linked against the stand-in of the device library (tests/hip_stub.c).  With the switch on, an
anchor that searches two or more past anchors goes out as a B slice whose two lists hold past anchors - list 0 = [a1, a3(, a4)], list 1 = [a2]; everything else about the stream
stays.  The lists are read back from the slice headers of the stream (tests/slice_headers.py: what a decoder constructs, ref_pic_lists_modification() included).  Off, the
streams are the parent behaviour's, pinned in tests/golden/gpb_off_stream_md5.json (written by tests/golden/gen_gpb_off_golden.py before the switch existed)."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from host_harness import HERE, ROOT, build_host_cli, build_host_lib
from host_harness import cli_encode as encode

REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")
GOLD = os.path.join(HERE, "golden", "gpb_off_stream_md5.json")
W, H = 200, 136                                             # no multiple of the CTU in either direction, more than one CTU row and column


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """the CLI and the library of the host, both on the stand-in, and a clip"""
    d = tmp_path_factory.mktemp("stubgpb")
    np.random.default_rng(5).integers(0, 256, 70 * W * H * 3 // 2, dtype=np.uint8).tofile(d / "in.yuv")
    return {"exe": build_host_cli(), "so": build_host_lib("hip_stub.c"), "yuv": str(d / "in.yuv")}


def decodes(tmp_path, name, n, size=(W, H)):
    if not os.path.exists(REF_DEC):
        return
    d = subprocess.run([REF_DEC, "-b", str(tmp_path / name), "-o", str(tmp_path / "d.yuv"), "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
    assert d.returncode == 0 and "decoder passed" in d.stdout and os.path.getsize(tmp_path / "d.yuv") == n * size[0] * size[1] * 3 // 2, d.stdout[-300:] + d.stderr[-300:]


def test_the_switch_is_a_process_default_of_its_own(stub):
    """ks265_enc_set_default("gpb", 0 | 1); other values are QY265_PARAM_BAD_VALUE (-2) and leave the default alone"""
    code = ("import ctypes as C, sys; l = C.CDLL(sys.argv[1]); print([l.ks265_enc_set_default(b'gpb', v) for v in (1, 0, 2, -1)], l.ks265_enc_set_default(b'gpbx', 1))")
    r = subprocess.run([sys.executable, "-c", code, stub["so"]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "[0, 0, -2, -2] -1", r.stdout + r.stderr


@pytest.mark.parametrize("opts,n,span", [(["-bframes", "3"], 17, 4), (["-lookahead", "0"], 25, 8)])
def test_anchors_with_two_or_more_past_anchors_are_b_slices_over_them(stub, tmp_path, opts, n, span):
    """-ref0 3, one GOP: the first anchor stays a P slice on [key]; the second is B with [a1] / [a2]; from the third on B with [a1, a3] / [a2].  Inner B pictures, reference
    picture sets, NAL types, QPs and the coding order are those of the stream without the switch; the reference's decoder takes the stream"""
    from slice_headers import pictures
    common = ["-ref0", "3", "-iper", "128", "-frms", str(n), *opts]
    on = pictures(encode(stub, tmp_path / "on.265", common + ["-gpb", "1"]))
    off = pictures(encode(stub, tmp_path / "off.265", common + ["-gpb", "0"]))
    assert len(on) == len(off) == n and all(p["list_mod"] == 1 for p in on) and all(p["list_mod"] == 0 for p in off)
    by = {p["poc"]: p for p in on}
    a = list(range(0, n, span))                                                # the anchors; a[0] is the key picture
    assert (by[a[1]]["slice_type"], by[a[1]]["l0"], by[a[1]]["l1"]) == ("P", [a[0]], [])
    assert (by[a[2]]["slice_type"], by[a[2]]["l0"], by[a[2]]["l1"]) == ("B", [a[1]], [a[0]])
    for k in range(3, len(a)):
        assert (by[a[k]]["slice_type"], by[a[k]]["l0"], by[a[k]]["l1"]) == ("B", [a[k - 1], a[k - 3]], [a[k - 2]]), (a[k], by[a[k]])
    if span == 4:
        assert [(by[t]["slice_type"], by[t]["l0"], by[t]["l1"]) for t in (4, 8, 12, 16)] == [("P", [0], []), ("B", [4], [0]), ("B", [8, 0], [4]), ("B", [12, 4], [8])]
    for p, q in zip(on, off):                                                  # coding order: everything but the anchors' slice type and lists
        assert (p["poc"], p["nal_type"], p["rps"], p["qp"]) == (q["poc"], q["nal_type"], q["rps"], q["qp"]), (p, q)
        if p["poc"] % span:
            assert p == dict(q, list_mod=1), (p, q)
        else:
            assert sorted(p["l0"] + p["l1"]) == sorted(q["l0"]) and q["slice_type"] in "IP" and q["l1"] == [], (p, q)
    decodes(tmp_path, "on.265", n)


def test_off_and_where_no_anchor_sees_two_anchors_nothing_moves(stub, tmp_path):
    """`gpb` 0, no `gpb` at all and KS265_GPB=0 over `-gpb 1` write the pinned streams of the behaviour before the switch (a pyramid and IPPP); with -bframes 0 and at zero
    latency `gpb` 1 is accepted and writes the stream of `gpb` 0"""
    gold = json.load(open(GOLD))["cases"]
    for name, case in sorted(gold.items()):
        for tag, extra, env in (("unset", [], None), ("zero", ["-gpb", "0"], None), ("env0", ["-gpb", "1"], {"KS265_GPB": 0}), ("envunset0", [], {"KS265_GPB": 0})):
            bs = encode(stub, tmp_path / f"{name}_{tag}.265", case["opts"] + extra, env)
            assert len(bs) == case["bytes"] and hashlib.md5(bs).hexdigest() == case["md5"], (name, tag, len(bs), case["bytes"])
    ippp = gold["ippp"]
    for tag, extra, env in (("cli", ["-gpb", "1"], None), ("env", [], {"KS265_GPB": 1})):
        assert hashlib.md5(encode(stub, tmp_path / f"i_{tag}.265", ippp["opts"] + extra, env)).hexdigest() == ippp["md5"], tag
    zl = ["-latency", "zerolatency", "-iper", "128", "-frms", "12"]
    assert encode(stub, tmp_path / "z1.265", zl + ["-gpb", "1"]) == encode(stub, tmp_path / "z0.265", zl + ["-gpb", "0"])
    # ... and the switch bites where it is in force: the pyramid's stream with it is another one
    assert hashlib.md5(encode(stub, tmp_path / "p1.265", gold["pyramid4"]["opts"] + ["-gpb", "1"])).hexdigest() != gold["pyramid4"]["md5"]


def test_two_gop_lanes_write_the_one_lane_stream(stub, tmp_path):
    """closed GOPs on two lanes: every lane opens with the switch; the stream is the one-lane stream byte for byte"""
    opts = ["-bframes", "3", "-ref0", "3", "-iper", "32", "-frms", "70", "-gpb", "1"]
    one = encode(stub, tmp_path / "l1.265", opts, {"KS265_GOP_LANES": 1, "KS265_STUB_ENCODE_US": 1000}, size=(128, 72))
    two = encode(stub, tmp_path / "l2.265", opts, {"KS265_GOP_LANES": 2, "KS265_STUB_ENCODE_US": 1000}, size=(128, 72))
    assert one == two
    from slice_headers import pictures
    # B slices over past pictures only: anchors 8, 12 .. 28 and 31 (the shortened mini-GOP in front of the key picture) of the two whole GOPs, picture 5 of the last (6 pictures)
    assert sum(p["slice_type"] == "B" and max(p["l0"] + p["l1"]) < p["poc"] for p in pictures(two)) == 2 * 7 + 1
    decodes(tmp_path, "l2.265", 70, size=(128, 72))


def test_cutree_does_not_see_the_switch(stub, tmp_path):
    """-rc 3 with the cuTree pass: the lookahead takes its slice types and distances from the GOP layout, in which such a picture is the anchor it replaces - the QP of every CTU
    of every picture is the same with and without the switch"""
    from cutree_mirror import read_qpmap_dump
    from ks265codec_amd.synth import make_clip
    w, h, n = 192, 128, 26
    make_clip(w, h, n, seed=11, abc=(17, 23, 9), pan=(3, 2)).tofile(tmp_path / "in.yuv")
    maps = {}
    for g in (0, 1):
        dump = tmp_path / f"maps{g}.bin"
        e = {k: v for k, v in os.environ.items() if k != "KS265_GPB"}
        r = subprocess.run([stub["exe"], "-i", str(tmp_path / "in.yuv"), "-wdt", str(w), "-hgt", str(h), "-fr", "50", "-preset", "slow", "-rc", "3", "-crf", "26", "-iper", "64", "-psnr", "2",
                            "-threads", "3", "-bframes", "3", "-gpb", str(g), "-b", str(tmp_path / f"c{g}.265")], capture_output=True, text=True, timeout=300, env=dict(e, KS265_DUMP_QPMAP=str(dump)))
        assert r.returncode == 0 and "cuTree over a lookahead" in r.stdout + r.stderr, r.stdout[-800:] + r.stderr[-800:]
        maps[g] = read_qpmap_dump(dump)
    assert sorted(maps[0]) == sorted(maps[1]) == list(range(n))
    spread = 0
    for d in range(n):
        (k0, q0, m0), (k1, q1, m1) = maps[0][d], maps[1][d]
        assert (k0, q0) == (k1, q1) and (m0 == m1).all(), f"picture {d}: {k0} qp {q0} / {k1} qp {q1}"
        spread = max(spread, int(m0.max()) - int(m0.min()))
    assert spread >= 2, "the maps are not flat"
    from slice_headers import pictures
    on = pictures(open(tmp_path / "c1.265", "rb").read())
    assert [p["slice_type"] for p in on if p["poc"] in (8, 12)] == ["B", "B"]                      # (the switch was in force)
