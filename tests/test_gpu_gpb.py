"""GPU: generalised-B anchors (`gpb`, include/ks265_enc.h) on the device - B pictures whose two lists hold PAST pictures, coded without the skip pass through the per-picture
setter ks265_frame_set_picture_skip, equal the oracle pipeline; the setter's contract; and a whole `ks265enc -gpb 1` stream equals the CPU mirror's byte for byte."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first)
torch.cuda.is_available()
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


def _same_records(ks, f, o, W, H, got_pic, exp_pic, what):
    from ks265codec_amd.lib import CU8
    cu = f.ws_read("cu8", f.geom.bytes_cu8).view(CU8)
    assert (cu["inter_dir"] == o.cu8["inter_dir"]).all(), f"{what}: {int((cu['inter_dir'] != o.cu8['inter_dir']).sum())} inter_dir (direction | list indices) differ"
    assert (cu.view(np.uint8) == o.cu8.view(np.uint8)).all(), f"{what}: {int((cu.view(np.uint8) != o.cu8.view(np.uint8)).sum())} CU record bytes differ"
    for comp, n in ((0, W * H), (1, W * H // 4), (2, W * H // 4)):
        lv = f.ws_read("levels", n * 2, comp).view(np.int16)
        assert (lv == o.lvl[comp]).all(), f"{what}: {int((lv != o.lvl[comp]).sum())} levels of component {comp} differ"
    sao = f.ws_read("sao", f.geom.bytes_sao)
    assert (sao == np.ascontiguousarray(o.sao).view(np.uint8).ravel()).all(), f"{what}: SAO records differ"
    got, exp = ks.host(f.store_i420(got_pic), np.uint8), o.store(exp_pic)
    assert (got == exp).all(), f"{what}: {int((got != exp).sum())} samples differ"
    return cu


@pytest.mark.parametrize("W,H,abc,pan,seed", [(200, 136, (17, 23, 9), (2, 1), 6), (416, 240, (17, 23, 9), (3, 2), 5)])
def test_anchors_over_past_pictures_equal_the_oracle(ks, W, H, abc, pan, seed):
    """ONE frame object created for the skip pass on B pictures (skip_rd 1), the tool set of -preset slow: key picture, a P anchor, an anchor with [a1] / [a2], an anchor with
    [a1, a3] / [a2] - both with the setter at 0 - then, the setter back at -1, a real B picture between two of them; every picture == OraclePipeline with its skip_rd attribute set
    the same way: CU records (inter_dir carries the list indices), levels, SAO records, samples.  The anchors use both lists, and the second one both pictures of list 0"""
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
    from oracle_lib import OraclePipeline
    assert ENCODER_TOOLS["skip_rd"] == 1
    clip = make_clip(W, H, 13, seed=seed, abc=abc, pan=pan)
    o = OraclePipeline(W, H, 27, lambda_q4(27), **ENCODER_TOOLS)
    with KsFrame(ks, W, H, 27, lambda_q4(27), bframes=3, refs=3, **ENCODER_TOOLS) as f:
        src, dg, do = f.new_pic(), {}, {}
        #        picture, list 0, list 1, QP offset, skip setter
        order = [(0, [], [], 0, -1), (4, [0], [], 1, -1), (8, [4], [0], 1, 0), (12, [8, 0], [4], 1, 0), (10, [8], [12], 2, -1)]
        for d, l0, l1, dq, skip in order:
            q = 27 + dq
            lam = lambda_q4(q, inter=bool(l0))
            o.set_qp(q, lam); f.set_qp(q, lam)
            f.set_picture_skip(skip); o.skip_rd = 1 if skip < 0 else skip
            f.load_i420(ks.dev(clip[d]), src)
            out = f.new_pic()
            if not l0:
                eo = o.encode(clip[d], "I"); f.encode_picture(src, out, True, out)
            elif not l1:
                eo = o.encode(clip[d], "P", do[l0[0]]); f.encode_picture(src, dg[l0[0]], False, out)
            else:
                eo = o.encode_b_mref(clip[d], [do[r] for r in l0], [do[r] for r in l1]); f.encode_picture_b_mref(src, [dg[r] for r in l0], [dg[r] for r in l1], out)
            cu = _same_records(ks, f, o, W, H, out, eo, f"picture {d} on {l0} / {l1}, skip setter {skip}")
            if l1:
                inter = cu["pred_mode"] == 0
                dirs = set((cu["inter_dir"][inter] & 3).tolist())
                assert {1, 2, 3} <= dirs or d == 10, (d, dirs)                               # list 0 alone, list 1 alone and both are all chosen somewhere
                if len(l0) > 1:
                    assert ((cu["inter_dir"][inter] >> 4) & 3).max() == 1, "no block predicts from the second picture of list 0"
            dg[d], do[d] = out, eo


def test_skip_setter_contract(ks):
    """-1 / 0 / the created value are taken, a value above the created one is KS265_NOTSUPPORTED; on a P picture of a frame object created with skip_rd 2, 0 gives the records of a
    frame object created without the pass - and they differ from those with it"""
    from ks265codec_amd.lib import CU8, KsFrame, Ks265Error
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
    W, H = 200, 136
    clip = make_clip(W, H, 2, seed=6, abc=(17, 23, 9), pan=(2, 1))
    with KsFrame(ks, W, H, 27, lambda_q4(27), bframes=3, **ENCODER_TOOLS) as f:                  # created with 1
        for v in (-1, 0, 1, -1):
            f.set_picture_skip(v)
        with pytest.raises(Ks265Error, match="rc=-?\\d+"):
            f.set_picture_skip(2)
    recs = {}
    for created, setter in ((2, None), (2, 0), (0, None), (0, -1)):
        with KsFrame(ks, W, H, 27, lambda_q4(27), bframes=3, **dict(ENCODER_TOOLS, skip_rd=created)) as f:
            if created == 0:
                with pytest.raises(Ks265Error):
                    f.set_picture_skip(1)
            src, key, out = f.new_pic(), f.new_pic(), f.new_pic()
            f.load_i420(ks.dev(clip[0]), src); f.encode_picture(src, key, True, key)
            if setter is not None:
                f.set_picture_skip(setter)
            f.set_qp(28, lambda_q4(28, inter=True))
            f.load_i420(ks.dev(clip[1]), src); f.encode_picture(src, key, False, out)
            cu = f.ws_read("cu8", f.geom.bytes_cu8)
            lv = [f.ws_read("levels", n * 2, c) for c, n in ((0, W * H), (1, W * H // 4), (2, W * H // 4))]
            recs[(created, setter)] = (cu, lv, ks.host(f.store_i420(out), np.uint8))
    for other in ((0, None), (0, -1)):
        a, b = recs[(2, 0)], recs[other]
        assert (a[0] == b[0]).all() and all((x == y).all() for x, y in zip(a[1], b[1])) and (a[2] == b[2]).all(), other
    assert not (recs[(2, None)][0] == recs[(2, 0)][0]).all(), "the pass changed no CU record of the P picture: the case shows nothing"


def test_whole_stream_is_the_mirrors(tmp_path, monkeypatch):
    """`ks265enc -gpb 1 -bframes 3 -ref0 3 -qp 30 -o rec.yuv`, 17 pictures of 416x240: the stream == tools/rd_eval.py --host with KS265_GPB=1 (oracle pipeline + this writer: the
    rule's lists, list_mod, no skip pass on anchors, the anchors' QP and lambda) byte for byte; where the reference's decoder is staged, it decodes to rec.yuv exactly"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rd_eval as R
    from ks265codec_amd import stream
    from ks265codec_amd.synth import ENCODER_TOOLS, make_clip
    from slice_headers import pictures
    stream.build()
    W, H, N = 416, 240, 17
    fsz = W * H * 3 // 2
    clip = make_clip(W, H, N, seed=W + N, abc=(17, 23, 9), pan=(5, 3))
    clip.tofile(tmp_path / "in.yuv")
    env = {k: v for k, v in os.environ.items() if k != "KS265_GPB"}
    r = subprocess.run([stream.CLI, "-i", str(tmp_path / "in.yuv"), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-preset", "slow", "-rc", "0", "-iper", "128", "-threads", "8",
                        "-gpb", "1", "-bframes", "3", "-ref0", "3", "-qp", "30", "-b", str(tmp_path / "o.265"), "-o", str(tmp_path / "rec.yuv")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-600:] + r.stderr[-600:]
    got = open(tmp_path / "o.265", "rb").read()
    assert [(p["slice_type"], p["l0"], p["l1"]) for p in pictures(got) if p["poc"] in (4, 8, 12, 16)] == [("P", [0], []), ("B", [4], [0]), ("B", [8, 0], [4]), ("B", [12, 4], [8])]
    monkeypatch.setenv("RD_G", "4"); monkeypatch.setenv("KS265_GPB", "1")
    seq, _ = R.adaptive_seq(clip, W, H, 30, decide=False)
    want, _, _ = R.encode_ours(clip, W, H, 30, "hier", dict(ENCODER_TOOLS), layer_qp=[0, 1, 2], lam_scale=-1.0, seq=seq)
    if got != want:
        a, b = pictures(got), pictures(want)
        assert [(p["poc"], p["slice_type"], p["l0"], p["l1"], p["rps"], p["qp"]) for p in a] == [(p["poc"], p["slice_type"], p["l0"], p["l1"], p["rps"], p["qp"]) for p in b]
    assert len(got) == len(want) and got == want, f"{len(got)} bytes, the mirror's {len(want)}"
    if os.path.exists(REF_DEC):
        d = subprocess.run([REF_DEC, "-b", str(tmp_path / "o.265"), "-o", str(tmp_path / "dec.yuv"), "-threads", "4"], capture_output=True, text=True, cwd=tmp_path)
        assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
        rec, dec = np.fromfile(tmp_path / "rec.yuv", np.uint8), np.fromfile(tmp_path / "dec.yuv", np.uint8)
        assert rec.size == dec.size == N * fsz
        bad = [t for t in range(N) if not (rec[t * fsz:(t + 1) * fsz] == dec[t * fsz:(t + 1) * fsz]).all()]
        assert not bad, f"pictures {bad} decode differently from the encoder's reconstruction"
