"""GPU: ks265_frame_cfg.sao = 3 - the reference's SAO decision with its left / up merge candidates (three launches: statistics + own decision per CTU, the merge chain along the
anti-diagonals in one work-group, the apply per CTU) against tests/sao_merge_ref.py, which drives the pinned ks265o_sao_mode_decision CTU by CTU in coding order."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


def _synthetic(W, H, seed):
    """a source and a 'deblocked' picture = the source plus a small smooth error: no encode needed"""
    rng = np.random.default_rng(seed)
    planes = []
    for w, h in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
        ys, xs = np.mgrid[0:h, 0:w]
        base = 118 + 10 * np.sin(xs / 151.0 + rng.random() * 6) * np.cos(ys / 173.0 + rng.random() * 6) + rng.integers(-4, 5, (h, w))     # a few bands, shared by neighbouring CTUs
        err = 2 + np.sin(xs / 301.0) + rng.integers(-2, 3, (h, w))
        planes.append((np.clip(base, 0, 255).astype(np.uint8), np.clip(base + err, 0, 255).astype(np.uint8)))
    return [p[0] for p in planes], [p[1] for p in planes]


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (W, H, source planes, deblocked planes, QP or a QP per CTU)"""
    import sao_merge_cases as K
    if name in ("416x240", "200x136", "416x240_qpmap"):
        W, H = (416, 240) if name.startswith("416") else (200, 136)
        p = K.ippp(W, H, 3)[2]                                       # a P picture of the mirror chain: source and deblocked picture of the oracle pipeline
        qp = p["qp"]
        if name.endswith("qpmap"):
            cols, rows = (W + 63) // 64, (H + 63) // 64
            qp = np.clip(qp + np.random.default_rng(3).integers(-6, 7, cols * rows), 10, 51).astype(np.int8)
        return W, H, p["src"], p["deb"], qp
    W, H = {"one_ctu": (64, 64), "one_row": (960, 64), "one_column": (64, 960), "partial_ctus": (136, 72)}[name]
    src, deb = _synthetic(W, H, W + H)
    return W, H, src, deb, 30


@pytest.mark.parametrize("name", ["416x240", "200x136", "416x240_qpmap", "one_ctu", "one_row", "one_column", "partial_ctus"])
def test_sao_stage_with_merge_candidates(ks, name):
    """KsFrame(sao=3).sao(): records (flags included) and the applied picture == the specification, byte for byte - pictures of the oracle pipeline (200x136: partial CTUs), a QP
    per CTU, and the chain's corner shapes: one CTU, one CTU row (left candidates only), one CTU column (upper candidates only)"""
    import sao_merge_ref as R
    from ks265codec_amd.lib import SAO_PARAM, KsFrame
    from ks265codec_amd.synth import lambda_q4
    W, H, src_p, deb_p, qp = _case(name)
    exp_rec, exp_planes = R.sao_merge(src_p, deb_p, qp)
    q0 = 30 if np.ndim(qp) else int(qp)
    with KsFrame(ks, W, H, q0, lambda_q4(q0), sao=3) as f:
        src, deb, dst = f.new_pic(), f.new_pic(), f.new_pic()
        f.load_i420(ks.dev(R.i420_of(src_p)), src)
        f.load_i420(ks.dev(R.i420_of(deb_p)), deb)
        if np.ndim(qp):
            f.set_qp_map(ks.dev(qp.view(np.uint8)))
        sao = ks.zeros(f.geom.bytes_sao)
        f.sao(src, deb, sao, dst)
        got_rec, got = ks.host(sao, SAO_PARAM), ks.host(f.store_i420(dst), np.uint8)
        f.set_qp_map(None)
    left, up, own = (int((exp_rec[0::3]["rsv"][:, 0] == 1).sum()), int((exp_rec[0::3]["rsv"][:, 1] == 1).sum()), int((exp_rec[0::3]["rsv"].sum(axis=1) == 0).sum()))
    print(f"{name}: {W}x{H}: merge left {left}, merge up {up}, own parameters {own}")
    bad = np.nonzero((got_rec.view(np.uint8).reshape(-1, 8) != exp_rec.view(np.uint8).reshape(-1, 8)).any(axis=1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} records differ, first: CTU {bad[0] // 3} component {bad[0] % 3}: {got_rec[bad[0]]} expected {exp_rec[bad[0]]}"
    exp = R.i420_of(exp_planes)
    assert (got == exp).all(), f"{name}: {int((got != exp).sum())} samples differ"
    if name == "one_ctu":
        assert left == up == 0
    elif name == "one_row":
        assert up == 0 and left > 0
    elif name == "one_column":
        assert left == 0 and up > 0
    elif name != "partial_ctus":
        assert left > 0 and up > 0 and own > 0


def test_pictures_end_to_end_with_merge_candidates(ks):
    """encode_picture for I, P, P and a B picture at 416x240 with sao = 3 == the mirror (the oracle's stages with tests/sao_merge_ref.py for its SAO stage, fed back as the reference
    picture): CU records, levels, SAO records, reconstruction"""
    import sao_merge_cases as K
    from ks265codec_amd.lib import CU8, SAO_PARAM, KsFrame
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
    W, H, qp = 416, 240, 31
    clip = make_clip(W, H, 5, 5, pan=(5, 3))
    order = [(0, "I"), (2, "P"), (4, "P"), (3, "B")]
    tools = dict(ENCODER_TOOLS, bi_refine=2)                      # the encoder host's tool set, with the joint refinement of B pictures
    exp = K.mirror(W, H, clip, qp, order, tools)
    flags = np.zeros(3, np.int64)
    with KsFrame(ks, W, H, qp, lambda_q4(qp), sao=3, bframes=1, **tools) as f:
        src, dev = f.new_pic(), {}
        for p in exp:
            d, kind = p["d"], p["kind"]
            f.set_qp(p["qp"], lambda_q4(p["qp"], inter=kind != "I"))
            f.load_i420(ks.dev(clip[d]), src)
            out = f.new_pic()
            if kind == "I":
                f.encode_picture(src, src, True, out)
            elif kind == "P":
                f.encode_picture(src, dev[d - 2], False, out)
            else:
                f.encode_picture_b(src, dev[d - 1], dev[d + 1], out)
            dev[d] = out
            gc = f.ws_read("cu8", f.geom.bytes_cu8).view(CU8)
            assert (gc == p["cu8"]).all(), f"picture {d} ({kind}): CU map differs"
            for c in range(3):
                assert (f.ws_read("levels", p["lvl"][c].size * 2, c).view(np.int16) == p["lvl"][c]).all(), f"picture {d} ({kind}): levels of component {c} differ"
            rec = f.ws_read("sao", f.geom.bytes_sao).view(SAO_PARAM)
            assert (rec.view(np.uint8) == p["records"].view(np.uint8)).all(), f"picture {d} ({kind}): SAO records differ"
            got = ks.host(f.store_i420(out), np.uint8)
            assert (got == p["recon"]).all(), f"picture {d} ({kind}): {int((got != p['recon']).sum())} reconstructed samples differ"
            flags += K.merge_counts(rec)
    assert (flags > 0).all(), flags


def test_lower_sao_modes_are_unchanged_on_the_same_frame_object(ks):
    """after a picture coded with sao = 3, set_picture_tools(sao=2) on the same frame object gives the records and pictures of the oracle's sao = 2 (test_reference_sao_decision),
    sao = 0 still codes in place, and -1 brings the merge candidates back"""
    from ks265codec_amd.lib import SAO_PARAM, KsFrame
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
    from oracle_lib import OraclePipeline
    W, H = 416, 240
    clip = make_clip(W, H, 3, seed=W, abc=(37, 53, 19), pan=(5, 3))
    o = OraclePipeline(W, H, 29, lambda_q4(29), sao=2, **ENCODER_TOOLS)
    with KsFrame(ks, W, H, 29, lambda_q4(29), sao=3, **ENCODER_TOOLS) as f:
        src, a, b = f.new_pic(), f.new_pic(), f.new_pic()
        f.load_i420(ks.dev(clip[0]), src)
        f.encode_picture(src, a, True, b)                             # a picture with the merge chain first
        assert (f.ws_read("sao", f.geom.bytes_sao).view(SAO_PARAM)["rsv"] != 0).any()
        f.set_picture_tools(sao=2)
        for t in range(3):
            q = 29 + (t > 0)
            lam = lambda_q4(q, inter=t > 0)
            o.set_qp(q, lam); f.set_qp(q, lam)
            exp = o.encode_picture(clip[t], t == 0)
            f.load_i420(ks.dev(clip[t]), src)
            f.encode_picture(src, a, t == 0, b)
            rec = f.ws_read("sao", f.geom.bytes_sao).view(SAO_PARAM)
            assert (rec.view(np.uint8) == o.sao.view(np.uint8)).all(), f"picture {t}: SAO records differ from sao = 2"
            assert (ks.host(f.store_i420(b), np.uint8) == exp).all(), f"picture {t}: reconstruction differs from sao = 2"
            a, b = b, a
        f.set_picture_tools(sao=0)
        f.load_i420(ks.dev(clip[2]), src)
        f.encode_picture(src, a, False, b)
        assert (f.ws_read("sao", f.geom.bytes_sao).view(SAO_PARAM)["type"] == -1).all()
        f.set_picture_tools(sao=-1)
        f.encode_picture(src, a, False, b)
        assert (f.ws_read("sao", f.geom.bytes_sao).view(SAO_PARAM)["rsv"] != 0).any()
    with KsFrame(ks, W, H, 29, lambda_q4(29), sao=2) as f:            # a frame object made for less has no chain workspace
        with pytest.raises(Exception):
            f.set_picture_tools(sao=3)


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="the reference's decoder was not staged (oracle/_ref/appdecoder)")
@pytest.mark.parametrize("W,H,n", [(416, 240, 5), (1920, 1080, 4)])
def test_cli_sao_ref_2_decodes_and_is_smaller(tmp_path, W, H, n):
    """ks265enc -sao-ref 2: the reference's decoder makes the -o reconstruction of the stream, which is smaller than the one -sao-ref 1 writes of the same clip"""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    stream.build()
    clip = make_clip(W, H, n, seed=W + n, abc=(37, 53, 19), pan=(5, 3))
    yuv = tmp_path / "in.yuv"
    clip.tofile(yuv)
    size = {}
    for mode in (1, 2):
        out, rec, dec = tmp_path / f"m{mode}.265", tmp_path / f"m{mode}.yuv", tmp_path / f"d{mode}.yuv"
        r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-rc", "0", "-preset", "slow", "-qp", "30", "-iper", "128", "-sao-ref", str(mode),
                            "-threads", "8", "-b", str(out), "-o", str(rec)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
        d = subprocess.run([REF_DEC, "-b", str(out), "-o", str(dec), "-threads", "4"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
        a, b = np.fromfile(rec, np.uint8), np.fromfile(dec, np.uint8)
        assert a.size == b.size == n * W * H * 3 // 2 and (a == b).all(), f"-sao-ref {mode}: the stream decodes differently from the encoder's reconstruction"
        size[mode] = os.path.getsize(out)
    print(f"{W}x{H}: -sao-ref 1 {size[1]} bytes, -sao-ref 2 {size[2]} bytes")
    assert size[2] < size[1]
