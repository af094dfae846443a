"""GPU: the HIP pipeline on adversarial content (tests/adversarial_clips.py) against the CPU oracle, bit for bit, no tolerances - flat pictures flipping 0 / 255,
full-scale checkerboards, uniform and binary noise, a full-scale edge: where the range arguments of the kernels (the biased 16-bit Hadamard sums of the MFMA path,
the 16-bit interpolation intermediates, the packed dot rows, the 14-bit bi average, the level clips at QP 0 / 51, the SAO clamps, the 16-bit lookahead costs,
cost words next to the 0xFFFFFFFF sentinel) hold or break.  The oracle at these inputs is decoder-verified (tests/test_adversarial_content_cpu.py, which also
asserts on the oracle's outputs that the content reaches those ranges).
  (a) P pictures stage by stage, (b) B pictures stage by stage, (c) intra decision / reconstruction and the key picture end to end, (d) the host's tool set end to
  end - the adversarial stream cases, rdoq, sao = 3, (e) lookahead operators and picture metrics, (g) the encoder CLI / API on incompressible pictures."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

from adversarial_clips import FAMILIES, make_adversarial, planes  # noqa: E402
from stream_cases import ADV_CASES, make_stream  # noqa: E402
from test_gpu_frame import _cmp_region  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "stream_adversarial_md5.json")))
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")
SIZES = [(136, 72), (72, 136), (64, 64)]
QPS = [0, 22, 51]


def _sizes(kind):
    return SIZES + ([(8, 8)] if kind in ("flat_flip", "cb1_flip") else [])


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


def _cmp_pic(name, ks, g, W, H, pic, exp, margin=False):
    """a device picture against three padded host planes"""
    org_y, org_c = g.pad_y * g.stride_y + g.pad_y, g.pad_c * g.stride_c + g.pad_c
    _cmp_region(name + ".y", ks.host(pic.y, np.uint8), exp[0], g.stride_y, org_y, W, H, margin=g.pad_y if margin else 0)
    _cmp_region(name + ".u", ks.host(pic.u, np.uint8), exp[1], g.stride_c, org_c, W // 2, H // 2, margin=g.pad_c if margin else 0)
    _cmp_region(name + ".v", ks.host(pic.v, np.uint8), exp[2], g.stride_c, org_c, W // 2, H // 2, margin=g.pad_c if margin else 0)


# ------------------------------------------------------------------ (a) P pictures, stage by stage
def _p_stages(ks, kind, W, H, qp, knobs, me, thr=0):
    from ks265codec_amd.lib import CU8, PU, SAO_PARAM, KsFrame
    from ks265codec_amd.synth import lambda_q4
    from oracle_lib import OraclePipeline
    nfr = 3
    clip = make_adversarial(kind, W, H, nfr, seed=W + qp)
    o = OraclePipeline(W, H, qp, lambda_q4(qp), me_method=me, me_hex_thr=thr, intra=False, **knobs)      # the stages by hand, with the flat key-picture stand-in
    tag = f"{kind} {W}x{H} qp {qp} me {me}"
    with KsFrame(ks, W, H, qp, lambda_q4(qp), me_method=me, me_hex_thr=thr, **knobs) as f:
        g = f.geom
        src, ref, deb, dst = f.new_pic(), f.new_pic(), f.new_pic(), f.new_pic()
        pu = [ks.zeros(g.bytes_pu), ks.zeros(g.bytes_pu)]
        cu8, sao = ks.zeros(g.bytes_cu8), ks.zeros(g.bytes_sao)
        lvl = [ks.zeros(W * H * 2), ks.zeros(W * H // 2), ks.zeros(W * H // 2)]
        have_prev = False
        bite = dict(frac=0, max_cost=0, max_level=0)          # what the ORACLE produced on these very pictures (the fixtures must bite)
        for t in range(nfr):
            q = qp if t == 0 else min(51, qp + 1)
            o.set_qp(q, lambda_q4(q)); f.set_qp(q, lambda_q4(q))
            key = t == 0
            o.encode_picture(clip[t], key)
            bite["max_level"] = max([bite["max_level"]] + [int(np.abs(l.astype(np.int32)).max()) for l in o.lvl])
            if not key:
                ok = o.prev_pu["cost"] != 0xFFFFFFFF
                bite["frac"] = max(bite["frac"], int((((o.prev_pu["mvx"] & 3) | (o.prev_pu["mvy"] & 3)) != 0)[ok].sum()))
                bite["max_cost"] = max(bite["max_cost"], int(o.prev_pu["cost"][ok].max()))
            f.load_i420(ks.dev(clip[t]), src)
            _cmp_pic(f"{tag}: src", ks, g, W, H, src, (o.src.y, o.src.u, o.src.v), margin=True)
            if key:
                f.cu_flat_intra(cu8)
            else:
                f.me_integer(src, ref, pu[1] if have_prev else None, pu[0])
                got = ks.host(pu[0], PU)
                assert (got == o.pu_int).all(), f"{tag}: integer ME: {int((got != o.pu_int).sum())} PU records differ (picture {t})"
                f.me_subpel(src, ref, pu[0])
                got = ks.host(pu[0], PU)
                exp = o.prev_pu                  # the oracle swapped its buffers after the picture
                bad = np.nonzero(got != exp)[0]
                assert len(bad) == 0, f"{tag}: sub-pel ME: {len(bad)} PU records differ (picture {t}), first {int(bad[0])}: {got[bad[0]]} != {exp[bad[0]]}"
                f.cu_decide(pu[0], cu8)
            f.reconstruct(src, ref, cu8, lvl, deb)
            gc = ks.host(cu8, CU8)
            assert (gc == o.cu8).all(), f"{tag}: cu8 map differs in {int((gc != o.cu8).sum())} blocks (picture {t})"
            for c in range(3):
                gl = ks.host(lvl[c], np.int16)[:o.lvl[c].size]
                assert (gl == o.lvl[c]).all(), f"{tag}: levels of component {c} differ in {int((gl != o.lvl[c]).sum())} places (picture {t})"
            _cmp_pic(f"{tag}: recon", ks, g, W, H, deb, o.rec_pre)
            f.deblock(cu8, deb)
            _cmp_pic(f"{tag}: deblock", ks, g, W, H, deb, (o.rec.y, o.rec.u, o.rec.v))
            f.sao(src, deb, sao, dst)
            gs = ks.host(sao, SAO_PARAM)
            assert (gs == o.sao).all(), f"{tag}: SAO parameters differ for {int((gs != o.sao).sum())} CTU components (picture {t})"
            _cmp_pic(f"{tag}: final", ks, g, W, H, dst, (o.ref.y, o.ref.u, o.ref.v), margin=True)
            ref, dst = dst, ref
            if not key:
                pu.reverse()
                have_prev = True
    return bite


# bnoise_pan at 136x72: the configurations (QP, preset, me_method) at which the oracle's largest PU cost reaches 2^20 (measured: 1 151 185, 1 132 554, 1 139 599).  Dropped
# for the others, where the measured maximum stays below: QP 0 with me_method 1 finds the exact pan in the near-lossless key picture (17 565 / 15 188), the Hadamard
# costs of veryslow reach 938 834 .. 995 364, veryfast at QP 51 reaches 1 003 470 (me_method 2: 995 902)
BNOISE_COST_MET = {(22, "veryfast", 1), (0, "veryfast", 2), (22, "veryfast", 2)}


@pytest.mark.parametrize("preset", ["veryfast", "veryslow"])          # candidates judged by SAD; full candidate sets judged by Hadamard (the MFMA path)
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("kind", FAMILIES)
def test_p_picture_stages_match_oracle(ks, kind, qp, preset):
    from ks265codec_amd.synth import subme_knobs
    bite = {}
    for W, H in _sizes(kind):
        bite[(W, H, 1)] = _p_stages(ks, kind, W, H, qp, subme_knobs(preset), 1)
    if kind == "bnoise_pan":
        bite[(136, 72, 2)] = _p_stages(ks, kind, 136, 72, qp, subme_knobs(preset), 2, 16)
    # the fixtures must bite: figures of the oracle's outputs on the pictures compared above, at 136x72
    print(f"{kind} qp {qp} {preset}: oracle figures {bite}")
    b = bite[(136, 72, 1)]
    if kind == "noise" and preset == "veryslow":
        assert b["frac"] > 50, b                                          # measured 195, 195, 174 (veryfast stays at full-sample vectors on noise: 0)
    if kind == "flat_flip" and qp == 0:
        assert b["max_level"] >= 8192, b                                  # measured 11 605
    if kind == "bnoise_pan":
        for me in (1, 2):
            if (qp, preset, me) in BNOISE_COST_MET:
                assert bite[(136, 72, me)]["max_cost"] >= 1 << 20, (me, bite[(136, 72, me)])


# ------------------------------------------------------------------ (b) B pictures, stage by stage
@pytest.mark.parametrize("refine", [0, 2])
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("kind", ["cb1_flip", "cb8_shift", "noise", "bnoise_pan"])
def test_b_picture_stages_match_oracle(ks, kind, qp, refine):
    """I0 P2 B1: both list searches, the records after ks265_bi_decide (refine 2: after ks265_bi_refine_chosen), CU records, levels, reconstruction"""
    from ks265codec_amd.lib import CU8, PU, PU_B, KsFrame
    from ks265codec_amd.synth import lambda_q4, subme_knobs
    from oracle_lib import OraclePipeline
    knobs = subme_knobs("veryslow")
    for W, H in _sizes(kind):
        tag = f"{kind} {W}x{H} qp {qp} refine {refine}"
        clip = make_adversarial(kind, W, H, 3, seed=W + qp + 1)
        o = OraclePipeline(W, H, qp, lambda_q4(qp), me_method=1, bi_refine=refine, decimate=2, **knobs)
        with KsFrame(ks, W, H, qp, lambda_q4(qp), me_method=1, bframes=1, bi_refine=refine, decimate=2, **knobs) as f:
            g = f.geom
            src = f.new_pic()
            dpb_o, dpb_g = {}, {}
            for t, k, r0, r1, dq in ((0, "I", None, None, 0), (2, "P", 0, None, 1), (1, "B", 0, 2, 3)):
                q = min(51, qp + dq)
                o.set_qp(q, lambda_q4(q)); f.set_qp(q, lambda_q4(q))
                dpb_o[t] = o.encode(clip[t], k, dpb_o.get(r0), dpb_o.get(r1))
                f.load_i420(ks.dev(clip[t]), src)
                out = f.new_pic()
                if k != "B":
                    f.encode_picture(src, dpb_g[r0] if r0 is not None else out, k == "I", out)
                else:
                    pu0, pu1, pub = ks.zeros(g.bytes_pu), ks.zeros(g.bytes_pu), ks.zeros(g.bytes_pu)
                    cu8, sao = ks.zeros(g.bytes_cu8), ks.zeros(g.bytes_sao)
                    lvl = [ks.zeros(W * H * 2), ks.zeros(W * H // 2), ks.zeros(W * H // 2)]
                    deb = f.new_pic()
                    f.me_integer(src, dpb_g[r0], None, pu0); f.me_subpel(src, dpb_g[r0], pu0)
                    f.me_integer(src, dpb_g[r1], None, pu1); f.me_subpel(src, dpb_g[r1], pu1)
                    h0, h1 = ks.host(pu0, PU), ks.host(pu1, PU)
                    assert (h0 == o.pu).all(), f"{tag}: list-0 search differs in {int((h0 != o.pu).sum())} PU records"
                    assert (h1 == o.pu1).all(), f"{tag}: list-1 search differs in {int((h1 != o.pu1).sum())} PU records"
                    f.bi_decide(src, dpb_g[r0], dpb_g[r1], pu0, pu1, pub)
                    if refine == 2:                 # the oracle's records are those behind the late refinement: decide, refine the chosen CUs, compare then
                        f.cu_decide_b(pub, cu8)
                        f.bi_refine_chosen(src, dpb_g[r0], dpb_g[r1], pu0, pu1, pub, cu8)
                    gb = ks.host(pub, PU_B)
                    bad = np.nonzero(gb != o.pub)[0]
                    assert len(bad) == 0, f"{tag}: bi decision differs for {len(bad)} PUs, first {int(bad[0])}: {gb[bad[0]]} != {o.pub[bad[0]]}"
                    if (W, H) == (136, 72) and qp == 51 and kind != "noise":      # the fixture must bite (on the oracle's records): L0, L1 and bi all occur
                        assert set(np.unique(o.pub["inter_dir"][o.pub["cost"] != 0xFFFFFFFF]).tolist()) == {1, 2, 3}, tag
                    if refine != 2:
                        f.cu_decide_b(pub, cu8)
                    f.reconstruct_b(src, dpb_g[r0], dpb_g[r1], cu8, lvl, deb)
                    gc = ks.host(cu8, CU8)
                    assert (gc == o.cu8).all(), f"{tag}: cu8 map differs in {int((gc != o.cu8).sum())} blocks"
                    for c in range(3):
                        gl = ks.host(lvl[c], np.int16)[:o.lvl[c].size]
                        assert (gl == o.lvl[c]).all(), f"{tag}: levels of component {c} differ"
                    _cmp_pic(f"{tag}: recon", ks, g, W, H, deb, o.rec_pre)
                    f.deblock(cu8, deb)
                    _cmp_pic(f"{tag}: deblock", ks, g, W, H, deb, (o.rec.y, o.rec.u, o.rec.v))
                    f.sao(src, deb, sao, out)
                dpb_g[t] = out
                got, exp = ks.host(f.store_i420(out), np.uint8), o.store(dpb_o[t])
                assert (got == exp).all(), f"{tag}: picture {t} ({k}): {int((got != exp).sum())} recon bytes differ"


# ------------------------------------------------------------------ (c) intra
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("kind", FAMILIES)
def test_intra_stages_match_oracle(ks, kind, qp):
    from ks265codec_amd.lib import CU8, KsFrame
    from ks265codec_amd.synth import lambda_q4
    from oracle_lib import OraclePipeline
    for W, H in _sizes(kind):
        tag = f"{kind} {W}x{H} qp {qp}"
        for t in (0, 1):                                              # (flat_flip: a black and a white picture)
            fr = make_adversarial(kind, W, H, 2, seed=H + qp)[t]
            o = OraclePipeline(W, H, qp, lambda_q4(qp), intra=True)
            with KsFrame(ks, W, H, qp, lambda_q4(qp)) as f:
                g = f.geom
                src, rec = f.new_pic(), f.new_pic()
                cu8 = ks.zeros(g.bytes_cu8)
                lvl = [ks.zeros(W * H * 2), ks.zeros(W * H // 2), ks.zeros(W * H // 2)]
                o.encode(fr, "I")
                f.load_i420(ks.dev(fr), src)
                f.intra_decide(src, cu8)
                gc = ks.host(cu8, CU8)
                oc = o.cu8.copy(); oc["cbf"] = 0                      # the oracle's map already carries the cbf of its reconstruction
                assert (gc == oc).all(), f"{tag}: intra decision differs in {int((gc != oc).sum())} of {gc.size} blocks"
                f.intra_reconstruct(src, cu8, lvl, rec)
                gc = ks.host(cu8, CU8)
                assert (gc == o.cu8).all(), f"{tag}: cbf differs in {int((gc != o.cu8).sum())} blocks"
                for k, (a, b) in enumerate(zip(lvl, o.lvl)):
                    assert (ks.host(a, np.int16)[:b.size] == b).all(), f"{tag}: intra levels differ (component {k})"
                _cmp_pic(f"{tag}: intra rec", ks, g, W, H, rec, o.rec_pre)


@pytest.mark.parametrize("kind", FAMILIES)
def test_key_picture_end_to_end(ks, kind):
    """ks265_encode_picture for a key picture (decision, wavefront reconstruction, deblocking, SAO) == the oracle's picture; QP 22, and the two extremes at 136x72"""
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import lambda_q4
    from oracle_lib import OraclePipeline
    for (W, H), qp in [(s, 22) for s in _sizes(kind)] + [((136, 72), 0), ((136, 72), 51)]:
        clip = make_adversarial(kind, W, H, 2, seed=7)
        o = OraclePipeline(W, H, qp, lambda_q4(qp))
        with KsFrame(ks, W, H, qp, lambda_q4(qp)) as f:
            src, a, b = f.new_pic(), f.new_pic(), f.new_pic()
            for t in (0, 1):
                exp = o.encode_picture(clip[t], True)
                f.load_i420(ks.dev(clip[t]), src)
                f.encode_picture(src, a, True, b)
                got = ks.host(f.store_i420(b), np.uint8)
                assert (got == exp).all(), f"{kind} {W}x{H} qp {qp} picture {t}: {int((got != exp).sum())} recon bytes differ"


# ------------------------------------------------------------------ (d) the host's tool set end to end
@pytest.mark.parametrize("name", list(ADV_CASES))
def test_hip_records_give_the_decoder_verified_adversarial_stream(ks, name):
    """the adversarial stream cases on the HIP pipeline (encode_picture, encode_picture_b, encode_picture_mref, encode_picture_b_mref with the host's switches: sdh,
    pre-search, merge, rdo = 4, intra_inter, propagate, skip_rd, part, tu_inter): every reconstruction == the oracle's, the stream == the decoder-verified one"""
    from test_gpu_stream import hip_encoder
    enc, f = hip_encoder(ks, name)
    try:
        bs, recs = make_stream(name, enc)
    finally:
        f.close()
    assert [hashlib.md5(recs[d].tobytes()).hexdigest() for d in sorted(recs)] == GOLD[name]["recon_md5"], f"{name}: reconstruction differs"
    assert hashlib.md5(bs).hexdigest() == GOLD[name]["stream_md5"], f"{name}: stream differs from the decoder-verified fixture ({len(bs)} vs {GOLD[name]['stream_bytes']} bytes)"


@pytest.mark.parametrize("kind,qp", [("noise", 0), ("bnoise_pan", 22), ("cb1_flip", 51)])
def test_rdoq_in_the_pixel_path(ks, kind, qp):
    """the host's tool set with rdoQuant at the seam of the reconstruction (tests/test_gpu_configs.py::test_rdoq_in_the_pixel_path) on I0 P2 B1 P3(2, 0)"""
    from ks265codec_amd import stream as S
    from ks265codec_amd.lib import CU8, KsFrame
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4
    from oracle_lib import OraclePipeline, lib as olib
    W, H = 136, 72
    clip = make_adversarial(kind, W, H, 4, seed=qp)
    tools = dict(ENCODER_TOOLS, tu_inter=1)
    w = S.StreamWriter(W, H)
    lam = np.array([int(256 * (0.85 * 2.0 ** ((q - 12) / 3.0)) + 0.5) for q in range(52)], np.int64)
    o = OraclePipeline(W, H, qp, lambda_q4(qp), **tools)
    with KsFrame(ks, W, H, qp, lambda_q4(qp), bframes=3, refs=2, **tools) as f:
        src = f.new_pic()
        dg, do = {}, {}
        for d, k, refs in [(0, "I", []), (2, "P", [0]), (1, "B", [0, 2]), (3, "P", [2, 0])]:
            q = qp if k == "I" else min(51, qp + 1 + (k == "B"))
            lq = lambda_q4(q, inter=k != "I")
            o.set_qp(q, lq); f.set_qp(q, lq)
            tab = w.rdoq_tables(None, S.SLICE_P if k == "P" else S.SLICE_B, q)
            if k != "I":
                olib().kso_experiment_rdoq(tab.ctypes.data_as(C.c_void_p), 1 | 8, None); f.set_rdoq(tab, lam, lam)
            else:
                olib().kso_experiment_rdoq(None, 0, None); f.set_rdoq(None)
            f.load_i420(ks.dev(clip[d]), src)
            out = f.new_pic()
            try:
                if k == "I":
                    eo = o.encode(clip[d], "I"); f.encode_picture(src, out, True, out)
                elif k == "B":
                    eo = o.encode(clip[d], "B", do[refs[0]], do[refs[1]]); f.encode_picture_b(src, dg[refs[0]], dg[refs[1]], out)
                elif len(refs) > 1:
                    eo = o.encode_mref(clip[d], [do[r] for r in refs]); f.encode_picture_mref(src, [dg[r] for r in refs], out)
                else:
                    eo = o.encode(clip[d], "P", do[refs[0]]); f.encode_picture(src, dg[refs[0]], False, out)
            finally:
                olib().kso_experiment_rdoq(None, 0, None)
            got, exp = ks.host(f.store_i420(out), np.uint8), o.store(eo)
            ly = f.ws_read("levels", W * H * 2, 0).view(np.int16)
            assert (ly == o.lvl[0]).all(), f"{kind} qp {qp} picture {d} ({k}): {int((ly != o.lvl[0]).sum())} luma levels differ"
            cu = f.ws_read("cu8", f.geom.bytes_cu8).view(CU8)
            assert (cu.view(np.uint8) == o.cu8.view(np.uint8)).all(), f"{kind} qp {qp} picture {d} ({k}): CU records differ"
            assert (got == exp).all(), f"{kind} qp {qp} picture {d} ({k}): {int((got != exp).sum())} recon bytes differ"
            dg[d], do[d] = out, eo


@pytest.mark.parametrize("kind,qp", [("noise", 22), ("edge_ramp", 0), ("cb8_shift", 51)])
def test_sao_merge_candidates_end_to_end(ks, kind, qp):
    """sao = 3 (tests/test_gpu_sao_merge.py) with the host's tool set on I0 P2 B1: CU records, levels, SAO records, reconstruction == the mirror"""
    import sao_merge_cases as K
    from ks265codec_amd.lib import CU8, SAO_PARAM, KsFrame
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4
    W, H = 136, 72
    q0 = min(qp, 49)                                                    # (the mirror codes P at + 1 and B at + 2)
    clip = make_adversarial(kind, W, H, 3, seed=qp + 2)
    tools = dict(ENCODER_TOOLS, bi_refine=2)
    exp = K.mirror(W, H, clip, q0, [(0, "I"), (2, "P"), (1, "B")], tools)
    with KsFrame(ks, W, H, q0, lambda_q4(q0), sao=3, bframes=1, **tools) as f:
        src, dev = f.new_pic(), {}
        for p in exp:
            d, k = p["d"], p["kind"]
            f.set_qp(p["qp"], lambda_q4(p["qp"], inter=k != "I"))
            f.load_i420(ks.dev(clip[d]), src)
            out = f.new_pic()
            if k == "I":
                f.encode_picture(src, src, True, out)
            elif k == "P":
                f.encode_picture(src, dev[0], False, out)
            else:
                f.encode_picture_b(src, dev[d - 1], dev[d + 1], out)
            dev[d] = out
            gc = f.ws_read("cu8", f.geom.bytes_cu8).view(CU8)
            assert (gc == p["cu8"]).all(), f"{kind} picture {d} ({k}): CU map differs"
            for c in range(3):
                assert (f.ws_read("levels", p["lvl"][c].size * 2, c).view(np.int16) == p["lvl"][c]).all(), f"{kind} picture {d} ({k}): levels of component {c} differ"
            rec = f.ws_read("sao", f.geom.bytes_sao).view(SAO_PARAM)
            assert (rec.view(np.uint8) == p["records"].view(np.uint8)).all(), f"{kind} picture {d} ({k}): SAO records differ"
            got = ks.host(f.store_i420(out), np.uint8)
            assert (got == p["recon"]).all(), f"{kind} picture {d} ({k}): {int((got != p['recon']).sum())} reconstructed samples differ"


# ------------------------------------------------------------------ (e) lookahead operators and picture metrics
def _lowres(frame, W, H):
    """the luma of an I420 picture at half resolution with the margin the lookahead operator's planes carry"""
    from cfc_cases import PAD
    from oracle_lib import lib as olib, ptr
    w, h = W // 2, H // 2
    out = np.zeros((h, w), np.uint8)
    y = np.ascontiguousarray(frame[:W * H])
    olib().ks265o_downsample(ptr(out), ptr(y), w, W, w, h)
    return np.ascontiguousarray(np.pad(out, PAD, mode="edge"))


# full size, log2 of the lookahead block, configuration words: the two shapes of the recorded calls of tests/golden/calc_frame_cost.npz (104x64 in 13 x 8 blocks of 8;
# 128x72 in 8 x 5 blocks of 16, the last block row ragged)
CFC_SHAPES = [(208, 128, 3, (64, 3, 0, 0, 30, 5, 0, 1, 1, 13, 1, 0, 1)), (256, 144, 4, (64, 4, 4, 1, 30, 2, 0, 1, 1, 13, 1, 0, 1))]


@pytest.mark.parametrize("W,H,lg,words", CFC_SHAPES, ids=["104x64_lg3", "128x72_lg4_ragged"])
@pytest.mark.parametrize("kind", FAMILIES)
def test_calc_frame_cost_matches_oracle(ks, kind, W, H, lg, words):
    """an intra pass, a P pass, a B pass that searches list 1 and reuses list 0 on half-resolution adversarial pictures: oracle == device on every array and sum"""
    from cfc_cases import ARR, CFG_WORDS, device_run, oracle_run
    from oracle_lib import lib as olib
    o = olib()
    clip = make_adversarial(kind, W, H, 3, seed=lg)
    p0, cur, p1 = (_lowres(clip[t], W, H) for t in range(3))
    w, h = W // 2, H // 2
    nx, ny = (w + (1 << lg) - 1) >> lg, (h + (1 << lg) - 1) >> lg
    n = nx * ny
    rng = np.random.default_rng(3)
    cfgw = dict(zip(CFG_WORDS, words))
    lam = np.array([max(1, int(round(0.85 * 2 ** ((q - 12) / 6.0)))) for q in range(52)], np.uint16)
    st = dict(intra=np.zeros(n, np.uint16), imode=np.zeros(n, np.uint8), invq=rng.integers(150, 500, n).astype(np.uint16), inter=np.zeros(n, np.uint16), bits=np.zeros((n + 3) // 4, np.uint8),
              mv0=np.full(n, 0x7fff, np.int32), c0=np.zeros(n, np.int32), mv1=np.full(n, 0x7fff, np.int32), c1=np.zeros(n, np.int32))
    sums, stats, done = [0, -1, -1, -1, -1], [0, 0, 0, 0], 0
    for (d0, d1, r0, r1, dl) in ((0, 0, cur, cur, (0, 0)), (1, 0, p0, None, (1, 0)), (1, 1, p0, p1, (0, 1))):
        a_o = {k: v.copy() for k, v in st.items()}
        s_in = sums if d0 + d1 == 0 else [sums[0], sums[1], sums[2], -1, -1]
        so, to, ro, do = oracle_run(o, w, h, nx, ny, cfgw, lam, cur, r0 if d0 else None, r1 if d1 else None, d0, d1, 0, 0, dl, done, a_o, s_in, stats)
        got, sg, tg, rg, dg = device_run(ks, w, h, nx, ny, cfgw, lam, cur, r0 if d0 else None, r1 if d1 else None, d0, d1, 0, 0, dl, done, st, s_in, stats)
        for name, _, _ in ARR:
            assert (got[name] == a_o[name]).all(), f"{kind} ({d0}, {d1}): {name} differs in {int((got[name] != a_o[name]).sum())} of {a_o[name].size}"
        assert (sg, tg, rg, dg) == (so, to, ro, do), f"{kind} ({d0}, {d1}): {(sg, tg, rg, dg)} != {(so, to, ro, do)}"
        st = a_o; done = do; sums = [so[0], so[1], so[2], -1, -1]; stats = to


@pytest.mark.parametrize("W,H", [(208, 128), (416, 240), (200, 136)], ids=["13x8", "26x15", "200x136_ragged"])       # the block counts of the recorded calls of tests/golden/lookahead_ref.npz; a picture with 8 columns and 8 rows beyond its whole blocks
def test_adapt_quant_and_ac_energy(ks, W, H):
    """calcFrameAdaptQuant on adversarial pictures == the oracle, doubles included; the AC energy map == the oracle's leaf operator at every block: 0 on the flat planes, the
    maximum n^2 * 255^2 / 4 on the 1-pixel checkerboard (8x8, 16x16: no wrap of the 32-bit sums)"""
    from oracle_lib import lib as olib, ptr
    o = olib()
    o.ks265o_ac_energy_plane.restype = C.c_uint32
    nx, ny = W // 16, H // 16
    for kind in FAMILIES:
        for fr in make_adversarial(kind, W, H, 2, seed=4):
            Y, U, V = (np.ascontiguousarray(p) for p in planes(fr, W, H))         # the device reads the whole planes (both operators take block counts and touch whole blocks only)
            Yc, Uc, Vc = np.ascontiguousarray(Y[:ny * 16, :nx * 16]), np.ascontiguousarray(U[:ny * 8, :nx * 8]), np.ascontiguousarray(V[:ny * 8, :nx * 8])   # the oracle's planes have no pitch
            want_off, want_inv = np.zeros(nx * ny), np.zeros(nx * ny, np.uint16)
            for s in (0.4, 1.0, 2.3):
                o.kso_ref_frame_adapt_quant(ptr(Yc), ptr(Uc), ptr(Vc), nx, ny, nx * ny, C.c_double(s), ptr(want_off), ptr(want_inv))
                off, inv = ks.frame_adapt_quant(ks.dev(Y), W, ks.dev(U), ks.dev(V), W // 2, nx, ny, s)
                assert (off.ravel() == want_off).all() and (inv.ravel() == want_inv).all(), (kind, s)
            for plane, pw, ph in ((Y, W, H), (U, W // 2, H // 2)):
                for log2 in (3, 4):
                    n = 1 << log2
                    m = ks.ac_energy_map(ks.dev(plane), pw, pw, ph, log2)
                    exp = np.array([[o.ks265o_ac_energy_plane(ptr(plane, y * n * pw + x * n), pw, log2) for x in range(pw >> log2)] for y in range(ph >> log2)], np.uint32)
                    assert (m == exp).all(), (kind, log2)
                    if kind == "flat_flip":
                        assert (m == 0).all()
                    if kind == "cb1_flip":
                        assert (m == n * n * 255 * 255 // 4).all()


@pytest.mark.parametrize("W,H", [(416, 240), (136, 72)], ids=["208x120", "68x36_ragged"])
def test_lookahead_picture_matches_oracle(ks, W, H):
    """tests/test_gpu_frame.py::test_lookahead_frame_cost on adversarial pictures: half-resolution pictures, intra pre-selection cost against integer-search cost, frame sums"""
    from ks265codec_amd.lib import KsFrame, PU
    from ks265codec_amd.synth import lambda_q4
    from oracle_lib import I, HostPic, OraclePipeline, lib as olib, ptr
    w, h = W // 2, H // 2
    if h % 8:
        h -= h % 8                                                           # (a frame object needs multiples of 8)
    w -= w % 8
    ol = olib()
    o_full, o_low = OraclePipeline(W, H, 30, lambda_q4(30)), OraclePipeline(w, h, 30, lambda_q4(30))
    with KsFrame(ks, W, H, 30, lambda_q4(30)) as ff, KsFrame(ks, w, h, 30, lambda_q4(30)) as fl:
        gf, gl = ff.geom, fl.geom
        of, olo = gf.pad_y * gf.stride_y + gf.pad_y, gl.pad_y * gl.stride_y + gl.pad_y
        src = ff.new_pic()
        for kind in FAMILIES:
            low_g, low_o = [], []
            for fr_ in make_adversarial(kind, W, H, 2, seed=6):
                ff.load_i420(ks.dev(fr_), src)
                lg = fl.new_pic()
                ks._chk(ks.lib.ks265_downsample_rect(ks.h, C.c_void_p(src.y.data_ptr() + of), C.c_int(gf.stride_y), C.c_void_p(lg.y.data_ptr() + olo), C.c_int(gl.stride_y), C.c_int(w), C.c_int(h)))
                fl.pad(lg)
                low_g.append(lg)
                o_full.load(o_full.src, fr_)
                lo = HostPic(o_low.geom)
                ol.ks265o_downsample(ptr(lo.y, olo), ptr(o_full.src.y, of), I(gl.stride_y), I(gf.stride_y), I(w), I(h))
                lo.u[:] = 0; lo.v[:] = 0
                ol.kso_pad_picture(C.byref(o_low.cfg), lo.c())
                low_o.append(lo)
                assert (ks.host(lg.y, np.uint8) == lo.y).all(), f"{kind}: low-resolution picture differs"
            got = fl.lookahead_picture(low_g[1], low_g[0])
            cost = np.zeros(o_low.nctu * 85, np.uint32)
            pu = np.zeros(o_low.nctu * 85, PU)
            exp = np.zeros(4, np.uint64)
            ol.kso_intra_decide_ex(C.byref(o_low.cfg), low_o[1].c(), ptr(o_low.cu8), ptr(cost))
            ol.kso_me_integer(C.byref(o_low.cfg), low_o[1].c(), low_o[0].c(), None, ptr(pu))
            ol.kso_lookahead_reduce(C.byref(o_low.cfg), ptr(cost), ptr(pu), ptr(exp))
            assert (got == exp).all(), (kind, got, exp)


@pytest.mark.parametrize("W,H", SIZES + [(200, 136)])
def test_picture_metrics(ks, W, H):
    """ks265_sse_picture == numpy int64; ks265_ssim_picture within one fixed-point unit per window of tests/ssim_ref.py (the bound of tests/test_gpu_ssim.py), its SSE bit for bit"""
    import ssim_ref
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import lambda_q4
    with KsFrame(ks, W, H, 27, lambda_q4(27)) as f:
        pa, pb = f.new_pic(), f.new_pic()
        for kind in FAMILIES:
            clip = make_adversarial(kind, W, H, 2, seed=8)
            for a, b, same in ((clip[0], clip[1], False), (clip[1], clip[1], True)):
                f.load_i420(ks.dev(a), pa); f.load_i420(ks.dev(b), pb)
                spec = [int(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum()) for x, y in zip(ssim_ref.planes_of(a, W, H), ssim_ref.planes_of(b, W, H))]
                assert f.sse_picture(pa, pb).tolist() == spec, kind
                res = ssim_ref.picture_ssim(a, b, W, H)
                sse, got = f.ssim_picture(pa, pb)
                assert sse.tolist() == spec, kind
                assert all(abs(int(gv) - fx) <= n for gv, (n, _, fx) in zip(got, res)), (kind, got.tolist(), [fx for _, _, fx in res])
                if same:
                    assert got.tolist() == [n << 30 for n, _, _ in res]


# ------------------------------------------------------------------ (g) the encoder CLI and API on incompressible pictures
def _decode(tmp_path, stream_path, tag):
    dec = tmp_path / f"{tag}_dec.yuv"
    d = subprocess.run([REF_DEC, "-b", str(stream_path), "-o", str(dec), "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
    assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
    return np.fromfile(dec, np.uint8)


@pytest.mark.parametrize("gop", ["default", "bframes0"])
@pytest.mark.parametrize("kind,qp", [("bnoise_pan", 0), ("noise", 0), ("flat_flip", 51)])
def test_cli_on_incompressible_pictures(tmp_path, kind, qp, gop):
    """`ks265enc -rc 0 -qp <q>` at 416x240: the encode succeeds although a picture costs more bytes than its samples, and the reference's decoder makes of the stream exactly
    the -o reconstruction"""
    from ks265codec_amd import stream
    stream.build()
    W, H, n = 416, 240, 6
    clip = make_adversarial(kind, W, H, n, seed=2)
    yuv, out, rec = tmp_path / "in.yuv", tmp_path / "out.265", tmp_path / "rec.yuv"
    clip.tofile(yuv)
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", str(qp), "-iper", "128", *(["-bframes", "0"] if gop == "bframes0" else []),
                        "-threads", "8", "-psnr", "1", "-b", str(out), "-o", str(rec)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-600:] + r.stderr[-600:]
    size = os.path.getsize(out)
    print(f"{kind} qp {qp} {gop}: {size} bytes, {size / n:.0f} per picture = {size / n / (W * H):.2f} x W x H")
    a = np.fromfile(rec, np.uint8)
    assert a.size == n * W * H * 3 // 2, a.size
    if qp == 0:
        assert size > n * W * H, "the fixture must cost more than a byte per sample"
    if os.path.exists(REF_DEC):                                          # (the decoder is staged by build() where the reference exists)
        b = _decode(tmp_path, out, "cli")
        assert a.size == b.size and (a == b).all(), "the decoder's pictures differ from the encoder's reconstruction"


def test_api_with_device_input_on_incompressible_pictures(tmp_path):
    """the C API with pictures in device memory: bnoise_pan at QP 0 - the stream of the host-input encode, decoded to the reconstruction"""
    from test_gpu_device_input import _dev, _nv12, encode
    W, H, n = 416, 240, 6
    clip = make_adversarial("bnoise_pan", W, H, n, seed=2)
    kw = dict(params=(("rc", 0), ("qp", 0), ("iper", 128)))
    rec = tmp_path / "rec.yuv"
    bs = encode(W, H, [("nv12", _dev(_nv12(f, W, H)), 0, 0) for f in clip], recon=rec, **kw)
    assert len(bs) > n * W * H
    assert bs == encode(W, H, list(clip), **kw), "device input and host input give one stream"
    assert rec.stat().st_size == n * W * H * 3 // 2
    if os.path.exists(REF_DEC):
        (tmp_path / "api.265").write_bytes(bs)
        assert _decode(tmp_path, tmp_path / "api.265", "api").tobytes() == rec.read_bytes()
