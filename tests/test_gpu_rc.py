"""GPU: the rate-controlled BASELINE configurations through the CLI (`-rc 3 -crf 24 -bframes 3` = config 4, `-preset veryslow -rc 1 -br N` = config 5;
north_star: "reconstructed YUV matches within +-1 LSB under -rc 1/3").  For every run: (1) what the MI355X reconstructed (-o) is byte for byte what the reference's own
decoder makes of the stream (bit-exact, which subsumes +-1 LSB); (2) the oracle pipeline fed the SAME per-picture QPs (read from the encoder's `-psnr 2` table) and the
host's GOP layout reproduces that reconstruction picture for picture; (3) for the bitrate targets: the achieved bitrate is near the target (the controller
had no test against real content)."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (see tests/test_gpu_enc_api.py: torch's HIP runtime first)
torch.cuda.is_available()
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")


def _encode(tmp_path, clip, W, H, opts, tag="o", env=None):
    from ks265codec_amd import stream
    stream.build()
    yuv, out, rec = tmp_path / f"{tag}.yuv", tmp_path / f"{tag}.265", tmp_path / f"{tag}_rec.yuv"
    clip.tofile(yuv)
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", *opts, "-threads", "16", "-psnr", "2", "-b", str(out), "-o", str(rec)],
                       capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-600:] + r.stderr[-600:]
    per = [(int(a), k, int(b), int(q)) for a, k, b, q in re.findall(r"^(\d+)\t([IPB])\t(\d+)\t[\d.]+\t[\d.]+\t[\d.]+\t(\d+)$", r.stdout, re.M)]      # coding order: poc, kind, bits, qp
    m = re.search(r"bitrate, psnr:\s*([\d.]+)\s+([\d.]+)", r.stdout)
    return r.stdout + r.stderr, per, float(m.group(1)), np.fromfile(rec, np.uint8), out


def _decoder_check(tmp_path, out, rec, n, fsz):
    if not os.path.exists(REF_DEC):
        pytest.skip("the reference's decoder was not staged (oracle/_ref/appdecoder)")
    dec = tmp_path / "dec.yuv"
    d = subprocess.run([REF_DEC, "-b", str(out), "-o", str(dec), "-threads", "4"], capture_output=True, text=True, cwd=tmp_path)
    assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
    b = np.fromfile(dec, np.uint8)
    assert rec.size == b.size == n * fsz, (rec.size, b.size)
    bad = [t for t in range(n) if not (rec[t * fsz:(t + 1) * fsz] == b[t * fsz:(t + 1) * fsz]).all()]
    assert not bad, f"pictures {bad} decode differently from the encoder's reconstruction"


def _aq_map(o, i420, qp, strength):
    """the host's -aq arithmetic on the CPU: the oracle's restatement of calcFrameAdaptQuant over the padded source picture, then one QP per CTU"""
    import ctypes as C
    from oracle_lib import HostPic, ptr
    g = o.geom
    W, H = o.cfg.width, o.cfg.height
    nx, ny = (W + 15) // 16, (H + 15) // 16
    tmp = HostPic(g)
    o.load(tmp, i420)
    Y = np.ascontiguousarray(tmp.y.reshape(-1, g.stride_y)[g.pad_y:g.pad_y + ny * 16, g.pad_y:g.pad_y + nx * 16])
    U, V = (np.ascontiguousarray(p.reshape(-1, g.stride_c)[g.pad_c:g.pad_c + ny * 8, g.pad_c:g.pad_c + nx * 8]) for p in (tmp.u, tmp.v))
    off, inv = np.zeros(nx * ny), np.zeros(nx * ny, np.uint16)
    o.o.kso_ref_frame_adapt_quant(ptr(Y), ptr(U), ptr(V), nx, ny, nx * ny, C.c_double(strength), ptr(off), ptr(inv))
    qmap = np.zeros(((nx + 3) // 4) * ((ny + 3) // 4), np.int8)
    o.o.kso_aq_ctu_map(ptr(off), nx, ny, qp, 0, 51, ptr(qmap))
    return qmap


def _mirror(clip, W, H, per, refs_of, rec, tools, upto, aq=0.0, maps=None, ref0=1):
    """the oracle pipeline with the encoder's per-picture QPs and reference pictures: reconstruction == the encoder's, for the first `upto` pictures in coding order"""
    from ks265codec_amd.synth import lambda_q4
    from oracle_lib import OraclePipeline
    fsz = W * H * 3 // 2
    o = OraclePipeline(W, H, 27, lambda_q4(27), **tools)
    dpb = {}
    spread = set()
    # the references of every picture first: a B picture nothing predicts from is coded without intra candidates, joint refinement and SAO (the host's lean B pictures, ks265_gop.h GopPic::lean)
    all_refs = [refs_of(i, poc, kind) for i, (poc, kind, _, _) in enumerate(per)]
    used = set()
    for a, b in all_refs:
        for r in (a, b):
            used |= set(r) if isinstance(r, list) else ({r} if r is not None else set())
    for i, (poc, kind, _, qp) in enumerate(per[:upto]):
        o.set_qp(qp, lambda_q4(qp, inter=kind != "I"))
        a0, a1 = all_refs[i]
        n0, n1 = (a0[0] if isinstance(a0, list) else a0), (a1[0] if isinstance(a1, list) else a1)
        near = kind == "B" and poc - n0 <= 2 and n1 - poc <= 2                    # ... and one others predict from whose references are at most two pictures away: no intra candidates, no SAO
        o.set_picture_tools(*((0, 0, 0) if kind == "B" and poc not in used else (0, -1, 0) if near else (-1, -1, -1)))
        if maps is not None:
            o.set_qp_map(maps[poc]); spread |= set(maps[poc].tolist())
        elif aq:
            qmap = _aq_map(o, clip[poc], qp, aq)
            o.set_qp_map(qmap)
            spread |= set(qmap.tolist())
        r0, r1 = all_refs[i]
        if kind == "P" and r0 is not None and not isinstance(r0, list):    # round 6: an anchor of a pyramid searches the last ref0 anchors of its GOP, nearest first (-ref0; ks265_gop.h gop_plan)
            last_key = max(j for j, (_, k, _, _) in enumerate(per[:i]) if k == "I")
            hist = [p for p, k, _, _ in per[last_key:i] if k != "B"][::-1]
            if ref0 > 1 and hist and hist[0] == r0:
                r0 = hist[:ref0]
        if kind == "P" and isinstance(r0, list):
            dpb[poc] = o.encode_mref(clip[poc], [dpb[r] for r in r0])
        elif isinstance(r0, list):                                        # several pictures per list (B pictures under -ref N): [nearest first]
            dpb[poc] = o.encode_b_mref(clip[poc], [dpb[r] for r in r0], [dpb[r] for r in r1])
        else:
            dpb[poc] = o.encode(clip[poc], kind, dpb.get(r0), dpb.get(r1))
        want = o.store(dpb[poc])
        assert (rec[poc * fsz:(poc + 1) * fsz] == want).all(), f"picture {poc} ({kind}, qp {qp}, coding position {i}): the encoder's reconstruction differs from the oracle pipeline fed the same QP"
    o.set_qp_map(None)
    return spread


def _crf_case(tmp_path, W, H, n, upto, extra=()):
    """config 4's command line: -preset slow -rc 3 -crf 24 -bframes 3.  The picture QPs are the ladder on crf (I = crf, anchors + 1, B + 2 / + 3: the reference's CRF with its tree on keeps
    picture QPs near-constant too); the QP of every CTU comes from the cuTree pass over the lookahead window (calcFrameCost enc@0x4a7410, cuTreePropagate enc@0x47d460, the finish) -
    held against tests/cutree_mirror.py, whose pass reproduces the reference's own per-picture offsets on whole runs (tests/test_calc_frame_cost.py)"""
    from cutree_mirror import CuTree, read_qpmap_dump
    from ks265codec_amd.synth import ENCODER_TOOLS, make_clip
    clip = make_clip(W, H, n, seed=W + n, abc=(37, 53, 19), pan=(5, 3))
    dump = tmp_path / "maps.bin"
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, ["-preset", "slow", "-rc", "3", "-crf", "24", "-bframes", "3", "-iper", "128", *extra], env={"KS265_DUMP_QPMAP": str(dump)})
    assert "cuTree over a lookahead" in log, log[:1500]
    # -bframes 3 is a pyramid of 4 as in the reference (its -psnr 2 lines: coding order 0 4 2 1 3 8 6 5 7 .., QP + 1 / + 2 / + 3 / + 3): the middle picture is a reference B
    assert len(per) == n and [(p, k) for p, k, _, _ in per[:9]] == [(0, "I"), (4, "P"), (2, "B"), (1, "B"), (3, "B"), (8, "P"), (6, "B"), (5, "B"), (7, "B")]
    assert {(k, q) for _, k, _, q in per} == {("I", 24), ("P", 25), ("B", 26), ("B", 27)}
    _decoder_check(tmp_path, out, rec, n, W * H * 3 // 2)
    got = read_qpmap_dump(dump)
    kw = dict(zip(extra[::2], extra[1::2]))
    ct = CuTree(clip, W, H, preset=5, gop_b=3, hier=True, iper=128, lookahead=int(kw.get("-lookahead", -1)), aq_strength=float(kw.get("-aqs", 1.0)) if kw.get("-aq") == "1" else 0.0)
    ct.run()
    maps, lowered = {}, 0
    for poc, kind, _, qp in per:
        maps[poc] = ct.ctu_map(poc, qp)
        assert got[poc][1] == qp and (got[poc][2] == maps[poc]).all(), f"picture {poc} ({kind}, qp {qp}): the encoder's QP per CTU differs from the cuTree mirror's in {int((got[poc][2] != maps[poc]).sum())} CTUs"
        lowered += int((maps[poc] < qp).sum())
    assert lowered > len(per), "the tree lowers QPs where later pictures predict from"
    coded = []

    def refs(i, poc, kind):                                                # the nearest pictures coded before on either side (the outer B pictures of a block come last)
        if kind == "I":
            coded.append(poc); return None, None
        lo = max(p for p in coded if p < poc)
        hi = min((p for p in coded if p > poc), default=None)
        coded.append(poc)
        return (lo, None) if kind == "P" else (lo, hi)
    spread = _mirror(clip, W, H, per, refs, rec, ENCODER_TOOLS, upto=upto, maps=maps, ref0=3)                  # (-preset slow: ref 1 / ref0 3)
    assert len(spread) >= 3
    return log


def test_crf_with_three_b_pictures(tmp_path):
    """config 4's command line at 1920x1080"""
    _crf_case(tmp_path, 1920, 1080, 13, upto=9)


def test_crf_with_three_b_pictures_and_adaptive_quantisation(tmp_path):
    """... with -aq 1: the tree's offsets start from the block-variance offsets (calcFrameAdaptQuant enc@0x4653c0 on the lookahead's grid, as the reference calls it); 1280x720, a window of 16"""
    _crf_case(tmp_path, 1280, 720, 21, upto=5, extra=("-aq", "1", "-aqs", "1.0", "-lookahead", "20"))


def test_crf_with_three_b_pictures_at_2160p(tmp_path):
    """config 4's command line at its own size, 3840x2160: decoder == -o, the QP per CTU == the cuTree mirror's for every picture, the oracle pipeline on those maps == -o for the first pictures"""
    _crf_case(tmp_path, 3840, 2160, 9, upto=3)


def test_bitrate_target_ippp(tmp_path):
    """-rc 1 on real content: the controller moves the QP, the stream decodes to the reconstruction, the oracle fed the same QPs agrees, and the bitrate lands near the target"""
    from ks265codec_amd.synth import ENCODER_TOOLS, make_clip
    W, H, n, target = 832, 480, 300, 1000
    base = make_clip(W, H, 31, seed=7, abc=(37, 53, 19), pan=(5, 3))
    order = list(range(31)) + list(range(29, 0, -1))
    clip = base[[order[t % len(order)] for t in range(n)]]
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, ["-preset", "slow", "-rc", "1", "-br", str(target), "-bframes", "0", "-iper", "100"])
    assert len(per) == n
    qps = [q for _, k, _, q in per if k == "P"]
    assert max(qps) - min(qps) >= 4, "the controller never moved the QP"
    _decoder_check(tmp_path, out, rec, n, W * H * 3 // 2)
    _mirror(clip, W, H, per, lambda i, poc, kind: (None, None) if kind == "I" else (poc - 1, None), rec, ENCODER_TOOLS, upto=40)
    bits = np.array([b for _, _, b, _ in per], np.float64)
    whole = bits.sum() / n * 50 / 1000
    tail = bits[n // 2:].sum() / (n - n // 2) * 50 / 1000
    print(f"target {target} kbit/s: whole run {whole:.0f}, second half {tail:.0f}; P-picture QPs {min(qps)}..{max(qps)}")
    assert abs(whole / target - 1) < 0.10 and abs(tail / target - 1) < 0.10, (whole, tail, target)      # within 3 % measured (971 / 1 000); VERDICT r4: the test holds it to 10 %


def test_config5_command_line(tmp_path):
    """config 5's command line at 1920x1080: -preset veryslow -latency offline(= default) -rc 1 -br N with the SDK's default (hierarchical) GOP - the sub-pel refinement
    runs as -subme 2 with the Hadamard measure (what veryslow resolves to); -part 1 acts on P and B pictures (round 5); what the host still narrows (4 references per list with B pictures) is in its log"""
    from ks265codec_amd.synth import ENCODER_TOOLS, make_clip, subme_knobs
    W, H, n = 1920, 1080, 25
    clip = make_clip(W, H, n, seed=W + n, abc=(37, 53, 19), pan=(5, 3))
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, ["-preset", "veryslow", "-rc", "1", "-br", "5000", "-iper", "128"])
    assert len(per) == n and "subme 2" in log, log[:800]
    _decoder_check(tmp_path, out, rec, n, W * H * 3 // 2)
    tools = dict(ENCODER_TOOLS, me_hex_thr=0, part=1, tu_inter=1, bi_refine=2, **subme_knobs("veryslow"))    # veryslow: always UMH, -subme 2 judged by Hadamard, -part 1 (P and B pictures)
    assert "up to 4 pictures per list" in log, log[:1200]
    st = {"keep": [], "anchor": None}                                          # the host's planner (ks265_gop.h gop_plan): the reference pictures of the mini-GOP coded so far (its two ends first)

    def refs(i, poc, kind):
        if kind == "I":
            st["anchor"] = poc; st["keep"] = [poc]; return None, None
        if kind == "P":
            lo = st["anchor"]; st["keep"] = [lo, poc]; st["anchor"] = poc
            return lo, None
        before, after = sorted([p for p in st["keep"] if p < poc], reverse=True)[:4], sorted([p for p in st["keep"] if p > poc])[:4]
        if poc - before[0] >= 2 or after[0] - poc >= 2:                        # a B picture others predict from
            st["keep"].append(poc)
        return before, after
    _mirror(clip, W, H, per, refs, rec, tools, upto=18, ref0=4)                                              # (-preset veryslow: ref 4 / ref0 4; 18 pictures: the second anchor has two past anchors)
    assert any(k == "B" for _, k, _, _ in per[:9])


def test_bitrate_target_at_2160p_decodes(tmp_path):
    """config 5 at its own size (property run): 3840x2160 -preset veryslow -rc 1 -br 20000 - the stream decodes to the MI355X's reconstruction"""
    from ks265codec_amd.synth import make_clip
    W, H, n = 3840, 2160, 9
    clip = make_clip(W, H, n, seed=7, abc=(67, 91, 33), pan=(8, 5))
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, ["-preset", "veryslow", "-rc", "1", "-br", "20000", "-iper", "128"])
    assert len(per) == n
    _decoder_check(tmp_path, out, rec, n, W * H * 3 // 2)


@pytest.mark.parametrize("W,H", [(200, 136), (416, 240)])
def test_adaptive_quantisation_small_pictures(tmp_path, W, H):
    """-aq at picture sizes that are no multiple of 16 / 64: the blocks that hang over the picture read the replicated edge, partial CTUs average the blocks they have"""
    from ks265codec_amd.synth import ENCODER_TOOLS, make_clip
    n = 7
    clip = make_clip(W, H, n, seed=W + n, abc=(17, 23, 9), pan=(5, 3))
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, ["-preset", "slow", "-rc", "0", "-qp", "28", "-iper", "128", "-bframes", "0", "-aq", "1", "-aqs", "2.0"])
    assert len(per) == n
    _decoder_check(tmp_path, out, rec, n, W * H * 3 // 2)
    spread = _mirror(clip, W, H, per, lambda i, poc, kind: (None, None) if kind == "I" else (poc - 1, None), rec, ENCODER_TOOLS, upto=n, aq=2.0)
    assert len(spread) >= 3, sorted(spread)


@pytest.mark.parametrize("gop", ["ippp", "hier"])
def test_adaptive_quantisation(tmp_path, gop):
    """-aq 1 -aqs S (iAqMode / fAqStrength, qy265enc.h:145-146): the QP of every CTU follows the reference's calcFrameAdaptQuant on the source picture (device operator pinned on
    recorded calls of the reference: tests/test_gpu_lookahead_ops.py) - (1) the reference's decoder makes of the stream exactly what the encoder reconstructed, cu_qp_delta
    and the deblocking at the decoder's QpY included; (2) the oracle pipeline fed the same QPs and maps (computed on the CPU) reproduces it picture for picture"""
    from ks265codec_amd.synth import ENCODER_TOOLS, make_clip
    W, H, n = 1920, 1080, 9
    clip = make_clip(W, H, n, seed=W + n, abc=(37, 53, 19), pan=(5, 3))
    opts = ["-preset", "slow", "-rc", "0", "-qp", "30", "-iper", "128", "-aq", "1", "-aqs", "1.2"] + (["-bframes", "0"] if gop == "ippp" else [])
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, opts)
    assert len(per) == n
    _decoder_check(tmp_path, out, rec, n, W * H * 3 // 2)
    coded = []

    def refs(i, poc, kind):
        if kind == "I":
            coded.append(poc); return None, None
        lo = max(p for p in coded if p < poc)
        hi = min((p for p in coded if p > poc), default=None)
        coded.append(poc)
        return (lo, None) if kind == "P" else (lo, hi)
    spread = _mirror(clip, W, H, per, refs, rec, ENCODER_TOOLS, upto=6, aq=1.2, ref0=3 if gop == "hier" else 1)
    assert len(spread) >= 4, f"the maps hold {sorted(spread)}: adaptive quantisation did nothing"
    plain = _encode(tmp_path, clip, W, H, [o for o in opts if o not in ("-aq", "1", "-aqs", "1.2")] + ["-aq", "0"], tag="plain")
    assert open(plain[4], "rb").read() != open(out, "rb").read()


@pytest.mark.parametrize("gop", ["ippp", "hier"])
def test_adaptive_quantisation_with_key_pictures_on_their_own_stream(tmp_path, gop):
    """with -iper >= 32 a key picture is coded on its own stream BESIDE the last pictures of the GOP before it; its QP map used to share the rotation slot's buffer
    with a picture still running.  The -o dump switches that overlap off, so: (1) with -o (no overlap) the stream decodes to the encoder's reconstruction; (2) WITHOUT -o (overlap on,
    three key pictures) the encoder writes the same bytes, run after run - a map overwritten under a running picture makes slice and pixels disagree and the bytes move"""
    from ks265codec_amd import stream
    from ks265codec_amd.synth import make_clip
    W, H, n = 1280, 720, 100
    base = make_clip(W, H, 26, seed=W + n, abc=(37, 53, 19), pan=(5, 3))
    order = list(range(26)) + list(range(24, 0, -1))
    clip = base[[order[t % len(order)] for t in range(n)]]
    opts = ["-preset", "slow", "-rc", "0", "-qp", "30", "-iper", "32", "-aq", "1", "-aqs", "1.5"] + (["-bframes", "0"] if gop == "ippp" else [])
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, opts)
    assert len(per) == n and sum(k == "I" for _, k, _, _ in per) == 4
    _decoder_check(tmp_path, out, rec, n, W * H * 3 // 2)
    want = open(out, "rb").read()
    yuv = tmp_path / "o.yuv"
    for run in range(3):
        o2 = tmp_path / f"overlap{run}.265"
        r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", *opts, "-threads", "16", "-b", str(o2)], capture_output=True, text=True)
        assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-600:] + r.stderr[-600:]
        assert open(o2, "rb").read() == want, f"run {run}: the stream coded with key pictures on their own stream differs from the one coded without the overlap"


def test_crf_job_over_two_lanes(tmp_path):
    """-rc 3 with the GOPs dealt to two lanes (KS265_DEVICES=0,0 names this box's one GPU twice) is byte for byte the one-lane stream"""
    from ks265codec_amd.synth import make_clip
    W, H, n = 416, 240, 140
    base = make_clip(W, H, 23, seed=77, abc=(17, 23, 9))
    clip = base[[t % 23 for t in range(n)]]
    opts = ["-preset", "slow", "-rc", "3", "-crf", "26", "-bframes", "3", "-iper", "32"]
    _, _, _, _, one = _encode(tmp_path, clip, W, H, opts, tag="one")
    log, _, _, _, two = _encode(tmp_path, clip, W, H, opts, tag="two", env={"KS265_DEVICES": "0,0"})
    assert "GOP lanes" in log or "lanes" in log
    assert open(one, "rb").read() == open(two, "rb").read()


def test_rdoq_command_line(tmp_path):
    """round 6: `ks265enc -preset slow -rdoq 1` - the SDK's rdoq field asked for by name sends the luma transform blocks of inter CUs through the reference's
    rdoQuant, with bit tables that follow the stream: a P picture is quantised with the tables built (ks265_rdoq_tables = estBitRdoq enc@0x46a8a0) from the context states the
    slice of the latest P picture coded at least 17 pictures earlier (in the same GOP) ended with, else from the initial states of its slice at its QP.  (1) the reference's decoder
    reproduces -o; (2) the mirror - oracle pipeline with the pinned rdoQuant restatement at its seam, this writer's slices, the same rule for the tables (built by the ORACLE's
    pinned estBitRdoq restatement from the writer's states) - reproduces -o picture for picture, past the point where the tables start to move; (3) the stream differs from the
    default's, and `-rdoq 0` / no option are the default stream"""
    import ctypes as C
    from ks265codec_amd import stream as S
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
    from oracle_lib import OraclePipeline, lib as olib
    W, H, n = 416, 240, 30
    fsz = W * H * 3 // 2
    clip = make_clip(W, H, n, seed=W + n, abc=(17, 23, 9), pan=(5, 3))
    opts = ["-preset", "slow", "-rc", "0", "-qp", "30", "-iper", "128", "-bframes", "0"]
    log, per, kbps, rec, out = _encode(tmp_path, clip, W, H, opts + ["-rdoq", "1"])
    assert len(per) == n and "rdoQuant" in log, log[:1200]
    _decoder_check(tmp_path, out, rec, n, fsz)
    plain = _encode(tmp_path, clip, W, H, opts, tag="plain")
    assert open(plain[4], "rb").read() != open(out, "rb").read()
    assert open(_encode(tmp_path, clip, W, H, opts + ["-rdoq", "0"], tag="zero")[4], "rb").read() == open(plain[4], "rb").read()
    # the mirror
    ez = np.load(os.path.join(HERE, "golden", "estbits.npz"))
    ent = np.zeros(128, np.int32)
    for i in range(int(ez["__n__"])):
        if str(ez[f"c{i}__kind"]) == "table":
            ent[int(ez[f"c{i}__ctx"][0])] = ez[f"c{i}__exp"][0]

    def tables_of(states, lay):                                       # the oracle's pinned estBitRdoq on this writer's states in the function's own order (tools/rd_eval.py --rdoq-adaptive)
        cbf_l, cbf_c, csbf, sig, lx, ly, g1, g2, root, _ = lay
        c = np.zeros(256, np.uint8)
        c[0x0d:0x0d + 2] = states[cbf_l:cbf_l + 2]; c[0x12:0x12 + 4] = states[cbf_c:cbf_c + 4]; c[0x1d:0x1d + 4] = states[csbf:csbf + 4]; c[0x21:0x21 + 42] = states[sig:sig + 42]
        c[0x4b:0x4b + 18] = states[lx:lx + 18]; c[0x69:0x69 + 18] = states[ly:ly + 18]; c[0x87:0x87 + 24] = states[g1:g1 + 24]; c[0x9f:0x9f + 6] = states[g2:g2 + 6]; c[0xaa] = states[root]
        T = np.zeros((4, 2, 180), np.int32)
        for lg in range(2, 6):
            for ch in (0, 1):
                olib().ks265o_est_bit_rdoq(T[lg - 2, ch].ctypes.data_as(C.c_void_p), lg, int(not ch), c.ctypes.data_as(C.c_void_p), ent.ctypes.data_as(C.c_void_p))
        return T
    o = OraclePipeline(W, H, 30, lambda_q4(30), **ENCODER_TOOLS)
    w = S.StreamWriter(W, H, max_dec_pic_buffering=2, max_num_reorder=0, sdh=1, wpp=1)
    init = S.StreamWriter(W, H, max_dec_pic_buffering=2, max_num_reorder=0, sdh=1, wpp=1)
    hist, ref, moved = {}, None, 0
    try:
        for s, (poc, kind, _, qp) in enumerate(per):
            assert poc == s
            o.set_qp(qp, lambda_q4(qp, inter=kind != "I"))
            T = None
            if kind != "I":
                src = next((q for q in range(s - 17, 0, -1) if q in hist), None)      # the latest P picture at least 17 pictures earlier, behind the key picture
                if src is not None:
                    T = tables_of(*hist[src]); moved += 1
                else:
                    st0, lay0 = np.zeros(256, np.uint8), None
                    T = init.rdoq_tables(None, S.SLICE_P, qp).reshape(4, 2, 180)
                    # (the initial tables through the oracle's function too: the writer's initial states of a P slice at this QP)
                olib().kso_experiment_rdoq(T.ctypes.data_as(C.c_void_p), 1 | 8, None)
            else:
                olib().kso_experiment_rdoq(None, 0, None)
            ref = o.encode(clip[poc], kind, ref, None)
            want = o.store(ref)
            assert (rec[poc * fsz:(poc + 1) * fsz] == want).all(), f"picture {poc} ({kind}, qp {qp}): the encoder's reconstruction differs from the mirror's ({'tables of picture %d' % src if kind != 'I' and src is not None else 'initial tables'})"
            w.slice(S.NAL_IDR_W_RADL if kind == "I" else S.NAL_TRAIL_R, S.SLICE_I if kind == "I" else S.SLICE_P, poc, qp, o.cu8, o.lvl, o.sao, rps=[(poc - 1, True)] if poc else [], l0=[poc - 1] if poc else [], l1=[])
            if kind == "P":
                hist[s] = w.final_contexts()
    finally:
        olib().kso_experiment_rdoq(None, 0, None)
    assert moved >= 10
