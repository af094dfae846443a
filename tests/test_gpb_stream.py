"""CPU: the rule of the `gpb` switch (include/ks265_enc.h) before any host code runs - the oracle pipeline codes the anchors of a pyramid of 4 as B pictures over past anchors
(list 0 = [a1, a3], list 1 = [a2], no skip pass), the stream writer signals the lists (list_mod), and the reference's decoder must reproduce every reconstruction; and the
CPU mirror of the host (tools/rd_eval.py --host with KS265_GPB=1) writes the slice headers the host writes."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")


def gpb_lists(hist: list, ref0: int = 3):
    """the rule: hist = the GOP's anchors so far, nearest first -> (list 0, list 1); one anchor: a P picture"""
    a = hist[:ref0]
    return ([a[0]] + a[2:], [a[1]]) if len(a) > 1 else (a, [])


@pytest.mark.skipif(not os.path.exists(DEC), reason="reference decoder only exists in the builder container")
def test_reference_decoder_reproduces_anchors_coded_as_b_pictures_over_past_anchors():
    from ks265codec_amd import stream as S
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
    from oracle_lib import OraclePipeline
    W, H, N = 416, 240, 13
    clip = make_clip(W, H, N, seed=11, abc=(17, 23, 9), pan=(5, 3))
    o = OraclePipeline(W, H, 30, lambda_q4(30), **ENCODER_TOOLS)
    assert o.skip_rd == 1
    w = S.StreamWriter(W, H, max_dec_pic_buffering=10, max_num_reorder=3, sdh=1, wpp=1, list_mod=1)
    bs, recs, dpb, hist, kinds = w.headers(), {}, {}, [], {}
    order = [(0, None, None)] + [x for a in (4, 8, 12) for x in ((a, None, None), (a - 2, a - 4, a), (a - 3, a - 4, a - 2), (a - 1, a - 2, a))]
    for d, b0, b1 in order:
        later = {r for (dd, x0, x1) in order[order.index((d, b0, b1)) + 1:] for r in (x0, x1) if r is not None}
        if d == 0:
            q, kind, l0, l1 = 30, "I", [], []
        elif b0 is None:                                                # an anchor
            l0, l1 = gpb_lists(hist)
            q, kind = 31, "B" if l1 else "P"
        else:
            q, kind, l0, l1 = 32 + (d & 1), "B", [b0], [b1]
        o.set_qp(q, lambda_q4(q, inter=kind != "I"))
        if b0 is None and l1:
            o.skip_rd = 0                                               # anchors run without the skip pass
            dpb[d] = o.encode_b_mref(clip[d], [dpb[r] for r in l0], [dpb[r] for r in l1])
            o.skip_rd = 1
        else:
            dpb[d] = o.encode(clip[d], kind, dpb.get(l0[0]) if l0 else None, dpb.get(l1[0]) if l1 else None)
        recs[d], kinds[d] = o.store(dpb[d]), (kind, l0, l1)
        if b0 is None:
            hist = [d] + hist
        keep = (set(hist[:3]) | {p for p in dpb if p in later}) - {d}    # what later pictures predict from + the anchors the next anchor searches
        rps = [(p, p in l0 + l1) for p in sorted(keep | set(l0 + l1))]
        isref = b0 is None or d in later
        st = {"I": S.SLICE_I, "P": S.SLICE_P, "B": S.SLICE_B}[kind]
        bs += w.slice(S.NAL_IDR_W_RADL if d == 0 else S.NAL_TRAIL_R if isref else S.NAL_TRAIL_N, st, d, q, o.cu8, o.lvl, o.sao, rps=rps, l0=l0, l1=l1)
    assert [kinds[a] for a in (4, 8, 12)] == [("P", [0], []), ("B", [4], [0]), ("B", [8, 0], [4])]
    sys.path.insert(0, HERE)
    from slice_headers import pictures
    got = {p["poc"]: (p["slice_type"], p["l0"], p["l1"]) for p in pictures(bs)}
    assert got == kinds                                                  # the stream says what was coded
    tmp = tempfile.mkdtemp(prefix="ks265dec_")
    try:
        shutil.copy(DEC, tmp); os.chmod(os.path.join(tmp, "appdecoder"), 0o755)
        open(os.path.join(tmp, "t.265"), "wb").write(bs)
        r = subprocess.run([os.path.join(tmp, "appdecoder"), "-b", "t.265", "-o", "t.yuv", "-threads", "1"], capture_output=True, text=True, cwd=tmp)
        assert "decoder passed" in r.stdout, r.stdout[-300:]
        dec = np.fromfile(os.path.join(tmp, "t.yuv"), np.uint8).reshape(-1, W * H * 3 // 2)
        assert len(dec) == N
        for d in range(N):
            assert (dec[d] == recs[d]).all(), f"decoded picture {d} {kinds[d]} differs in {int((dec[d] != recs[d]).sum())} samples"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_host_mirror_follows_the_switch(tmp_path, monkeypatch):
    """tools/rd_eval.py --host with KS265_GPB=1 against the host itself (on the stand-in of the device library): the same picture order, slice types, lists, reference picture sets,
    NAL types and QPs in every slice header - and without the switch as well.  (The payloads are the device's business: tests/test_gpu_gpb.py holds the whole streams equal.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rd_eval as R
    from ks265codec_amd.synth import ENCODER_TOOLS, make_clip
    from slice_headers import pictures
    from host_harness import build_host_cli, cli_encode
    W, H, N = 64, 64, 17
    clip = make_clip(W, H, N, seed=3, abc=(17, 23, 9), pan=(1, 1))
    clip.tofile(tmp_path / "in.yuv")
    exe = build_host_cli()
    monkeypatch.setenv("RD_G", "4")
    for g in ("1", "0"):
        monkeypatch.setenv("KS265_GPB", g)
        seq, _ = R.adaptive_seq(clip, W, H, 30, decide=False)
        bs, _, _ = R.encode_ours(clip, W, H, 30, "hier", dict(ENCODER_TOOLS), layer_qp=[0, 1, 2], lam_scale=-1.0, seq=seq)
        host = cli_encode({"exe": exe, "yuv": str(tmp_path / "in.yuv")}, tmp_path / "h.265", ["-bframes", "3", "-ref0", "3", "-iper", "128", "-gpb", g], size=(W, H))
        keys = ("poc", "nal_type", "slice_type", "rps", "l0", "l1", "qp", "list_mod", "sao")
        assert [[p[k] for k in keys] for p in pictures(bs)] == [[p[k] for k in keys] for p in pictures(host)], g
        nh = [i for i in range(len(host) - 3) if host[i:i + 3] == b"\x00\x00\x01"][3]          # the first slice's start code: VPS, SPS and PPS lie in front of it
        assert bs[:nh] == host[:nh], "parameter sets"
