"""The searches of a picture share their launches (KsSearchBatch, csrc/frame_common.h): every stage of the search chain takes up to four searches in one grid, more go in
chunks.  The GPU is held to OraclePipeline at the smallest shapes at which the batch dimension can go wrong:

    64x48     one CTU: a grid of one work-group per search, a sub-pel group with seven idle waves
    200x136   4x3 CTUs, ragged right and bottom; 12 CTUs = two sub-pel groups, the second half empty
    576x64    nine CTUs in one row: a CTU count that is neither a multiple of 8 nor of the search count

each as a B picture (2 searches), a P picture with 3 and with 4 list-0 pictures, a B picture with 2 + 2 and with 4 + 4 pictures (two chunks), with -me 0, 1 and 2 and once
without the pre-search.  Compared per picture: the CU map, the levels of the three planes, the reconstruction and - for the P pictures, whose records the frame object hands
out - the PU records of the nearest picture.  The pictures of one case run on ONE frame object, so the P pictures also seed each other (temporal predictors, record ping-pong).
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (200, 136), (576, 64)]
# (name, pictures in list 0, pictures in list 1; 0 = a P picture)
KINDS = [("B 1+1", 1, 1), ("P 3", 3, 0), ("P 4", 4, 0), ("B 2+2", 2, 2), ("B 4+4", 4, 4)]


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


_CLIPS = {}


def _clip(W, H):
    """nine pictures of a panning clip per shape, made once: [4] is the picture coded, [3] .. [0] its list 0, [5] .. [8] its list 1 (nearest first)"""
    from ks265codec_amd.synth import make_clip
    if (W, H) not in _CLIPS:
        c = make_clip(W, H, 9, seed=31 + W, abc=(17, 23, 9), pan=(3, 2))
        c.setflags(write=False)
        _CLIPS[(W, H)] = c
    return _CLIPS[(W, H)]


def _tools(me, pre_search):
    from ks265codec_amd.synth import ENCODER_TOOLS
    return dict(ENCODER_TOOLS, me_method=me, me_hex_thr=16 if me == 2 else 0, pre_search=pre_search)


class _Pair:
    """one frame object and one oracle on the same pictures"""

    def __init__(self, ks, W, H, tools, qp=28):
        from ks265codec_amd.lib import KsFrame
        from ks265codec_amd.synth import lambda_q4
        from oracle_lib import HostPic, OraclePipeline
        self.ks, self.W, self.H = ks, W, H
        self.o = OraclePipeline(W, H, qp, lambda_q4(qp), **tools)
        self.f = KsFrame(ks, W, H, qp, lambda_q4(qp), bframes=7, refs=4, **tools)
        self.src = self.f.new_pic()
        self.HostPic = HostPic
        self.set_qp(qp, True)

    def set_qp(self, qp, inter):
        from ks265codec_amd.synth import lambda_q4
        lam = lambda_q4(qp, inter=inter)
        self.o.set_qp(qp, lam); self.f.set_qp(qp, lam)

    def picture(self, i420):
        """a picture both sides predict from: the same samples, padded by each side's own loader"""
        g, h = self.f.new_pic(), self.HostPic(self.o.geom)
        self.f.load_i420(self.ks.dev(i420), g)
        self.o.load(h, i420)
        return g, h

    def code(self, i420, kind, l0=(), l1=()):
        """code one picture on both sides (kind 'I', 'P', 'B'; l0 / l1: lists of (device, host) pictures); returns the pair of reconstructed pictures"""
        f, o = self.f, self.o
        f.load_i420(self.ks.dev(i420), self.src)
        out = f.new_pic()
        g0, h0, g1, h1 = [p[0] for p in l0], [p[1] for p in l0], [p[0] for p in l1], [p[1] for p in l1]
        if kind == "I":
            eo = o.encode(i420, "I"); f.encode_picture(self.src, out, True, out)
        elif kind == "P":
            eo = o.encode_mref(i420, h0); f.encode_picture_mref(self.src, g0, out)
        elif len(g0) == 1 and len(g1) == 1:
            eo = o.encode(i420, "B", h0[0], h1[0]); f.encode_picture_b(self.src, g0[0], g1[0], out)
        else:
            eo = o.encode_b_mref(i420, h0, h1); f.encode_picture_b_mref(self.src, g0, g1, out)
        return out, eo

    def check(self, what, out, eo, p_records):
        from ks265codec_amd.lib import CU8, PU
        f, o, W, H = self.f, self.o, self.W, self.H
        if p_records:                                                  # the records of the last coded P picture = its nearest picture's search (the oracle has swapped sides too)
            pu = f.ws_read("pu", f.geom.bytes_pu).view(PU)
            assert (pu == o.prev_pu.view(PU).ravel()).all(), f"{what}: PU records differ"
        cu = f.ws_read("cu8", f.geom.bytes_cu8).view(CU8)
        assert (cu == o.cu8.view(CU8).ravel()).all(), f"{what}: CU map differs"
        for c, n in enumerate((W * H, W * H // 4, W * H // 4)):
            lv = f.ws_read("levels", n * 2, c).view(np.int16)
            assert (lv == o.lvl[c]).all(), f"{what}: levels of plane {c} differ"
        got, exp = self.ks.host(f.store_i420(out), np.uint8), o.store(eo)
        assert (got == exp).all(), f"{what}: {int((got != exp).sum())} reconstructed bytes differ"

    def close(self):
        self.f.close()


@pytest.mark.parametrize("me,pre_search", [(0, 1), (1, 1), (2, 1), (2, 0)])
@pytest.mark.parametrize("W,H", SHAPES)
def test_batched_searches_match_the_oracle(ks, W, H, me, pre_search):
    clip = _clip(W, H)
    p = _Pair(ks, W, H, _tools(me, pre_search))
    try:
        pics = [p.picture(clip[i]) for i in range(9)]
        past, future = [pics[3], pics[2], pics[1], pics[0]], [pics[5], pics[6], pics[7], pics[8]]
        for name, n0, n1 in KINDS:
            out, eo = p.code(clip[4], "B" if n1 else "P", past[:n0], future[:n1])
            p.check(f"{W}x{H} me {me} pre_search {pre_search} {name}", out, eo, p_records=n1 == 0)
    finally:
        p.close()


@pytest.mark.parametrize("W,H", SHAPES)
def test_kinds_of_picture_in_turn_on_one_frame_object(ks, W, H):
    """I, P, B, P with three list-0 pictures, B on one frame object, every picture predicting from the coded ones: the workspace sets (one, two, three, two searches), the P
    pictures' record ping-pong and the CTU work counters survive the change of kind"""
    clip = _clip(W, H)
    p = _Pair(ks, W, H, _tools(2, 1))
    try:
        rec = {}
        # display index, kind, list 0, list 1 (coded pictures by display index, nearest first)
        for d, kind, l0, l1 in [(0, "I", [], []), (2, "P", [0], []), (1, "B", [0], [2]), (6, "P", [2, 0, 1], []), (4, "B", [2], [6])]:
            p.set_qp(27 if kind == "I" else 28, kind != "I")
            out, eo = p.code(clip[d], kind, [rec[r] for r in l0], [rec[r] for r in l1])
            p.check(f"{W}x{H} picture {d} ({kind}, lists {l0} {l1})", out, eo, p_records=kind == "P")
            rec[d] = (out, eo)
    finally:
        p.close()
