"""GPU: the one inter sequencer (frame_api.hip encode_inter) and the skip pass's barriers.

1. every kind of picture on ONE frame object - key, P over 1 / 2 / 3 pictures, B over 1/1 and 2/1 pictures, a lean B picture (ks265_frame_set_picture_tools), P again - at sizes
   with a ragged last CTU row and column: after every picture the device holds what OraclePipeline, driven the same way, holds (CU records, levels, SAO records, samples), and
   ks265_frame_p_state moved as the kind says (advanced by every P kind, untouched by a B picture); created with skip_rd 2 and with skip_rd 1 (no skip pass on the P kinds).
2. the skip pass alone on a hand-made CU map in which one wave of every work-group has no inter lane: half of every CTU flat intra, the other half 32x32 inter CUs with residual.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#         picture, list 0, list 1, QP offset, lean (set_picture_tools(0, -1, 0))
ORDER = [(0, [], [], 0, False), (4, [0], [], 1, False), (8, [4, 0], [], 1, False), (12, [8, 4, 0], [], 1, False), (10, [8], [12], 2, False), (6, [4, 0], [8], 2, False),
         (16, [12], [], 1, False), (14, [12], [16], 3, True), (20, [16], [], 1, False)]


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


def _tools(skip):
    from ks265codec_amd.synth import ENCODER_TOOLS
    t = dict(ENCODER_TOOLS, skip_rd=skip)
    assert t["pre_search"] and t["propagate"] and t["merge"] and t["intra_inter"]
    return t


def _clip(W, H):
    from ks265codec_amd.synth import make_clip
    return make_clip(W, H, 21, seed=W + H, abc=(17, 23, 9), pan=(2, 1))


def _oracle_picture(o, clip, do, d, l0, l1, dq, lean):
    from ks265codec_amd.synth import lambda_q4
    q = 27 + dq
    o.set_qp(q, lambda_q4(q, inter=bool(l0)))
    o.set_picture_tools(*((0, -1, 0) if lean else (-1, -1, -1)))
    if not l0:
        return o.encode(clip[d], "I")
    if not l1:
        return o.encode_mref(clip[d], [do[r] for r in l0])
    return o.encode_b_mref(clip[d], [do[r] for r in l0], [do[r] for r in l1])


@pytest.mark.parametrize("skip", [2, 1])
@pytest.mark.parametrize("W,H", [(200, 136), (136, 72), (64, 48)])
def test_all_kinds_on_one_frame_object(ks, W, H, skip):
    from ks265codec_amd import stream as S
    from ks265codec_amd.lib import CU8, KsFrame
    from ks265codec_amd.synth import lambda_q4
    from oracle_lib import OraclePipeline
    clip, tools = _clip(W, H), _tools(skip)
    o = OraclePipeline(W, H, 27, lambda_q4(27), sao=1, **tools)
    w = S.StreamWriter(W, H, max_dec_pic_buffering=10, max_num_reorder=3, sdh=1, wpp=1, list_mod=1)
    w.headers()
    sizes = []
    with KsFrame(ks, W, H, 27, lambda_q4(27), sao=1, bframes=3, refs=3, **tools) as f:
        p_state = lambda: int(f.lib.ks265_frame_p_state(f.h))
        src, dg, do = f.new_pic(), {}, {}
        cur, have = p_state() & 1, False
        assert p_state() == cur
        for n, (d, l0, l1, dq, lean) in enumerate(ORDER):
            eo = _oracle_picture(o, clip, do, d, l0, l1, dq, lean)
            q = 27 + dq
            f.set_qp(q, lambda_q4(q, inter=bool(l0)))
            f.set_picture_tools(*((0, -1, 0) if lean else (-1, -1, -1)))
            f.load_i420(ks.dev(clip[d]), src)
            out = f.new_pic()
            if not l0:
                f.encode_picture(src, out, True, out); have = False
            elif not l1:
                if len(l0) == 1:
                    f.encode_picture(src, dg[l0[0]], False, out)
                else:
                    f.encode_picture_mref(src, [dg[r] for r in l0], out)
                cur, have = cur ^ 1, True
            elif len(l0) == 1:
                f.encode_picture_b(src, dg[l0[0]], dg[l1[0]], out)
            else:
                f.encode_picture_b_mref(src, [dg[r] for r in l0], [dg[r] for r in l1], out)
            what = f"{W}x{H} skip_rd {skip} picture {d} on {l0} / {l1}{' (lean)' if lean else ''}"
            assert p_state() == (cur | (2 if have else 0)), f"{what}: ks265_frame_p_state {p_state()}"
            cu = f.ws_read("cu8", f.geom.bytes_cu8).view(CU8)
            assert (cu.view(np.uint8) == o.cu8.view(np.uint8)).all(), f"{what}: {int((cu.view(np.uint8) != o.cu8.view(np.uint8)).sum())} CU record bytes differ"
            lvl = [f.ws_read("levels", m * 2, comp).view(np.int16) for comp, m in ((0, W * H), (1, W * H // 4), (2, W * H // 4))]
            for comp in range(3):
                assert (lvl[comp] == o.lvl[comp]).all(), f"{what}: {int((lvl[comp] != o.lvl[comp]).sum())} levels of component {comp} differ"
            sao = f.ws_read("sao", f.geom.bytes_sao)
            assert (sao == np.ascontiguousarray(o.sao).view(np.uint8).ravel()).all(), f"{what}: SAO records differ"
            got, exp = ks.host(f.store_i420(out), np.uint8), o.store(eo)
            assert (got == exp).all(), f"{what}: {int((got != exp).sum())} samples differ"
            # the bytes the stream writer makes of the device's records
            later = {r for (_, a, b, _, _) in ORDER[n + 1:] for r in a + b}
            rps = [(p, p in l0 + l1) for p in sorted(({p for p in dg if p in later} | set(l0 + l1)) - {d})]
            st = S.SLICE_I if not l0 else S.SLICE_B if l1 else S.SLICE_P
            nal = S.NAL_IDR_W_RADL if d == 0 else S.NAL_TRAIL_R if d in later else S.NAL_TRAIL_N
            sizes.append((d, len(w.slice(nal, st, d, q, cu, lvl, sao.view(o.sao.dtype), rps=rps, l0=l0, l1=l1))))
            dg[d], do[d] = out, eo
    print(f"{W}x{H} skip_rd {skip}: bytes per picture (picture, bytes) {sizes}")


def _half_intra_map(W, H, mirrored, mv_left, mv_right):
    """every CTU: one 64x32 half flat intra, the other half two 32x32 inter CUs (list 0; the left one mv_left, the right one mv_right); where a 32x32 CU does not fit into the
    picture, 8x8 CUs of the same kind.  mirrored: the intra half is the lower one"""
    from oracle_lib import CU8
    cu = np.zeros((H // 8, W // 8), CU8)
    for by in range(H // 8):
        for bx in range(W // 8):
            fits = (bx // 4 * 4 + 4) * 8 <= W and (by // 4 * 4 + 4) * 8 <= H
            intra = ((by % 8) < 4) != mirrored
            c = cu[by, bx]
            c["log2_cu"] = 5 if fits else 3
            if intra:
                c["pred_mode"] = 1
            else:
                c["pred_mode"], c["inter_dir"] = 0, 1
                c["mvx"], c["mvy"] = mv_right if (bx % 8) >= 4 else mv_left
    return cu.ravel()


@functools.lru_cache(maxsize=None)
def _skip_stage_oracle(W, H, mirrored):
    """the oracle's side, once per case: reconstruction of the hand-made map, then kso_skip_pass; returns the oracle object and the map between the two"""
    from ks265codec_amd.synth import lambda_q4, make_clip
    from oracle_lib import HostPic, OPic, OraclePipeline, ptr
    clip = make_clip(W, H, 2, seed=W, abc=(17, 23, 9), pan=(2, 1))
    o = OraclePipeline(W, H, 28, lambda_q4(28, inter=True), **_tools(2))
    cfg, null = C.byref(o.cfg), OPic(None, None, None)
    ref = HostPic(o.geom)
    o.load(ref, clip[0]); o.load(o.src, clip[1])
    o.o.kso_ref_planes(cfg, ref.c(), ptr(o.planes))
    # the clip pans by (2, 1) samples a picture: the left CU follows it, the right one is a quarter sample off (its first candidate is the left CU's motion)
    o.cu8[:] = _half_intra_map(W, H, mirrored, (8, 4), (9, 4))
    o.o.kso_reconstruct(cfg, o.src.c(), ref.c(), ptr(o.planes), null, None, ptr(o.cu8), ptr(o.lvl[0]), ptr(o.lvl[1]), ptr(o.lvl[2]), o.rec.c())
    before = o.cu8.copy()
    o.skip_pass(ref.c(), null)
    return o, clip, before


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("W,H", [(64, 64), (200, 136)])
def test_skip_pass_wave_without_inter_lane(ks, W, H, mirrored):
    from ks265codec_amd.lib import CU8, KsFrame
    from ks265codec_amd.synth import lambda_q4
    o, clip, before = _skip_stage_oracle(W, H, mirrored)
    # the case is met on the oracle's map: a CTU with an all-intra 64x32 half inside the picture beside an inter CU with residual
    m = before.reshape(H // 8, W // 8)
    met = 0
    for cy in range(0, H // 8, 8):
        for cx in range(0, W // 8, 8):
            up, low = m[cy:cy + 4, cx:cx + 8], m[cy + 4:cy + 8, cx:cx + 8]
            a, b = (low, up) if mirrored else (up, low)
            met += a.size > 0 and b.size > 0 and bool((a["pred_mode"] != 0).all()) and bool(((b["pred_mode"] == 0) & (b["cbf"] != 0)).any())
    assert met > 0, "no CTU with an all-intra half beside an inter CU with residual"
    if W > 64:                                                            # (the one CTU of 64x64 keeps every residual; at 200x136 the oracle's pass changes 48 / 33 blocks)
        assert (o.cu8 != before).any(), "the oracle's pass changed no record"
    with KsFrame(ks, W, H, 28, lambda_q4(28, inter=True), **_tools(2)) as f:
        src, ref, rec = f.new_pic(), f.new_pic(), f.new_pic()
        f.load_i420(ks.dev(clip[0]), ref); f.load_i420(ks.dev(clip[1]), src)
        cu8 = ks.dev(_half_intra_map(W, H, mirrored, (8, 4), (9, 4)).view(np.uint8))
        lvl = [ks.zeros(W * H * 2), ks.zeros(W * H // 2), ks.zeros(W * H // 2)]
        f.reconstruct(src, ref, cu8, lvl, rec)
        assert (ks.host(cu8, CU8) == before).all(), "the maps differ before the pass"
        f.skip_pass(src, ref, None, cu8, lvl, rec)
        got = ks.host(cu8, CU8)
        assert (got.view(np.uint8) == o.cu8.view(np.uint8)).all(), f"{int((got != o.cu8).sum())} CU records differ"
        for comp in range(3):
            lv = ks.host(lvl[comp], np.int16)
            assert (lv == o.lvl[comp]).all(), f"{int((lv != o.lvl[comp]).sum())} levels of component {comp} differ"
        px, exp = ks.host(f.store_i420(rec), np.uint8), o.store(o.rec)
        assert (px == exp).all(), f"{int((px != exp).sum())} samples differ"
