"""CPU: properties of the analysis specification (tests/analysis_ref.py) on hand-made records - what the GPU tests then hold the kernels to."""
from __future__ import annotations

import numpy as np
import pytest

import analysis_ref as ar

W, H = 72, 40                                          # 9 x 5 blocks, 2 x 1 CTUs


def _records(**fields):
    w8, h8, _, _ = ar.dims(W, H)
    r = np.zeros(w8 * h8, ar.CU8)
    r["log2_cu"] = 3
    for k, v in fields.items():
        r[k] = v
    return r


def _flat(v=100):
    return np.full(W * H * 3 // 2, v, np.uint8)


def _run(r, qp_map=None, qp=30, deltas=ar.DELTAS, src=None, rec=None):
    return ar.analysis(r, qp_map, qp, deltas, _flat() if src is None else src, _flat() if rec is None else rec, W, H)


def test_shapes_and_dtypes():
    a = _run(_records(inter_dir=1))
    assert {k: (v.dtype, v.shape) for k, v in a.items()} == {
        "mv": (np.dtype(np.int16), (2, 5, 9, 2)), "ref": (np.dtype(np.int8), (2, 5, 9)), "cu": (np.dtype(np.uint8), (5, 5, 9)),
        "qp": (np.dtype(np.int8), (1, 2)), "sse": (np.dtype(np.int32), (3, 5, 9))}


@pytest.mark.parametrize("direction", [1, 2, 3])
def test_unused_list_is_zero(direction):
    a = _run(_records(inter_dir=direction, mvx=5, mvy=-6, mv1x=7, mv1y=-8))
    for L, vec in ((0, (5, -6)), (1, (7, -8))):
        if direction >> L & 1:
            assert (a["mv"][L] == vec).all() and (a["ref"][L] == ar.DELTAS[L][0]).all()
        else:
            assert not a["mv"][L].any() and not a["ref"][L].any()
    assert (a["cu"][0] == direction).all() and (a["cu"][4] == 255).all()


def test_every_index_form():
    for i0 in range(4):
        for i1 in range(4):
            for direction in (1, 2, 3):
                a = _run(_records(inter_dir=direction | i0 << 4 | i1 << 6))
                assert (a["ref"][0] == (ar.DELTAS[0][i0] if direction & 1 else 0)).all()
                assert (a["ref"][1] == (ar.DELTAS[1][i1] if direction & 2 else 0)).all()
                assert (a["cu"][0] == direction).all()


@pytest.mark.parametrize("pred_mode", [1, 2])
def test_intra_blocks(pred_mode):
    a = _run(_records(pred_mode=pred_mode, inter_dir=3 | 1 << 4 | 2 << 6, mvx=26, mvy=9, mv1x=-3, mv1y=4, cbf=5, log2_cu=4 | 3 << 4))
    assert not a["mv"].any() and not a["ref"].any() and not a["cu"][0].any()
    assert (a["cu"][1] == 4).all() and (a["cu"][2] == 3).all() and (a["cu"][3] == 5).all()
    assert (a["cu"][4] == (26 if pred_mode == 2 else 255)).all()


def test_tree_planes():
    r = _records(inter_dir=1)
    r["log2_cu"][:4] = [3, 4 | 1 << 4, 5 | 2 << 4, 6 | 3 << 4]
    a = _run(r)
    assert a["cu"][1].reshape(-1)[:4].tolist() == [3, 4, 5, 6] and a["cu"][2].reshape(-1)[:4].tolist() == [0, 1, 2, 3]


def test_extreme_vectors_survive():
    a = _run(_records(inter_dir=3, mvx=32767, mvy=-32767, mv1x=-32767, mv1y=32767))
    assert (a["mv"][0] == (32767, -32767)).all() and (a["mv"][1] == (-32767, 32767)).all()


def test_qp_constant_without_a_map_and_the_map_with_one():
    assert (_run(_records(inter_dir=1), None, 33)["qp"] == 33).all()
    m = np.array([-128, 127], np.int8)
    assert (_run(_records(inter_dir=1), m, 33)["qp"] == m.reshape(1, 2)).all()


def test_sse_of_identical_pictures_is_zero():
    src, _ = ar.make_pictures(W, H, 3)
    assert not _run(_records(inter_dir=1), src=src, rec=src.copy())["sse"].any()


def test_sse_maxima():
    src, rec = ar.make_pictures(W, H, extreme=True)
    s = _run(_records(inter_dir=1), src=src, rec=rec)["sse"]
    assert (s[0] == ar.SSE_MAX_LUMA).all() and (s[1:] == ar.SSE_MAX_CHROMA).all() and ar.SSE_MAX_LUMA == 4161600 and ar.SSE_MAX_CHROMA == 1040400


@pytest.mark.parametrize("plane,x,y", [(0, 0, 0), (0, 71, 39), (0, 8, 7), (1, 35, 19), (1, 4, 3), (2, 0, 19), (2, 31, 8)])
def test_one_differing_sample_lands_in_one_block_of_one_plane(plane, x, y):
    src = _flat()
    rec = src.copy()
    off = (0, W * H, W * H * 5 // 4)[plane]
    pw = W if plane == 0 else W // 2
    rec[off + y * pw + x] += 3
    s = _run(_records(inter_dir=1), src=src, rec=rec)["sse"]
    n = 8 if plane == 0 else 4
    assert s[plane, y // n, x // n] == 9 and s.sum() == 9


def test_generators_cover_the_cases():
    r = ar.make_cu8(416, 240, 1)
    inter = r[r["pred_mode"] == 0]
    assert set(r["pred_mode"]) == {0, 1, 2} and set(inter["inter_dir"] & 3) == {1, 2, 3}
    for direction in (1, 2, 3):
        assert len(set(inter["inter_dir"][(inter["inter_dir"] & 3) == direction] >> 4)) == 16
    assert set(r["log2_cu"] & 15) == {3, 4, 5, 6} and set(r["log2_cu"] >> 4) == {0, 1, 2, 3} and set(r["cbf"]) == set(range(8))
    for f in ("mvx", "mvy", "mv1x", "mv1y"):
        assert inter[f].max() == 32767 and inter[f].min() == -32767
    assert set(r["mvx"][r["pred_mode"] == 2]) == set(range(35))
    small = ar.make_cu8(72, 40, 0)                       # 45 blocks still see every kind and both lists' indices move
    assert set(small["pred_mode"]) == {0, 1, 2} and len(set(small["inter_dir"] >> 4)) > 4


def test_moving_window_clip_moves_by_the_stated_step():
    a, b = ar.moving_window_clip(64, 48, 2, dx=6, dy=-2)
    ya, yb = ar.planes(a, 64, 48)[0], ar.planes(b, 64, 48)[0]
    # a block of picture 1 at (x, y) is picture 0's content at (x + 6, y - 2)
    assert (yb[8:40, 8:50] == ya[6:38, 14:56]).all()
