"""GPU: `analysis` through the encoder (include/ks265_enc.h ks265_enc_get_device_analysis, Encoder(analysis=True)), 416x240 and - for partial CTUs - 200x136.
  * the stream with the switch equals the stream without it: IPPP, the default GOP, two lanes, -aq 1;
  * with recon="i420" beside it, every picture's sse is the per-block squared error of (source, fetched reconstruction) computed in numpy, exactly, and the planes' sums over
    the session are quality()'s SSE totals;
  * with roi=True, -rc 0 and no -aq, qp - qp[a CTU with offset 0] is the map of offsets handed in with the picture (roi_block=64, offsets in [-6, 6]);
  * structure: key pictures are intra everywhere with ref == 0; IPPP with ref0=1 has ref[0] == -1 and ref[1] == 0 in every inter block; with -bframes 3 every ref value of a
    picture points at a picture of that picture's lists (list 0: past pictures; list 1, B pictures only: future ones; all coded before it); mv and ref are zero wherever cu[0]
    says the list is unused;
  * the sign convention: a crop window that moves by (+6, -2) samples per picture over a still image (content moves by (-6, +2)) gives, in every P picture, a median list-0
    vector over the inter blocks of exactly (24, -8) quarter samples.  The CPU oracle's CU maps of this clip hold (24, -8) in at least 99.0 % of the inter blocks of every P
    picture at 416x240 (96.9 % at 200x136), so the median is a condition, not a tolerance."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import analysis_ref as ar  # noqa: E402
from test_gpu_device_input import _clip  # noqa: E402

W, H, N = 416, 240, 12
CONFIGS = {
    "ippp": dict(params=dict(bframes=0, ref0=1, iper=32)),
    "default_gop": dict(params=dict(iper=32)),
    "two_lanes": dict(params=dict(iper=32), lanes=2, key_at=6),         # (lanes need a key period of 32 or more: a key request opens the second GOP, on the second lane)
    "aq": dict(params=dict(iper=32, aq=1)),
    "bframes3": dict(params=dict(bframes=3, iper=32)),
}
_cache = {}


def run(w, h, clip, analysis, lanes=1, recon=None, roi_maps=None, key_at=None, **params):
    """one session through Encoder: (stream, [analysis dicts as numpy, coding order], {poc: reconstruction}, quality())"""
    from ks265codec_amd.encoder import Encoder
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda().view(h * 3 // 2, w) for f in clip]
    old = os.environ.get("KS265_GOP_LANES")
    os.environ["KS265_GOP_LANES"] = str(lanes)
    try:
        enc = Encoder(w, h, "slow", rc=0, threads=8, fr=50, analysis=analysis, recon=recon, roi=roi_maps is not None, **{"qp": 30, **params})
    finally:
        os.environ.pop("KS265_GOP_LANES")
        if old is not None:
            os.environ["KS265_GOP_LANES"] = old
    assert enc.lib.ks265_enc_lanes(C.c_void_p(enc.h)) == lanes
    bs, ans, rec = bytearray(), [], {}
    with enc:
        if not analysis:
            with pytest.raises(RuntimeError):
                enc.analysis()
        for t in range(len(dev)):
            if t == key_at:
                enc.lib.QY265EncoderKeyFrameRequest(C.c_void_p(enc.h))
            if roi_maps is not None:
                bs += enc.encode(dev[t], "i420", roi=torch.from_numpy(roi_maps[t]).cuda(), roi_block=64)
            else:
                bs += enc.encode(dev[t], "i420")
            if analysis:
                ans += enc.analysis()
            if recon:
                rec.update(enc.recon())
        bs += enc.flush()
        if analysis:
            ans += enc.analysis()
            assert enc.analysis() == [], "fetched once"
        if recon:
            rec.update(enc.recon())
        q = enc.quality()
    torch.cuda.synchronize()
    ans = [{k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in a.items()} for a in ans]
    return bytes(bs), ans, {p: t_.cpu().numpy().reshape(-1) for p, t_ in rec.items()}, q


def session(name, analysis):
    key = (name, analysis)
    if key not in _cache:
        c = CONFIGS[name]
        _cache[key] = run(W, H, _clip(W, H, N, seed=5), analysis, lanes=c.get("lanes", 1), key_at=c.get("key_at"), **c["params"])
    return _cache[key]


def check_shapes(a, w, h):
    w8, h8, cc, cr = ar.dims(w, h)
    assert {k: (v.dtype, v.shape) for k, v in a.items() if k not in ("poc", "slice_type")} == {
        "mv": (np.dtype(np.int16), (2, h8, w8, 2)), "ref": (np.dtype(np.int8), (2, h8, w8)), "cu": (np.dtype(np.uint8), (5, h8, w8)),
        "qp": (np.dtype(np.int8), (cr, cc)), "sse": (np.dtype(np.int32), (3, h8, w8))}


def check_structure(a):
    """what holds for every picture: lists that a block does not use show neither vector nor reference; a used list has a reference; the tree planes are in range"""
    kind = a["cu"][0]
    assert kind.max() <= 3
    for L in (0, 1):
        unused = (kind & (1 << L)) == 0
        assert not a["mv"][L][unused].any() and not a["ref"][L][unused].any(), (a["poc"], L, "a list that is not used shows motion")
        assert (a["ref"][L][~unused] != 0).all(), (a["poc"], L, "a used list without a reference")
    assert ((a["cu"][1] >= 3) & (a["cu"][1] <= 6)).all() and (a["cu"][2] <= 3).all() and (a["cu"][3] <= 7).all()
    intra = kind == 0
    assert ((a["cu"][4] == 255) | intra).all() and (a["cu"][4][intra] <= 34).all()
    if a["slice_type"] == 2:
        assert intra.all() and not a["ref"].any() and not a["mv"].any(), (a["poc"], "a key picture")


@pytest.mark.parametrize("name", ["ippp", "default_gop", "two_lanes", "aq"])
def test_stream_is_the_one_without_the_switch(name):
    off, none, _, _ = session(name, False)
    on, ans, _, _ = session(name, True)
    assert on == off and len(on) > 1000 and none == []
    assert sorted(a["poc"] for a in ans) == list(range(N)), "every picture's analysis, once"
    for a in ans:
        check_shapes(a, W, H)
        check_structure(a)
    if name == "default_gop":
        assert [a["poc"] for a in ans] != list(range(N)) and {a["slice_type"] for a in ans} == {0, 1, 2}
    if name == "aq":
        assert any(a["qp"].max() != a["qp"].min() for a in ans), "-aq 1 reached the analysis"
    else:
        assert all(a["qp"].max() == a["qp"].min() for a in ans)


def test_structure_ippp_and_bframes3():
    _, ans, _, _ = session("ippp", True)
    assert [a["slice_type"] for a in ans] == [2] + [1] * (N - 1)
    for a in ans[1:]:
        inter = a["cu"][0] != 0
        assert inter.any() and (a["cu"][0][inter] == 1).all()
        assert (a["ref"][0][inter] == -1).all() and not a["ref"][1].any()
    _, ans, _, _ = session("bframes3", True)
    assert {a["slice_type"] for a in ans} == {0, 1, 2}
    coded = set()                                                        # display indices in coding order: a picture's lists hold pictures coded before it
    for a in ans:
        check_structure(a)
        for L, past in ((0, True), (1, False)):
            for d in np.unique(a["ref"][L]).tolist():
                if d == 0:
                    continue
                assert a["slice_type"] != 2 and (L == 0 or a["slice_type"] == 0), (a["poc"], L, d)
                assert (d < 0) == past and a["poc"] + d in coded, (a["poc"], L, d, "list 0: past pictures, list 1 (B pictures): future ones; all coded before this picture")
        coded.add(a["poc"])
    assert any((a["ref"][1] > 0).any() for a in ans), "no block of any B picture uses list 1: nothing is tested"


def test_sse_is_the_block_error_of_source_and_reconstruction():
    w, h, n = 200, 136, 9                                                # 25 x 17 blocks, partial CTUs both ways
    clip = _clip(w, h, n, seed=5)
    _, ans, rec, q = run(w, h, clip, True, recon="i420", psnr=1, iper=32)
    assert sorted(rec) == list(range(n)) and len(ans) == n
    total = np.zeros(3, np.int64)
    for a in ans:
        check_shapes(a, w, h)
        s, r = ar.planes(clip[a["poc"]], w, h), ar.planes(rec[a["poc"]], w, h)
        exp = np.stack([ar.block_sse(s[0], r[0], 8), ar.block_sse(s[1], r[1], 4), ar.block_sse(s[2], r[2], 4)])
        assert (a["sse"] == exp).all(), (a["poc"], int((a["sse"] != exp).sum()))
        total += a["sse"].sum(axis=(1, 2), dtype=np.int64)
    assert q["frames"] == n and [int(x) for x in q["sse"]] == total.tolist() and total.min() > 0


def test_qp_is_the_picture_qp_plus_the_roi_offsets():
    w, h, n = 200, 136, 9                                                # 4 x 3 CTUs, the last column 8 wide, the last row 8 high
    _, _, cc, cr = ar.dims(w, h)
    rng = np.random.default_rng(77)
    maps = [rng.integers(-6, 7, (cr, cc)).astype(np.int8) for _ in range(n)]
    for m in maps:
        m[1, 1] = 0
    _, ans, _, _ = run(w, h, _clip(w, h, n, seed=5), True, roi_maps=maps, iper=32)
    assert sorted(a["poc"] for a in ans) == list(range(n))
    for a in ans:
        d = a["qp"].astype(int) - int(a["qp"][1, 1])
        assert (d == maps[a["poc"]]).all(), (a["poc"], d.tolist(), maps[a["poc"]].tolist())
        assert 30 <= int(a["qp"][1, 1]) <= 34


@pytest.mark.parametrize("w,h", [(416, 240), (200, 136)])
def test_sign_convention(w, h):
    n = 5
    _, ans, _, _ = run(w, h, ar.moving_window_clip(w, h, n, dx=6, dy=-2), True, qp=27, bframes=0, ref0=1, iper=32)
    assert [a["slice_type"] for a in ans] == [2, 1, 1, 1, 1]
    for a in ans[1:]:
        inter = a["cu"][0] == 1
        mv = a["mv"][0][inter]
        share = float(((mv[:, 0] == 24) & (mv[:, 1] == -8)).mean())
        print(f"{w}x{h} poc {a['poc']}: {int(inter.sum())} of {inter.size} blocks inter, {share:.3f} of them at (24, -8)")
        assert inter.sum() > inter.size // 2
        assert (float(np.median(mv[:, 0])), float(np.median(mv[:, 1]))) == (24.0, -8.0), (a["poc"], share)
        assert (a["ref"][0][inter] == -1).all()
