"""GPU: the analysis entries of the device library (include/ks265_hip.h ks265_analysis_*, csrc/analysis.hip) against tests/analysis_ref.py, element for element.
Sizes: 8 x 8 (one block, a partial CTU), 72 x 40 (9 x 5 blocks: an odd block count per row, so the last lane of a row owns one block; partial CTUs both ways), 200 x 136
and 416 x 240 (more than one work-group's worth of CTU rows; 25 blocks per row: odd again).  ks265_frame_create accepts all four.
  * pack + export equals the specification in all five fields: synthetic CU maps (every kind, index pair, size, shape, extreme vectors), a random QP map and none, random
    pictures and 0 against 255
  * padded pitches and offset bases: canaries in the padding, in front and behind stay
  * a subset of fields: the others are not touched
  * every refusal of ks265_analysis_validate is decided on the host: nothing is launched
  * a real key, P and B picture: the fields rebuilt from the compact block's CU map equal the export; the planes' sums are ks265_sse_picture's"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first)
torch.cuda.is_available()

import analysis_ref as ar  # noqa: E402

SIZES = [(8, 8), (72, 40), (200, 136), (416, 240)]
CANARY = 0x5A
FIELDS = ("mv", "ref", "cu", "qp", "sse")


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


class Rig:
    """a frame object of one size with two padded pictures; the packed block of a case is made once and shared"""

    def __init__(self, ks, W, H):
        from ks265codec_amd.lib import KsFrame
        from ks265codec_amd.synth import lambda_q4
        self.ks, self.W, self.H = ks, W, H
        self.f = KsFrame(ks, W, H, 30, lambda_q4(30))
        self.src, self.rec = self.f.new_pic(), self.f.new_pic()
        self.cases = {}

    def case(self, seed, with_map, extreme):
        """(expected arrays, packed block) for the generators' inputs"""
        key = (seed, with_map, extreme)
        if key not in self.cases:
            W, H, f, ks = self.W, self.H, self.f, self.ks
            r = ar.make_cu8(W, H, seed)
            s, t = ar.make_pictures(W, H, seed, extreme)
            qm = ar.make_qp_map(W, H, seed) if with_map else None
            f.load_i420(ks.dev(s), self.src); f.load_i420(ks.dev(t), self.rec)
            d_cu8 = ks.dev(r)
            d_qm = torch.from_numpy(qm).to(ks.device) if with_map else None
            blk = torch.full((f.analysis_bytes(),), CANARY, dtype=torch.uint8, device=ks.device)
            f.analysis_pack(self.src, self.rec, 33, ar.DELTAS, qp_map=d_qm, cu8=d_cu8, block=blk)
            ks.sync()
            self.cases[key] = (ar.analysis(r, qm, 33, ar.DELTAS, s, t, W, H), blk)
        return self.cases[key]

    def close(self):
        self.f.close()


@pytest.fixture(scope="module")
def rigs(ks):
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = Rig(ks, W, H)
        return made[(W, H)]

    yield get
    for r in made.values():
        r.close()


def _same(got: dict, exp: dict, what=""):
    for n in exp:
        g = got[n].cpu().numpy() if hasattr(got[n], "cpu") else got[n]
        assert g.dtype == exp[n].dtype and g.shape == exp[n].shape, (what, n, g.dtype, g.shape)
        bad = np.flatnonzero(g.reshape(-1) != exp[n].reshape(-1))
        assert bad.size == 0, (what, n, f"{bad.size} elements differ, first at {bad[:6]}", g.reshape(-1)[bad[:6]], exp[n].reshape(-1)[bad[:6]])


@pytest.mark.parametrize("extreme", [False, True], ids=["random", "0-vs-255"])
@pytest.mark.parametrize("with_map", [True, False], ids=["qp-map", "no-map"])
@pytest.mark.parametrize("W,H", SIZES)
def test_pack_export_equals_the_spec(ks, rigs, W, H, with_map, extreme):
    rig = rigs(W, H)
    exp, blk = rig.case(W + H, with_map, extreme)
    got = ks.analysis_tensors(blk, W, H)
    ks.sync()
    _same(got, exp)
    if extreme:
        assert (exp["sse"][0] == ar.SSE_MAX_LUMA).all() and (exp["sse"][1:] == ar.SSE_MAX_CHROMA).all()
    if not with_map:
        assert (exp["qp"] == 33).all()


def test_packed_block_layout(ks, rigs):
    """the documented layout: segments on multiples of 256, rows of round_up(w8, 4) entries; the pack writes nothing behind the block's last segment"""
    for W, H in SIZES:
        rig = rigs(W, H)
        w8, h8, cc, cr = ar.dims(W, H)
        P, Pq = (w8 + 3) & ~3, (cc + 3) & ~3
        off = rig.f.analysis_layout()
        n = P * h8
        up = lambda v: (v + 255) & ~255
        assert off == [0, up(8 * n), up(8 * n) + up(2 * n), up(8 * n) + up(2 * n) + up(5 * n), up(8 * n) + up(2 * n) + up(5 * n) + up(12 * n),
                       up(8 * n) + up(2 * n) + up(5 * n) + up(12 * n) + up(Pq * cr)] and off[5] == rig.f.analysis_bytes()
        exp, blk = rig.case(W + H, True, False)
        b = blk.cpu().numpy()
        assert (b[off[0]:off[0] + 8 * n].view("<i2").reshape(2, h8, P, 2)[:, :, :w8] == exp["mv"]).all()
        assert (b[off[3]:off[3] + 12 * n].view("<i4").reshape(3, h8, P)[:, :, :w8] == exp["sse"]).all()
        assert (b[off[4]:off[4] + Pq * cr].view(np.int8).reshape(cr, Pq)[:, :cc] == exp["qp"]).all()
        for i, sz in enumerate((8 * n, 2 * n, 5 * n, 12 * n, Pq * cr)):
            assert (b[off[i] + sz:off[i + 1]] == CANARY).all(), (W, H, f"padding behind segment {i}")


def _padded(ks, W, H, lead, extra):
    """per field a flat canary buffer [256 bytes | lead elements | planes of rows at pitch = row + extra elements, extra more elements between planes | 256 bytes] and
    the strided view of the field inside it"""
    w8, h8, cc, cr = ar.dims(W, H)
    geo = {"mv": (torch.int16, 2, h8, 2 * w8), "ref": (torch.int8, 2, h8, w8), "cu": (torch.uint8, 5, h8, w8), "qp": (torch.int8, 1, cr, cc), "sse": (torch.int32, 3, h8, w8)}
    flat, view = {}, {}
    for n, (tdt, planes, rows, inner) in geo.items():
        es = torch.empty(0, dtype=tdt).element_size()
        pitch = inner + extra
        plane = pitch * rows + extra
        start = 256 // es + lead
        fl = torch.full(((start + plane * planes) * es + 256,), CANARY, dtype=torch.uint8, device=ks.device).view(tdt)
        if n == "mv":
            v = torch.as_strided(fl, (planes, rows, w8, 2), (plane, pitch, 2, 1), start)
        elif n == "qp":
            v = torch.as_strided(fl, (rows, inner), (pitch, 1), start)
        else:
            v = torch.as_strided(fl, (planes, rows, inner), (plane, pitch, 1), start)
        flat[n], view[n] = fl, v
    return flat, view


@pytest.mark.parametrize("lead,extra", [(0, 4), (1, 3), (3, 1)], ids=["aligned-base", "base+1-element", "base+3-elements"])
@pytest.mark.parametrize("W,H", SIZES)
def test_padded_pitches_and_offset_bases_write_nothing_else(ks, rigs, W, H, lead, extra):
    rig = rigs(W, H)
    exp, blk = rig.case(W + H, True, False)
    flat, view = _padded(ks, W, H, lead, extra)
    ks.analysis_export(blk, ks.analysis_desc(W, H, **view))
    ks.sync()
    _same(view, exp, (lead, extra))
    for n in FIELDS:                                                     # whatever the views do not cover is still the canary
        mask = torch.ones(flat[n].numel(), dtype=torch.bool, device=ks.device)
        torch.as_strided(mask, view[n].shape, view[n].stride(), view[n].storage_offset()).fill_(False)
        assert int(mask.sum()) >= 512 // flat[n].element_size() + lead
        assert bool((flat[n][mask].view(torch.uint8) == CANARY).all()), (n, "bytes outside the rows were written")


@pytest.mark.parametrize("wanted", [("mv",), ("sse", "qp"), ("ref", "cu")])
def test_a_subset_of_fields_leaves_the_others(ks, rigs, wanted):
    W, H = 200, 136
    rig = rigs(W, H)
    exp, blk = rig.case(W + H, True, False)
    flat, view = _padded(ks, W, H, 0, 0)
    ks.analysis_export(blk, ks.analysis_desc(W, H, **{n: view[n] for n in wanted}))
    ks.sync()
    _same({n: view[n] for n in wanted}, {n: exp[n] for n in wanted})
    for n in FIELDS:
        if n not in wanted:
            assert bool((flat[n].view(torch.uint8) == CANARY).all()), (n, "a field that was not wanted was written")


def test_refusals_launch_nothing(ks, rigs):
    from ks265codec_amd.lib import AnalysisDesc, AnField
    POINTER, NOTSUPPORTED = -3, -4
    W, H = 72, 40                                                        # 9 x 5 blocks, 2 x 1 CTUs
    rig = rigs(W, H)
    _, blk = rig.case(W + H, True, False)
    lib = ks.lib

    def dev_malloc(nbytes):                                              # allocations of their own (a tensor is a piece of a larger block of torch's allocator)
        p = C.c_void_p()
        assert lib.ks265_dev_malloc(ks.h, C.byref(p), C.c_size_t(nbytes)) == 0
        assert lib.ks265_memset_async(ks.h, p, CANARY, C.c_size_t(nbytes)) == 0
        return p

    mv_bytes = 2 * 5 * 9 * 4
    mv, mv_short, ref, sse = dev_malloc(mv_bytes), dev_malloc(mv_bytes - 1), dev_malloc(2 * 5 * 9), dev_malloc(3 * 5 * 9 * 4)
    ks.sync()

    def content(p, nbytes):
        out = np.zeros(nbytes, np.uint8)
        ks.sync()
        assert lib.ks265_memcpy_d2h_async(ks.h, C.c_void_p(out.ctypes.data), p, C.c_size_t(nbytes)) == 0
        ks.sync()
        return out

    def desc(**f):
        d = AnalysisDesc(W, H)
        for k, v in f.items():
            setattr(d, k, AnField(*v))
        return d

    def both(d, code):
        assert ks.analysis_validate(d) == code
        assert lib.ks265_analysis_export(ks.h, C.c_void_p(blk.data_ptr()), C.byref(d)) == code

    good = desc(mv=(mv.value, 36, 180), ref=(ref.value, 9, 45), sse=(sse.value, 36, 180))
    assert ks.analysis_validate(good) == 0
    host = np.zeros(mv_bytes, np.uint8)
    both(desc(mv=(host.ctypes.data, 36, 180)), POINTER)                                    # host memory
    both(desc(mv=(mv_short.value, 36, 180)), POINTER)                                      # one byte short
    both(desc(mv=(mv.value + 2, 36, 180)), POINTER)                                        # begins inside the allocation, ends behind it
    both(desc(ref=(ref.value, 9, 45), mv=(mv_short.value, 36, 180)), POINTER)              # one bad field among good ones
    both(desc(mv=(mv.value, 32, 180)), NOTSUPPORTED)                                       # pitch below the row
    both(desc(ref=(ref.value, 8, 45)), NOTSUPPORTED)
    both(desc(mv=(mv.value, 37, 185)), NOTSUPPORTED)                                       # pitch no multiple of the element
    both(desc(sse=(sse.value, 38, 190)), NOTSUPPORTED)
    both(desc(sse=(sse.value + 2, 36, 180)), NOTSUPPORTED)                                 # address no multiple of the element
    both(desc(mv=(mv.value, 36, 179)), NOTSUPPORTED)                                       # planes that overlap
    both(desc(), NOTSUPPORTED)                                                             # no field wanted
    d = desc(mv=(mv.value, 36, 180)); d.width = 76
    both(d, NOTSUPPORTED)
    assert lib.ks265_analysis_export(ks.h, None, C.byref(good)) == POINTER
    for p, n in ((mv, mv_bytes), (mv_short, mv_bytes - 1), (ref, 90), (sse, 540)):
        assert (content(p, n) == CANARY).all(), "a refusal launched something"
    assert lib.ks265_analysis_export(ks.h, C.c_void_p(blk.data_ptr()), C.byref(good)) == 0     # and the context still works
    exp = rig.case(W + H, True, False)[0]
    assert (content(mv, mv_bytes).view("<i2").reshape(2, 5, 9, 2) == exp["mv"]).all()
    assert (content(sse, 540).view("<i4").reshape(3, 5, 9) == exp["sse"]).all()
    for p in (mv, mv_short, ref, sse):
        assert lib.ks265_dev_free(ks.h, p) == 0


def test_real_pictures(ks):
    """one key, one P and one B picture at 416 x 240 with the encoder host's tools (merge, skip pass, intra CUs in inter pictures): the export equals the specification applied
    to the CU map that ks265_frame_pack_compact ships to the slice writers, and the planes' sums are ks265_sse_picture's three sums"""
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
    W, H = 416, 240
    assert ENCODER_TOOLS["merge"] and ENCODER_TOOLS["skip_rd"] and ENCODER_TOOLS["intra_inter"]
    f = KsFrame(ks, W, H, 27, lambda_q4(27), bframes=1, **ENCODER_TOOLS)
    try:
        clip = make_clip(W, H, 3, seed=11)
        src, r0, r2, r1 = f.new_pic(), f.new_pic(), f.new_pic(), f.new_pic()
        off = f.compact_layout()
        cblk = ks.zeros(off[7])
        seen = set()
        # coding order: picture 0 (key), picture 2 (P from 0), picture 1 (B between them)
        for poc, kind, out, deltas in ((0, "key", r0, ((0, 0, 0, 0), (0, 0, 0, 0))), (2, "P", r2, ((-2, 0, 0, 0), (0, 0, 0, 0))), (1, "B", r1, ((-1, 0, 0, 0), (1, 0, 0, 0)))):
            qp = 27 if kind == "key" else 29
            f.set_qp(qp, lambda_q4(qp, inter=kind != "key"))
            f.load_i420(ks.dev(clip[poc]), src)
            if kind == "B":
                f.encode_picture_b(src, r0, r2, out)
            else:
                f.encode_picture(src, r0, kind == "key", out)
            cblk.zero_()
            f.pack_compact(cblk)
            ablk = f.analysis_pack(src, out, qp, deltas)
            got = ks.analysis_tensors(ablk, W, H)
            sums = f.sse_picture(src, out)
            ks.sync()
            records = cblk[off[0]:off[0] + int(f.geom.bytes_cu8)].cpu().numpy()
            exp = ar.analysis(records, None, qp, deltas, clip[poc], ks.host(f.store_i420(out), np.uint8), W, H)
            _same(got, exp, kind)
            assert got["sse"].sum(dim=(1, 2), dtype=torch.int64).cpu().tolist() == [int(x) for x in sums], kind
            seen |= set(np.unique(exp["cu"][0]).tolist())
            if kind == "key":
                assert not exp["cu"][0].any() and not exp["ref"].any() and (exp["cu"][4] <= 34).all()
            elif kind == "P":
                assert set(np.unique(exp["ref"][0]).tolist()) <= {0, -2} and not exp["ref"][1].any() and (exp["cu"][0] == 1).any()
            else:
                assert set(np.unique(exp["ref"][0]).tolist()) <= {0, -1} and set(np.unique(exp["ref"][1]).tolist()) <= {0, 1}
        assert {0, 1} <= seen and (seen & {2, 3}), f"the three pictures show kinds {sorted(seen)}: a B picture without list 1 tests nothing"
    finally:
        f.close()
