"""GPU: stage parity for the decision stages of the encoder's tool set (ENCODER_TOOLS, and with part=1, bi_refine=2).

For every case of tests/decision_stage_cases.py and every picture: the oracle's inputs of ONE stage go up (its PU / two-list records, its CU map, its reconstructions as
reference pictures, its levels), that one device stage runs, and its whole output must equal what the oracle's stage wrote (OraclePipeline.snap) bit for bit - all 85 records
per CTU, losers and 0xFFFFFFFF entries included, every block of the map, levels and samples over the picture.  The next stage starts from the oracle's inputs again, so a wrong
stage fails under its own name and nothing else does.  No tolerance anywhere.

  device stage                    pictures that call it                               held to
  ks265_ref_decide                P over 2 and 3 pictures                             snap pub_decide (kso_ref_decide)
  ks265_ref_pick                  B over 2/1 (both lists), the P pictures' records    snap pick_out / pick_idx, kso_ref_pick on the three-picture list
  ks265_intra_candidates          every P and B picture                               snap icost << 6 | imode (all ones = none)
  ks265_cu_decide_ii              P over one picture                                  snap cu_decide
  ks265_cu_decide_b_ii            P over several, B over 1/1, B over 2/1              snap cu_decide
  ks265_cu_decide_part            P over one picture, part=1                          snap cu_decide
  ks265_cu_decide_part_b          B over 1/1, part=1                                  snap cu_decide
  ks265_bi_refine_chosen          B over 1/1, bi_refine=2                             snap pub_refine, cu_refine
  ks265_merge_pass                P over one picture, B over 1/1                      snap cu_merge
  ks265_reconstruct_mref          P over 2 and 3 pictures                             snap cu / lvl / rec "recon"
  ks265_intra_inter_reconstruct   every P and B picture                               snap cu / lvl / rec "post_ii"
  ks265_intra_decide_ex           half-size pictures of both clips                    kso_intra_decide_ex (map and all costs)
  ks265_lookahead_reduce          the same                                            kso_lookahead_reduce
The exported partition decision, refinement and merge pass take one picture per list: for a picture with several pictures in a list (P over several, B over 2/1) they run
inside ks265_encode_picture_[b_]mref only, which test_gpu_inter_sequencer.py compares end to end.

Cost edits (decision_stage_cases.decide_edits / ref_edits) run the CU decision and the per-PU reference choice on the oracle's records with a tie or a clamp built in."""
from __future__ import annotations

import numpy as np
import pytest

import decision_stage_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


class _Check:
    """collects every stage's verdict: all stages of a case run, each from the oracle's inputs"""

    def __init__(self, what):
        self.what, self.errs, self.n = what, [], 0

    def records(self, stage, got, exp):
        self.n += 1
        a, b = np.ascontiguousarray(got).view(np.uint8).ravel(), np.ascontiguousarray(exp).view(np.uint8).ravel()
        if a.size != b.size:
            self.errs.append(f"{stage}: {a.size} bytes against the oracle's {b.size}")
            return
        isz = np.ascontiguousarray(exp).dtype.itemsize
        bad = np.flatnonzero((a != b).reshape(-1, isz).any(axis=1))
        if len(bad):
            i = int(bad[0])
            self.errs.append(f"{stage}: {len(bad)} of {a.size // isz} records differ, first at {i}: gpu={np.ascontiguousarray(got).ravel()[i]} oracle={np.ascontiguousarray(exp).ravel()[i]}")

    def plane(self, stage, got, exp, stride, org, w, h):
        """the picture area of two padded planes (the margin rule of test_gpu_frame._cmp_region for a reconstruction: margin 0 - the padding is made after the loop filters)"""
        self.n += 1
        oy, ox = divmod(org, stride)
        sa, sb = got.reshape(-1, stride)[oy:oy + h, ox:ox + w], exp.reshape(-1, stride)[oy:oy + h, ox:ox + w]
        bad = np.argwhere(sa != sb)
        if len(bad):
            self.errs.append(f"{stage}: {len(bad)} samples differ, first at (y,x)={tuple(bad[0])} gpu={sa[tuple(bad[0])]} oracle={sb[tuple(bad[0])]}")

    def done(self):
        print(f"{self.what}: {self.n} comparisons, {len(self.errs)} failed")
        assert self.n > 0
        assert not self.errs, f"{self.what}: {len(self.errs)} of {self.n} comparisons failed\n" + "\n".join(self.errs)


def _junk(ks, nbytes):
    """an output buffer whose every byte the stage has to write"""
    return ks.zeros(nbytes).fill_(0xA5)


def _up_pic(ks, f, hp):
    p = f.new_pic()
    p.y, p.u, p.v = ks.dev(hp.y), ks.dev(hp.u), ks.dev(hp.v)
    return p


def _up_state(ks, f, snap, tag):
    """(cu8, [levels], recon picture) of a snapshot taken by OraclePipeline._keep_state"""
    rec = f.new_pic()
    rec.y, rec.u, rec.v = (ks.dev(x) for x in snap["rec_" + tag])
    return ks.dev(snap["cu_" + tag]), [ks.dev(x) for x in snap["lvl_" + tag]], rec


def _cmp_state(ks, f, chk, stage, cu8, lvl, rec, snap, tag):
    g, W, H = f.geom, f.width, f.height
    chk.records(f"{stage}: CU map", ks.host(cu8, D.CU8), snap["cu_" + tag])
    for c in range(3):
        chk.records(f"{stage}: levels of component {c}", ks.host(lvl[c], np.int16), snap["lvl_" + tag][c])
    org_y, org_c = g.pad_y * g.stride_y + g.pad_y, g.pad_c * g.stride_c + g.pad_c
    chk.plane(f"{stage}: Y", ks.host(rec.y, np.uint8), snap["rec_" + tag][0], g.stride_y, org_y, W, H)
    chk.plane(f"{stage}: Cb", ks.host(rec.u, np.uint8), snap["rec_" + tag][1], g.stride_c, org_c, W // 2, H // 2)
    chk.plane(f"{stage}: Cr", ks.host(rec.v, np.uint8), snap["rec_" + tag][2], g.stride_c, org_c, W // 2, H // 2)


def _run_decide(ks, f, which, rec, ibest):
    cu = _junk(ks, f.geom.bytes_cu8)
    (f.cu_decide_ii if which == "pu" else f.cu_decide_b_ii)(ks.dev(rec), ks.dev(ibest) if ibest is not None else None, cu)
    return ks.host(cu, D.CU8)


def _run_ref(ks, f, stage, pus):
    n = len(pus[0])
    d = [ks.dev(p) for p in pus]
    if stage == "ref_decide":
        pub = _junk(ks, n * 16)
        f.ref_decide(d, pub)
        return (ks.host(pub, D.PU_B),)
    out, idx = _junk(ks, n * 16), _junk(ks, n)
    f.ref_pick(d, out, idx)
    return ks.host(out, D.PU), ks.host(idx, np.uint8)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_decision_stages_match_oracle(ks, case):
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import lambda_q4
    cs = D.run_case(*case)
    W, H, tools = cs.W, cs.H, cs.tools
    chk = _Check(D.case_id(case))
    keep = []

    def up(a):                                                   # an input of a launch: alive until the picture's comparisons have read the outputs back
        keep.append(ks.dev(a))
        return keep[-1]

    with KsFrame(ks, W, H, 27, lambda_q4(27), sao=1, bframes=3, refs=3, **tools) as f:
        nrec, src = f.nctu * 85, f.new_pic()
        refs = {d: _up_pic(ks, f, hp) for d, hp in cs.out.items()}
        for pic in cs.pictures:
            if pic.kind == "I":
                continue
            s, tag = pic.snap, f"picture {pic.d} ({pic.kind} over {pic.l0} / {pic.l1})"
            f.set_qp(pic.qp, pic.lam)
            f.load_i420(up(cs.clip[pic.d]), src)
            r0, r1 = refs[pic.l0[0]], refs[pic.l1[0]] if pic.l1 else None
            rec, which = D.records_of(pic)
            # ---- the per-PU choice among a list's pictures
            if pic.kind == "PN":
                chk.records(f"{tag} ref_decide", _run_ref(ks, f, "ref_decide", s["decide_in"])[0], s["pub_decide"])
                for name, got, exp in zip(("records", "indices"), _run_ref(ks, f, "ref_pick", s["decide_in"]), D.oracle_ref_pick(cs, pic, s["decide_in"])):
                    chk.records(f"{tag} ref_pick on the list-0 records: {name}", got, exp)
            if pic.kind == "BN":
                for L in range(2):
                    got = _run_ref(ks, f, "ref_pick", s[f"pick_in{L}"])
                    chk.records(f"{tag} ref_pick list {L}: records", got[0], s[f"pick_out{L}"])
                    chk.records(f"{tag} ref_pick list {L}: indices", got[1], s[f"pick_idx{L}"])
            # ---- intra candidates, gated by the picture's records
            exp_best = D.packed_candidates(s["icost"], s["imode"])
            best = _junk(ks, nrec * 4)
            f.intra_candidates(src, up(rec), best)
            chk.records(f"{tag} intra_candidates", ks.host(best, np.uint32), exp_best)
            # ---- the CU decision
            part, one = bool(tools.get("part")) and pic.kind != "PN", pic.kind in ("P1", "B11")
            cu, ib = _junk(ks, f.geom.bytes_cu8), up(exp_best)
            if not part:
                (f.cu_decide_ii if which == "pu" else f.cu_decide_b_ii)(up(rec), ib, cu)
                chk.records(f"{tag} cu_decide{'' if which == 'pu' else '_b'}_ii", ks.host(cu, D.CU8), s["cu_decide"])
            elif pic.kind == "P1":
                f.cu_decide_part(src, r0, up(rec), ib, cu)
                chk.records(f"{tag} cu_decide_part", ks.host(cu, D.CU8), s["cu_decide"])
            elif pic.kind == "B11":
                f.cu_decide_part_b(src, r0, r1, up(s["pu0"]), up(s["pu1"]), up(rec), ib, cu)
                chk.records(f"{tag} cu_decide_part_b", ks.host(cu, D.CU8), s["cu_decide"])
            # ---- the joint refinement of the chosen CUs, the merge pass (one picture per list)
            cu_in, pub_in = s["cu_decide"], rec
            if pic.kind == "B11" and tools.get("bi_refine") == 2:
                pub, cu = up(s["pub_decide"]), up(s["cu_decide"])
                f.bi_refine_chosen(src, r0, r1, up(s["pu0"]), up(s["pu1"]), pub, cu)
                chk.records(f"{tag} bi_refine_chosen: records", ks.host(pub, D.PU_B), s["pub_refine"])
                chk.records(f"{tag} bi_refine_chosen: CU map", ks.host(cu, D.CU8), s["cu_refine"])
                cu_in, pub_in = s["cu_refine"], s["pub_refine"]
            if one:
                cu = _junk(ks, f.geom.bytes_cu8)
                f.merge_pass(src, r0, r1, up(rec) if which == "pu" else None, up(pub_in) if which == "pub" else None, up(cu_in), cu)
                chk.records(f"{tag} merge_pass", ks.host(cu, D.CU8), s["cu_merge"])
            # ---- the reconstruction from several list-0 pictures, the intra CUs' pass
            if pic.kind == "PN":
                cu, lvl, rp = _up_state(ks, f, s, "recon_in")
                f.reconstruct_mref(src, [refs[r] for r in pic.l0], cu, lvl, rp)
                _cmp_state(ks, f, chk, f"{tag} reconstruct_mref", cu, lvl, rp, s, "recon")
            cu, lvl, rp = _up_state(ks, f, s, "pre_ii")
            f.intra_inter_reconstruct(src, cu, lvl, rp)
            _cmp_state(ks, f, chk, f"{tag} intra_inter_reconstruct", cu, lvl, rp, s, "post_ii")
            del keep[:]
            # ---- cost edits on the picture's own records
            if case[2] != "tools":
                continue
            edits = D.decide_edits(cs, pic)
            if pic.kind == "PN":
                edits += D.ref_edits(cs, pic, s["decide_in"], "ref_decide") + D.ref_edits(cs, pic, s["decide_in"], "ref_pick")
            if pic.kind == "BN":
                edits += D.ref_edits(cs, pic, s["pick_in0"], "ref_pick")
            for e in edits:
                if not e.count:
                    continue
                if e.stage.startswith("cu_decide"):
                    erec, eic, eim = e.inputs
                    got = (_run_decide(ks, f, which, erec, None if eic is None else D.packed_candidates(eic, eim)),)
                else:
                    got = _run_ref(ks, f, e.stage, e.inputs)
                for k, (g_, x_) in enumerate(zip(got, e.expect)):
                    chk.records(f"{tag} {e.stage}, edit '{e.name}' ({e.count} records), output {k}", g_, x_)
        ks.sync()
    chk.done()


@pytest.mark.parametrize("clip", ["natural", "foreign"])
@pytest.mark.parametrize("W,H", D.SIZES)
def test_lowres_intra_costs_and_reduce_match_oracle(ks, W, H, clip):
    from ks265codec_amd.lib import KsFrame
    lr = D.lowres_case(W, H, clip)
    chk = _Check(f"{W}x{H} {clip} at {lr.w}x{lr.h}")
    with KsFrame(ks, lr.w, lr.h, lr.qp, lr.lam) as f:
        cur = _up_pic(ks, f, lr.pics[1])
        cu, cost = _junk(ks, f.geom.bytes_cu8), _junk(ks, f.nctu * 85 * 4)
        f.intra_decide_ex(cur, cu, cost)
        chk.records("intra_decide_ex: CU map", ks.host(cu, D.CU8), lr.cu8)
        chk.records("intra_decide_ex: costs", ks.host(cost, np.uint32), lr.cost)
        got = f.lookahead_reduce(ks.dev(lr.cost), ks.dev(lr.pu))
        chk.records("lookahead_reduce", got, lr.sums)
    chk.done()
