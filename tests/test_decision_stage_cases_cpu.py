"""CPU: the cases of tests/decision_stage_cases.py reach what test_gpu_decision_stages.py is for - on the oracle alone.

These are conditions on the inputs, not measurements: where one does not hold, the case is to be changed, not the condition.
  - picture 2 of the foreign-B clip (content neither of its reference pictures holds) is a B picture with intra CUs at every size (64x48: 21 of 48 blocks); with part=1 it
    also holds CUs in two partitions and bi-predictive CUs
  - the merge pass changes a CU in a P picture and in a B picture of every size
  - kso_ref_pick on the records of a P picture over three pictures chooses every index
  - the intra candidates hold losers: more candidates than intra CUs
  - the half-size pictures' sums count every block; the foreign-B clip's hold blocks whose intra cost is the smaller one
  - every cost edit changes the oracle's output against the unedited records: the compare it aims at was reached"""
from __future__ import annotations

import numpy as np
import pytest

import decision_stage_cases as D


def _case(c):
    return D.run_case(*c)


def _n_intra(cu):
    return int((cu["pred_mode"] == 2).sum())


@pytest.mark.parametrize("tools", list(D.TOOLSETS))
@pytest.mark.parametrize("W,H", D.SIZES)
def test_foreign_b_picture_holds_intra_cus(W, H, tools):
    case = _case((W, H, tools, "foreign", "hier"))
    pic = next(p for p in case.pictures if p.d == 2)
    assert pic.kind == "B11"
    cu = pic.cu8
    nintra, npart, nbi = _n_intra(cu), int(((cu["log2_cu"] >> 4) != 0).sum()), int(((cu["pred_mode"] == 0) & ((cu["inter_dir"] & 3) == 3)).sum())
    print(f"{W}x{H} {tools}: picture 2 holds {nintra} intra, {npart} two-partition, {nbi} bi-predictive 8x8 blocks of {len(cu)}; "
          f"pictures 1 / 3: {[_n_intra(p.cu8) for p in case.pictures if p.d in (1, 3)]} intra")
    assert nintra > 0
    assert _n_intra(pic.snap["cu_decide"]) > 0 and _n_intra(pic.snap["cu_pre_ii"]) > 0
    if case.tools.get("part"):
        assert npart > 0 and nbi > 0


@pytest.mark.parametrize("W,H", D.SIZES)
def test_merge_pass_changes_p_and_b_pictures(W, H):
    changed = {"P": 0, "B": 0}
    for c in D.CASES:
        if c[:2] != (W, H):
            continue
        for pic in _case(c).pictures:
            if pic.kind in ("P1", "B11"):                        # the kinds whose merge pass the device exports (one picture per list)
                before = pic.snap["cu_refine"] if "cu_refine" in pic.snap else pic.snap["cu_decide"]
                changed[pic.kind[0]] += int((before != pic.snap["cu_merge"]).sum())
    print(f"{W}x{H}: blocks the merge pass changed {changed}")
    assert changed["P"] > 0 and changed["B"] > 0


@pytest.mark.parametrize("case", [c for c in D.CASES if c[4] == "mref"], ids=D.case_id)
def test_ref_pick_chooses_every_picture(case):
    cs = _case(case)
    pic = next(p for p in cs.pictures if p.kind == "PN" and len(p.l0) == 3)
    _, idx = D.oracle_ref_pick(cs, pic, pic.snap["decide_in"])
    counts = np.bincount(idx, minlength=3)
    print(f"{D.case_id(case)}: ref_pick index counts {counts.tolist()}")
    assert (counts[:3] > 0).all()
    pub = pic.snap["pub_decide"]
    assert (np.bincount((pub["inter_dir"] >> 4).astype(np.int64), minlength=3)[:3] > 0).all()
    b = next(p for p in cs.pictures if p.kind == "BN")
    assert (np.bincount(b.snap["pick_idx0"], minlength=2)[:2] > 0).all()


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_candidates_hold_losers(case):
    cs = _case(case)
    total = 0
    for pic in cs.pictures:
        if pic.kind == "I":
            continue
        ncand, nint = int((pic.snap["icost"] != D.COST_INVALID).sum()), _n_intra(pic.snap["cu_decide"])
        total += ncand
        assert ncand == 0 or ncand > nint, f"picture {pic.d}: {ncand} candidates, {nint} intra blocks"
    assert total > 0, "no picture of the case has an intra candidate"


@pytest.mark.parametrize("case", [c for c in D.CASES if c[2] == "tools"], ids=D.case_id)
def test_cost_edits_change_the_oracles_output(case):
    cs = _case(case)
    seen = {}
    for pic in cs.pictures:
        if pic.kind == "I":
            continue
        edits = D.decide_edits(cs, pic)
        if pic.kind == "PN":
            edits += D.ref_edits(cs, pic, pic.snap["decide_in"], "ref_decide") + D.ref_edits(cs, pic, pic.snap["decide_in"], "ref_pick")
        if pic.kind == "BN":
            edits += D.ref_edits(cs, pic, pic.snap["pick_in0"], "ref_pick")
        for e in edits:
            if e.count:
                assert e.changes_output(), f"picture {pic.d} ({pic.kind}), {e.stage}, {e.name}: {e.count} records edited, the output is the unedited one"
            seen.setdefault((e.stage, e.name), []).append(e.count)
    print(D.case_id(case), seen)
    for key, counts in seen.items():
        if key == ("cu_decide_b_ii", "intra cost + bias = inter cost") and case[3] != "foreign":
            continue                                             # intra CUs in B pictures are the foreign-B clip's (above); the natural clip's B pictures may hold none
        assert sum(counts) > 0, f"{key}: no record of the case qualifies for the edit"


@pytest.mark.parametrize("clip", ["natural", "foreign"])
@pytest.mark.parametrize("W,H", D.SIZES)
def test_lowres_sums_count_every_block(W, H, clip):
    lr = D.lowres_case(W, H, clip)
    blocks, cheaper = int(lr.sums[3]) & 0xFFFFFFFF, int(lr.sums[3]) >> 32
    print(f"{W}x{H} {clip} at {lr.w}x{lr.h}: sums {lr.sums[:3].tolist()}, {blocks} blocks, {cheaper} intra-cheaper")
    assert blocks == (lr.w // 8) * (lr.h // 8)
    assert (lr.cost != D.COST_INVALID).sum() > blocks, "costs of the larger blocks too"
    if clip == "foreign":
        assert cheaper > 0
