"""Shared cases of the decision-stage parity tests (test_decision_stage_cases_cpu.py, test_gpu_decision_stages.py).

A case = one picture size, one tool set, one clip, one coding sequence, coded once by OraclePipeline; every picture keeps what each stage read and wrote (OraclePipeline.snap).
The GPU test uploads a stage's inputs, runs that one device stage and compares with the snapshot; the CPU test checks that the cases reach what the GPU test is for.

Cost edits: copies of the oracle's own records with a few costs changed so that a compare natural costs rarely hit is reached (a tie, a clamp); the expectation is the oracle's
stage function on the edited records.  Vectors are never changed and no intra candidate is added: the node of a candidate that is not wholly inside the picture makes the
oracle write outside its CU map."""
from __future__ import annotations

import ctypes as C
import functools
import itertools

import numpy as np

from ks265codec_amd.gop import hier_order
from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4, make_clip
from oracle_lib import CU8, PU, PU_B, HostPic, I, OFrameCfg, OraclePipeline, lib as olib, ptr

COST_INVALID = 0xFFFFFFFF
COST_MAX = 0xFFFFFFFE
INTRA_BIAS_BITS, SPLIT_BITS_P, SPLIT_BITS_B = 96, 40, 80        # oracle/ks265_pipeline_oracle.c (csrc/frame_me.hip: KS_INTRA_BIAS_BITS, KS_SPLIT_BITS_P / _B)
LEVEL_BASE = (0, 1, 5, 21)

SIZES = [(64, 48), (136, 72), (200, 136)]                       # one CTU with a ragged bottom; ragged last column and row; 4 x 3 CTUs, both ragged
TOOLSETS = {"tools": dict(ENCODER_TOOLS), "part_refine": dict(ENCODER_TOOLS, part=1, bi_refine=2)}
# (picture, kind, list 0, list 1, layer): the first mini-GOP of hier_order(4, 128) - P over one picture, B over 1/1 - and a sequence with P over three pictures and B over 2/1
HIER = [(d, k, [] if r0 is None else [r0], [] if r1 is None else [r1], layer) for d, k, r0, r1, layer in itertools.islice(hier_order(4, 128), 5)]
MREF = [(0, "I", [], [], 0), (1, "P", [0], [], 0), (2, "P", [1, 0], [], 0), (4, "P", [2, 1, 0], [], 0), (3, "B", [2, 1], [4], 1)]
SEQUENCES = {"hier": HIER, "mref": MREF}
CASES = [(W, H, t, c, s) for (W, H) in SIZES for t in TOOLSETS for (c, s) in (("natural", "hier"), ("foreign", "hier"), ("natural", "mref"))]


def case_id(case) -> str:
    W, H, t, c, s = case
    return f"{W}x{H}-{t}-{c}-{s}"


def clip_of(W: int, H: int, name: str) -> np.ndarray:
    if name == "natural":
        return make_clip(W, H, 5, seed=W + H)
    a = make_clip(W, H, 5, seed=3)                               # foreign B: picture 2 is from another clip - nothing in its two reference pictures predicts it
    b = make_clip(W, H, 5, seed=99, abc=(11, 7, 5), pan=(0, 0))
    c = a.copy(); c[2] = b[2]
    return c


def pu_index(l: int, px: int, py: int) -> int:
    return LEVEL_BASE[l] + py * (1 << l) + px


class Picture:
    """one coded picture of a case: d, kind ('I', 'P1' one list-0 picture, 'PN' several, 'B11', 'BN'), l0 / l1 (display indices), qp, lam, snap, cu8 / lvl (final), out (HostPic)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Case:
    def __init__(self, W, H, tools, clip, pictures, oracle):
        self.W, self.H, self.tools, self.clip, self.pictures, self.o = W, H, tools, clip, pictures, oracle
        self.out = {p.d: p.out for p in pictures}

    def cfg(self, pic: Picture) -> OFrameCfg:
        c = OFrameCfg.from_buffer_copy(self.o.cfg)
        c.qp, c.lambda_q4 = pic.qp, pic.lam
        return c

    def ctu_origin(self, ctu: int):
        return ctu % self.o.geom.ctu_cols * 64, ctu // self.o.geom.ctu_cols * 64


@functools.lru_cache(maxsize=None)
def run_case(W: int, H: int, tools_name: str, clip_name: str, seq_name: str) -> Case:
    """the oracle's side of a case, once per process; nothing of it is changed afterwards"""
    tools, clip = TOOLSETS[tools_name], clip_of(W, H, clip_name)
    o = OraclePipeline(W, H, 27, lambda_q4(27), sao=1, **tools)
    done, pics = {}, []
    for d, k, l0, l1, layer in SEQUENCES[seq_name]:
        q = 27 if k == "I" else 28 + layer
        lam = lambda_q4(q, inter=k != "I")
        o.set_qp(q, lam)
        if k == "I":
            out, kind = o.encode(clip[d], "I"), "I"
        elif k == "P":
            out, kind = o.encode_mref(clip[d], [done[r] for r in l0]), "P1" if len(l0) == 1 else "PN"
        else:
            out, kind = o.encode_b_mref(clip[d], [done[r] for r in l0], [done[r] for r in l1]), "B11" if len(l0) == 1 and len(l1) == 1 else "BN"
        done[d] = out
        pics.append(Picture(d=d, kind=kind, l0=l0, l1=l1, qp=q, lam=lam, snap=o.snap, cu8=o.cu8.copy(), lvl=[x.copy() for x in o.lvl], out=out))
    return Case(W, H, tools, clip, pics, o)


def records_of(pic: Picture):
    """the records the picture's CU decision reads: (array, 'pu' | 'pub')"""
    return (pic.snap["pu0"], "pu") if pic.kind == "P1" else (pic.snap["pub_decide"], "pub")


def packed_candidates(icost: np.ndarray, imode: np.ndarray) -> np.ndarray:
    """dev_best of ks265_intra_candidates: cost << 6 | mode, all ones where there is no candidate"""
    return np.where(icost == COST_INVALID, np.uint32(COST_INVALID), (icost << np.uint32(6)) | imode.astype(np.uint32)).astype(np.uint32)


# ------------------------------------------------------------------ the oracle's stage functions on given records
def oracle_cu_decide(case: Case, pic: Picture, rec: np.ndarray, which: str, icost, imode) -> np.ndarray:
    cfg, cu = case.cfg(pic), np.zeros((case.H // 8) * (case.W // 8), CU8)
    fn = olib().kso_cu_decide_ii if which == "pu" else olib().kso_cu_decide_b_ii
    fn(C.byref(cfg), ptr(rec), ptr(icost) if icost is not None else None, ptr(imode) if icost is not None else None, ptr(cu))
    return cu


def oracle_ref_pick(case: Case, pic: Picture, pus: list):
    cfg, out, idx = case.cfg(pic), np.zeros(len(pus[0]), PU), np.zeros(len(pus[0]), np.uint8)
    arr = (C.c_void_p * len(pus))(*[p.ctypes.data for p in pus])
    olib().kso_ref_pick(C.byref(cfg), C.c_int(len(pus)), arr, ptr(out), ptr(idx))
    return out, idx


def oracle_ref_decide(case: Case, pic: Picture, pus: list) -> np.ndarray:
    cfg, pub = case.cfg(pic), np.zeros(len(pus[0]), PU_B)
    arr = (C.c_void_p * len(pus))(*[p.ctypes.data for p in pus])
    olib().kso_ref_decide(C.byref(cfg), C.c_int(len(pus)), arr, ptr(pub))
    return pub


# ------------------------------------------------------------------ the CU tree's values, to find the nodes an edit is for (the expectation is always the oracle's)
def tree_of_ctu(W, H, lam, split_bits, x0c, y0c, cost, icost):
    """decide_node of one CTU without partitions: per node (value, own, split, use_intra, reached by the emit walk, wholly inside the picture)"""
    val, own_, split, ui, reach, whole = ([0] * 85 for _ in range(6))
    pen, bias = (lam * split_bits) >> 4, (lam * INTRA_BIAS_BITS) >> 4

    def node(l, px, py):
        s, idx = 64 >> l, pu_index(l, px, py)
        x0, y0 = x0c + px * s, y0c + py * s
        if x0 >= W or y0 >= H:
            return 0
        whole[idx] = x0 + s <= W and y0 + s <= H
        own = int(cost[idx])
        if icost is not None and l > 0 and int(icost[idx]) != COST_INVALID:
            ic = int(icost[idx]) + bias
            if own == COST_INVALID or ic < own:
                ui[idx], own = 1, min(ic, COST_MAX)
        own_[idx] = own
        if l == 3:
            val[idx] = own
            return own
        total = pen + sum(node(l + 1, px * 2 + (k & 1), py * 2 + (k >> 1)) for k in range(4))
        if own != COST_INVALID and own <= total:
            val[idx] = own
        else:
            split[idx], val[idx] = 1, min(total, COST_MAX)
        return val[idx]

    def walk(l, px, py):
        s, idx = 64 >> l, pu_index(l, px, py)
        if x0c + px * s >= W or y0c + py * s >= H:
            return
        reach[idx] = 1
        if l < 3 and split[idx]:
            for k in range(4):
                walk(l + 1, px * 2 + (k & 1), py * 2 + (k >> 1))

    node(0, 0, 0); walk(0, 0, 0)
    return val, own_, split, ui, reach, whole


def _children(idx: int):
    l = max(i for i in range(4) if LEVEL_BASE[i] <= idx)
    i = idx - LEVEL_BASE[l]
    px, py = i & ((1 << l) - 1), i >> l
    return [pu_index(l + 1, px * 2 + (k & 1), py * 2 + (k >> 1)) for k in range(4)]


def _trees(case: Case, pic: Picture, rec, which, icost):
    bits = SPLIT_BITS_P if which == "pu" else SPLIT_BITS_B
    for ctu in range(case.o.nctu):
        x0, y0 = case.ctu_origin(ctu)
        b = ctu * 85
        yield b, tree_of_ctu(case.W, case.H, pic.lam, bits, x0, y0, rec["cost"][b:b + 85], None if icost is None else icost[b:b + 85])


class Edit:
    """a stage's edited inputs, the oracle's output on them and on the unedited ones, and how many records were changed"""

    def __init__(self, name, stage, inputs, expect, plain, count):
        self.name, self.stage, self.inputs, self.expect, self.plain, self.count = name, stage, inputs, expect, plain, count

    def changes_output(self) -> bool:
        a, b = (self.expect, self.plain)
        return any((np.ascontiguousarray(x).view(np.uint8) != np.ascontiguousarray(y).view(np.uint8)).any() for x, y in zip(a, b))


def decide_edits(case: Case, pic: Picture) -> list:
    """the CU decision without partitions (ks265_cu_decide_ii / _b_ii) on the picture's own records"""
    rec0, which = records_of(pic)
    icost, imode = pic.snap["icost"], pic.snap["imode"]
    stage = "cu_decide_ii" if which == "pu" else "cu_decide_b_ii"
    plain_ii, plain_no = oracle_cu_decide(case, pic, rec0, which, icost, imode), oracle_cu_decide(case, pic, rec0, which, None, None)
    out = []
    bias = (pic.lam * INTRA_BIAS_BITS) >> 4

    # a split node's own cost = the sum of its children + the split term: '<=' keeps the node whole
    rec, n = rec0.copy(), 0
    for b, (val, own, split, ui, reach, whole) in _trees(case, pic, rec0, which, icost):
        for idx in range(21):
            if not (reach[idx] and split[idx] and whole[idx]):
                continue
            total = val[idx]                                   # a split node's value is the sum (below the clamp: checked)
            ic = int(icost[b + idx])
            if total >= COST_MAX or (idx > 0 and ic != COST_INVALID and ic + bias < total):
                continue
            rec["cost"][b + idx] = total; n += 1
    out.append(Edit("own cost = children + split term", stage, (rec, icost, imode), (oracle_cu_decide(case, pic, rec, which, icost, imode),), (plain_ii,), n))

    # an intra CU's candidate made to tie with its inter cost: strict '<', the inter CU stays
    ic2, n = icost.copy(), 0
    for b, (val, own, split, ui, reach, whole) in _trees(case, pic, rec0, which, icost):
        for idx in range(1, 85):
            inter = int(rec0["cost"][b + idx])
            if reach[idx] and ui[idx] and not split[idx] and inter != COST_INVALID and inter >= bias:
                ic2[b + idx] = inter - bias; n += 1
    out.append(Edit("intra cost + bias = inter cost", stage, (rec0, ic2, imode), (oracle_cu_decide(case, pic, rec0, which, ic2, imode),), (plain_ii,), n))

    # a node sum above 0xFFFFFFFE: a split node P, its first child N without a cost of its own over four children of 2^31 each - N's value is the clamp, and P, one below
    # it, stays whole (a sum kept in 32 bits wraps to almost nothing and splits P).  Without candidates: an intra candidate of N would keep N whole
    rec, n = rec0.copy(), 0
    for b, (val, own, split, ui, reach, whole) in _trees(case, pic, rec0, which, None):
        for idx in range(5):
            if reach[idx] and split[idx] and whole[idx]:
                nn = _children(idx)[0]
                rec["cost"][b + idx] = COST_MAX; rec["cost"][b + nn] = COST_INVALID
                for c in _children(nn):
                    rec["cost"][b + c] = 0x80000000
                n += 1
                break
    out.append(Edit("node sum above 0xFFFFFFFE", stage, (rec, None, None), (oracle_cu_decide(case, pic, rec, which, None, None),), (plain_no,), n))
    return out


def _idx_bits(r: int, nref: int) -> int:
    return 0 if nref <= 1 else (r + 1 if r < nref - 1 else nref - 1)


def ref_edits(case: Case, pic: Picture, pus0: list, stage: str) -> list:
    """ks265_ref_pick / ks265_ref_decide on a list's records: ties between two pictures (the nearest wins) and a nearest-picture record without a cost"""
    nref = len(pus0)
    run = (lambda p: oracle_ref_pick(case, pic, p)) if stage == "ref_pick" else (lambda p: (oracle_ref_decide(case, pic, p),))
    plain = run(pus0)
    _, widx = oracle_ref_pick(case, pic, pus0)                 # (both stages choose by the same rule)
    tot = lambda r, i: int(pus0[r]["cost"][i]) + ((pic.lam * _idx_bits(r, nref)) >> 4)
    out = []
    pus, n = [p.copy() for p in pus0], 0
    for i in np.flatnonzero(widx > 0):
        w = int(widx[i])
        near = w - 1 if (n & 1) else 0                         # the tie is with picture 0 or with the picture in front of the winner, in turn
        c = tot(w, i) - ((pic.lam * _idx_bits(near, nref)) >> 4)
        if c >= 0 and all(tot(r, i) > tot(w, i) for r in range(near)):
            pus[near]["cost"][i] = c; n += 1
    out.append(Edit("two pictures of equal total cost", stage, pus, run(pus), plain, n))
    pus, n = [p.copy() for p in pus0], 0
    for i in np.flatnonzero(widx > 0)[::3]:
        pus[0]["cost"][i] = COST_INVALID; n += 1
    out.append(Edit("nearest picture's record without a cost", stage, pus, run(pus), plain, n))
    return out


# ------------------------------------------------------------------ low-resolution pictures (ks265_intra_decide_ex, ks265_lookahead_reduce)
class LowRes:
    pass


@functools.lru_cache(maxsize=None)
def lowres_case(W: int, H: int, clip_name: str) -> LowRes:
    """pictures 1 and 2 of the clip at half size (rounded down to a multiple of 8): kso_intra_decide_ex of picture 2, its integer search in picture 1, kso_lookahead_reduce
    (the foreign-B clip: a scene cut, blocks whose intra cost is the smaller one)"""
    r = LowRes()
    w, h = W // 2 // 8 * 8, H // 2 // 8 * 8
    clip, q = clip_of(W, H, clip_name), 28
    full, low = OraclePipeline(W, H, q, lambda_q4(q)), OraclePipeline(w, h, q, lambda_q4(q))
    gf, gl, ol = full.geom, low.geom, olib()
    of, olo = gf.pad_y * gf.stride_y + gf.pad_y, gl.pad_y * gl.stride_y + gl.pad_y
    r.w, r.h, r.qp, r.lam, r.pics, r.o = w, h, q, lambda_q4(q), [], low
    for d in (1, 2):
        full.load(full.src, clip[d])
        lo = HostPic(gl)
        ol.ks265o_downsample(ptr(lo.y, olo), ptr(full.src.y, of), I(gl.stride_y), I(gf.stride_y), I(w), I(h))
        ol.kso_pad_picture(C.byref(low.cfg), lo.c())
        r.pics.append(lo)
    r.cu8, r.cost, r.pu, r.sums = np.zeros((h // 8) * (w // 8), CU8), np.zeros(low.nctu * 85, np.uint32), np.zeros(low.nctu * 85, PU), np.zeros(4, np.uint64)
    ol.kso_intra_decide_ex(C.byref(low.cfg), r.pics[1].c(), ptr(r.cu8), ptr(r.cost))
    ol.kso_me_integer(C.byref(low.cfg), r.pics[1].c(), r.pics[0].c(), None, ptr(r.pu))
    ol.kso_lookahead_reduce(C.byref(low.cfg), ptr(r.cost), ptr(r.pu), ptr(r.sums))
    return r
