"""Adversarial content on the CPU (tests/adversarial_clips.py): what the families promise, the oracle's leaf operators against plain numpy int64 at the extremes
the recorded golden vectors may not reach (the comparison base of tests/test_gpu_adversarial.py), the decoder-verified stream fixtures of the adversarial cases
(tests/golden/stream_adversarial_md5.json, written by tests/golden/gen_stream_adversarial_golden.py), and that the fixtures bite: on the ORACLE's outputs the
content reaches the ranges the kernels' range arguments are about."""
from __future__ import annotations

import ctypes as C
import functools
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from adversarial_clips import FAMILIES, make_adversarial, planes
from oracle_lib import I, L, lib as olib, ptr
from stream_cases import ADV_CASES, ADV_CONTENT, ADV_TOOLSETS, CASES, case_params, make_stream, oracle_encoder

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "stream_adversarial_md5.json")))
DEC = "/root/reference/ubuntu_x64/appdecoder"
SIZES = [(136, 72), (72, 136), (64, 64), (8, 8)]


# ------------------------------------------------------------------ the helper keeps its promises
@pytest.mark.parametrize("W,H", SIZES)
def test_families_are_what_they_promise(W, H):
    n = 4
    for kind in FAMILIES:
        clip = make_adversarial(kind, W, H, n, seed=3)
        assert clip.dtype == np.uint8 and clip.shape == (n, W * H * 3 // 2)
        assert (clip == make_adversarial(kind, W, H, n, seed=3)).all(), f"{kind} is not deterministic"
    d = lambda c: np.abs(c[1:].astype(np.int16) - c[:-1].astype(np.int16))
    flat = make_adversarial("flat_flip", W, H, n)
    for t in range(n):
        y, u, v = planes(flat[t], W, H)
        assert (y == 255 * (t & 1)).all() and (u == 255 * ((t + 1) & 1)).all() and (v == u).all()
    cb1 = make_adversarial("cb1_flip", W, H, n)
    assert (d(cb1) == 255).all(), "cb1_flip: every sample differs by exactly 255 from the co-located sample of the picture before"
    y, u, v = planes(cb1[0], W, H)
    assert (np.abs(np.diff(y.astype(np.int16), axis=0)) == 255).all() and (np.abs(np.diff(y.astype(np.int16), axis=1)) == 255).all()
    assert (u.astype(np.int16) + v == 255).all(), "cb1_flip: U and V in opposite phase"
    cb8 = make_adversarial("cb8_shift", W, H, n)
    for t in range(1, n):
        y0, u0, v0 = planes(cb8[t - 1], W, H)
        y1, u1, v1 = planes(cb8[t], W, H)
        assert (y1[:, 3:] == y0[:, :-3]).all() and (u1[1:] == u0[:-1]).all() and (v1[1:] == v0[:-1]).all()
        assert set(np.unique(cb8[t])) <= {0, 255}
    if W >= 16:
        assert (planes(cb8[0], W, H)[0][:8, :16] == np.repeat([0, 255], 8)).all()
    noise = make_adversarial("noise", W, H, n)
    if W * H >= 4096:
        assert noise.min() == 0 and noise.max() == 255 and abs(float(noise.mean()) - 127.5) < 3 and (d(noise) > 0).mean() > 0.98
    assert (make_adversarial("noise", W, H, n, seed=1) != noise).any()
    bn = make_adversarial("bnoise_pan", W, H, n)
    assert set(np.unique(bn)) <= {0, 255}
    for t in range(1, n):
        y0, u0, v0 = planes(bn[t - 1], W, H)
        y1, u1, v1 = planes(bn[t], W, H)
        assert (y1[:-1, :-2] == y0[1:, 2:]).all() and (u1[:, :-1] == u0[:, 1:]).all() and (v1[:, :-1] == v0[:, 1:]).all(), "bnoise_pan: one field panned by (2, 1)"
    if W * H >= 4096:
        assert abs(float((bn[0] == 255).mean()) - 0.5) < 0.03
    er = make_adversarial("edge_ramp", W, H, n)
    for t in range(n):
        y, u, v = planes(er[t], W, H)
        x0 = W // 2 + t
        assert (y[:, :x0] == 0).all() and (y[:, x0] == 128).all() and (y[:, x0 + 1:] == 255).all() and (u == 0).all() and (v == 255).all()
    with pytest.raises(ValueError):
        make_adversarial("plaid", W, H, 1)


# ------------------------------------------------------------------ the oracle's leaf operators against plain numpy int64
def _block_pairs(h, w):
    """pairs of (h, w) uint8 blocks: the four corner cases, then blocks cut from the families (source against the co-located block of the picture before)"""
    yy, xx = np.mgrid[0:h, 0:w]
    cb = (((xx + yy) & 1) * 255).astype(np.uint8)
    z, f = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    out = [("0 vs 255", z, f), ("255 vs 0", f, z), ("equal", cb, cb.copy()), ("checkerboard vs inverse", cb, 255 - cb)]
    for kind in FAMILIES:
        clip = make_adversarial(kind, 136, 72, 2, seed=5)
        a, b = planes(clip[1], 136, 72)[0], planes(clip[0], 136, 72)[0]
        for (y0, x0) in ((0, 0), (72 - h, 136 - w), ((72 - h) // 2 + 1 if h < 72 else 0, 68 - w // 2 + 1)):
            out.append((f"{kind}@{y0},{x0}", np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(b[y0:y0 + h, x0:x0 + w])))
    return out


def _hadamard(n):
    h = np.array([[1]], np.int64)
    while len(h) < n:
        h = np.block([[h, h], [h, -h]])
    return h


def _had_ref(a, b):
    """the oracle's definition: 8x8 tiles (sum |H d Ht| + 2) >> 2; 4x4 tiles (sum + 1) >> 1 where a side is no multiple of 8"""
    h, w = a.shape
    n, rnd, sh = (8, 2, 2) if (h | w) & 7 == 0 else (4, 1, 1)
    H = _hadamard(n)
    d = a.astype(np.int64) - b.astype(np.int64)
    return sum((int(np.abs(H @ d[y:y + n, x:x + n] @ H.T).sum()) + rnd) >> sh for y in range(0, h, n) for x in range(0, w, n))


@pytest.mark.parametrize("h,w", [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 4), (4, 8), (16, 8), (8, 16), (32, 16), (16, 32), (64, 32), (32, 64), (12, 16), (16, 12), (24, 32), (64, 48)])
def test_distortion_operators_at_the_extremes(h, w):
    o = olib()
    for name, a, b in _block_pairs(h, w):
        d = a.astype(np.int64) - b.astype(np.int64)
        assert o.ks265o_sad(ptr(a), ptr(b), L(w), L(w), L(h), L(w)) == int(np.abs(d).sum()), ("sad", name)
        assert o.ks265o_had(ptr(a), ptr(b), L(w), L(w), L(h), L(w)) == _had_ref(a, b), ("had", name)
        if h == w:
            assert o.ks265o_sse(ptr(a), ptr(b), I(w), I(w), I(w)) == int((d * d).sum()), ("sse", name)
            res = np.full((h, w + 3), -7, np.int16)
            o.ks265o_calc_residual(ptr(res), ptr(a), ptr(b), I(w), I(w), I(w + 3), I(w))
            assert (res[:, :w] == d).all() and (res[:, w:] == -7).all(), ("residual", name)
    z, f = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    assert o.ks265o_sad(ptr(z), ptr(f), L(w), L(w), L(h), L(w)) == 255 * h * w
    if (h | w) & 7 == 0:
        assert o.ks265o_had(ptr(z), ptr(f), L(w), L(w), L(h), L(w)) == (h * w // 64) * ((64 * 255 + 2) >> 2)      # a flat difference: the DC coefficient alone, 64 * 255 per tile


@pytest.mark.parametrize("h,w", [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 4), (16, 8), (64, 32), (2, 8), (6, 2)])
def test_bi_average_at_the_extremes(h, w):
    """DefaultWeightedBi on 14-bit intermediates: full-sample predictions (pixel << 6) of the extreme pairs, then the whole range an 8-tap interpolation of 0 / 255
    samples can reach (- 16 * 255 .. 80 * 255 at 64x gain: the negative taps sum to - 16, the positive ones to 80) against numpy int64"""
    o = olib()
    rng = np.random.default_rng(h * 100 + w)
    cases = [(name, a.astype(np.int16) << 6, b.astype(np.int16) << 6) for name, a, b in _block_pairs(h, w)]
    lo, hi = -16 * 255, 80 * 255
    cases += [("range", rng.integers(lo, hi + 1, (h, w)).astype(np.int16), rng.integers(lo, hi + 1, (h, w)).astype(np.int16)),
              ("low", np.full((h, w), lo, np.int16), np.full((h, w), lo, np.int16)), ("high", np.full((h, w), hi, np.int16), np.full((h, w), hi, np.int16)),
              ("low + high", np.full((h, w), lo, np.int16), np.full((h, w), hi, np.int16))]
    for name, p0, p1 in cases:
        dst = np.full((h, w + 5), 0xA5, np.uint8)
        o.ks265o_default_weighted_bi(ptr(dst), ptr(p0), ptr(p1), I(w + 5), I(w), I(w), I(h))
        exp = np.clip((p0.astype(np.int64) + p1.astype(np.int64) + 64) >> 7, 0, 255)
        assert (dst[:, :w] == exp).all() and (dst[:, w:] == 0xA5).all(), name
    a = np.full((h, w), 255, np.int16) << 6
    dst, zero = np.zeros((h, w), np.uint8), np.zeros_like(a)
    o.ks265o_default_weighted_bi(ptr(dst), ptr(a), ptr(zero), I(w), I(w), I(w), I(h))
    assert (dst == 128).all()                                             # (255 * 64 + 64) >> 7


@pytest.mark.parametrize("W,H", [(136, 72), (72, 136), (64, 64), (8, 8), (18, 6)])
def test_downsample_at_the_extremes(W, H):
    o = olib()
    o.ks265o_downsample.restype = None
    w, h = W // 2, H // 2
    for kind in FAMILIES:
        for fr in make_adversarial(kind, W, H, 2, seed=9):
            y = np.ascontiguousarray(planes(fr, W, H)[0])
            out = np.full((h, w + 3), 0x5A, np.uint8)
            o.ks265o_downsample(ptr(out), ptr(y), I(w + 3), I(W), I(w), I(h))
            s = y.astype(np.int64)
            a, b = (s[0::2, 0::2] + s[1::2, 0::2] + 1) >> 1, (s[0::2, 1::2] + s[1::2, 1::2] + 1) >> 1
            assert (out[:, :w] == (a + b + 1) >> 1).all() and (out[:, w:] == 0x5A).all(), kind
            if kind == "cb1_flip":
                assert (out[:, :w] == 128).all()                            # every 2x2 holds two 0 and two 255: the two rounded halves (128, 128)
            if kind == "flat_flip":
                assert (out[:, :w] == y[0, 0]).all()


@pytest.mark.parametrize("log2", [2, 3, 4, 5])
def test_ac_energy_at_the_extremes(log2):
    """acEnergyPlane: ssd - (sum^2 >> 2 log2) in 32-bit unsigned arithmetic (the wrap of sum^2 for a bright 32x32 block is part of the contract): numpy int64 with
    the wrap written out; flat blocks have energy 0 where sum^2 does not wrap, the 1-pixel checkerboard has the maximum n^2 * 255^2 / 4"""
    o = olib()
    o.ks265o_ac_energy_plane.restype = C.c_uint32
    n = 1 << log2
    M = 1 << 32
    seen = {}
    for name, a, _ in _block_pairs(n, n) + [("grey", np.full((n, n), 128, np.uint8), None), ("one", np.full((n, n), 1, np.uint8), None)]:
        s, q = int(a.astype(np.int64).sum()), int((a.astype(np.int64) ** 2).sum())
        exp = (q - (((s * s) % M) >> (2 * log2))) % M
        got = o.ks265o_ac_energy_plane(ptr(np.ascontiguousarray(a)), I(n), I(log2))
        assert got == exp, (name, got, exp)
        seen[name] = got
    assert seen["0 vs 255"] == 0 and seen["one"] == 0 and seen["grey"] == (0 if log2 <= 4 else n * n * 128 * 128)      # grey 32x32: sum^2 = 2^34 wraps to 0
    if log2 <= 4:
        assert seen["255 vs 0"] == 0                                        # 255 * n^2 squared stays below 2^32 up to 16x16
    assert seen["equal"] == n * n * 255 * 255 // 4 if log2 <= 4 else True   # the checkerboard: half the samples 255, variance 255^2 / 4 (32x32: sum^2 wraps)


# ------------------------------------------------------------------ the stream fixtures
def test_adversarial_cases_cover_families_qps_and_tool_sets():
    assert 24 <= len(ADV_CASES) <= 30 and set(GOLD) == set(ADV_CASES)
    fam = [ADV_CONTENT[n][0] for n in ADV_CASES]
    ts = [ADV_CONTENT[n][1] for n in ADV_CASES]
    qp = [ADV_CASES[n][2] for n in ADV_CASES]
    assert all(fam.count(f) >= 2 for f in FAMILIES) and all(qp.count(q) >= 2 for q in (0, 22, 51)) and set(qp) == {0, 22, 51}
    assert all(ts.count(b) >= 2 for b, _, _ in ADV_TOOLSETS.values())
    for n, c in ADV_CASES.items():
        base = ADV_CONTENT[n][1]
        assert c[3:] == CASES[base][3:] and (c[0], c[1]) in ((136, 72), (72, 136), (64, 64)) and case_params(n) == c and n not in CASES


@pytest.mark.parametrize("name", list(ADV_CASES))
def test_oracle_pipeline_writes_the_decoder_verified_adversarial_stream(name):
    bs, recs = make_stream(name, oracle_encoder(name))
    assert hashlib.md5(bs).hexdigest() == GOLD[name]["stream_md5"], f"{name}: stream differs from the decoder-verified fixture ({len(bs)} vs {GOLD[name]['stream_bytes']} bytes)"
    assert [hashlib.md5(recs[d].tobytes()).hexdigest() for d in sorted(recs)] == GOLD[name]["recon_md5"]


@pytest.mark.skipif(not os.path.exists(DEC), reason="reference decoder only exists in the builder container")
@pytest.mark.parametrize("name", ["adv_bnoise_pan_enc_qp0", "adv_cb1_flip_rqt_qp0", "adv_flat_flip_wpp_qp51"])
def test_reference_decoder_reproduces_the_adversarial_reconstruction_live(name):
    W, H = ADV_CASES[name][:2]
    bs, recs = make_stream(name, oracle_encoder(name))
    tmp = tempfile.mkdtemp(prefix="ks265dec_")
    try:
        shutil.copy(DEC, tmp); os.chmod(os.path.join(tmp, "appdecoder"), 0o755)
        open(os.path.join(tmp, "t.265"), "wb").write(bs)
        r = subprocess.run([os.path.join(tmp, "appdecoder"), "-b", "t.265", "-o", "t.yuv", "-threads", "1"], capture_output=True, text=True, cwd=tmp)
        assert "decoder passed" in r.stdout, r.stdout[-300:]
        dec = np.fromfile(os.path.join(tmp, "t.yuv"), np.uint8).reshape(-1, W * H * 3 // 2)
        assert len(dec) == len(recs)
        for d in sorted(recs):
            assert (dec[d] == recs[d]).all(), f"decoded picture {d} differs"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ------------------------------------------------------------------ the fixtures must bite (on the oracle's outputs)
@functools.lru_cache(maxsize=None)
def oracle_ipb(kind: str, qp: int, preset: str, W: int = 136, H: int = 72):
    """I0 P2 B1 of the family through the oracle pipeline (hexagon search, late bi refinement, the preset's sub-pel knobs): what tests/test_gpu_adversarial.py compares
    the device with, reduced to the figures the range arguments are about"""
    from ks265codec_amd.synth import lambda_q4, subme_knobs
    from oracle_lib import OraclePipeline
    clip = make_adversarial(kind, W, H, 3, seed=1)
    o = OraclePipeline(W, H, qp, lambda_q4(qp), me_method=1, bi_refine=2, decimate=2, **subme_knobs(preset))
    a = o.encode(clip[0], "I")
    lv = max(int(np.abs(l.astype(np.int32)).max()) for l in o.lvl)
    b = o.encode(clip[2], "P", a)
    lv = max([lv] + [int(np.abs(l.astype(np.int32)).max()) for l in o.lvl])
    pu = o.prev_pu.copy()
    o.encode(clip[1], "B", a, b)
    lv = max([lv] + [int(np.abs(l.astype(np.int32)).max()) for l in o.lvl])
    ok = pu["cost"] != 0xFFFFFFFF
    okb = o.pub["cost"] != 0xFFFFFFFF
    return dict(frac=int((((pu["mvx"] & 3) | (pu["mvy"] & 3)) != 0)[ok].sum()), max_cost=int(pu["cost"][ok].max()), max_level=lv,
                dirs=set(np.unique(o.pub["inter_dir"][okb]).tolist()))


@pytest.mark.parametrize("preset", ["slower", "veryslow"])
@pytest.mark.parametrize("qp", [0, 22, 51])
def test_noise_exercises_the_sub_pel_refinement(preset, qp):
    r = oracle_ipb("noise", qp, preset)
    print(f"noise qp {qp} {preset}: {r['frac']} valid PUs with a fractional vector")
    assert r["frac"] > 50


@pytest.mark.parametrize("kind", ["cb1_flip", "cb8_shift", "bnoise_pan"])
def test_b_pictures_take_every_direction_at_qp51(kind):
    r = oracle_ipb(kind, 51, "veryslow")
    print(f"{kind} qp 51: inter_dir {sorted(r['dirs'])}")
    assert r["dirs"] == {1, 2, 3}


def test_flat_flip_reaches_the_level_range_at_qp0():
    r = oracle_ipb("flat_flip", 0, "veryfast")
    print(f"flat_flip qp 0: max |level| {r['max_level']}")
    assert r["max_level"] >= 8192


@pytest.mark.parametrize("qp", [0, 22])         # not at QP 51: against the coarse reconstruction of the key picture the largest cost measured is 1 009 632, below 2^20
def test_bnoise_pan_reaches_costs_next_to_the_sentinel_range(qp):
    r = oracle_ipb("bnoise_pan", qp, "veryfast")
    print(f"bnoise_pan qp {qp}: largest PU cost {r['max_cost']}")
    assert r["max_cost"] >= 1 << 20


# ------------------------------------------------------------------ the writer's own bound for a picture's NAL unit
def test_nal_bound_covers_an_incompressible_key_picture():
    """bnoise_pan at 416x240, QP 0: the key picture costs 2.5 bytes per luma sample.  ks265_wpp_finish refuses the capacity the encoder host used to give a picture
    (2 x W x H + 65536: the picture failed with an error); with ks265_wpp_nal_bound, the writer's own worst case for the rows it has coded, it writes the same NAL unit"""
    from ks265codec_amd import stream as S
    from ks265codec_amd.synth import ENCODER_TOOLS, lambda_q4
    from oracle_lib import OraclePipeline
    W, H = 416, 240
    fr = make_adversarial("bnoise_pan", W, H, 1, seed=2)[0]
    o = OraclePipeline(W, H, 0, lambda_q4(0), **ENCODER_TOOLS)
    o.encode(fr, "I")
    w = S.StreamWriter(W, H, sdh=1, wpp=1)
    nal = w.slice(S.NAL_IDR_W_RADL, S.SLICE_I, 0, 0, o.cu8, o.lvl, o.sao)
    print(f"bnoise_pan 416x240 qp 0 key picture: {len(nal)} bytes = {len(nal) / (W * H):.2f} x W x H")
    assert len(nal) > 2 * W * H
    # the same picture row by row, as the encoder host writes it
    si = S.SliceIn()
    si.nal_type, si.slice_type, si.poc, si.qp = S.NAL_IDR_W_RADL, S.SLICE_I, 0, 0
    keep = [np.ascontiguousarray(o.cu8)] + [np.ascontiguousarray(a, dtype=np.int16) for a in o.lvl] + [np.ascontiguousarray(o.sao)]
    si.cu8, si.sao = keep[0].ctypes.data, keep[4].ctypes.data
    for i in range(3):
        si.lvl[i] = keep[1 + i].ctypes.data
    l = w.l
    l.ks265_wpp_bytes.restype = l.ks265_wpp_nal_bound.restype = C.c_size_t
    l.ks265_wpp_finish.restype = C.c_long
    job = np.zeros(l.ks265_wpp_bytes(C.byref(w.cfg)), np.uint8)
    mem = job.ctypes.data_as(C.c_void_p)
    assert l.ks265_wpp_begin(C.byref(w.cfg), C.byref(si), mem) == 0
    for row in range(l.ks265_wpp_rows(mem)):
        assert l.ks265_wpp_code_row(mem, C.c_int(row)) == 0
    bound = l.ks265_wpp_nal_bound(mem)
    assert len(nal) <= bound <= len(nal) * 3 // 2 + 4096
    out = np.zeros(bound, np.uint8)
    assert l.ks265_wpp_finish(mem, out.ctypes.data_as(C.c_void_p), C.c_size_t(W * H * 2 + 65536)) < 0
    assert l.ks265_wpp_finish(mem, out.ctypes.data_as(C.c_void_p), C.c_size_t(bound)) == len(nal) and out[:len(nal)].tobytes() == nal
    assert l.ks265_wpp_nal_bound(None) == 0
