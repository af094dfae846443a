"""An SPS reader that knows the conformance window (tests/slice_headers.py's parse_sps asserts a zero flag): the fields of that reader plus
"window" = (conf_win_left_offset, right, top, bottom) in chroma units, (0, 0, 0, 0) without the flag, and "end" = the bit position behind strong_intra_smoothing."""
from __future__ import annotations

from slice_headers import Bits, nal_units

NAL_SPS = 33


def parse_sps(rbsp: bytes) -> dict:
    b = Bits(rbsp)
    b.u(4); assert b.u(3) == 0; b.u(1)
    b.u(88); b.u(8)                                          # profile_tier_level() of one sub-layer
    b.ue(); assert b.ue() == 1                               # 4:2:0
    w, h = b.ue(), b.ue()
    flag = b.u(1)
    window = (b.ue(), b.ue(), b.ue(), b.ue()) if flag else (0, 0, 0, 0)
    assert b.ue() == 0 and b.ue() == 0                       # 8 bits
    poc_bits = b.ue() + 4
    assert b.u(1) == 1
    dpb, reorder = b.ue() + 1, b.ue()
    b.ue()
    for _ in range(6):
        b.ue()
    b.u(2)
    sao = b.u(1)
    assert b.u(1) == 0 and b.ue() == 0 and b.u(1) == 0 and b.u(1) == 0    # no PCM, no RPS in the SPS, no long-term pictures, no temporal MVP
    b.u(1)                                                   # strong_intra_smoothing_enabled_flag
    assert b.u(1) == 0 and b.u(1) == 0                       # no VUI, no extension
    assert b.u(1) == 1                                       # rbsp_stop_one_bit
    return {"width": w, "height": h, "flag": flag, "window": window, "poc_bits": poc_bits, "sao": sao, "dpb": dpb, "reorder": reorder}


def stream_sps(stream: bytes) -> dict:
    """the first SPS of an Annex-B stream"""
    for t, rbsp in nal_units(stream):
        if t == NAL_SPS:
            return parse_sps(rbsp)
    raise AssertionError("no SPS")


def output_size(sps: dict) -> tuple[int, int]:
    """what a decoder writes (4:2:0: offsets in units of 2 luma samples)"""
    l, r, t, b = sps["window"]
    return sps["width"] - 2 * (l + r), sps["height"] - 2 * (t + b)
