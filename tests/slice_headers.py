"""Reads what a stream of this project's writer (ks265codec_amd/host/ks265_stream.c) SAYS about every picture: NAL type, slice type, POC, reference picture set and the two
reference lists as a decoder constructs them (H.265 8.3.2 - 8.3.4, ref_pic_lists_modification() included).  Only the syntax that writer emits: one SPS / PPS, every slice with its
own short-term RPS, no long-term pictures, no temporal MVP, no weighted prediction."""
from __future__ import annotations


class Bits:
    def __init__(self, rbsp: bytes):
        self.b, self.p = rbsp, 0

    def u(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = v << 1 | (self.b[self.p >> 3] >> (7 - (self.p & 7)) & 1)
            self.p += 1
        return v

    def ue(self) -> int:
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + self.u(z)

    def se(self) -> int:
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)


def nal_units(stream: bytes):
    """(nal_unit_type, rbsp without the two header bytes) of every NAL unit of an Annex-B stream"""
    starts, i = [], 0
    while True:
        i = stream.find(b"\x00\x00\x01", i)
        if i < 0:
            break
        starts.append(i + 3)
        i += 3
    for k, s in enumerate(starts):
        e = len(stream) if k + 1 == len(starts) else starts[k + 1] - 3
        nal = stream[s:e].rstrip(b"\x00") if k + 1 < len(starts) else stream[s:e]
        rbsp, zeros = bytearray(), 0
        for byte in nal[2:]:
            if zeros >= 2 and byte == 3:
                zeros = 0
                continue
            rbsp.append(byte)
            zeros = zeros + 1 if byte == 0 else 0
        yield (nal[0] >> 1) & 63, bytes(rbsp)


def parse_sps(rbsp: bytes) -> dict:
    b = Bits(rbsp)
    b.u(4); assert b.u(3) == 0; b.u(1)
    b.u(88); b.u(8)                                          # profile_tier_level() of one sub-layer
    b.ue(); assert b.ue() == 1
    w, h = b.ue(), b.ue()
    assert b.u(1) == 0
    b.ue(); b.ue()
    poc_bits = b.ue() + 4
    assert b.u(1) == 1
    dpb, reorder = b.ue() + 1, b.ue()
    b.ue()
    for _ in range(6):
        b.ue()
    b.u(2)
    sao = b.u(1)
    assert b.u(1) == 0 and b.ue() == 0 and b.u(1) == 0 and b.u(1) == 0    # no PCM, no RPS in the SPS, no long-term pictures, no temporal MVP
    return {"width": w, "height": h, "poc_bits": poc_bits, "sao": sao, "dpb": dpb, "reorder": reorder}


def parse_pps(rbsp: bytes) -> dict:
    b = Bits(rbsp)
    b.ue(); b.ue()
    assert b.u(2) == 0 and b.u(3) == 0
    b.u(1)
    assert b.u(1) == 0                                       # cabac_init_present_flag
    assert b.ue() == 0 and b.ue() == 0                       # one active picture per list by default
    b.se(); b.u(2)
    if b.u(1):
        b.ue()
    b.se(); b.se()
    assert b.u(5) == 0                                       # no slice chroma offsets, no weighted prediction, no bypass, no tiles
    wpp = b.u(1)
    b.u(1)
    assert b.u(1) == 1 and b.u(1) == 0
    if b.u(1) == 0:
        b.se(); b.se()
    assert b.u(1) == 0
    return {"wpp": wpp, "list_mod": b.u(1)}


def parse_slice(nal_type: int, rbsp: bytes, sps: dict, pps: dict) -> dict:
    b = Bits(rbsp)
    assert b.u(1) == 1
    idr = nal_type in (19, 20)
    if 16 <= nal_type <= 23:
        b.u(1)
    assert b.ue() == 0
    st = b.ue()                                              # 0 B, 1 P, 2 I
    out = {"nal_type": nal_type, "slice_type": "BPI"[st], "poc": 0, "rps": [], "l0": [], "l1": []}
    if not idr:
        out["poc"] = b.u(sps["poc_bits"])                    # (the tests' GOPs are shorter than the POC's range: lsb = POC)
        assert b.u(1) == 0
        nn, npos = b.ue(), b.ue()
        neg, pos, prev = [], [], out["poc"]
        for _ in range(nn):
            prev -= b.ue() + 1
            neg.append((prev, b.u(1)))
        prev = out["poc"]
        for _ in range(npos):
            prev += b.ue() + 1
            pos.append((prev, b.u(1)))
        out["rps"] = sorted(neg + pos)
    if sps["sao"]:
        out["sao"] = (b.u(1), b.u(1))
    if st != 2:
        n = [1, 1]
        if b.u(1):
            n[0] = b.ue() + 1
            if st == 0:
                n[1] = b.ue() + 1
        before, after = [p for p, used in neg if used], [p for p, used in pos if used]
        tot = len(before) + len(after)
        assert tot > 0
        temp = [before + after, after + before]              # RefPicListTemp0 / 1 (8.3.4), repeated cyclically up to the active count
        bits = max(0, (tot - 1).bit_length())
        for x in range(2 if st == 0 else 1):
            t = [temp[x][i % tot] for i in range(max(n[x], tot))]
            if pps["list_mod"] and tot > 1 and b.u(1):
                lst = [t[b.u(bits)] for _ in range(n[x])]
            else:
                lst = t[:n[x]]
            out["l0" if x == 0 else "l1"] = lst
        if st == 0:
            assert b.u(1) == 0                               # mvd_l1_zero_flag
        b.ue()
    out["qp"] = 26 + b.se()
    return out


def pictures(stream: bytes) -> list[dict]:
    """every picture of the stream in coding order; the parameter sets' values of interest come along in every entry (`list_mod`)"""
    sps = pps = None
    out = []
    for t, rbsp in nal_units(stream):
        if t == 33:
            sps = parse_sps(rbsp)
        elif t == 34:
            pps = parse_pps(rbsp)
        elif t < 32:
            s = parse_slice(t, rbsp, sps, pps)
            s["list_mod"] = pps["list_mod"]
            out.append(s)
    return out
