"""Specification of the decoded picture hash SEI message (H.265 D.2.19 / D.3.19, payload type 132) for 8-bit 4:2:0 pictures, written from the standard's text: picture_crc
(hash_type 1) and picture_checksum (hash_type 2) of a plane, and a reader of the messages in a stream of this project's writer.  The judge of the encoder's `hash` switch and of
ks265_picture_hash: no decoder at hand verifies the values, so they are held to this file, applied to what a decoder outputs.

Planes are 2-D uint8 arrays (rows x columns): the coded picture, W x H luma and W/2 x H/2 per chroma plane (sizes are multiples of 8: no conformance window)."""
from __future__ import annotations

import numpy as np

import slice_headers

POLY = 0x1021                                              # x^16 + x^12 + x^5 + 1


def checksum(plane: np.ndarray) -> int:
    """D.3.19: sum += (sample ^ xorMask), xorMask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8), modulo 2^32 (one byte per sample at bit depth 8)"""
    p = np.asarray(plane, np.uint8)
    h, w = p.shape
    x, y = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    mask = ((x & 0xFF) ^ (x >> 8))[None, :] ^ ((y & 0xFF) ^ (y >> 8))[:, None]
    return int((p.astype(np.int64) ^ mask).sum()) & 0xFFFFFFFF


def checksum_scalar(plane: np.ndarray) -> int:
    """the same as the standard's double loop"""
    p = np.asarray(plane, np.uint8)
    s = 0
    for y in range(p.shape[0]):
        for x in range(p.shape[1]):
            s = (s + (int(p[y, x]) ^ (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8))) & 0xFFFFFFFF
    return s


def crc_bitserial(data) -> int:
    """D.3.19 verbatim: crc = 0xFFFF; the bytes in raster order and two zero bytes behind them; per bit, MSB first, crc = (((crc << 1) + bit) & 0xFFFF) ^ (msb * 0x1021).
    (The catalogued CRC-16/SPI-FUJITSU alias AUG-CCITT: check value 0xE5CC for b"123456789".)  data: bytes, or a plane (taken in raster order)"""
    buf = bytes(data) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8).tobytes()
    crc = 0xFFFF
    for byte in buf + b"\x00\x00":
        for k in range(7, -1, -1):
            msb = crc >> 15 & 1
            crc = (((crc << 1) + (byte >> k & 1)) & 0xFFFF) ^ (msb * POLY)
    return crc


def _times_x(v: int, nbits: int) -> int:
    """v x^nbits mod the polynomial: what nbits zero bits do to the register of the loop above.  Square and multiply on shift-and-xor products"""
    def mul(a: int, b: int) -> int:
        r = 0
        while b:
            if b & 1:
                r ^= a
            a <<= 1
            if a & 0x10000:
                a ^= 0x10000 | POLY
            b >>= 1
        return r
    r, q = v, 2                                            # q = x
    while nbits:
        if nbits & 1:
            r = mul(r, q)
        q = mul(q, q)
        nbits >>= 1
    return r


_BYTE_TABLE = None


def crc(plane: np.ndarray) -> int:
    """crc_bitserial of a plane, fast: the loop's register after eight more bits b is ((crc << 8 | b) & 0xFFFF) ^ T[crc >> 8] (T[v] = v x^16 mod the polynomial: the eight
    feedback decisions depend on the top byte alone).  That map is linear over GF(2) in (register, bits), so every row is run from a ZERO register, all rows together byte by
    byte, and the rows are chained afterwards: a register s in front of a row of w bytes becomes row_result ^ s x^(8 w)."""
    global _BYTE_TABLE
    if _BYTE_TABLE is None:
        t = np.zeros(256, np.uint32)
        for v in range(256):
            c = v << 8
            for _ in range(8):
                c = ((c << 1) & 0xFFFF) ^ ((c >> 15 & 1) * POLY)
            t[v] = c
        _BYTE_TABLE = t
    p = np.ascontiguousarray(plane, np.uint8)
    h, w = p.shape
    rows = np.zeros(h, np.uint32)
    cols = p.T.astype(np.uint32)                           # cols[x] = column x, contiguous
    for x in range(w):
        rows = (((rows << 8) | cols[x]) & 0xFFFF) ^ _BYTE_TABLE[rows >> 8]
    s = 0xFFFF
    for r in range(h):
        s = int(rows[r]) ^ _times_x(s, 8 * w)
    return _times_x(s, 16)                                 # the two zero bytes


def picture_hashes(y: np.ndarray, u: np.ndarray, v: np.ndarray, fast: bool = True) -> list[int]:
    """[crc Y, U, V, checksum Y, U, V]: the layout of ks265_picture_hash's output"""
    c = crc if fast else crc_bitserial
    return [c(y), c(u), c(v), checksum(y), checksum(u), checksum(v)]


def i420_planes(buf, w: int, h: int):
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1)
    n = w * h
    return a[:n].reshape(h, w), a[n:n + n // 4].reshape(h // 2, w // 2), a[n + n // 4:n + n // 2].reshape(h // 2, w // 2)


def expected(buf, w: int, h: int, hash_type: int) -> list[int]:
    """the three values a message of hash_type (1 CRC, 2 checksum) must carry for the I420 picture in buf"""
    f = {1: crc, 2: checksum}[hash_type]
    return [f(p) for p in i420_planes(buf, w, h)]


def _split(stream: bytes):
    """(first byte of the start code, first byte of the NAL header, end) of every NAL unit; a start code is 00 00 01 with the zero bytes in front of it"""
    marks, i = [], 0
    while True:
        i = stream.find(b"\x00\x00\x01", i)
        if i < 0:
            break
        marks.append(i)
        i += 3
    out = []
    for k, m in enumerate(marks):
        end = len(stream)
        if k + 1 < len(marks):
            end = marks[k + 1]
            while end > m + 3 and stream[end - 1] == 0:    # the next start code's leading zero bytes (a NAL unit never ends in a zero byte)
                end -= 1
        begin = out[-1][2] if out else 0
        out.append((begin, m + 3, end))
    return out


def _rbsp(nal: bytes) -> bytes:
    out, zeros = bytearray(), 0
    for b in nal:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def parse_hash_sei(rbsp: bytes):
    """(hash_type, [three values]) of an SEI RBSP (behind the NAL header) that holds exactly one decoded picture hash message of a 4:2:0 picture"""
    assert rbsp[0] == 132, f"payload type {rbsp[0]}"
    size, t = rbsp[1], rbsp[2]
    nb = {1: 2, 2: 4}[t]
    assert size == 1 + 3 * nb, f"payload size {size} for hash_type {t}"
    vals = [int.from_bytes(rbsp[3 + k * nb:3 + (k + 1) * nb], "big") for k in range(3)]
    assert rbsp[3 + 3 * nb:] == b"\x80", "rbsp_trailing_bits and nothing behind them"
    return t, vals


def sei_hashes(stream: bytes):
    """Splits an Annex-B stream.  Returns (pictures, stripped): per picture in coding order a dict - `poc` (slice header), `disp` (display index in the stream: closed GOPs, every
    IDR starts one), `hashes` = [(hash_type, [three values]), ...] of the suffix SEI NAL units (type 40, payload 132) DIRECTLY behind the picture's slice NAL unit - and the stream
    with every type-40 NAL unit removed.  A type-40 NAL unit anywhere else is an error."""
    pics, keep, last_was_picture = [], bytearray(), False
    for begin, hdr, end in _split(stream):
        t = stream[hdr] >> 1 & 63
        if t == 40:
            assert stream[hdr] & 0x81 == 0 and stream[hdr + 1] == 1, "layer 0, temporal id 0"
            assert last_was_picture, "a suffix SEI NAL unit that does not follow a picture's slice NAL unit"
            pics[-1]["hashes"].append(parse_hash_sei(_rbsp(stream[hdr + 2:end])))
            continue
        keep += stream[begin:end]
        last_was_picture = t < 32
        if t < 32:
            pics.append({"hashes": []})
    stripped = bytes(keep)
    heads = slice_headers.pictures(stripped)
    assert len(heads) == len(pics)
    base = 0
    for n, (p, s) in enumerate(zip(pics, heads)):
        if s["nal_type"] in (19, 20):
            base = n
        p["poc"], p["disp"], p["slice_type"] = s["poc"], base + s["poc"], s["slice_type"]
    return pics, stripped
