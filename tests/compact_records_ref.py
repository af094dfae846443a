"""The record blocks of include/ks265_hip.h restated in numpy (no GPU, no C): the layouts of ks265_frame_records_layout / ks265_frame_compact_layout, the compact
form of the three level planes (ks265_frame_pack_compact), its expansion as the encoder host does it (expand_levels, host/ks265_enc.c) and the invariants of a
compact block that hold in whatever order the device's work-groups placed their chunks.  tests/test_compact_records_ref.py holds it against the CPU stand-in,
tests/test_gpu_compact_records.py holds the kernels against it.

The compact form: the planes Y, Cb, Cr (int16, W x H and two W/2 x H/2, packed) are cut into lines of 64 bytes, each plane rounded up to whole lines (a partial last
line is padded with zeros); a line is stored iff one of its bytes is non-zero.  Bit L of the bitmap (little-endian 64-bit words) says that line L is stored.  1024 lines
make a chunk; a chunk's stored lines lie back to back in the data area, in line order, from line index table[chunk] on; the chunks themselves lie in any order.  The
header is four uint32: two running counters that are zero between pictures, the number of stored lines, the number of lines."""
from __future__ import annotations

import numpy as np

LINE = 64                      # bytes per line
CHUNK = 1024                   # lines per chunk
CHUNK_WORDS = CHUNK // 64      # bitmap words per chunk (128 bytes)
CU8_BYTES = 12                 # sizeof(ks265_cu8), one per 8x8 luma block
SAO_BYTES = 8                  # sizeof(ks265_sao_param), three per CTU


def _seg_offsets(sizes):
    off, o = [], 0
    for s in sizes:
        off.append(o)
        o += (int(s) + 255) & ~255
    return off + [o]


def geometry_bytes(W: int, H: int):
    """(bytes_cu8, bytes_sao) of ks265_frame_geometry"""
    return (W // 8) * (H // 8) * CU8_BYTES, ((W + 63) // 64) * ((H + 63) // 64) * 3 * SAO_BYTES


def plane_bytes(W: int, H: int):
    return [W * H * 2, W * H // 2, W * H // 2]


def first_lines(W: int, H: int):
    """first line of Y, Cb, Cr and the number of lines"""
    fl = [0]
    for b in plane_bytes(W, H):
        fl.append(fl[-1] + (b + LINE - 1) // LINE)
    return fl


def nlines(W: int, H: int) -> int:
    return first_lines(W, H)[3]


def nchunks(W: int, H: int) -> int:
    return (nlines(W, H) + CHUNK - 1) // CHUNK


def records_sizes(bytes_cu8: int, bytes_sao: int, W: int, H: int):
    return [bytes_cu8, *plane_bytes(W, H), bytes_sao, 64]


def records_layout(bytes_cu8: int, bytes_sao: int, W: int, H: int):
    """off[7]: CU map, levels Y, Cb, Cr, SAO records, 64 caller bytes - each aligned to 256 - and the size of the block"""
    return _seg_offsets(records_sizes(bytes_cu8, bytes_sao, W, H))


def compact_sizes(bytes_cu8: int, bytes_sao: int, W: int, H: int):
    return [bytes_cu8, bytes_sao, 64, 64, nchunks(W, H) * 4, nchunks(W, H) * (CHUNK // 8), nlines(W, H) * LINE]


def compact_layout(bytes_cu8: int, bytes_sao: int, W: int, H: int):
    """off[8]: CU map, SAO records, 64 caller bytes, header, chunk table, line bitmap, data area (sized for every line), capacity of the block"""
    return _seg_offsets(compact_sizes(bytes_cu8, bytes_sao, W, H))


def lines_of(planes) -> np.ndarray:
    """the three planes as [nlines, 64] bytes, every plane's last line padded with zeros"""
    parts = []
    for p in planes:
        b = np.ascontiguousarray(p, dtype="<i2").reshape(-1).view(np.uint8)
        pad = -len(b) % LINE
        parts.append(b if not pad else np.concatenate([b, np.zeros(pad, np.uint8)]))
    return np.concatenate(parts).reshape(-1, LINE)


def _bitmap_of(stored: np.ndarray, nchunk: int) -> np.ndarray:
    bits = np.zeros(nchunk * CHUNK, np.uint8)
    bits[:len(stored)] = stored
    return np.packbits(bits, bitorder="little").view("<u8")


def _bits_of(bitmap: np.ndarray) -> np.ndarray:
    """one byte per bit, in line order (a fresh array)"""
    return np.unpackbits(np.ascontiguousarray(bitmap, dtype="<u8").view(np.uint8), bitorder="little")


def pack(planes, chunk_order=None) -> dict:
    """hdr (4 x uint32), table (uint32 per chunk), bitmap (uint64 words, 16 per chunk), data ([data_lines, 64] bytes) of the planes' compact form, the chunks laid into
    the data area in chunk_order (a permutation of the chunk indices; default ascending).  A chunk without a stored line takes no room; its table entry is where it would
    have begun."""
    lines = lines_of(planes)
    n = len(lines)
    nchunk = (n + CHUNK - 1) // CHUNK
    stored = lines.view("<u8").any(axis=1)
    order = list(range(nchunk)) if chunk_order is None else [int(c) for c in chunk_order]
    assert sorted(order) == list(range(nchunk)), "chunk_order is not a permutation of the chunks"
    table = np.zeros(nchunk, "<u4")
    data, at = [], 0
    for c in order:
        sel = np.flatnonzero(stored[c * CHUNK:(c + 1) * CHUNK]) + c * CHUNK
        table[c] = at
        data.append(lines[sel])
        at += len(sel)
    data = np.concatenate(data) if data else np.zeros((0, LINE), np.uint8)
    return {"hdr": np.array([0, 0, at, n], "<u4"), "table": table, "bitmap": _bitmap_of(stored, nchunk), "data": data.reshape(-1, LINE)}


def assemble(p: dict, off, fill: int = 0) -> np.ndarray:
    """a whole block (off[7] bytes, `fill` where pack() says nothing) around what pack() returned"""
    blk = np.full(off[7], fill, np.uint8)
    for seg, a in ((3, p["hdr"]), (4, p["table"]), (5, p["bitmap"]), (6, p["data"])):
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        blk[off[seg]:off[seg] + len(b)] = b
    return blk


def _parts(block: np.ndarray, off, W: int, H: int):
    nchunk = nchunks(W, H)
    blk = np.ascontiguousarray(block, np.uint8)
    hdr = blk[off[3]:off[3] + 16].view("<u4")
    table = blk[off[4]:off[4] + 4 * nchunk].view("<u4")
    bitmap = blk[off[5]:off[5] + (CHUNK // 8) * nchunk].view("<u8")
    return hdr, table, bitmap, blk[off[6]:]


def _data_index(table: np.ndarray, bits: np.ndarray, n: int) -> np.ndarray:
    """index in the data area of every line (meaningful where the line's bit is set): the chunk's base + the set bits of the chunk below the line - the host counts them
    as the popcounts of the chunk's earlier bitmap words + the word's lower bits"""
    b = bits[:len(table) * CHUNK].astype(np.int64).reshape(-1, CHUNK)
    rank = np.cumsum(b, axis=1) - b
    return (table.astype(np.int64)[:, None] + rank).reshape(-1)[:n]


def expand(block: np.ndarray, off, W: int, H: int):
    """the three int16 planes ([H, W], [H/2, W/2], [H/2, W/2]) a block stands for.  `block` may end behind its last stored line."""
    hdr, table, bitmap, data = _parts(block, off, W, H)
    fl = first_lines(W, H)
    n = fl[3]
    bits = _bits_of(bitmap)
    idx = _data_index(table, bits, n)
    sel = np.flatnonzero(bits[:n])
    assert len(sel) == 0 or (idx[sel].max() + 1) * LINE <= len(data), "a stored line lies behind the end of the data area"
    lines = np.zeros((n, LINE), np.uint8)
    lines[sel] = data[:len(data) // LINE * LINE].reshape(-1, LINE)[idx[sel]]
    out = []
    for p, nb in enumerate(plane_bytes(W, H)):
        flat = lines[fl[p]:fl[p + 1]].reshape(-1)[:nb].view("<i2")
        out.append(flat.reshape((H, W) if p == 0 else (H // 2, W // 2)))
    return out


def stored_line(block: np.ndarray, off, W: int, H: int, L: int):
    """the 64 bytes line L has in the data area, or None if its bit is not set"""
    hdr, table, bitmap, data = _parts(block, off, W, H)
    bits = _bits_of(bitmap)
    if not bits[L]:
        return None
    k = int(_data_index(table, bits, nlines(W, H))[L])
    return data[k * LINE:(k + 1) * LINE]


def check_block(block: np.ndarray, off, W: int, H: int) -> int:
    """what holds for every valid block, wherever its chunks lie; returns data_lines"""
    hdr, table, bitmap, _ = _parts(block, off, W, H)
    n = nlines(W, H)
    assert hdr[0] == 0 and hdr[1] == 0, f"running counters not cleared: {hdr[0]}, {hdr[1]}"
    assert hdr[3] == n, f"hdr[3] = {hdr[3]}, {n} lines"
    bits = _bits_of(bitmap)
    words = (n + 63) // 64                                            # (the packer leaves words that lie wholly behind the last line alone, and nobody reads them)
    assert not bits[n:words * 64].any(), "bitmap bits at or above the number of lines"
    bits[words * 64:] = 0
    count = bits.reshape(-1, CHUNK).sum(axis=1).astype(np.int64)
    assert int(hdr[2]) == int(count.sum()), f"hdr[2] = {hdr[2]}, bitmap holds {int(count.sum())} lines"
    used = np.flatnonzero(count)
    start = table.astype(np.int64)[used]
    o = np.argsort(start, kind="stable")
    start, cnt = start[o], count[used][o]
    at = 0
    for s, c, ch in zip(start, cnt, used[o]):                         # sorted by start: disjoint and without gaps iff every interval begins where the last one ended
        assert s == at, f"chunk {ch} begins at line {s} of the data area, the lines before it end at {at}"
        at += int(c)
    assert at == int(hdr[2])
    return int(hdr[2])


# ---------------------------------------------------------------- the sizes and contents the packer is held against (both test modules)
SIZES = [(8, 8), (88, 248), (144, 152), (200, 136), (416, 240), (1280, 720)]
LEVELS = (1, -1, -32768, 0x0100, 0x00FF)


def zero_planes(W: int, H: int):
    return [np.zeros((H, W), np.int16), np.zeros((H // 2, W // 2), np.int16), np.zeros((H // 2, W // 2), np.int16)]


def line_elems(W: int, H: int, L: int):
    """(plane, index of the line's first element in the flat plane, number of valid elements) of line L"""
    fl = first_lines(W, H)
    p = 2 if L >= fl[2] else 1 if L >= fl[1] else 0
    e0 = (L - fl[p]) * (LINE // 2)
    return p, e0, min(LINE // 2, plane_bytes(W, H)[p] // 2 - e0)


def content_zero(W: int, H: int):
    return zero_planes(W, H)


def content_every_line(W: int, H: int):
    """one level per line: its place cycles through the first, the last and the middle valid element, its value through LEVELS (so that a line is non-zero in one byte of
    the low or of the high half of a 16-bit word only)"""
    pl = zero_planes(W, H)
    for L in range(nlines(W, H)):
        p, e0, nv = line_elems(W, H, L)
        pos = (0, nv - 1, nv // 2)[L % 3]
        pl[p].reshape(-1)[e0 + pos] = LEVELS[L % 5]
    return pl


def content_random(W: int, H: int, seed: int = 1):
    """about one line in 50 holds one to four levels"""
    rng = np.random.default_rng([seed, W, H])
    pl = zero_planes(W, H)
    for L in np.flatnonzero(rng.random(nlines(W, H)) < 0.02):
        p, e0, nv = line_elems(W, H, int(L))
        for _ in range(int(rng.integers(1, 5))):
            pl[p].reshape(-1)[e0 + int(rng.integers(0, nv))] = np.int16(rng.integers(-300, 301) or 7)
    return pl


def single_lines(W: int, H: int):
    """the lines content (d) stores ALONE in a picture, as (line, element of the line that holds the level): line 0, every plane's last line (level in its last valid
    element), every chroma plane's first line, the lines either side of every multiple of 64 (so of 256 and 1024 too) below the number of lines"""
    fl = first_lines(W, H)
    n = fl[3]
    want = {}
    for L in [0] + [fl[1], fl[2]] + [m + d for m in range(64, n, 64) for d in (-1, 0)]:
        if 0 <= L < n:
            want.setdefault(L, 0 if L in (0, fl[1], fl[2]) else 31 if L % 64 == 63 else 0)
    for p in range(3):
        L = fl[p + 1] - 1
        want[L] = line_elems(W, H, L)[2] - 1
    return sorted((L, min(e, line_elems(W, H, L)[2] - 1)) for L, e in want.items())
