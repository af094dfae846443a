"""CPU: the numpy restatement of the compact record block (tests/compact_records_ref.py) against itself - what pack() stores, expand() gives back, wherever the
chunks lie - and against the device library's CPU stand-in (tests/hip_stub.c: ks265_frame_compact_layout, ks265_frame_pack_compact), at the sizes and contents
tests/test_gpu_compact_records.py holds the kernels to."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import compact_records_ref as R
from host_harness import build_host_lib, load_host_lib


def chunk_orders(nchunk: int):
    rng = np.random.default_rng(nchunk)
    return {"ascending": None, "reversed": list(range(nchunk))[::-1], "seed1": list(rng.permutation(nchunk)), "seed2": list(rng.permutation(nchunk))}


def contents(W: int, H: int):
    """(name, planes) of contents (a) .. (d); (d) is one picture per line of single_lines()"""
    yield "zero", R.content_zero(W, H)
    yield "every_line", R.content_every_line(W, H)
    yield "random", R.content_random(W, H)
    pl = R.zero_planes(W, H)
    for L, e in R.single_lines(W, H):                           # (one set of planes, the level moved from line to line)
        p, e0, _ = R.line_elems(W, H, L)
        pl[p].reshape(-1)[e0 + e] = -3
        yield f"line{L}", pl
        pl[p].reshape(-1)[e0 + e] = 0


def test_lines_and_chunks_of_the_listed_sizes():
    """the table of the sizes: what each one is there for"""
    assert [R.nlines(W, H) for W, H in R.SIZES] == [4, 1024, 1026, 1276, 4680, 43200]
    assert [R.nchunks(W, H) for W, H in R.SIZES] == [1, 1, 2, 2, 5, 43]
    assert R.first_lines(88, 248) == [0, 682, 853, 1024] and R.first_lines(8, 8) == [0, 2, 3, 4]
    assert R.line_elems(8, 8, 2) == (1, 0, 16) and R.line_elems(88, 248, 852) == (1, 170 * 32, 16)          # partial chroma lines: 16 valid elements
    assert R.first_lines(200, 136)[1] % 64 != 0 and R.first_lines(200, 136)[2] % 64 != 0                     # plane boundaries inside a bitmap word
    assert R.compact_layout(12, 24, 8, 8) == [0, 256, 512, 768, 1024, 1280, 1536, 1792]
    assert R.records_layout(12, 24, 8, 8) == [0, 256, 512, 768, 1024, 1280, 1536]


@pytest.mark.parametrize("W,H", R.SIZES)
def test_expand_gives_back_what_pack_stored(W, H):
    off = R.compact_layout(*R.geometry_bytes(W, H), W, H)
    for name, pl in contents(W, H):
        for oname, order in chunk_orders(R.nchunks(W, H)).items():
            if name.startswith("line") and oname != "ascending":
                continue                                                    # (one stored line: every order gives the same block)
            p = R.pack(pl, order)
            blk = R.assemble(p, off, fill=0xA5)
            n = R.check_block(blk, off, W, H)
            assert n == len(p["data"]) == {"zero": 0, "every_line": R.nlines(W, H)}.get(name, n), (name, oname)
            got = R.expand(blk, off, W, H)
            assert all(np.array_equal(g, x) for g, x in zip(got, pl)), (W, H, name, oname)
            if name.startswith("line"):
                assert n == 1
            if oname == "reversed" and R.nchunks(W, H) > 1 and name == "every_line":
                assert not np.array_equal(p["table"], R.pack(pl)["table"]), "the order did not move a chunk"


def test_check_block_sees_what_is_wrong():
    """the invariants are not vacuous: a counter left standing, a wrong total, a bit past the last line, chunks that overlap or leave a gap"""
    W, H = 144, 152
    off = R.compact_layout(*R.geometry_bytes(W, H), W, H)
    good = R.assemble(R.pack(R.content_every_line(W, H)), off)
    R.check_block(good, off, W, H)

    def broken(at, value, dtype="<u4"):
        b = good.copy()
        b[at:at + np.dtype(dtype).itemsize] = np.array([value], dtype).view(np.uint8)
        with pytest.raises(AssertionError):
            R.check_block(b, off, W, H)

    broken(off[3], 5); broken(off[3] + 4, 1); broken(off[3] + 8, 1025); broken(off[3] + 12, 1027)
    broken(off[4] + 4, 1023); broken(off[4] + 4, 1025)                                               # the second chunk one line early / late
    broken(off[5] + 16 * 8, 7, "<u8")                                                                # bits 1026 ..: past the last line (and the total no longer fits)


@pytest.fixture(scope="module")
def stub():
    """the stand-in as tests/test_host_pipeline_cpu.py has it"""
    lib = load_host_lib(build_host_lib("hip_stub.c"))
    lib.ks265_frame_levels.restype = C.c_void_p
    ctx = C.c_void_p()
    assert lib.ks265_create(C.byref(ctx), 0) == 0
    yield lib, ctx
    lib.ks265_destroy(ctx)


@pytest.mark.parametrize("W,H", R.SIZES)
def test_layout_and_pack_equal_the_stand_in(stub, W, H):
    """ks265_frame_compact_layout of the stand-in == compact_layout; what its ks265_frame_pack_compact writes from the header to the last stored line == pack() in
    ascending order, byte for byte"""
    from ks265codec_amd.lib import FrameCfg, FrameGeom
    lib, ctx = stub
    cfg = FrameCfg(width=W, height=H, qp=30, lambda_q4=64, me_range=64)
    geom, f = FrameGeom(), C.c_void_p()
    assert lib.ks265_frame_geometry(C.byref(cfg), C.byref(geom)) == 0
    assert (geom.bytes_cu8, geom.bytes_sao) == R.geometry_bytes(W, H)
    assert lib.ks265_frame_create(ctx, C.byref(cfg), C.byref(f)) == 0
    try:
        coff = (C.c_size_t * 8)()
        assert lib.ks265_frame_compact_layout(f, coff) == 0
        off = R.compact_layout(geom.bytes_cu8, geom.bytes_sao, W, H)
        assert list(coff) == off
        for name, pl in contents(W, H):
            for p in range(3):
                C.memmove(lib.ks265_frame_levels(f, p), pl[p].ctypes.data, pl[p].nbytes)
            dst = np.full(off[7], 0xA5, np.uint8)
            assert lib.ks265_frame_pack_compact(f, C.c_void_p(dst.ctypes.data), None) == 0
            ref = R.pack(pl)
            exp = R.assemble(ref, off, fill=0xA5)
            exp[off[3] + 16:off[3] + 64] = 0                                       # (the stand-in clears the whole header segment)
            end = off[6] + int(dst[off[3] + 8:off[3] + 12].view("<u4")[0]) * 64
            assert end == off[6] + len(ref["data"]) * 64, name
            assert np.array_equal(dst[off[3]:end], exp[off[3]:end]), (W, H, name)
            assert (dst[end:] == 0xA5).all(), (W, H, name)
    finally:
        lib.ks265_frame_destroy(f)
