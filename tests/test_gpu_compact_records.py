"""GPU: the seam every coded picture leaves the device through - ks265_frame_pack_compact[_on], ks265_copy_out_compact_async, ks265_copy_out_compact_dma_async and
ks265_frame_pack_records (csrc/frame_api.hip) - against the numpy restatement of the block formats (tests/compact_records_ref.py), bit for bit.  The level planes,
the CU map and the SAO records are written into the frame object's workspace by the test (no picture is coded, except for content (e)), the block is filled with a
sentinel first, so that every byte the kernels must not touch can be told from the ones they wrote.

Which test sees what:
  the reservation (atomicAdd on hdr[0], table[])     test_pack_compact[1280-720-*], [416-240-*] (check_block: the chunks' intervals tile the data area; expand == planes)
  the counter reset of the last work-group            test_block_reused_without_memset (and every second pack of test_pack_compact's single lines)
  zero padding of partial chroma lines                test_pack_compact[8-8-*], [88-248-*], [200-136-*] (every_line, single_lines: the level sits in element 15)
  plane boundaries inside a bitmap word / a wave      test_pack_compact[200-136-*], [88-248-*]
  the copy kernel behind the copy engine              test_copy_out (data_bytes 0 and 64)
  the tail of pack_records_kernel (4-byte words)      test_pack_records[8-8] (CU map of 12 bytes, SAO records of 24), test_pack_compact[8-8-*]"""
from __future__ import annotations

import numpy as np
import pytest

import compact_records_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5         # what the device block holds before a pack
HSENT = 0x5A        # what the pinned memory holds before a copy-out


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ks2():
    """a second context with a stream of its own, as the encoder host's drain and copy-out contexts are"""
    from ks265codec_amd.lib import KsContext
    c = KsContext(0, own_stream=True)
    yield c
    c.close()


class Rig:
    """a frame object of one size whose records are the test's: random CU map, SAO records and caller bytes, level planes as set_planes() leaves them"""

    def __init__(self, ks, W, H):
        from ks265codec_amd.lib import KsFrame
        from ks265codec_amd.synth import lambda_q4
        self.ks, self.W, self.H = ks, W, H
        self.f = KsFrame(ks, W, H, 30, lambda_q4(30))
        self.bytes_cu8, self.bytes_sao = int(self.f.geom.bytes_cu8), int(self.f.geom.bytes_sao)
        self.off = self.f.compact_layout()
        self.sizes = R.compact_sizes(self.bytes_cu8, self.bytes_sao, W, H)
        rng = np.random.default_rng([W, H])
        self.cu8 = rng.integers(0, 256, self.bytes_cu8, dtype=np.uint8)
        self.sao = rng.integers(0, 256, self.bytes_sao, dtype=np.uint8)
        self.extra = rng.integers(0, 256, 64, dtype=np.uint8)
        self.f.ws_write("cu8", self.cu8)
        self.f.ws_write("sao", self.sao)
        self.d_extra = ks.dev(self.extra)
        self.blk = ks.zeros(self.off[7])
        self.planes = R.zero_planes(W, H)
        self.set_planes(self.planes)

    def set_planes(self, planes):
        self.planes = [np.array(p, np.int16) for p in planes]
        for p in range(3):
            self.f.ws_write("levels", self.planes[p], p)

    def set_element(self, L, e, value):
        """one element of line L, on the device and in the host's copy"""
        p, e0, _ = R.line_elems(self.W, self.H, L)
        self.planes[p].reshape(-1)[e0 + e] = value
        self.f.ws_write("levels", np.array([value], np.int16), p, offset=2 * (e0 + e))

    def prepare(self):
        """the block as the host allocates it - header zero - with a sentinel everywhere else"""
        self.blk.fill_(SENT)
        self.blk[self.off[3]:self.off[3] + 64] = 0

    def fetch(self, before=None):
        """the block up to its last stored line, and whether everything behind that is what it was before the pack (`before`: a copy of the block; None: the sentinel)"""
        self.ks.sync()
        off = self.off
        fixed = self.blk[:off[6]].cpu().numpy()
        dl = int(fixed[off[3] + 8:off[3] + 12].view("<u4")[0])
        assert dl <= R.nlines(self.W, self.H), f"hdr[2] = {dl}"
        end = off[6] + dl * 64
        tail = self.blk[end:]
        untouched = bool((tail == SENT).all()) if before is None else bool((tail == before[end:]).all())
        return np.concatenate([fixed, self.blk[off[6]:end].cpu().numpy()]), untouched

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


def verify(rig, blk, untouched, with_extra=True, what=""):
    """every assertion on a block after ks265_frame_pack_compact; blk = Rig.fetch()"""
    W, H, off, sz = rig.W, rig.H, rig.off, rig.sizes
    fl = R.first_lines(W, H)
    n = R.check_block(blk, off, W, H)
    ref = R.pack(rig.planes)
    assert n == int(ref["hdr"][2]), (what, n, int(ref["hdr"][2]))
    words = (fl[3] + 63) // 64
    got_bm = blk[off[5]:off[5] + sz[5]].view("<u8")
    assert np.array_equal(got_bm[:words], ref["bitmap"][:words]), (what, "bitmap")
    assert (blk[off[5] + 8 * words:off[5] + sz[5]] == SENT).all(), (what, "bitmap words past the last line were written")
    got = R.expand(blk, off, W, H)
    for p in range(3):
        assert np.array_equal(got[p], rig.planes[p]), (what, f"plane {p}: {int((got[p] != rig.planes[p]).sum())} levels differ")
    for p in range(3):                                                  # a plane's partial last line is stored with a zero tail
        L = fl[p + 1] - 1
        nv = R.line_elems(W, H, L)[2]
        line = R.stored_line(blk, off, W, H, L)
        if nv < 32 and line is not None:
            assert not line[2 * nv:].any(), (what, f"line {L}: bytes behind the plane's end")
    assert untouched, (what, "the data area behind the last stored line was written")
    assert np.array_equal(blk[off[0]:off[0] + sz[0]], rig.cu8), (what, "CU map")
    assert np.array_equal(blk[off[1]:off[1] + sz[1]], rig.sao), (what, "SAO records")
    if with_extra:
        assert np.array_equal(blk[off[2]:off[2] + 64], rig.extra), (what, "caller bytes")
    else:
        assert (blk[off[2]:off[2] + 64] == SENT).all(), (what, "caller segment written without a source")
    assert not blk[off[3] + 16:off[3] + 64].any(), (what, "header segment behind the four words")
    for i in range(6):                                                  # the padding between the segments
        assert (blk[off[i] + sz[i]:off[i + 1]] == SENT).all(), (what, f"padding behind segment {i}")
    return n


def pack_and_verify(rig, with_extra=True, what="", fresh=True):
    if fresh:
        rig.prepare()
    before = None if fresh else rig.blk.clone()
    rig.f.pack_compact(rig.blk, rig.d_extra if with_extra else None)
    blk, untouched = rig.fetch(before)
    return verify(rig, blk, untouched, with_extra, what), blk


CONTENTS = ["zero", "every_line", "random", "single_lines"]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("W,H", R.SIZES)
def test_pack_compact(rigs, W, H, content):
    """contents (a) .. (d) at every size: (a) nothing stored, (b) every line stored with one level (first / last / middle element; 1, -1, -32768, 0x0100, 0x00FF), (c) one
    line in 50, (d) one picture per line of compact_records_ref.single_lines() with nothing else in it"""
    rig = rigs(W, H)
    if content != "single_lines":
        rig.set_planes({"zero": R.content_zero, "every_line": R.content_every_line, "random": R.content_random}[content](W, H))
        n, _ = pack_and_verify(rig, with_extra=content != "zero", what=content)
        assert n == {"zero": 0, "every_line": R.nlines(W, H)}.get(content, n)
        return
    rig.set_planes(R.content_zero(W, H))
    for i, (L, e) in enumerate(R.single_lines(W, H)):
        rig.set_element(L, e, R.LEVELS[i % 5])
        n, blk = pack_and_verify(rig, what=f"line {L} element {e}")
        assert n == 1 and blk[rig.off[4]:rig.off[4] + rig.sizes[4]].view("<u4").max() == 0       # one stored line: at the start of the data area, every chunk's base is 0
        rig.set_element(L, e, 0)


def test_pack_compact_real_pictures(rigs, ks):
    """content (e): what one key picture and one P picture leave in the frame object at 416x240"""
    from ks265codec_amd.synth import make_clip
    W, H = 416, 240
    rig = rigs(W, H)
    f = rig.f
    clip = make_clip(W, H, 2, seed=7)
    src, a, b = f.new_pic(), f.new_pic(), f.new_pic()
    try:
        for t in range(2):
            f.load_i420(ks.dev(clip[t]), src)
            f.encode_picture(src, a, t == 0, b)
            rig.planes = [f.ws_read("levels", nb, p).view("<i2").reshape((H, W) if p == 0 else (H // 2, W // 2)) for p, nb in enumerate(R.plane_bytes(W, H))]
            rig.cu8, rig.sao = f.ws_read("cu8", rig.bytes_cu8), f.ws_read("sao", rig.bytes_sao)
            assert rig.planes[0].any() and rig.cu8.any(), "the picture left no levels: nothing is tested"
            n, _ = pack_and_verify(rig, what="key picture" if t == 0 else "P picture")
            assert n > 0
            a, b = b, a
    finally:                                                            # the rig goes back to records of the test's own
        rig.cu8 = np.random.default_rng([W, H, 1]).integers(0, 256, rig.bytes_cu8, dtype=np.uint8)
        rig.sao = np.random.default_rng([W, H, 2]).integers(0, 256, rig.bytes_sao, dtype=np.uint8)
        f.ws_write("cu8", rig.cu8); f.ws_write("sao", rig.sao)
        rig.set_planes(R.content_zero(W, H))


def test_block_reused_without_memset(rigs):
    """one block, prepared once: (b), (c), (a), (b) packed into it one after the other.  The last work-group of a pack leaves both running counters zero, so the next
    pack starts from an empty data area although nothing clears the block in between; the lines the earlier pictures left behind the last stored line stay as they were
    and do not show in what the block expands to"""
    W, H = 416, 240
    rig = rigs(W, H)
    rig.prepare()
    for i, c in enumerate((R.content_every_line, R.content_random, R.content_zero, R.content_every_line)):
        rig.set_planes(c(W, H))
        n, _ = pack_and_verify(rig, what=f"pack {i}", fresh=False)
        assert n == (R.nlines(W, H), n, 0, R.nlines(W, H))[i]
    rig.set_planes(R.content_zero(W, H))


@pytest.mark.parametrize("W,H", [(88, 248), (416, 240)])
def test_pack_compact_on_another_stream(rigs, ks, ks2, W, H):
    """ks265_frame_pack_compact_on: the pack on a second context's stream behind an event of the frame's own context, as the host drains a picture - the same block
    (byte for byte where one chunk leaves no freedom; otherwise the same but for where the chunks lie)"""
    rig = rigs(W, H)
    rig.set_planes(R.content_random(W, H, seed=5))
    _, own = pack_and_verify(rig, what="own stream")
    ev = ks.event_create()
    try:
        rig.prepare()                                                   # (on the frame's own stream: the event is all that orders the second stream behind it)
        ks.event_record(ev)
        ks2.stream_wait_event(ev)
        rig.f.pack_compact(rig.blk, rig.d_extra, on=ks2)
        ks2.sync()
        other, untouched = rig.fetch()
        verify(rig, other, untouched, what="second stream")
    finally:
        ks.event_destroy(ev)
    off = rig.off
    assert np.array_equal(own[:off[4]], other[:off[4]]) and np.array_equal(own[off[5]:off[6]], other[off[5]:off[6]])
    if R.nchunks(W, H) == 1:
        assert np.array_equal(own, other)
    rig.set_planes(R.content_zero(W, H))


def _copy_out(rig, ks, ks2, pinned, view, data_bytes):
    """the block to pinned memory on the second context's stream, behind the pack"""
    view[:] = HSENT
    ev = ks.event_create()
    try:
        ks.event_record(ev)
        ks2.stream_wait_event(ev)
        rig.f.copy_out_compact(ks2, pinned, rig.blk, data_bytes)
        ks2.sync()
    finally:
        ks.event_destroy(ev)
    return view.copy()


@pytest.mark.parametrize("W,H", R.SIZES)
def test_copy_out(rigs, ks, ks2, W, H):
    """ks265_copy_out_compact_async (the kernel alone) and ks265_copy_out_compact_dma_async with data_bytes = 0, 64 (rounds to 256: less than the stored lines need),
    exactly the stored lines, 4096 more, and the block's capacity (what the host passes for key pictures: clamped to the data area) on content (c); content (b) with
    data_bytes = 0, where the kernel behind the copy engine carries the whole data area.  Pinned memory: the block up to its last stored line, nothing behind what the
    copy engine was asked to take"""
    rig = rigs(W, H)
    off = rig.off
    pinned, view = ks.host_malloc(off[7])
    try:
        for content, sizes in ((R.content_random, None), (R.content_every_line, [0])):
            rig.set_planes(content(W, H))
            n, blk = pack_and_verify(rig, what="copy-out source")
            end = off[6] + n * 64
            assert len(blk) == end
            if sizes is None:
                got = _copy_out(rig, ks, ks2, pinned, view, None)
                assert np.array_equal(got[:end], blk), "kernel copy-out: the block"
                assert (got[end:] == HSENT).all(), "kernel copy-out: bytes behind the last stored line"
                sizes = [0, 64, n * 64, n * 64 + 4096, off[7]]
            for db in sizes:
                got = _copy_out(rig, ks, ks2, pinned, view, db)
                assert np.array_equal(got[:end], blk), (db, "the block")
                keep = off[6] + max(n * 64, min((db + 255) & ~255, off[7] - off[6]))
                assert (got[keep:] == HSENT).all(), (db, "bytes behind what was to be copied")
    finally:
        ks.sync(); ks2.sync()
        ks.host_free(pinned)
        rig.set_planes(R.content_zero(W, H))


@pytest.mark.parametrize("extra", [True, False])
@pytest.mark.parametrize("W,H", [(8, 8), (200, 136), (416, 240)])
def test_pack_records(rigs, ks, W, H, extra):
    """ks265_frame_pack_records: the six segments at records_layout's offsets equal their sources over exactly their sizes, nothing else in the block is written"""
    rig = rigs(W, H)
    off = rig.f.records_layout()
    assert off == R.records_layout(rig.bytes_cu8, rig.bytes_sao, W, H)
    sz = R.records_sizes(rig.bytes_cu8, rig.bytes_sao, W, H)
    assert all(s % 4 == 0 for s in sz), "a segment that is no multiple of 4 bytes: the kernel's tail would drop bytes"
    rng = np.random.default_rng([W, H, 9])
    rig.set_planes([rng.integers(-32768, 32768, p.shape).astype(np.int16) for p in R.zero_planes(W, H)])
    dst = ks.zeros(off[6])
    dst.fill_(SENT)
    try:
        rig.f.pack_records(dst, rig.d_extra if extra else None)
        ks.sync()
        got = dst.cpu().numpy()
        src = [rig.cu8, *[p.reshape(-1).view(np.uint8) for p in rig.planes], rig.sao, rig.extra if extra else np.full(64, SENT, np.uint8)]
        for i in range(6):
            assert np.array_equal(got[off[i]:off[i] + sz[i]], src[i]), f"segment {i}"
            assert (got[off[i] + sz[i]:off[i + 1]] == SENT).all(), f"padding behind segment {i}"
    finally:
        rig.set_planes(R.content_zero(W, H))
