"""GPU: the ROI map entries of the device library (include/ks265_hip.h ks265_roi_*, csrc/roi_map.hip) against tests/roi_map_ref.py, word for word.
  * ks265_roi_reduce: 64 x 64, 72 x 72 and 200 x 136 (partial CTUs on both edges) for every log2_block and both types, with base and pitch 16-byte aligned (the 16-byte
    loads), pitch + one element and base + one element (the element loads); 1920 x 1080 once for the per-pixel float map (last CTU row 56 high); values: the spec test's
    ties, clips and non-finite values.  A canary in front of and behind the records stays intact.
  * ks265_roi_ctu_map: the spec with records, and with NULL records exactly ks265_aq_ctu_map / ks265_qoff_ctu_map.
  * ks265_roi_validate: every refusal is decided on the host - nothing is launched."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first)
torch.cuda.is_available()

import roi_cases  # noqa: E402
import roi_map_ref as R  # noqa: E402

CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


def _place(ks, m: np.ndarray, layout: str):
    """the map on the device: 'aligned' (base and pitch multiples of 16), 'pitch' (pitch + one element), 'base' (base + one element); a 2-D view of one flat allocation"""
    rows, cols = m.shape
    es = m.dtype.itemsize
    per16 = 16 // es
    pitch_e = (cols + per16 - 1) // per16 * per16 + (1 if layout == "pitch" else 0)
    lead = 1 if layout == "base" else 0
    host = np.zeros(lead + pitch_e * rows, m.dtype)
    host[:] = 77 if m.dtype == np.int8 else np.float32(-33.25)            # what lies behind a row must not count
    v = host[lead:].reshape(rows, pitch_e)
    v[:, :cols] = m
    flat = torch.from_numpy(host).to(ks.device)
    assert flat.data_ptr() % 16 == 0
    t = flat[lead:].view(rows, pitch_e)[:, :cols]
    assert (t.data_ptr() % 16 == 0) == (layout != "base") and ((t.stride(0) * es) % 16 == 0) == (layout != "pitch")
    return flat, t


def _reduce(ks, m, lb, w, h, layout):
    n = ((w + 63) // 64) * ((h + 63) // 64)
    buf = torch.full((n + 8,), CANARY, dtype=torch.int32, device=ks.device)
    keep, t = _place(ks, m, layout)
    ks.roi_reduce(t, lb, w, h, out=buf[4:4 + n])
    ks.sync()
    got = buf.cpu().numpy()
    assert (got[:4] == CANARY).all() and (got[4 + n:] == CANARY).all(), "the canaries around the records"
    return got[4:4 + n]


@pytest.mark.parametrize("dtype", [np.int8, np.float32], ids=["int8", "float32"])
@pytest.mark.parametrize("lb", range(7))
def test_reduce_equals_the_spec(ks, lb, dtype):
    for w, h in ((64, 64), (72, 72), (200, 136)):
        m = roi_cases.special_map(1000 * lb + w, w, h, lb, dtype)
        exp = R.reduce(m, w, h, lb)
        for layout in ("aligned", "pitch", "base"):
            got = _reduce(ks, m, lb, w, h, layout)
            assert (got == exp).all(), (w, h, lb, layout, np.flatnonzero(got != exp)[:8], got[:8], exp[:8])


def test_reduce_1080p_per_pixel_float(ks):
    w, h = 1920, 1080                                                      # 30 x 17 CTUs, the last row 56 high
    m = roi_cases.special_map(11, w, h, 0, np.float32)
    exp = R.reduce(m, w, h, 0)
    for layout in ("aligned", "base"):
        got = _reduce(ks, m, 0, w, h, layout)
        assert (got == exp).all(), (layout, np.flatnonzero(got != exp)[:8])


def test_reduce_element_conversion_and_half_means(ks):
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)            # any bit pattern, one element per CTU: the record is the element's Q8 value
    ties = (rng.integers(-13100 * 2, 13100 * 2, 4096) / np.float32(512)).astype(np.float32)
    for m in (bits.view(np.float32).reshape(64, 64), ties.reshape(64, 64)):
        with np.errstate(invalid="ignore", over="ignore"):
            exp = R.to_q8(m).reshape(-1)
        assert (_reduce(ks, m, 6, 4096, 4096, "aligned") == exp).all()
    for k in (-3, -1, 0, 4):
        for lb in (0, 3, 5):
            m = roi_cases.half_mean_map(128, 64, lb, k)
            for layout in ("aligned", "pitch"):
                assert _reduce(ks, m, lb, 128, 64, layout).tolist() == [k + 1, k + 1]


def test_ctu_map_equals_the_spec_and_the_existing_kernels(ks):
    rng = np.random.default_rng(9)
    lib = ks.lib
    for nx, ny in ((13, 9), (5, 5), (30, 17), (4, 4)):                      # 16 x 16 blocks of 200 x 136, 72 x 72, 480 x 272, 64 x 64: nx, ny no multiples of 4 but the last
        cols, rows = (nx + 3) // 4, (ny + 3) // 4
        off = rng.standard_normal((ny, nx)) * 5
        off[: min(4, ny), : min(4, nx)] = 2.5                             # exact means of k + 0.5
        if nx > 4:
            off[:4, 4:8] = -3.5
        d_off = torch.from_numpy(off.reshape(-1).copy()).to(ks.device)
        rec = rng.integers(-14 * 256, 14 * 256, cols * rows).astype(np.int32)
        rec[0] = 128; rec[-1] = -128                                       # + 0.5 / - 0.5 on top of a mean of k + 0.5
        d_rec = torch.from_numpy(rec).to(ks.device)
        for qp, lo, hi in ((30, 0, 51), (30, 24, 36), (4, 0, 51), (49, 10, 51)):
            aq = ks.zeros(cols * rows)
            ks._chk(lib.ks265_aq_ctu_map(ks.h, C.c_void_p(d_off.data_ptr()), nx, ny, qp, lo, hi, C.c_void_p(aq.data_ptr())))
            got0 = ks.roi_ctu_map(None, d_off, nx, ny, 4, cols, rows, qp, lo, hi)
            assert (got0 == ks.host(aq, np.int8)).all() and (got0 == R.ctu_map(None, off, nx, ny, 4, cols, rows, qp, lo, hi)).all()
            got = ks.roi_ctu_map(d_rec, d_off, nx, ny, 4, cols, rows, qp, lo, hi)
            assert (got == R.ctu_map(rec, off, nx, ny, 4, cols, rows, qp, lo, hi)).all()
            got = ks.roi_ctu_map(d_rec, None, 0, 0, 4, cols, rows, qp, lo, hi)
            assert (got == R.ctu_map(rec, None, 0, 0, 4, cols, rows, qp, lo, hi)).all()
            got = ks.roi_ctu_map(None, None, 0, 0, 4, cols, rows, qp, lo, hi)
            assert (got == qp).all()
    # the cuTree's blocks: lg 3 (16 x 16 luma, 4 x 4 per CTU) and lg 4 (32 x 32, 2 x 2 per CTU) of a 200 x 136 picture, whose CTU grid the caller gives
    for lg, nx, ny in ((3, 13, 9), (4, 7, 5), (3, 12, 8), (4, 5, 3)):
        bpc, cols, rows = 64 >> (lg + 1), 4, 3
        off = rng.standard_normal((ny, nx)) * 5
        off[:bpc, :bpc] = -1.5
        d_off = torch.from_numpy(off.reshape(-1).copy()).to(ks.device)
        rec = rng.integers(-14 * 256, 14 * 256, cols * rows).astype(np.int32)
        d_rec = torch.from_numpy(rec).to(ks.device)
        for qp, lo, hi in ((30, 0, 51), (30, 24, 36)):
            qo = ks.zeros(cols * rows)
            ks._chk(lib.ks265_qoff_ctu_map(ks.h, C.c_void_p(d_off.data_ptr()), nx, ny, lg, cols, rows, qp, lo, hi, C.c_void_p(qo.data_ptr())))
            got0 = ks.roi_ctu_map(None, d_off, nx, ny, bpc, cols, rows, qp, lo, hi)
            assert (got0 == ks.host(qo, np.int8)).all() and (got0 == R.ctu_map(None, off, nx, ny, bpc, cols, rows, qp, lo, hi)).all()
            got = ks.roi_ctu_map(d_rec, d_off, nx, ny, bpc, cols, rows, qp, lo, hi)
            assert (got == R.ctu_map(rec, off, nx, ny, bpc, cols, rows, qp, lo, hi)).all()


def test_refusals_are_decided_on_the_host(ks):
    from ks265codec_amd.lib import ROI_FLOAT32, ROI_INT8, RoiDesc
    POINTER, NOTSUPPORTED = -3, -4
    w, h = 200, 136
    lib = ks.lib

    def dev_malloc(nbytes):                                                # allocations of their own (a tensor is a piece of a larger block of torch's allocator)
        p = C.c_void_p()
        assert lib.ks265_dev_malloc(ks.h, C.byref(p), C.c_size_t(nbytes)) == 0
        assert lib.ks265_memset_async(ks.h, p, 0, C.c_size_t(nbytes)) == 0
        return p

    ok, short, row_short, f, rec = dev_malloc(135 * 208 + 200), dev_malloc(135 * 208 + 199), dev_malloc(134 * 208 + 200), dev_malloc(136 * 800), dev_malloc(48)
    d = RoiDesc(ROI_INT8, 0, 200, 136, ok.value, 208)
    assert ks.roi_validate(d) == 0
    assert ks.roi_validate(RoiDesc(ROI_FLOAT32, 0, 200, 136, f.value, 800)) == 0
    seven = np.full(12, 7, np.int32)
    ks.sync()
    assert lib.ks265_memcpy_h2d_sync(ks.h, rec, C.c_void_p(seven.ctypes.data), C.c_size_t(48)) == 0

    def records():
        out = np.zeros(12, np.int32)
        ks.sync()
        assert lib.ks265_memcpy_d2h_async(ks.h, C.c_void_p(out.ctypes.data), rec, C.c_size_t(48)) == 0
        ks.sync()
        return out

    def both(desc, code):
        assert ks.roi_validate(desc) == code
        assert lib.ks265_roi_reduce(ks.h, C.byref(desc), w, h, rec) == code

    host = np.zeros((136, 208), np.int8)
    both(RoiDesc(ROI_INT8, 0, 200, 136, host.ctypes.data, 208), POINTER)                  # host memory
    both(RoiDesc(ROI_INT8, 0, 200, 136, None, 208), POINTER)
    both(RoiDesc(ROI_INT8, 0, 200, 136, short.value, 208), POINTER)                       # one byte short of the last row
    both(RoiDesc(ROI_INT8, 0, 200, 136, row_short.value, 208), POINTER)                   # one row short
    both(RoiDesc(ROI_INT8, 0, 200, 136, ok.value + 1, 208), POINTER)                      # begins inside the allocation, ends one byte behind it
    both(RoiDesc(ROI_FLOAT32, 0, 200, 136, f.value + 2, 800), POINTER)                    # a float map at an odd address
    both(RoiDesc(ROI_INT8, 0, 200, 136, ok.value, 199), NOTSUPPORTED)                     # pitch below the row
    both(RoiDesc(ROI_FLOAT32, 0, 200, 136, f.value, 802), NOTSUPPORTED)                   # no multiple of the element
    both(RoiDesc(ROI_INT8, 7, 2, 2, ok.value, 208), NOTSUPPORTED)
    both(RoiDesc(ROI_INT8, -1, 200, 136, ok.value, 208), NOTSUPPORTED)
    both(RoiDesc(2, 0, 200, 136, ok.value, 208), NOTSUPPORTED)
    both(RoiDesc(ROI_INT8, 0, 0, 136, ok.value, 208), NOTSUPPORTED)
    # a valid map of another picture size; records in host memory; records one word short; no records
    assert lib.ks265_roi_reduce(ks.h, C.byref(d), 208, h, rec) == NOTSUPPORTED
    hrec = np.zeros(12, np.int32)
    assert lib.ks265_roi_reduce(ks.h, C.byref(d), w, h, C.c_void_p(hrec.ctypes.data)) == POINTER
    assert lib.ks265_roi_reduce(ks.h, C.byref(d), w, h, C.c_void_p(rec.value + 4)) == POINTER
    assert lib.ks265_roi_reduce(ks.h, C.byref(d), w, h, None) == POINTER
    assert (records() == 7).all(), "no refusal launched anything"
    assert lib.ks265_roi_reduce(ks.h, C.byref(d), w, h, rec) == 0                         # and the context still works
    assert (records() == 0).all()
    for p in (ok, short, row_short, f, rec):
        assert lib.ks265_dev_free(ks.h, p) == 0
