"""GPU: `roi` through the encoder (include/ks265_enc.h ks265_enc_set_next_roi, Encoder(roi=True), `ks265enc -roi`), 200x136, 17 pictures, the default GOP.
  * maps per picture from an int8 CUDA tensor, a per-pixel float32 CUDA tensor, a NumPy array, none: every picture's QP map (KS265_DUMP_QPMAP) is tests/roi_map_ref.py applied to
    the map handed in with its display index; one lane and two lanes give the same bytes; the stream decoded by the reference's decoder (where staged) is the reconstruction
    the encoder hands out (recon=); overwriting a map tensor on the same stream right after encode() returns changes nothing - the ordering contract;
  * `ks265enc -roi 0:0:64:64:-6 -roi 64:0:136:136:4`: the maps are the rasteriser's + the spec's, the stream decodes to -o;
  * refusals (host memory as a device map, a buffer one row short, a pitch below the row, log2_block 7, the wrong device, the switch off) are decided before any launch: the
    handle still encodes and nothing is pending."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import roi_map_ref as R  # noqa: E402
from cutree_mirror import read_qpmap_dump  # noqa: E402
from test_gpu_device_input import REF_DEC, _clip  # noqa: E402

QY_OK, QY_POINTER, QY_NOTSUPPORTED = 0, -0x7FFFFFFD, -0x7FFFFFFC
W, H, N = 200, 136, 17
FSZ = W * H * 3 // 2
COLS, ROWS = (W + 63) // 64, (H + 63) // 64
KEY_AT = 9                                                                # a key request: the second GOP (with two lanes: on the second lane)


def host_map(t):
    """(NumPy map, block) of display index t, or None: int8 at 16 x 16, per-pixel float32, int8 at 8 x 8, none"""
    rng = np.random.default_rng(500 + t)
    kind = t % 4
    if kind == 3:
        return None
    b = (16, 1, 8)[kind]
    rows, cols = R.map_shape(W, H, b.bit_length() - 1)
    if kind == 1:
        m = (rng.standard_normal((rows, cols)) * 5).astype(np.float32)
        m[:, : cols // 3] -= np.float32(6.25)
        m[0, :8] = [np.nan, np.inf, -np.inf, 1e9, -1e9, -0.0, 0.5 / 256, 1.5 / 256]
        return m, b
    m = rng.integers(-9, 10, (rows, cols)).astype(np.int8)
    m[rows // 2:] += np.int8(t % 5 - 2)
    return m, b


def expected(t, qp, maps=host_map):
    m = maps(t)
    rec = R.reduce(m[0], W, H, m[1].bit_length() - 1) if m is not None else None
    return R.ctu_map(rec, None, 0, 0, 4, COLS, ROWS, qp, 0, 51)


def session(tmp_path, lanes, scribble, maps=host_map, roi=True):
    """17 pictures through Encoder(roi=True, recon="i420").  kind 0 and 1 maps go in as CUDA tensors (kind 1 with a pitch above the row), kind 2 as the NumPy array.
    scribble: every CUDA map is overwritten on torch's current stream as soon as encode() has returned (else it stays alive and untouched to the end).
    Returns the stream, {poc: reconstruction}, the dump"""
    from ks265codec_amd.encoder import Encoder
    clip = _clip(W, H, N, seed=5)
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda().view(H * 3 // 2, W) for f in clip]
    dump = tmp_path / f"qp_{lanes}_{int(scribble)}.bin"
    env = {"KS265_GOP_LANES": str(lanes), "KS265_DUMP_QPMAP": str(dump)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        enc = Encoder(W, H, "slow", rc=0, qp=30, iper=32, threads=8, fr=50, psnr=1, roi=roi, recon="i420")
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    bs, rec, alive = bytearray(), {}, []
    assert enc.lib.ks265_enc_lanes(C.c_void_p(enc.h)) == lanes
    with enc:
        for t in range(N):
            m = maps(t)
            if t == KEY_AT:
                enc.lib.QY265EncoderKeyFrameRequest(C.c_void_p(enc.h))
            if m is None:
                bs += enc.encode(dev[t], "i420")
            elif m[0].dtype == np.int8 and m[1] == 8:
                arr = m[0].copy()
                bs += enc.encode(dev[t], "i420", roi=arr, roi_block=m[1])
                arr[:] = 99                                               # a host map is the caller's again when the call returns
            else:
                rows, cols = m[0].shape
                pad = 3 if m[0].dtype == np.float32 else 0
                full = torch.zeros((rows, cols + pad), dtype=torch.float32 if pad else torch.int8, device="cuda")
                full[:, :cols] = torch.from_numpy(m[0]).cuda()
                bs += enc.encode(dev[t], "i420", roi=full[:, :cols], roi_block=m[1])
                if scribble:
                    full.fill_(40)                                        # same stream, right behind the call: ordered behind the encoder's read
                else:
                    alive.append(full)
            rec.update(enc.recon())
        bs += enc.flush()
        rec.update(enc.recon())
    torch.cuda.synchronize()
    return bytes(bs), {p: t_.cpu().numpy().reshape(-1) for p, t_ in rec.items()}, dump


def test_maps_streams_lanes_and_the_ordering_contract(tmp_path):
    one, rec, dump = session(tmp_path, 1, scribble=True)
    got = read_qpmap_dump(str(dump))
    assert sorted(got) == list(range(N)) and sorted(rec) == list(range(N))
    flat = 0
    for d in range(N):
        kind, qp, qm = got[d]
        exp = expected(d, qp)
        assert (qm == exp).all(), (d, kind, qp, qm.tolist(), exp.tolist())
        flat += int(qm.max() == qm.min())
    assert [d for d in got if got[d][0] == "I"] == [0, KEY_AT] and {k for k, _, _ in got.values()} == {"I", "P", "B"}
    assert flat < N // 2, "the offsets reached the pictures"
    calm, rec_calm, _ = session(tmp_path, 1, scribble=False)
    assert calm == one, "a map overwritten on the same stream right after encode() returned: the stream of the run that left its maps alone"
    two, rec2, _ = session(tmp_path, 2, scribble=True)
    assert two == one, "one lane and two lanes give the same bytes"
    assert all((rec2[p] == rec[p]).all() for p in range(N))
    none, _, dump0 = session(tmp_path, 1, scribble=True, maps=lambda t: None)
    assert none != one and all(qm.max() == qm.min() == qp for _, qp, qm in read_qpmap_dump(str(dump0)).values())
    if os.path.exists(REF_DEC):
        (tmp_path / "a.265").write_bytes(one)
        d = subprocess.run([REF_DEC, "-b", "a.265", "-o", "dec.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
        assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
        dec = np.fromfile(str(tmp_path / "dec.yuv"), np.uint8).reshape(-1, FSZ)
        assert len(dec) == N and all((dec[p] == rec[p]).all() for p in range(N)), "the decoder shows the encoder's reconstruction: QpY, cu_qp_delta and the deblocking agree"


def test_cli_rectangles(tmp_path):
    from ks265codec_amd import stream
    stream.build()
    clip = _clip(W, H, N, seed=5)
    yuv, out, rec, dump = tmp_path / "in.yuv", tmp_path / "o.265", tmp_path / "rec.yuv", tmp_path / "qp.bin"
    clip.tofile(yuv)
    rects = [(0, 0, 64, 64, -6), (64, 0, 136, 136, 4)]
    args = [stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "30", "-threads", "8", "-b", str(out), "-o", str(rec)]
    for r in rects:
        args += ["-roi", "%d:%d:%d:%d:%d" % r]
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, KS265_DUMP_QPMAP=str(dump), KS265_GOP_LANES="1"))
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-600:] + r.stderr[-600:]
    got = read_qpmap_dump(str(dump))
    assert sorted(got) == list(range(N))
    m = R.rasterise(rects, W, H)
    records = R.reduce(m, W, H, 4)
    assert records.tolist() == [-6 * 256, 4 * 256, 4 * 256, 4 * 256, 0, 4 * 256, 4 * 256, 4 * 256, 0, 4 * 256, 4 * 256, 4 * 256]
    for d in range(N):
        kind, qp, qm = got[d]
        assert (qm == R.ctu_map(records, None, 0, 0, 4, COLS, ROWS, qp, 0, 51)).all(), (d, qp, qm.tolist())
    bad = subprocess.run(args + ["-roi", "1:2:3"], capture_output=True, text=True)
    assert bad.returncode == 2 and "bad value for -roi" in bad.stderr
    if os.path.exists(REF_DEC):
        d = subprocess.run([REF_DEC, "-b", str(out), "-o", "dec.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path)
        assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
        assert (np.fromfile(str(tmp_path / "dec.yuv"), np.uint8) == np.fromfile(str(rec), np.uint8)).all()


def test_refusals_launch_nothing_and_leave_nothing_pending(tmp_path):
    from ks265codec_amd.encoder import Encoder, EncoderError, Roi, describe_roi
    from ks265codec_amd.lib import load_library
    hl = load_library()
    ctx = C.c_void_p()
    assert hl.ks265_create(C.byref(ctx), 0) == 0
    rows, cols = R.map_shape(W, H, 0)
    short, ok = C.c_void_p(), C.c_void_p()
    assert hl.ks265_dev_malloc(ctx, C.byref(short), C.c_size_t(cols * (rows - 1))) == 0            # one row short
    assert hl.ks265_dev_malloc(ctx, C.byref(ok), C.c_size_t(cols * rows)) == 0
    assert hl.ks265_memset_async(ctx, ok, 5, C.c_size_t(cols * rows)) == 0 and hl.ks265_synchronize(ctx) == 0
    host = np.full((rows, cols), 5, np.int8)

    def roi(data, device=0, lb=0, pitch=cols):
        r = Roi()
        r.type, r.log2_block, r.device, r.data, r.pitch, r.stream = 0, lb, device, data, pitch, None
        return r

    cases = [(roi(host.ctypes.data), QY_POINTER),                          # host memory passed as a device map
             (roi(short.value), QY_POINTER),                                # a buffer one row short
             (roi(None), QY_POINTER),
             (roi(ok.value, pitch=cols - 1), QY_NOTSUPPORTED),              # a pitch below the row
             (roi(ok.value, lb=7), QY_NOTSUPPORTED),
             (roi(ok.value, device=1), QY_NOTSUPPORTED)]                    # the wrong device
    clip = _clip(W, H, len(cases) + 2, seed=5)
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda().view(H * 3 // 2, W) for f in clip]
    dump = tmp_path / "qp.bin"
    os.environ["KS265_DUMP_QPMAP"] = str(dump)
    try:
        enc = Encoder(W, H, "slow", rc=0, qp=30, iper=32, bframes=0, threads=8, fr=50, roi=True)
    finally:
        os.environ.pop("KS265_DUMP_QPMAP")
    with enc:
        for t, (r, code) in enumerate(cases):
            assert enc.lib.ks265_enc_set_next_roi(C.c_void_p(enc.h), C.byref(roi(ok.value))) == QY_OK   # something IS pending: the refusal clears it
            assert enc.lib.ks265_enc_set_next_roi(C.c_void_p(enc.h), C.byref(r)) == code, t
            enc.encode(dev[t], "i420")                                     # the handle still encodes, without a map
        assert enc.lib.ks265_enc_set_next_roi(C.c_void_p(enc.h), C.byref(roi(ok.value))) == QY_OK       # and takes a good map
        enc.encode(dev[len(cases)], "i420")
        with pytest.raises(ValueError):
            enc.encode(dev[len(cases) + 1], "i420", roi=host[:-1], roi_block=1)                         # the wrong shape: refused in Python, nothing pending
        enc.encode(dev[len(cases) + 1], "i420")
        enc.flush()
    got = read_qpmap_dump(str(dump))
    assert sorted(got) == list(range(len(cases) + 2))
    for d, (_, qp, qm) in got.items():
        assert (qm == min(51, qp + (5 if d == len(cases) else 0))).all(), (d, qp, qm.tolist())
    # the switch off: QY_NOTSUPPORTED, and encode(roi=) says so
    with Encoder(W, H, "slow", rc=0, qp=30, iper=32, bframes=0, threads=8, fr=50) as off:
        assert off.lib.ks265_enc_set_next_roi(C.c_void_p(off.h), C.byref(roi(ok.value))) == QY_NOTSUPPORTED
        with pytest.raises(RuntimeError):
            off.encode(dev[0], "i420", roi=host, roi_block=1)
        assert len(off.encode(dev[0], "i420") + off.flush()) > 100
    assert describe_roi(host, 1).device == -1 and EncoderError is not None
    for p in (short, ok):
        hl.ks265_dev_free(ctx, p)
    hl.ks265_destroy(ctx)
