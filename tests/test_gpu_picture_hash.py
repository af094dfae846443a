"""GPU: the decoded picture hash - ks265_picture_hash (ks265codec_amd/csrc/frame_metrics.hip) against tests/picture_hash_ref.py, exactly, and the `hash` switch
of `ks265enc` and of Encoder end to end.
  * kernel: all six values (picture_crc and picture_checksum of Y, Cb, Cr) equal the specification's on pictures whose borders hold random bytes - sizes with chroma rows shorter
    than a lane's bytes, ragged rows at 4-byte granularity, more than 256 samples each way, rows one step wider than a wave's row item (luma, and chroma), planes that are only
    8- or 4-byte aligned, and 2160p once;
  * state: calls back to back on one frame object give what single calls give (the accumulators are left zeroed); the _on form on a second context's stream;
  * end to end: the messages of `-hash 2 | 3` equal the specification on the -o dump and on the reference decoder's output; minus the messages the stream is the plain one."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
import torch  # noqa: E402  (torch's HIP runtime first, as in the other GPU modules)
torch.cuda.is_available()

import picture_hash_ref as ph  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "ks265codec_amd", "csrc", "frame_metrics.hip")).read()
    return int(re.search(rf"^#define {name} (\d+)\s", src, re.M).group(1))


# what a wave covers per row item; a work-group's four waves take different rows, so per row item it covers the same (frame_metrics.hip, "Shape")
WAVE_SAMPLES = 64 * _kernel_constant("KS_HASH_LANE_BYTES")
SIZES = [(64, 64),                      # chroma rows of 32 samples: one lane's bytes, every other lane of the wave in front of the row
         (72, 40),                      # chroma width 36: ragged at 4-byte granularity
         (200, 136), (264, 264),
         (520, 520),                    # the masks' `>> 8` terms in luma and in chroma, both ways
         (WAVE_SAMPLES + 8, 16),        # luma rows one 8-sample step wider than a row item: two items, the first holds one lane's quarter
         (2 * WAVE_SAMPLES + 8, 16)]    # ... and chroma rows one step (4 samples) wider than a row item; luma: three items


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


_frames = {}


@pytest.fixture(scope="module")
def frame_of(ks):
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import lambda_q4

    def get(size):
        if size not in _frames:
            _frames[size] = KsFrame(ks, size[0], size[1], 27, lambda_q4(27))
        return _frames[size]
    yield get
    for f in _frames.values():
        f.close()
    _frames.clear()


class _Pic:
    """a padded picture whose borders (and slack) hold random bytes; `shift` moves every plane that many bytes: rows that are only 8- or 4-byte aligned"""

    def __init__(self, ks, fr, i420, rng, shift=0):
        from ks265codec_amd.lib import Pic
        g, W, H = fr.geom, fr.width, fr.height
        self.t = []
        for content, stride, rows, pad, nbytes in zip(ph.i420_planes(i420, W, H), (g.stride_y, g.stride_c, g.stride_c), (g.rows_y, g.rows_c, g.rows_c), (g.pad_y, g.pad_c, g.pad_c),
                                                      (g.bytes_y, g.bytes_c, g.bytes_c)):
            buf = rng.integers(0, 256, nbytes + 16, dtype=np.uint8)
            v = buf[shift:shift + stride * rows].reshape(rows, stride)
            v[pad:pad + content.shape[0], pad:pad + content.shape[1]] = content
            self.t.append(ks.dev(buf))
        self.pic = Pic(*[t.data_ptr() + shift for t in self.t])

    def c(self):
        return self.pic


def _spec(i420, W, H):
    return ph.picture_hashes(*ph.i420_planes(i420, W, H))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_against_the_specification(ks, frame_of, size):
    W, H = size
    fr, rng, n = frame_of(size), np.random.default_rng(W * 7 + H), W * H * 3 // 2
    a = rng.integers(0, 256, n, dtype=np.uint8)
    b = a.copy(); b[-1] ^= 0x40                                          # differs from `a` in its last chroma byte alone
    for name, pic in (("random", a), ("zero", np.zeros(n, np.uint8)), ("all255", np.full(n, 255, np.uint8)), ("last_chroma_byte", b)):
        got, exp = fr.picture_hash(_Pic(ks, fr, pic, rng)).tolist(), _spec(pic, W, H)
        print(f"{W}x{H} {name}: device {got} spec {exp}")
        assert got == exp, name
    sa, sb = _spec(a, W, H), _spec(b, W, H)
    assert sa[:2] + sa[3:5] == sb[:2] + sb[3:5] and sa[2] != sb[2] and sa[5] != sb[5]


@pytest.mark.parametrize("shift", [4, 8, 12])
@pytest.mark.parametrize("size", [(72, 40), (200, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_planes_that_are_only_8_or_4_byte_aligned(ks, frame_of, size, shift):
    W, H = size
    fr, rng = frame_of(size), np.random.default_rng(shift)
    pic = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    assert fr.picture_hash(_Pic(ks, fr, pic, rng, shift=shift)).tolist() == _spec(pic, W, H)


def test_back_to_back_calls_leave_the_accumulators_zeroed(ks, frame_of):
    W, H = 520, 520
    fr, rng = frame_of((W, H)), np.random.default_rng(3)
    pics = [rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8) for _ in range(2)]
    dev = [_Pic(ks, fr, p, rng) for p in pics]
    spec = [_spec(p, W, H) for p in pics]
    order = [0, 1, 1, 0]
    outs = [ks.zeros(24) for _ in order]
    for out, i in zip(outs, order):                                       # no host synchronisation in between
        ks._chk(fr.lib.ks265_picture_hash(fr.h, dev[i].c(), C.c_void_p(out.data_ptr())))
    for out, i in zip(outs, order):
        assert ks.host(out, np.uint32).tolist() == spec[i]


def test_on_a_second_context(ks, frame_of):
    from ks265codec_amd.lib import KsContext
    W, H = 264, 264
    fr, rng = frame_of((W, H)), np.random.default_rng(9)
    pic = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    dev = _Pic(ks, fr, pic, rng)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = KsContext(0)                                              # bound to the side stream
        try:
            assert fr.picture_hash(dev, on=other).tolist() == _spec(pic, W, H)
        finally:
            other.close()
    assert fr.picture_hash(dev).tolist() == _spec(pic, W, H)             # and the frame's own stream finds the accumulators zeroed


def test_2160p(ks):
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import lambda_q4
    W, H = 3840, 2160
    fr, rng = KsFrame(ks, W, H, 27, lambda_q4(27)), np.random.default_rng(2160)
    try:
        pic = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
        assert fr.picture_hash(_Pic(ks, fr, pic, rng)).tolist() == _spec(pic, W, H)
    finally:
        fr.close()


# ---------------------------------------------------------------- end to end
W2, H2, N2 = 200, 136, 17
FSZ2 = W2 * H2 * 3 // 2


def _cli(tmp_path, tag, clip, *opts, dump=True):
    from ks265codec_amd import stream
    stream.build()
    yuv, out, rec = tmp_path / "in.yuv", tmp_path / f"{tag}.265", tmp_path / f"{tag}.yuv"
    if not yuv.exists():
        clip.tofile(str(yuv))
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W2), "-hgt", str(H2), "-fr", "25", "-preset", "slow", "-rc", "0", "-qp", "32", "-threads", "4", *opts, "-b", str(out),
                        *(("-o", str(rec)) if dump else ())], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-800:] + r.stderr[-800:]
    return out.read_bytes(), np.fromfile(str(rec), np.uint8).reshape(-1, FSZ2) if dump else None


def _decode(tmp_path, bs, n):
    (tmp_path / "d.265").write_bytes(bs)
    d = subprocess.run([REF_DEC, "-b", "d.265", "-o", "d.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
    dec = np.fromfile(str(tmp_path / "d.yuv"), np.uint8).reshape(-1, FSZ2)
    assert len(dec) == n
    return dec


def _check_messages(bs, hash_switch, pictures_of, n):
    pics, stripped = ph.sei_hashes(bs)
    assert len(pics) == n and sorted(p["disp"] for p in pics) == list(range(n))
    for p in pics:
        assert len(p["hashes"]) == 1 and p["hashes"][0][0] == hash_switch - 1, p
        assert p["hashes"][0][1] == ph.expected(pictures_of[p["disp"]], W2, H2, hash_switch - 1), (p["disp"], p["slice_type"])
    return stripped


@pytest.mark.parametrize("hash_switch", [2, 3], ids=["crc", "checksum"])
@pytest.mark.parametrize("gop", [(), ("-bframes", "0")], ids=["default_gop", "ippp"])
def test_cli_messages_against_the_specification(tmp_path, gop, hash_switch):
    from ks265codec_amd.synth import make_clip
    clip = make_clip(W2, H2, N2, seed=21, abc=(17, 23, 9))
    plain, rec0 = _cli(tmp_path, "plain", clip, *gop, "-hash", "0")
    bs, rec = _cli(tmp_path, "hash", clip, *gop, "-hash", str(hash_switch))
    assert (rec == rec0).all() and len(rec) == N2
    assert _check_messages(bs, hash_switch, rec, N2) == plain
    # without the reconstruction dump: the key pictures' and the anchors' streams, the split pipeline's drain on the copy-out stream
    plain2, _ = _cli(tmp_path, "plain2", clip, *gop, "-hash", "0", dump=False)
    bs2, _ = _cli(tmp_path, "hash2", clip, *gop, "-hash", str(hash_switch), dump=False)
    pics, stripped = ph.sei_hashes(bs2)
    assert stripped == plain2 and [len(p["hashes"]) for p in pics] == [1] * N2
    if os.path.exists(REF_DEC):
        _check_messages(bs2, hash_switch, _decode(tmp_path, bs2, N2), N2)
        _check_messages(bs, hash_switch, _decode(tmp_path, bs, N2), N2)


def test_encoder_from_an_rgba_tensor(tmp_path):
    from ks265codec_amd.encoder import Encoder
    N = 9
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (H2 // 8, W2 // 8, 4), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
    frames = [torch.from_numpy(np.roll(base, 3 * t, axis=1).copy()).cuda() for t in range(N)]
    res = {}
    for h in (3, 0, None):
        enc = Encoder(W2, H2, "slow", rc=0, qp=30, iper=128, threads=4, fr=25, log=3, **({} if h is None else {"hash": h}))
        res[h] = b"".join(enc.encode(t, "rgba") for t in frames) + enc.flush()
        enc.close()
    assert res[None] == res[0], "the switch is this handle's alone: the next handle opens without it"
    pics, stripped = ph.sei_hashes(res[3])
    assert stripped == res[0] and [len(p["hashes"]) for p in pics] == [1] * N and all(p["hashes"][0][0] == 2 for p in pics)
    with pytest.raises(ValueError):
        Encoder(W2, H2, "slow", hash=1)
    if os.path.exists(REF_DEC):
        _check_messages(res[3], 3, _decode(tmp_path, res[3], N), N)
