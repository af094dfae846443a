"""GPU: -ssim - the fused SSIM + SSE pass (ks265_ssim_picture, ks265codec_amd/csrc/frame_metrics.hip) against tests/ssim_ref.py, the ` ssim:` line of
`ks265enc`, and Encoder.quality() / ks265_enc_get_quality.
  * kernel: per plane the fixed-point sum is within one unit per window of the specification's (exactly windows x 2^30 for a picture against itself), the SSE sums are bit for
    bit ks265_sse_picture's, the borders of the padded pictures (random bytes here) and the samples outside the whole windows enter no SSIM sum;
  * state: calls back to back on one stream give what single calls give (the accumulators are left zeroed, integer sums are order-free);
  * end to end: the three values of the ` ssim:` line are the specification's means over (input, -o reconstruction); -ssim leaves the stream as it is."""
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

import ssim_ref  # noqa: E402
from golden_io import load_cases  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "appdecoder")
SIZES = [(64, 64),          # one partly filled wave; 16 chroma windows
         (200, 136),        # chroma 100x68: partial windows both ways
         (520, 264)]        # 65 luma windows per row, one past a wave; chroma 260x132
LINE_BOUND = 5e-5 + 1e-6    # printing at four decimals + the fixed-point bound


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    k = KsContext(0)
    yield k
    k.close()


@pytest.fixture(scope="module")
def frames(ks):
    from ks265codec_amd.lib import KsFrame
    from ks265codec_amd.synth import lambda_q4
    fr = {s: KsFrame(ks, s[0], s[1], 27, lambda_q4(27)) for s in SIZES}
    yield fr
    for f in fr.values():
        f.close()


def _contents(W, H, rng):
    """(name, a, b) I420 pictures"""
    n = W * H * 3 // 2
    rnd = lambda: rng.integers(0, 256, n, dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    smooth = np.concatenate([((x + 2 * y) // 3 % 254 + 1).astype(np.uint8).reshape(-1), ((cx + 60) % 254 + 1).astype(np.uint8).reshape(-1), ((cy * 2 + 30) % 254 + 1).astype(np.uint8).reshape(-1)])
    a = rnd()
    return [("random", a, rnd()), ("self", a, a), ("flat0_flat255", np.zeros(n, np.uint8), np.full(n, 255, np.uint8)), ("flat_noise", np.full(n, 131, np.uint8), rnd()),
            ("smooth_pm1", smooth, (smooth.astype(np.int16) + rng.choice([-1, 1], n)).astype(np.uint8))]


class _Pic:
    """a padded picture whose borders (and slack) hold random bytes; `shift` moves every plane 4 bytes: rows that are only 4-byte aligned"""

    def __init__(self, ks, fr, i420, rng, shift=0):
        from ks265codec_amd.lib import Pic
        g, W, H = fr.geom, fr.width, fr.height
        self.t = []
        for content, stride, rows, pad, nbytes in zip(ssim_ref.planes_of(i420, W, H), (g.stride_y, g.stride_c, g.stride_c), (g.rows_y, g.rows_c, g.rows_c), (g.pad_y, g.pad_c, g.pad_c),
                                                      (g.bytes_y, g.bytes_c, g.bytes_c)):
            buf = rng.integers(0, 256, nbytes + 8, dtype=np.uint8)
            v = buf[shift:shift + stride * rows].reshape(rows, stride)
            v[pad:pad + content.shape[0], pad:pad + content.shape[1]] = content
            self.t.append(ks.dev(buf))
        self.pic = Pic(*[t.data_ptr() + shift for t in self.t])

    def c(self):
        return self.pic


def _spec(a, b, W, H):
    res = ssim_ref.picture_ssim(a, b, W, H)
    sse = [int(((pa.astype(np.int64) - pb.astype(np.int64)) ** 2).sum()) for pa, pb in zip(ssim_ref.planes_of(a, W, H), ssim_ref.planes_of(b, W, H))]
    return [n for n, _, _ in res], [f for _, _, f in res], sse


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_against_the_specification(ks, frames, size):
    W, H = size
    fr, rng = frames[size], np.random.default_rng(W)
    for name, a, b in _contents(W, H, rng):
        pa, pb = _Pic(ks, fr, a, rng), _Pic(ks, fr, b, rng)
        windows, fixed, sse_spec = _spec(a, b, W, H)
        assert windows == [(W // 8) * (H // 8), (W // 16) * (H // 16), (W // 16) * (H // 16)]        # partial windows are dropped (tests/test_ssim_ref.py)
        sse, got = fr.ssim_picture(pa, pb)
        only_sse = fr.sse_picture(pa, pb)
        _, got_alone = fr.ssim_picture(pa, pb, with_sse=False)
        print(f"{W}x{H} {name}: device {got.tolist()} spec {fixed} windows {windows} sse {sse.tolist()}")
        assert sse.tolist() == only_sse.tolist() == sse_spec, name                                   # bit for bit the SSE pass (which counts what the window rule leaves out)
        assert got_alone.tolist() == got.tolist(), name
        if name == "self":
            assert got.tolist() == [n << 30 for n in windows]
        else:
            assert all(abs(int(g) - f) <= n for g, f, n in zip(got, fixed, windows)), name           # one fixed-point unit per window: a last bit rounded the other way


def test_rows_that_are_only_4_byte_aligned(ks, frames):
    W, H = 200, 136
    fr, rng = frames[(W, H)], np.random.default_rng(77)
    a, b = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8), rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    pa, pb = _Pic(ks, fr, a, rng, shift=4), _Pic(ks, fr, b, rng, shift=4)
    windows, fixed, sse_spec = _spec(a, b, W, H)
    sse, got = fr.ssim_picture(pa, pb)
    assert sse.tolist() == fr.sse_picture(pa, pb).tolist() == sse_spec
    assert all(abs(int(g) - f) <= n for g, f, n in zip(got, fixed, windows))


def test_back_to_back_calls_leave_the_accumulators_zeroed(ks, frames):
    W, H = 520, 264
    fr, rng = frames[(W, H)], np.random.default_rng(3)
    pairs = [(_Pic(ks, fr, a, rng), _Pic(ks, fr, b, rng)) for _, a, b in _contents(W, H, rng)[:3]]
    single = [fr.ssim_picture(pa, pb) for pa, pb in pairs]
    order = [0, 1, 2, 0]
    outs = [(ks.zeros(24), ks.zeros(24)) for _ in order]
    for (sse, ssim), i in zip(outs, order):                                                          # no host synchronisation in between
        ks._chk(fr.lib.ks265_ssim_picture(fr.h, pairs[i][0].c(), pairs[i][1].c(), C.c_void_p(sse.data_ptr()), C.c_void_p(ssim.data_ptr())))
    for (sse, ssim), i in zip(outs, order):
        assert ks.host(sse, np.uint64).tolist() == single[i][0].tolist() and ks.host(ssim, np.int64).tolist() == single[i][1].tolist()


# ---------------------------------------------------------------- end to end: the CLI's line
def _cli(tmp_path, tag, W, H, clip, *opts, env=None, dump=True):
    from ks265codec_amd import stream
    stream.build()
    yuv, out, rec = tmp_path / "in.yuv", tmp_path / f"{tag}.265", tmp_path / f"{tag}.yuv"
    if not yuv.exists():
        clip.tofile(str(yuv))
    r = subprocess.run([stream.CLI, "-i", str(yuv), "-wdt", str(W), "-hgt", str(H), "-fr", "25", "-preset", "slow", "-rc", "0", "-qp", "32", "-threads", "4", *opts, "-b", str(out), *(("-o", str(rec)) if dump else ())],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-800:] + r.stderr[-800:]
    return r.stdout, out.read_bytes(), np.fromfile(str(rec), np.uint8) if dump else None


def _ssim_lines(stdout):
    return [ln + "\n" for ln in stdout.split("\n") if "ssim:" in ln]


def _check_line(stdout, clip, rec, W, H):
    lines = _ssim_lines(stdout)
    assert len(lines) == 1, stdout[-600:]
    fixture_line = load_cases("ssim_ref")[0]["line"].tobytes().decode()
    shape = lambda s: re.sub(r"\d+", "0", s)                                                         # the reference's bytes with every number's digits folded
    assert shape(lines[0]) == shape(fixture_line) and re.fullmatch(r"\t ssim: \d+\.\d{4}\t\d\.\d{4}\t\d\.\d{4}\t\d\.\d{4}\n", lines[0]), lines[0]
    vals = [float(x) for x in lines[0].split("\t")[2:]]
    spec = ssim_ref.stream_ssim(clip, rec.reshape(len(clip), -1), W, H)
    print("line", vals, "spec", spec.tolist(), "max |diff|", np.abs(np.array(vals) - spec).max())
    assert (np.abs(np.array(vals) - spec) <= LINE_BOUND).all()
    psnr = [ln for ln in stdout.split("\n") if ln.startswith("bitrate, psnr:")]
    if psnr:
        assert stdout.index("bitrate, psnr:") < stdout.index("\t ssim:") and lines[0].split("\t")[1] == " ssim: " + psnr[0].split("\t")[0].split(": ")[1]   # behind it, the same kbit/s
    return lines[0]


@pytest.mark.parametrize("gop", [(), ("-bframes", "0")], ids=["default_gop", "ippp"])
def test_cli_line_against_the_specification(tmp_path, gop):
    from ks265codec_amd.synth import make_clip
    W, H, N = 200, 136, 9
    clip = make_clip(W, H, N, seed=21, abc=(17, 23, 9))
    plain, bs0, _ = _cli(tmp_path, "plain", W, H, clip, "-psnr", "1", *gop)
    out, bs1, rec = _cli(tmp_path, "ssim", W, H, clip, "-psnr", "1", "-ssim", "1", *gop)
    assert not _ssim_lines(plain) and bs0 == bs1, "-ssim leaves the stream as it is"
    assert [ln for ln in out.split("\n") if ln.startswith("bitrate, psnr:")] == [ln for ln in plain.split("\n") if ln.startswith("bitrate, psnr:")]
    line = _check_line(out, clip, rec, W, H)
    alone, bs2, rec2 = _cli(tmp_path, "alone", W, H, clip, "-psnr", "0", "-ssim", "1", *gop)          # no SSE wanted: the line alone
    assert "bitrate, psnr:" not in alone and bs2 == bs0 and _check_line(alone, clip, rec2, W, H) == line
    per_pic, _, _ = _cli(tmp_path, "two", W, H, clip, "-psnr", "2", "-ssim", "2", *gop)               # -ssim 2: a line per picture of this build's own, the -psnr 2 table untouched
    mine = [ln for ln in per_pic.split("\n") if ln.startswith("ks265enc: poc ") and " ssim " in ln]
    assert len(mine) == N and sorted(int(ln.split()[2]) for ln in mine) == list(range(N)) and _ssim_lines(per_pic) == [line]
    table = [ln for ln in per_pic.split("\n") if re.fullmatch(r"\d+\t[IPB]\t\d+\t[\d.]+\t[\d.]+\t[\d.]+\t\d+", ln)]
    assert len(table) == N
    mean = np.mean([[float(x) for x in ln.split()[4:7]] for ln in mine], axis=0)
    assert (np.abs(mean - np.array([float(x) for x in line.split("\t")[2:]])) <= 1e-4).all()


def test_cli_two_gop_lanes_print_the_one_lane_line(tmp_path):
    from ks265codec_amd.synth import make_clip
    W, H, N = 200, 136, 64
    clip = np.concatenate([make_clip(W, H, 16, seed=4, abc=(17, 23, 9))] * 4)
    outs = {}
    for lanes in (1, 2):                                                                             # (no -o: the reconstruction dump keeps a handle on one lane)
        outs[lanes] = _cli(tmp_path, f"l{lanes}", W, H, clip, "-psnr", "1", "-ssim", "1", "-iper", "32", "-bframes", "0", env={"KS265_GOP_LANES": str(lanes)}, dump=False)
    assert ("GOP lanes" in outs[2][0]) and "GOP lanes" not in outs[1][0] and outs[1][1] == outs[2][1]
    assert _ssim_lines(outs[1][0]) == _ssim_lines(outs[2][0]) and len(_ssim_lines(outs[2][0])) == 1
    if os.path.exists(REF_DEC):                                                                      # the key pictures' stream and the copy-out stream, which a run with -o does not use
        d = subprocess.run([REF_DEC, "-b", "l2.265", "-o", "d.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
        _check_line(outs[2][0], clip, np.fromfile(str(tmp_path / "d.yuv"), np.uint8), W, H)


# ---------------------------------------------------------------- the API: Encoder.quality()
class _Stats(C.Structure):
    _fields_ = [("frames", C.c_long), ("bytes", C.c_longlong), ("sse", C.c_double * 3), ("rest", C.c_uint8 * 512)]


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="the reference's decoder was not staged (oracle/_ref/appdecoder)")
def test_encoder_quality_against_the_decoded_stream(tmp_path):
    from ks265codec_amd.encoder import Encoder
    from ks265codec_amd.synth import make_clip
    W, H, N = 200, 136, 12
    clip = make_clip(W, H, N, seed=8, abc=(17, 23, 9))
    dev = [torch.from_numpy(f.copy()).cuda().view(H * 3 // 2, W) for f in clip]
    res = {}
    for ssim in (1, 0):
        enc = Encoder(W, H, "slow", rc=0, qp=30, iper=128, threads=4, fr=25, psnr=1, ssim=ssim, log=3)
        bs = b"".join(enc.encode(t, "i420") for t in dev) + enc.flush()
        st = _Stats()
        assert enc.lib.ks265_enc_get_stats(C.c_void_p(enc.h), C.byref(st)) == 0
        res[ssim] = (bs, enc.quality(), (st.frames, st.bytes, list(st.sse)))
        enc.close()
    (bs, q, st), (bs0, q0, st0) = res[1], res[0]
    assert bs == bs0 and st == st0 and st[0] == N, "the stream and ks265_enc_get_stats are what they were"
    assert q0["ssim"] is None and q0["last"]["ssim"] is None and q0["frames"] == N and q0["sse"] == st0[2]
    (tmp_path / "a.265").write_bytes(bs)
    d = subprocess.run([REF_DEC, "-b", "a.265", "-o", "d.yuv", "-threads", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert "decoder passed" in d.stdout, d.stdout[-400:] + d.stderr[-400:]
    dec = np.fromfile(str(tmp_path / "d.yuv"), np.uint8).reshape(N, -1)
    spec = ssim_ref.stream_ssim(clip, dec, W, H)
    print("quality", q, "spec", spec.tolist())
    assert q["frames"] == N and q["sse"] == st[2] and (np.abs(np.array(q["ssim"]) - spec) <= LINE_BOUND).all()
    sse = [[int(((pa.astype(np.int64) - pb.astype(np.int64)) ** 2).sum()) for pa, pb in zip(ssim_ref.planes_of(a, W, H), ssim_ref.planes_of(b, W, H))] for a, b in zip(clip, dec)]
    assert q["sse"] == np.sum(sse, axis=0).tolist()
    last = q["last"]["poc"]
    assert 0 <= last < N
    assert q["last"]["sse"] == sse[last]
    assert (np.abs(np.array(q["last"]["ssim"]) - np.array([m for _, m, _ in ssim_ref.picture_ssim(clip[last], dec[last], W, H)])) <= 1e-6).all()
