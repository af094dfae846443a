"""Float tensors in and out (KS265_IN_RGB_F16 / _BF16 / _F32, include/ks265_hip.h) at 3840x2160: what the direct kernels cost beside the uint8 ones and beside the route a
caller takes without them.

Everything runs on ONE stream (torch's current one, which the context adopts), timed by events around --reps back-to-back warm launches, --rounds times with the cases
alternated; the figure is the median round's microseconds per launch.  Bytes moved are what the conversion has to touch: the source samples once (all four elements of a
four-element pixel) and the packed I420 picture, 1.5 bytes per pixel.
  input    ks265_input_convert of uint8 planar and RGBA (the yardstick: that code is the parent's), of the three float types in planar and four-element layout, and the
           route without them: x.mul(255).round().clamp(0, 255).to(torch.uint8), then the uint8 conversion.
  output   ks265_output_convert the same way, against the uint8 conversion followed by .float().div(255) (and .to(dtype)).
  --encode N   also: N uint8 RGBA pictures through Encoder at the default GOP (-preset slow -rc 0 -qp 27 -iper 128), pictures per second - the path that gains no call.

    python tools/float_io_bench.py [--reps 50] [--rounds 7] [--size 3840x2160] [--encode 0] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ks265codec_amd.lib import IN_RGB, IN_RGB_BF16, IN_RGB_F16, IN_RGB_F32, InDesc, load_library  # noqa: E402

TYPES = {"u8": (torch.uint8, IN_RGB), "f16": (torch.float16, IN_RGB_F16), "bf16": (torch.bfloat16, IN_RGB_BF16), "f32": (torch.float32, IN_RGB_F32)}


def desc_of(t, code, W, H, planar):
    """ks265_in_desc of a (3, H, W) or (H, W, 4) tensor"""
    es = t.element_size()
    d = InDesc()
    d.format, d.width, d.height = code, W, H
    for k in range(3):
        d.plane[k] = t.data_ptr() + (k * W * H * es if planar else k * es)
    d.pitch[0], d.pixel_step = (W * es, es) if planar else (4 * W * es, 4 * es)
    return d


def cases(lib, h, W, H):
    """name -> (callable that enqueues one conversion on the current stream, MB it has to move)"""
    i420 = torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")
    out, keep = {}, [i420]                                              # keep: every tensor a descriptor points into
    for layout, planar in (("planar", True), ("rgba", False)):
        shape, n = ((3, H, W), 3) if planar else ((H, W, 4), 4)
        u8 = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
        tmp8 = torch.empty_like(u8)
        dt8 = desc_of(tmp8, IN_RGB, W, H, planar)
        for name, (dtype, code) in TYPES.items():
            x = u8 if name == "u8" else (u8.float() / 255).to(dtype)
            d = desc_of(x, code, W, H, planar)
            keep += [x, tmp8]
            mb = W * H * (n * x.element_size() + 1.5) / 1e6

            def conv_in(d=d):
                rc = lib.ks265_input_convert(h, C.byref(d), C.c_void_p(i420.data_ptr()))
                assert rc == 0, (rc, lib.ks265_last_error(h))

            def conv_out(d=d):
                rc = lib.ks265_output_convert(h, C.c_void_p(i420.data_ptr()), C.byref(d))
                assert rc == 0, (rc, lib.ks265_last_error(h))
            out[f"in  {name:4s} {layout:6s} direct"] = (conv_in, mb)
            out[f"out {name:4s} {layout:6s} direct"] = (conv_out, mb)
            if name == "u8":
                continue

            def today_in(x=x, planar=planar):
                y = x.mul(255).round().clamp(0, 255).to(torch.uint8)
                dy = desc_of(y, IN_RGB, W, H, planar)
                rc = lib.ks265_input_convert(h, C.byref(dy), C.c_void_p(i420.data_ptr()))
                assert rc == 0, (rc, lib.ks265_last_error(h))

            def today_out(dtype=dtype, tmp8=tmp8, dt8=dt8):
                rc = lib.ks265_output_convert(h, C.c_void_p(i420.data_ptr()), C.byref(dt8))
                assert rc == 0, (rc, lib.ks265_last_error(h))
                tmp8.float().div(255).to(dtype)
            out[f"in  {name:4s} {layout:6s} today "] = (today_in, mb)
            out[f"out {name:4s} {layout:6s} today "] = (today_out, mb)
    return out, keep


def measure(W, H, reps, rounds):
    lib = load_library()
    h = C.c_void_p()
    assert lib.ks265_create(C.byref(h), 0) == 0
    assert lib.ks265_set_stream(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0   # one stream for the library's kernels and torch's
    cs, keep = cases(lib, h, W, H)
    for f, _ in cs.values():                                            # warm: code objects, the allocator's blocks of every shape
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in cs}
    for _ in range(rounds):
        for k, (f, _) in cs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / reps)
    lib.ks265_destroy(h)
    return [{"case": k, "us": statistics.median(v), "us_min": min(v), "us_max": max(v), "MB": cs[k][1], "GBps": cs[k][1] / statistics.median(v) * 1e3} for k, v in us.items()]


def encode_rate(W, H, n):
    from ks265codec_amd.encoder import Encoder
    pics = [torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(4)]
    base = torch.linspace(0, 255, W, device="cuda").to(torch.uint8)[None, :, None].expand(H, W, 4)
    pics = [(base // 2 + p // 8).contiguous() for p in pics]           # a ramp with some noise: pictures an encoder can spend time on
    with Encoder(W, H, "slow", rc=0, qp=27, iper=128, fr=50) as enc:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nbytes = sum(len(enc.encode(pics[t % len(pics)], "rgba")) for t in range(n)) + len(enc.flush())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"pictures": n, "pictures_per_s": n / dt, "bytes": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--encode", type=int, default=0, metavar="N", help="also code N uint8 RGBA pictures at the default GOP and print pictures per second")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    rows = measure(W, H, a.reps, a.rounds)
    by = {r["case"]: r for r in rows}
    lines = [f"{W}x{H}, events around {a.reps} back-to-back warm launches on one stream, median of {a.rounds} alternated rounds: microseconds per launch (min .. max), MB the conversion "
             "has to move, GB/s"]
    for r in rows:
        line = f"{r['case']}  {r['us']:8.2f} us ({r['us_min']:7.2f} .. {r['us_max']:7.2f})  {r['MB']:6.1f} MB  {r['GBps']:6.0f} GB/s"
        if "direct" in r["case"] and " u8 " not in r["case"]:
            t = by[r["case"].replace("direct", "today ")]
            line += f"   = {100.0 * r['us'] / t['us']:5.1f} % of today's route"
        lines.append(line)
    raw = {"rows": rows}
    if a.encode:
        raw["encode"] = encode_rate(W, H, a.encode)
        lines.append(f"uint8 RGBA through Encoder, -preset slow -rc 0 -qp 27 -iper 128, default GOP: {raw['encode']['pictures']} pictures, {raw['encode']['pictures_per_s']:.1f} pictures/s, "
                     f"{raw['encode']['bytes']} bytes")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
