"""The device-input scaler measured, in two parts.

Kernel: ks265_input_scale alone, 3840x2160 -> 1920x1080 and -> 1280x720, I420 and RGBA sources, both filters: device events around 200 back-to-back warm launches, the median of
7 such windows, the sources cycling through more than 256 MiB of distinct buffers so that every launch reads from HBM.  Beside each, ks265_input_convert of the SAME sources
timed the same way in the same run, as the yardstick: us, bytes moved, TB/s, the share of the yardstick's rate, and the floor (the source's bytes at the yardstick's rate).
One result per case is checked against tests/yuv_scale_ref.py on a 512-row band.

API: a 3840x2160 device I420 source into a 1920x1080 encoder (-preset slow -rc 0 -qp 27 -iper 128, default GOP) through Encoder(scale=...), against the same encoder fed the
pre-scaled 1920x1080 device I420 pictures; alternating runs, medians of pictures per second; the two streams must be equal.

Parent (--part parent --parent TREE, TREE = a built checkout of the parent commit): the switch never enabled.  A 1920x1080 encoder fed pre-scaled device I420 through
Encoder.encode, one process per run (--part plain --tree DIR: the second, warm pass counts; pictures/s and the stream's MD5), the parent's tree and this one alternating --runs
times - the MD5s must be equal - and then `bench.py --gpus 1 --steps 128 --warmup 6` in either tree, alternating --bench-runs times.

profiles/input_scale.txt is what one job wrote: the --out file of --part both followed by the --out file of --part parent, unedited.

    python tools/input_scale_rate.py [--part kernel|api|both|parent|plain] [--parent TREE] [--launches 200] [--windows 7] [--frames 256] [--runs 5] [--bench-runs 3] [--out FILE]"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class InDesc(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


class Lines(list):
    """the report: every line is printed as it is made, a long job shows where it stands"""
    def append(self, s):
        print(s, flush=True)
        super().append(s)


def timed(ks, launch, launches, windows):
    for i in range(launches):
        launch(i)
    ks.sync()
    per = []
    for _ in range(windows):
        ks._chk(ks.lib.ks265_timer_start(ks.h))
        for i in range(launches):
            launch(i)
        ms = C.c_float(0)
        ks._chk(ks.lib.ks265_timer_stop_ms(ks.h, C.byref(ms)))
        per.append(ms.value / launches)
    return statistics.median(per), min(per), max(per)


def desc_of(t, fmt, W, H):
    d = InDesc()
    d.width, d.height = W, H
    if fmt == "rgba":
        d.format, d.pixel_step = 2, 4
        d.plane[0], d.plane[1], d.plane[2], d.pitch[0] = t.data_ptr(), t.data_ptr() + 1, t.data_ptr() + 2, W * 4
    else:
        d.format = 0
        d.plane[0], d.plane[1], d.plane[2] = t.data_ptr(), t.data_ptr() + W * H, t.data_ptr() + W * H * 5 // 4
        d.pitch[0], d.pitch[1], d.pitch[2] = W, W // 2, W // 2
    return d


def kernel_part(a, lines):
    import yuv_convert_ref as cref
    import yuv_scale_ref as ys
    from ks265codec_amd.lib import KsContext
    ks = KsContext(0)
    dev = ks.device
    SW, SH = 3840, 2160
    lines.append(f"kernel alone: {SW}x{SH} sources, {a.launches} back-to-back launches per window, median (min .. max) of {a.windows} windows, device events; sources cycle through > 256 MiB")
    for fmt in ("i420", "rgba"):
        nbytes = SW * SH * (4 if fmt == "rgba" else 3) // (1 if fmt == "rgba" else 2)
        nbuf = int(300e6 // nbytes) + 1
        gen = torch.Generator(device=dev).manual_seed(5)
        bufs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(nbuf)]
        descs = [desc_of(b, fmt, SW, SH) for b in bufs]
        full = torch.empty(SW * SH * 3 // 2, dtype=torch.uint8, device=dev)
        med, lo, hi = timed(ks, lambda i: ks._chk(ks.lib.ks265_input_convert(ks.h, C.byref(descs[i % nbuf]), C.c_void_p(full.data_ptr()))), a.launches, a.windows)
        ybytes = nbytes + SW * SH * 3 // 2
        yard = ybytes / (med * 1e-3)
        lines.append(f"{fmt:5s} ks265_input_convert {SW}x{SH} (yardstick), {nbuf} buffers in turn   {ybytes / 1e6:6.1f} MB  {med * 1e3:8.2f} us ({lo * 1e3:.2f} .. {hi * 1e3:.2f})  {yard / 1e12:5.2f} TB/s")
        for DW, DH in ((1920, 1080), (1280, 720)):
            dst = torch.empty(DW * DH * 3 // 2, dtype=torch.uint8, device=dev)
            for filt, fname in ((0, "triangle"), (1, "Catmull-Rom")):
                plan = ks.scale_plan(SW, SH, DW, DH, filt)
                scr = full if fmt == "rgba" else None
                # one result against the specification: the top 256 source rows' share of the luma plane (rows whose taps all lie inside the band)
                ks.input_scale(plan, descs[0], dst, scr); ks.sync()
                got = dst.cpu().numpy()
                host = bufs[0].cpu().numpy()
                if fmt == "rgba":
                    px = host.reshape(SH, SW, 4)[:512]
                    band = cref.rgb_to_i420(px[:, :, 0], px[:, :, 1], px[:, :, 2])[:SW * 512].reshape(512, SW)
                else:
                    band = host[:SW * 512].reshape(512, SW)
                ty = ys.table(SH, DH, filt)
                rows = [r for r in range(DH) if ty[0][r] + ty[2] - 1 < 512]
                exp = ys.scale_plane(np.concatenate([band, np.zeros((SH - 512, SW), np.uint8)]), ys.table(SW, DW, filt), ty)[rows]
                assert (got[:DW * DH].reshape(DH, DW)[rows] == exp).all(), (fmt, DW, DH, fname)
                med, lo, hi = timed(ks, lambda i: ks.input_scale(plan, descs[i % nbuf], dst, scr), a.launches, a.windows)
                moved = nbytes + DW * DH * 3 // 2 + (2 * SW * SH * 3 // 2 if fmt == "rgba" else 0)     # RGBA: the I420 picture at the source's size is written and read back
                bw = moved / (med * 1e-3)
                floor_us = nbytes / yard * 1e6
                lines.append(f"{fmt:5s} ks265_input_scale -> {DW}x{DH} {fname:11s}  {moved / 1e6:6.1f} MB  {med * 1e3:8.2f} us ({lo * 1e3:.2f} .. {hi * 1e3:.2f})  {bw / 1e12:6.3f} TB/s"
                             f"  = {100 * bw / yard:5.1f} % of the yardstick's rate; floor {floor_us:6.2f} us = {100 * floor_us / (med * 1e3):5.1f} % of the time")
                ks.scale_plan_destroy(plan)
        del bufs, descs
        torch.cuda.empty_cache()
    ks.close()


def api_part(a, lines):
    import yuv_scale_ref as ys
    from ks265codec_amd.encoder import Encoder
    from ks265codec_amd.synth import make_clip
    SW, SH, DW, DH, NSRC = 3840, 2160, 1920, 1080, 8
    clip = make_clip(SW, SH, NSRC, seed=3, abc=(37, 53, 19), pan=(5, 3))
    src = [torch.from_numpy(np.ascontiguousarray(f)).cuda().view(SH * 3 // 2, SW) for f in clip]
    pre = [torch.from_numpy(ys.scale_i420(f, SW, SH, DW, DH, ys.CATMULL_ROM)).cuda().view(DH * 3 // 2, DW) for f in clip]
    params = dict(rc=0, qp=27, iper=128)

    def run(scaled):
        enc = Encoder(DW, DH, "slow", **(dict(scale="bicubic", scale_from=(SW, SH)) if scaled else {}), **params)
        pics = src if scaled else pre
        bs = bytearray()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with enc:
            for t in range(a.frames):
                bs += enc.encode(pics[t % NSRC], "i420")
            bs += enc.flush()
        torch.cuda.synchronize()
        return a.frames / (time.perf_counter() - t0), bytes(bs)

    run(True); run(False)                                              # warm
    fps = {True: [], False: []}
    streams = {}
    for _ in range(a.runs):
        for scaled in (False, True):
            f, bs = run(scaled)
            fps[scaled].append(f)
            assert streams.setdefault(scaled, bs) == bs, "a handle's stream changed between runs"
    assert streams[True] == streams[False], "the scaled handle's stream is not the pre-scaled handle's"
    lines.append(f"through the API: {SW}x{SH} device I420 -> {DW}x{DH} encoder, -preset slow -rc 0 -qp 27 -iper 128, {a.frames} pictures, {a.runs} alternating runs; streams equal, {len(streams[True])} bytes")
    for scaled, name in ((False, "pre-scaled 1920x1080 source"), (True, "3840x2160 source, scale=bicubic")):
        v = fps[scaled]
        lines.append(f"  {name:34s} median {statistics.median(v):7.1f} pictures/s  (min {min(v):.1f}, max {max(v):.1f}; runs {' '.join(f'{x:.1f}' for x in v)})")
    lines.append(f"  the scaler costs {100 * (1 - statistics.median(fps[True]) / statistics.median(fps[False])):.2f} % of the pre-scaled rate; the pre-scaled handle's own spread is "
                 f"{100 * (max(fps[False]) - min(fps[False])) / statistics.median(fps[False]):.2f} %")


def plain_part(a):
    """one process, one line: the 1080p encoder of the package under --tree fed device I420 with the switch never enabled"""
    import hashlib
    sys.path.insert(0, os.path.abspath(a.tree))
    from ks265codec_amd.encoder import Encoder
    from ks265codec_amd.synth import make_clip
    W, H, NSRC = 1920, 1080, 8
    clip = make_clip(W, H, NSRC, seed=3, abc=(37, 53, 19), pan=(5, 3))
    pics = [torch.from_numpy(np.ascontiguousarray(f)).cuda().view(H * 3 // 2, W) for f in clip]
    for _ in range(2):                                                  # the second, warm pass counts
        enc = Encoder(W, H, "slow", rc=0, qp=27, iper=128)
        bs = bytearray()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with enc:
            for t in range(a.frames):
                bs += enc.encode(pics[t % NSRC], "i420")
            bs += enc.flush()
        torch.cuda.synchronize()
        fps = a.frames / (time.perf_counter() - t0)
    print(f"RESULT {fps:.1f} pictures/s {len(bs)} bytes md5 {hashlib.md5(bs).hexdigest()}", flush=True)


def parent_part(a, lines):
    import json
    import subprocess
    trees = (("parent", os.path.abspath(a.parent)), ("this", ROOT))
    lines.append(f"the switch never enabled against the parent commit's libraries: a 1920x1080 encoder fed pre-scaled device I420 (Encoder.encode), -preset slow -rc 0 -qp 27 -iper 128, "
                 f"{a.frames} pictures, one process per run (its second, warm pass counts), alternating")
    fps, md5 = {"parent": [], "this": []}, set()
    for _ in range(a.runs):
        for name, tree in trees:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "plain", "--tree", tree, "--frames", str(a.frames)], capture_output=True, text=True, cwd=tree, timeout=300)
            res = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")]
            if r.returncode != 0 or not res:
                raise SystemExit(f"{name}: the run failed ({r.returncode}); nothing more is started\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            lines.append(f"  {name:6s} {res[0][7:]}")
            fps[name].append(float(res[0].split()[1])); md5.add(res[0].split()[-1])
    assert len(md5) == 1, "the stream with the switch unused is not the parent's"
    lines.append(f"  medians: parent {statistics.median(fps['parent']):.1f}, this {statistics.median(fps['this']):.1f} pictures/s; one MD5 in all {2 * a.runs} runs")
    lines.append(f"bench.py --gpus 1 --steps 128 --warmup 6 beside the parent, alternating: value (frames/s), psnr_y")
    for _ in range(a.bench_runs):
        for name, tree in trees:
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "6"], capture_output=True, text=True, cwd=tree, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{name}: bench.py failed ({r.returncode}); nothing more is started\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            d = json.loads(r.stdout.strip().split("\n")[-1])
            lines.append(f"  {name:6s} {d['value']} {d['psnr_y']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=("kernel", "api", "both", "parent", "plain"))
    ap.add_argument("--parent", default=None, help="--part parent: a built checkout of the parent commit")
    ap.add_argument("--tree", default=ROOT, help="--part plain: the tree whose package runs")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part == "plain":
        return plain_part(a)
    if a.part == "parent" and not a.parent:
        ap.error("--part parent needs --parent TREE")
    lines = Lines()
    lines.append(f"# tools/input_scale_rate.py --part {a.part} on one MI355X (gfx950), GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}; DESIGN.md 4m")
    if a.part == "parent":
        parent_part(a, lines)
    if a.part in ("kernel", "both"):
        kernel_part(a, lines)
        lines.append("")
    if a.part in ("api", "both"):
        api_part(a, lines)
    if a.out:                                                           # profiles/input_scale.txt is the --part both file followed by the --part parent file of one job
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
