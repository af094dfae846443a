#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (builder container: needs the reference encoder, oracle/_ref/appencoder).  Runs the reference with `-ssim` on small clips and records, per case,
the input planes, the reconstruction it wrote (`-o`), the four numbers of its ` ssim:` line and the line's bytes in ssim_ref.npz.  tests/test_ssim_ref.py holds
tests/ssim_ref.py against these numbers: the fixture is what decides the definition (window rule at plane sizes that are no multiple of 8, pooling over pictures).
Data the reference read and wrote only; prints what the candidate window rules give beside the printed value, for DESIGN.md 4i."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssim_ref  # noqa: E402
from golden_io import save_cases  # noqa: E402
from ks265codec_amd.synth import make_clip  # noqa: E402

ENC = os.path.join(ROOT, "oracle", "_ref", "appencoder")


def smooth_clip(W, H, N):
    """gradients without texture: at a low QP the encoder reproduces them almost exactly"""
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    return np.stack([np.concatenate([((x + 2 * y + 3 * t) // 2 % 256).astype(np.uint8).reshape(-1), ((100 + cx + t) % 256).astype(np.uint8).reshape(-1),
                                     ((140 + cy) % 256).astype(np.uint8).reshape(-1)]) for t in range(N)])


# name: (W, H, pictures, clip, extra arguments)
CASES = {
    "64x64_qp22": (64, 64, 1, "synth", ["-qp", "22"]),
    "64x64_qp45": (64, 64, 1, "synth", ["-qp", "45"]),
    "72x40_qp30": (72, 40, 1, "synth", ["-qp", "30"]),                 # chroma 36x20
    "136x72_qp45": (136, 72, 1, "synth", ["-qp", "45"]),               # chroma 68x36
    "200x136_qp34": (200, 136, 1, "synth", ["-qp", "34"]),             # chroma 100x68
    "flat_64x64": (64, 64, 1, "flat", ["-qp", "30"]),
    "smooth_64x64_qp4": (64, 64, 1, "smooth", ["-qp", "4"]),
    "72x40_5pics": (72, 40, 5, "synth", ["-qp", "34"]),                # default GOP
    "136x72_4pics_ippp": (136, 72, 4, "synth", ["-qp", "38", "-bframes", "0"]),
    "64x64_9pics_psnr2_ssim2": (64, 64, 9, "synth", ["-qp", "30", "-psnr", "2", "-ssim", "2"]),
}


def run(name, tmp):
    W, H, N, kind, extra = CASES[name]
    clip = make_clip(W, H, N, seed=7 + len(name), abc=(17, 23, 9)) if kind == "synth" else smooth_clip(W, H, N) if kind == "smooth" else np.full((N, W * H * 3 // 2), 97, np.uint8)
    clip.tofile(os.path.join(tmp, "in.yuv"))
    args = ["-i", "in.yuv", "-wdt", str(W), "-hgt", str(H), "-fr", "25", "-frms", str(N), "-preset", "slow", "-rc", "0", "-b", "o.265", "-o", "r.yuv"]
    if "-ssim" not in extra:
        args += ["-ssim", "1"]
    r = subprocess.run([os.path.join(tmp, "appencoder")] + args + extra, capture_output=True, cwd=tmp)
    lines = [ln for ln in r.stdout.split(b"\n") if b"ssim" in ln]
    assert r.returncode == 0 and len(lines) == 1, (name, r.stdout[-400:])
    line = lines[0] + b"\n"
    m = re.fullmatch(rb"\t ssim: ([0-9.]+)\t([0-9.]+)\t([0-9.]+)\t([0-9.]+)\n", line)
    assert m, line
    rec = np.fromfile(os.path.join(tmp, "r.yuv"), np.uint8).reshape(N, -1)
    assert rec.shape == clip.shape
    return dict(name=np.bytes_(name.encode()), W=W, H=H, N=N, src=clip, rec=rec, printed=np.array([float(g) for g in m.groups()]), line=np.frombuffer(line, np.uint8),
                args=np.bytes_(" ".join(args + extra).encode())), r.stdout


def rule_values(src, rec, W, H):
    """mean over pictures of plane SSIM under three window rules: partial windows dropped / clipped to the plane / counted whole over an edge-replicated plane"""
    out = {}
    for rule in ("drop", "clip", "replicate"):
        acc = []
        for a, b in zip(src, rec):
            row = []
            for pa, pb in zip(ssim_ref.planes_of(a, W, H), ssim_ref.planes_of(b, W, H)):
                if rule == "drop":
                    row.append(ssim_ref.plane_ssim(pa, pb)[1])
                    continue
                h, w = pa.shape
                vals = []
                for y in range(0, h, 8):
                    for x in range(0, w, 8):
                        if rule == "clip":
                            wa, wb = pa[y:y + 8, x:x + 8].astype(np.float64), pb[y:y + 8, x:x + 8].astype(np.float64)
                        else:
                            iy, ix = np.minimum(np.arange(y, y + 8), h - 1), np.minimum(np.arange(x, x + 8), w - 1)
                            wa, wb = pa[np.ix_(iy, ix)].astype(np.float64), pb[np.ix_(iy, ix)].astype(np.float64)
                        ma, mb = wa.mean(), wb.mean()
                        va, vb, cv = (wa * wa).mean() - ma * ma, (wb * wb).mean() - mb * mb, (wa * wb).mean() - ma * mb
                        vals.append((2 * ma * mb + ssim_ref.C1) * (2 * cv + ssim_ref.C2) / ((ma * ma + mb * mb + ssim_ref.C1) * (va + vb + ssim_ref.C2)))
                row.append(float(np.mean(vals)))
            acc.append(row)
        out[rule] = np.mean(acc, axis=0)
    return out


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="ks265ssim_")
    try:
        shutil.copy(ENC, os.path.join(tmp, "appencoder")); os.chmod(os.path.join(tmp, "appencoder"), 0o755)
        cases = []
        for name in CASES:
            c, stdout = run(name, tmp)
            cases.append(c)
            print(name, c["line"].tobytes())
            for rule, v in rule_values(c["src"], c["rec"], c["W"], c["H"]).items():
                print(f"   {rule:9s} " + " ".join(f"{x:.6f}" for x in v) + "   max |diff| " + f"{np.abs(v - c['printed'][1:]).max():.2e}")
            if "ssim2" in name:
                print(stdout.decode(errors="replace")[-900:])
        path = save_cases("ssim_ref", cases)
        print(path, os.path.getsize(path), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
