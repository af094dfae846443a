"""CPU: the scaler's plain-C table builder (ks265codec_amd/host/ks265_scale.h) under the sanitizers, against tests/yuv_scale_ref.py word for word.  tests/scale_plan_main.c is
a stand-alone program built with -fsanitize=address,undefined and run as a child process: every table sits in a heap block of exactly its extent."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import yuv_scale_ref as ys

from host_harness import build_host_program


@pytest.fixture(scope="module")
def exe():
    return build_host_program("scale_plan_main.c")


@pytest.mark.parametrize("filt", [ys.TRIANGLE, ys.CATMULL_ROM])
@pytest.mark.parametrize("cosited", [0, 1])
def test_tables_equal_the_spec_word_for_word(exe, tmp_path, filt, cosited):
    out = str(tmp_path / "tables.bin")
    args = [str(v) for S, D in ys.AXIS_PAIRS for v in (S, D, filt, cosited)]
    r = subprocess.run([exe, "axis", out, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(ys.AXIS_PAIRS)
    blob, at = np.fromfile(out, np.uint8), 0
    for (S, D), line in zip(ys.AXIS_PAIRS, lines):
        first, coef, T = ys.table(S, D, filt, bool(cosited))
        assert line == f"axis {S} {D} {filt} {cosited} {T}", line
        got_first = blob[at:at + 4 * D].view(np.int32); at += 4 * D
        got_coef = blob[at:at + 2 * D * T].view(np.int16).reshape(D, T); at += 2 * D * T
        assert (got_first == first).all() and (got_coef == coef).all(), (S, D)
    assert at == blob.size


def test_refused_axes_and_the_size_rules(exe, tmp_path):
    out = str(tmp_path / "t.bin")
    r = subprocess.run([exe, "axis", out, "520", "64", "1", "0", "64", "520", "0", "0", "64", "32", "2", "0", "0", "8", "1", "0", "8200", "8200", "1", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.count("refused") == 5 and "axis" not in r.stdout, r.stdout + r.stderr[-2000:]
    for size in [(3840, 2160, 1920, 1080), (200, 136, 128, 72), (512, 256, 64, 32), (64, 64, 512, 512), (520, 256, 64, 32), (132, 96, 64, 48), (128, 97, 64, 48), (128, 96, 60, 48),
                 (128, 96, 64, 44), (8200, 96, 4096, 48), (0, 96, 64, 48), (64, 64, 64, 520)]:
        r = subprocess.run([exe, "size", *map(str, size)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == ("ok" if ys.size_ok(*size) else "refused"), (size, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("filt", [ys.TRIANGLE, ys.CATMULL_ROM])
def test_the_stand_ins_plane_scaler_equals_the_spec(exe, tmp_path, filt):
    """ks265_scale_plane_host, which the CPU stand-in of the device library scales with"""
    rng = np.random.default_rng(5)
    for sw, sh, dw, dh, cos in [(128, 96, 64, 48, 0), (100, 68, 64, 36, 1), (64, 64, 104, 88, 0), (256, 128, 32, 16, 1), (32, 32, 52, 44, 1)]:
        src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        src[: sh // 2, : sw // 2] = ((np.add.outer(np.arange(sh // 2), np.arange(sw // 2)) & 1) * 255).astype(np.uint8)
        src.tofile(str(tmp_path / "in.bin"))
        r = subprocess.run([exe, "plane", str(tmp_path / "out.bin"), *map(str, (sw, sh, dw, dh, filt, cos)), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-400:] + r.stderr[-3000:]
        exp = ys.scale_plane(src, ys.table(sw, dw, filt, bool(cos)), ys.table(sh, dh, filt))
        assert (np.fromfile(str(tmp_path / "out.bin"), np.uint8).reshape(dh, dw) == exp).all(), (sw, sh, dw, dh)
