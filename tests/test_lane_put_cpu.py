"""CPU: the one failure exit of the encoder host's lane_put (ks265codec_amd/host/ks265_enc.c), walked.  tests/lane_put_main.c lets the k-th call the calling thread makes to
the device library's stand-in fail while it hands a picture in (ks265_stub_fail_call), for every k of one picture's call: the call returns the code the host of
tests/golden/input_order.json's commit returned (`walks`), nothing more is handed in, and after the close nothing of the stand-in's is alive - for a device picture, a device
picture with a device ROI map, and a host picture uploaded asynchronously from where it lies.  The program only: built plain and with ASan + UBSan, each run as it is."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from host_harness import HERE, build_host_program, lane_put_env

WALKS = json.load(open(os.path.join(HERE, "golden", "input_order.json")))["walks"]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitizers"])
def program(request):
    return build_host_program("lane_put_main.c", stub="hip_stub_window.c", sanitize=request.param)


@pytest.mark.parametrize("name", sorted(WALKS))
def test_lane_put_failure_walk(program, name):
    walk = WALKS[name]
    r = subprocess.run([program, "walk", str(walk["size"][0]), str(walk["size"][1]), walk["ways"], *[str(a) for a in walk["args"]]],
                       capture_output=True, text=True, timeout=600, env=lane_put_env(walk, ASAN_OPTIONS="detect_leaks=1"))
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out[-1] == "walk: ok", r.stdout[-1500:] + r.stderr[-3000:]
    assert [int(ln.split()[2]) for ln in out if ln.startswith("k ")] == walk["codes"]
