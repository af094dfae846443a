"""CPU: the order in which the encoder host's scheduler thread calls the device library (ks265codec_amd/host/ks265_enc.c: submit() and what runs around it), pinned.  The
stand-in of the device library (tests/hip_stub.c) writes one line per call that enqueues work, records an event, waits for one or changes a frame object's state
(KS265_STUB_CALL_LOG): the entry's name and the creation ordinals of the context, frame object and event it was given.  A wait that moves to another stream or another
place in a picture's sequence is a race on the GPU that no stream comparison shows; here it changes the SHA-256 of the scheduler thread's lines, which
tests/golden/submit_order.json holds for every case (tests/golden/submit_order_gen.py writes them)."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "submit_order.json")
CASES = json.load(open(GOLDEN))["cases"]


def build_stub(d) -> str:
    """the host + the stand-in, the stand-in with its two -ssim entries (-DKS265_STUB_SSIM) so that the `-ssim` case runs the fused pass"""
    from oracle_lib import build_oracle
    build_oracle()
    so = os.path.join(str(d), "libks265enc_stub.so")
    host = os.path.join(ROOT, "ks265codec_amd", "host")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-Wall", "-Wextra", "-DKS265_STUB_SSIM", "-I", os.path.join(ROOT, "include"), "-shared", "-o", so,
                           os.path.join(host, "ks265_enc.c"), os.path.join(host, "ks265_stream.c"), os.path.join(HERE, "hip_stub.c"),
                           "-L", os.path.join(ROOT, "oracle"), "-lks265_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-lpthread", "-lm"])
    return so


def scheduler_trace(so: str, case: dict, log: str) -> list[str]:
    """one run of tests/host_driver.py (128x72, one lane); the lines of the thread that issued the ks265_encode_picture* calls, without the thread column"""
    if os.path.exists(log):
        os.remove(log)
    env = dict(os.environ, KS265_STUB_LIB=so, KS265_STUB_CALL_LOG=log, KS265_GOP_LANES="1", **{k: str(v) for k, v in case["env"].items()})
    args = [sys.executable, os.path.join(HERE, "host_driver.py"), ROOT, str(case["n"]), str(case["iper"]), str(case["bframes"]), "128", "72"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-1200:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["vcl"] == case["n"]
    lines = [ln.split(" ", 1) for ln in open(log).read().splitlines()]
    threads = sorted({t for t, rest in lines if rest.startswith("ks265_encode_picture")})
    assert len(threads) == 1, threads
    return [rest for t, rest in lines if t == threads[0]]


def digest(lines: list[str]) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


@pytest.fixture(scope="module")
def stub_lib(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("stuborder"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_scheduler_thread_call_order(stub_lib, tmp_path, name):
    case = CASES[name]
    lines = scheduler_trace(stub_lib, case, str(tmp_path / "calls.log"))
    for entry in case["must_call"]:                            # the case exercises the path it is there for
        assert any(ln.startswith(entry + " ") for ln in lines), entry
    assert len(lines) == case["lines"] and digest(lines) == case["sha256"], f"{name}: the scheduler thread's calls to the device library changed ({len(lines)} lines, {case['lines']} pinned)"
