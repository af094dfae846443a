"""CPU: the order in which the thread that CALLS the encoder's API calls the device library while it hands pictures in (ks265codec_amd/host/ks265_enc.c: lane_put and what runs
around it), pinned - the counterpart of tests/test_submit_order_cpu.py, which pins the scheduler thread's.  The ordering of a picture's way in against the caller's stream lives in
these calls: a wait that moves is a race on the GPU that no stream comparison shows; here it changes the SHA-256 of the calling thread's lines of the stand-in's call log
(KS265_STUB_CALL_LOG), restricted to the input entries each case names.  tests/lane_put_main.c hands the pictures in, every case in a process of its own;
tests/golden/input_order.json holds per case the line count and digest, the stream's MD5 and the return code of every API call, as the host of the commit named there gave them
(tests/golden/input_order_gen.py writes them).  The lookahead's queue is also looked at by the scheduler thread, so every case but one runs without it.
(`acquired_unused`: the slot stays acquired and a free one takes the picture; lane_put's last resort - no slot free but an acquired one - needs every slot of the lane taken,
which one lane never reaches.)"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess

import pytest

from host_harness import HERE, ROOT, build_host_program, digest  # noqa: F401  (ROOT: tests/golden/input_order_gen.py's)
from host_harness import lane_put_env as case_env

GOLDEN = os.path.join(HERE, "golden", "input_order.json")
DOC = json.load(open(GOLDEN))
CASES = DOC["cases"]


def build_program(host: str | None = None) -> str:
    """tests/lane_put_main.c with the host (of `host`, else the tree's) and the stand-in that has every way in"""
    return build_host_program("lane_put_main.c", stub="hip_stub_window.c", sanitize=False, host_dir=host)


def run_case(exe: str, case: dict, d) -> dict:
    """one run: the calling thread's lines of the case's entries (without the thread column), the stream's MD5, the API calls' codes"""
    log, out = os.path.join(str(d), "calls.log"), os.path.join(str(d), "out.265")
    if os.path.exists(log):
        os.remove(log)
    args = [exe, "run", out, str(case["size"][0]), str(case["size"][1]), str(case["n"]), case["ways"], *[str(a) for a in case.get("args", [])]]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=case_env(case, KS265_STUB_CALL_LOG=log))
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "live 0", r.stdout[-600:] + r.stderr[-1200:]
    rcs = [[ln.split()[1], int(ln.split()[2])] for ln in r.stdout.splitlines() if ln.startswith("rc ")]
    # (tests/hip_stub_float.c carries the 8-bit entries it wraps under ks265_u8_* identifiers, and their log lines say so)
    lines = [ln.replace(" ks265_u8_", " ks265_", 1).split(" ", 1) for ln in open(log).read().splitlines()]
    caller = [t for t, rest in lines if rest.startswith("mark ")]
    assert len(caller) == 1, caller
    mine = [rest for t, rest in lines if t == caller[0] and rest.split(" ", 1)[0] in case["entries"]]
    return {"lines": mine, "md5": hashlib.md5(open(out, "rb").read()).hexdigest(), "rc": rcs}


@pytest.fixture(scope="module")
def program():
    return build_program()


@pytest.mark.parametrize("name", sorted(CASES))
def test_calling_thread_call_order(program, tmp_path, name):
    case = CASES[name]
    got = run_case(program, case, tmp_path)
    for entry in case["must_call"]:                            # the case exercises the branch it is there for
        assert any(ln.startswith(entry + " ") for ln in got["lines"]), entry
    for entry in case.get("never_calls", []):
        assert not any(ln.startswith(entry + " ") for ln in got["lines"]), entry
    assert got["rc"] == case["rc"], "the API calls' return codes changed"
    assert got["md5"] == case["md5"], "the stream changed"
    if "same_md5_as" in case:                                  # a refused call in between leaves no trace in the stream
        assert case["md5"] == CASES[case["same_md5_as"]]["md5"] and any(c != 0 for _, c in case["rc"])
    assert len(got["lines"]) == case["lines"] and digest(got["lines"]) == case["sha256"], \
        f"{name}: the calling thread's calls to the device library changed ({len(got['lines'])} lines, {case['lines']} pinned)"
