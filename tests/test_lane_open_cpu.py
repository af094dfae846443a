"""CPU: what the encoder host creates when it opens a lane (ks265codec_amd/host/ks265_enc.c: lane_open) and what it gives back when it closes one, pinned.  The order in which a
lane creates its streams, and where its pictures lie against each other in device memory, are measured results that no stream comparison shows.  The stand-in of
the device library (tests/hip_stub.c) writes one line per creating call - contexts, frame objects, device and pinned blocks, events, ks265_memset_async - in call order;
tests/lane_open_main.c opens a lane and prints those lines, then the host's log lines.  tests/golden/lane_open.json holds line count and SHA-256 of both for every case
(tests/golden/lane_open_gen.py writes them).  The failure walk lets every creating call of an open fail in turn, under ASan and UBSan: the open fails with QY_OUTOFMEMORY or
takes one of its designed fall-backs, and after the close nothing of the stand-in's is alive."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from host_harness import HERE, build_host_program, digest

GOLDEN = os.path.join(HERE, "golden", "lane_open.json")
DOC = json.load(open(GOLDEN))
CASES = DOC["cases"]


def build_program(sanitize: bool = False) -> str:
    """tests/lane_open_main.c with the host and the stand-in (with its -ssim and `hash` entries, so that those switches allocate what they allocate on the device library)"""
    return build_host_program("lane_open_main.c", stub="hip_stub_hash.c", sanitize=sanitize, defines=("KS265_STUB_SSIM",))


def case_env(case: dict) -> dict:
    """the case's variables; nothing else of KS265_* (or the queue count a two-lane open's log line names) comes in from outside"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("KS265_") and k != "GPU_MAX_HW_QUEUES"}
    env.update({k: str(v) for k, v in case.get("env", {}).items()})
    return env


def run(exe: str, mode: str, case: dict, timeout: int = 300) -> subprocess.CompletedProcess:
    """one run of the program with the case's size, pairs and variables"""
    return subprocess.run([exe, mode, str(case["size"][0]), str(case["size"][1]), *[str(a) for a in case.get("args", [])]], capture_output=True, text=True, timeout=timeout, env=case_env(case))


def open_trace(exe: str, case: dict) -> tuple[list[str], str]:
    """(creating calls + log lines, the program's closing `open: ...` line)"""
    r = run(exe, "trace", case)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-1200:]
    lines = r.stdout.splitlines()
    assert lines and lines[-1].startswith("open: "), r.stdout[-600:]
    return lines[:-1], lines[-1]


@pytest.fixture(scope="module")
def program():
    return build_program()


@pytest.fixture(scope="module")
def program_asan():
    return build_program(sanitize=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_open_creation_order(program, name):
    case = CASES[name]
    lines, end = open_trace(program, case)
    if "error" in case:                                          # refused before anything is created
        assert end == "open: error " + case["error"] and not [ln for ln in lines if not ln.startswith("log: ")], (end, lines[:4])
        return
    assert end.startswith("open: ok, %d lane(s)" % case.get("lanes", 1)), end
    for must in case["must"]:                                    # the case exercises the branch it is there for
        assert any(must in ln for ln in lines), must
    assert len(lines) == case["lines"] and digest(lines) == case["sha256"], f"{name}: what a lane creates, in which order, or what it logs changed ({len(lines)} lines, {case['lines']} pinned)"


def popen(exe: str, mode: str, case: dict) -> subprocess.Popen:
    return subprocess.Popen([exe, mode, str(case["size"][0]), str(case["size"][1]), *[str(a) for a in case.get("args", [])]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=case_env(case))


@pytest.mark.parametrize("name", DOC["walk"])
def test_lane_open_failure_walk(program_asan, name):
    n = max(1, min(8, os.cpu_count() or 1))                    # the k are dealt to n processes: an open under the sanitizers costs up to a tenth of a second
    procs = [popen(program_asan, f"walk:{i}/{n}", CASES[name]) for i in range(n)]
    outs = [p.communicate(timeout=600) + (p.returncode,) for p in procs]
    for out, err, rc in outs:
        print(out[-1000:])
        assert rc == 0 and out.splitlines()[-1].endswith(": ok"), out[-1500:] + err[-3000:]
