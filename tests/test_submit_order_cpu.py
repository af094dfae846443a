"""CPU: the order in which the encoder host's scheduler thread calls the device library (ks265codec_amd/host/ks265_enc.c: submit() and what runs around it), pinned.  The
stand-in of the device library (tests/hip_stub.c) writes one line per call that enqueues work, records an event, waits for one or changes a frame object's state
(KS265_STUB_CALL_LOG): the entry's name and the creation ordinals of the context, frame object and event it was given.  A wait that moves to another stream or another
place in a picture's sequence is a race on the GPU that no stream comparison shows; here it changes the SHA-256 of the scheduler thread's lines, which
tests/golden/submit_order.json holds for every case (tests/golden/submit_order_gen.py writes them)."""
from __future__ import annotations

import os

import pytest

from host_harness import HERE, build_host_lib, digest, scheduler_trace, submit_order_cases

GOLDEN = os.path.join(HERE, "golden", "submit_order.json")
CASES = submit_order_cases()
STUB = ("hip_stub.c", ("KS265_STUB_SSIM",))                      # the stand-in with its two -ssim entries, so that the `-ssim` case runs the fused pass


@pytest.fixture(scope="module")
def stub_lib():
    return build_host_lib(*STUB)


@pytest.mark.parametrize("name", sorted(CASES))
def test_scheduler_thread_call_order(stub_lib, tmp_path, name):
    case = CASES[name]
    lines = scheduler_trace(stub_lib, case, str(tmp_path / "calls.log"))
    for entry in case["must_call"]:                            # the case exercises the path it is there for
        assert any(ln.startswith(entry + " ") for ln in lines), entry
    assert len(lines) == case["lines"] and digest(lines) == case["sha256"], f"{name}: the scheduler thread's calls to the device library changed ({len(lines)} lines, {case['lines']} pinned)"
