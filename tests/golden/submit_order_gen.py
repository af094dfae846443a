"""Writes the pinned values of tests/golden/submit_order.json (tests/test_submit_order_cpu.py): every case is run three times; its line count and SHA-256 are stored when the
three traces are identical, else the case is reported and left as it was.  Run it at the commit whose call order is to be kept: python tests/golden/submit_order_gen.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_submit_order_cpu as T  # noqa: E402
from host_harness import build_host_lib, digest, scheduler_trace  # noqa: E402

doc = json.load(open(T.GOLDEN))
with tempfile.TemporaryDirectory() as d:
    so = build_host_lib(*T.STUB)
    for name, case in sorted(doc["cases"].items()):
        runs = [scheduler_trace(so, case, os.path.join(d, "calls.log")) for _ in range(3)]
        missing = [m for m in case["must_call"] if not any(ln.startswith(m + " ") for ln in runs[0])]
        if runs[0] != runs[1] or runs[0] != runs[2] or missing:
            print(f"{name}: NOT STORED - " + (f"never calls {missing}" if missing else "the three traces differ"))
            continue
        case["lines"], case["sha256"] = len(runs[0]), digest(runs[0])
        print(f"{name}: {case['lines']} lines {case['sha256'][:16]}")
json.dump(doc, open(T.GOLDEN, "w"), indent=1, sort_keys=True)
open(T.GOLDEN, "a").write("\n")
