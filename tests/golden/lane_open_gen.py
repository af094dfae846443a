"""Writes the pinned values of tests/golden/lane_open.json (tests/test_lane_open_cpu.py): every case is run three times; its line count and SHA-256 are stored when the three
outputs are identical and hold every line the case must show, else the case is reported and left as it was.  Run it at the commit whose creation order is to be kept:
python tests/golden/lane_open_gen.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_lane_open_cpu as T  # noqa: E402

doc = json.load(open(T.GOLDEN))
exe = T.build_program()
for name, case in sorted(doc["cases"].items()):
    if "error" in case:
        continue
    runs = [T.open_trace(exe, case)[0] for _ in range(3)]
    missing = [m for m in case["must"] if not any(m in ln for ln in runs[0])]
    if runs[0] != runs[1] or runs[0] != runs[2] or missing:
        print(f"{name}: NOT STORED - " + (f"never shows {missing}" if missing else "the three outputs differ"))
        continue
    case["lines"], case["sha256"] = len(runs[0]), T.digest(runs[0])
    print(f"{name}: {case['lines']} lines {case['sha256'][:16]}")
json.dump(doc, open(T.GOLDEN, "w"), indent=1, sort_keys=True)
open(T.GOLDEN, "a").write("\n")
