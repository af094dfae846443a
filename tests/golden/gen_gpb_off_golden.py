"""Writes tests/golden/gpb_off_stream_md5.json (tests/test_gpb_host_cpu.py): size and MD5 of the streams the encoder host writes on the stand-in of the device library for a
pyramid GOP and for IPPP, WITHOUT the `gpb` switch.  Run it at the commit whose streams are to be kept (it was run on the host sources before the switch existed):
python tests/golden/gen_gpb_off_golden.py [directory with ks265_enc.c, ks265_cli.c, ks265_stream.c]"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)
import test_gpb_host_cpu as T  # noqa: E402
from host_harness import build_host_cli  # noqa: E402

CASES = {"pyramid4": ["-bframes", "3", "-ref0", "3", "-iper", "16", "-frms", "33"], "ippp": ["-bframes", "0", "-iper", "16", "-frms", "20"]}
host = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "ks265codec_amd", "host")
with tempfile.TemporaryDirectory() as d:
    exe = build_host_cli(host_dir=host)
    yuv = os.path.join(d, "in.yuv")
    np.random.default_rng(5).integers(0, 256, 70 * T.W * T.H * 3 // 2, dtype=np.uint8).tofile(yuv)
    doc = {"cases": {}}
    for name, opts in sorted(CASES.items()):
        runs = [T.encode({"exe": exe, "yuv": yuv}, os.path.join(d, "o.265"), opts) for _ in range(2)]
        assert runs[0] == runs[1], name
        doc["cases"][name] = {"opts": opts, "bytes": len(runs[0]), "md5": hashlib.md5(runs[0]).hexdigest()}
        print(name, doc["cases"][name])
json.dump(doc, open(T.GOLD, "w"), indent=1, sort_keys=True)
open(T.GOLD, "a").write("\n")
