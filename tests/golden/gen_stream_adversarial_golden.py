#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (builder container: needs the reference decoder).  gen_stream_golden.py for the adversarial cases of tests/stream_cases.py (ADV_CASES):
encode with the CPU oracle pipeline, write the stream with the host writer, decode it with the reference's own decoder and require every decoded picture to equal the
pipeline's reconstruction; only then record the MD5 of the stream and of every reconstructed picture in stream_adversarial_md5.json."""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, HERE)
from gen_stream_golden import decode  # noqa: E402
from stream_cases import ADV_CASES, make_stream, oracle_encoder  # noqa: E402

if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="ks265dec_")
    res = {}
    try:
        for name, c in ADV_CASES.items():
            bs, recs = make_stream(name, oracle_encoder(name))
            dec = decode(bs, c[0], c[1], tmp)
            assert len(dec) == len(recs), (name, len(dec), len(recs))
            for d in sorted(recs):
                assert (dec[d] == recs[d]).all(), f"{name}: decoded picture {d} differs from the pipeline's reconstruction"
            res[name] = {"stream_md5": hashlib.md5(bs).hexdigest(), "stream_bytes": len(bs), "decoder": "appdecoder V2.6.1.3: output == reconstruction",
                         "recon_md5": [hashlib.md5(recs[d].tobytes()).hexdigest() for d in sorted(recs)]}
            print(name, len(bs), "bytes,", len(recs), "pictures: decoded == reconstruction")
        json.dump(res, open(os.path.join(HERE, "stream_adversarial_md5.json"), "w"), indent=1)
        print(len(res), "cases, every one decoder-verified")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
