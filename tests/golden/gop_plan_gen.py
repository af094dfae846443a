"""Writes tests/golden/gop_plan.json (tests/test_gop_plan_cpu.py): what the streams of the encoder host say about every picture - POC, slice type, NAL type, both reference lists,
reference picture set, QP - for cases that reach every branch of its GOP decisions.  The host is built from the sources of ANOTHER commit, the one whose decisions are to be kept
(never from the code under test), and runs on the stand-in of the device library:
python tests/golden/gop_plan_gen.py [git revision, default HEAD^ | directory with ks265_enc.c and ks265_stream.c]
With the slice-type decision or scene cuts in force the flags the lookahead put on the pictures are recovered from the stream and stored with the case as inputs of the planner
alone: an anchor at offset 4 of a block of 8 whose block was completed = `mini4` on the block's last picture; a key picture that neither the period nor a request explains = a cut."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)
import test_gop_plan_cpu as T  # noqa: E402
from host_harness import build_host_lib  # noqa: E402


def case(n, iper, bframes, size=(128, 72), **env):
    return {"n": n, "iper": iper, "bframes": bframes, "size": list(size), "env": {k: str(v) for k, v in env.items()}}


CASES = {}
for b in (0, 1, 2, 3, 7):                                      # every kind of mini-GOP; 45 pictures: the flush ends the clip inside a mini-GOP
    CASES[f"bframes{b}"] = case(45, 32, b, KS_TEST_LOOKAHEAD=0)
CASES["bframes15"] = case(40, 0, 15, KS_TEST_LOOKAHEAD=0)
CASES["bframes16"] = case(70, 0, 16, KS_TEST_LOOKAHEAD=0)          # the longest mini-GOP the host codes: past QY265ConfigParse's 15, through the struct
CASES["default_gop"] = case(60, 32, -1)                         # the SDK's default: pyramid of 8, the slice-type decision by itself
for r in (1, 2, 3, 4):
    CASES[f"ref{r}_ippp"] = case(20, 16, 0, KS_TEST_REF=r)
    CASES[f"ref{r}_pyramid8"] = case(40, 32, 7, KS_TEST_REF=r, KS_TEST_LOOKAHEAD=0)
    for g in (0, 1):
        CASES[f"ref0_{r}_gpb{g}"] = case(50, 40, 7, KS_TEST_REF0=r, KS265_GPB=g, KS_TEST_LOOKAHEAD=0)
CASES["ref3_pyramid4"] = case(30, 24, 3, KS_TEST_REF=3, KS_TEST_LOOKAHEAD=0)
CASES["ref0_4_gpb1_pyramid4"] = case(40, 32, 3, KS_TEST_REF0=4, KS265_GPB=1, KS_TEST_LOOKAHEAD=0)
CASES["ref0_3_gpb1_ref2"] = case(50, 40, 7, KS_TEST_REF0=3, KS_TEST_REF=2, KS265_GPB=1, KS_TEST_LOOKAHEAD=0)
for ip in (13, 30, 256):                                       # periods that cut a mini-GOP short (to 4, to 5), and one longer than the clip
    CASES[f"iper{ip}_pyramid8"] = case(70, ip, 7, KS_TEST_LOOKAHEAD=0)
    CASES[f"iper{ip}_pyramid4"] = case(40, ip, 3, KS_TEST_LOOKAHEAD=0)
CASES["iper13_plain_b"] = case(40, 13, 2, KS_TEST_LOOKAHEAD=0)
CASES["iper30_default_gop"] = case(70, 30, -1)
for n in (42, 43, 47):                                         # the flush: 1, 2 and 6 pictures behind the last full mini-GOP
    CASES[f"flush{n}"] = case(n, 0, 7, KS_TEST_LOOKAHEAD=0)
for b in (0, 2, 3, 7):
    CASES[f"keyreq_bframes{b}"] = case(60, 32, b, KS_TEST_KEYREQ=1, KS_TEST_LOOKAHEAD=0)
    CASES[f"lanes2_keyreq_bframes{b}"] = case(100, 32, b, KS_TEST_KEYREQ=1, KS265_GOP_LANES=2, KS_TEST_LOOKAHEAD=0)
CASES["keyreq_default_gop"] = case(60, 32, -1, KS_TEST_KEYREQ=1)
CASES["lanes2_keyreq_default_gop"] = case(100, 32, -1, KS_TEST_KEYREQ=1, KS265_GOP_LANES=2)
CASES["lanes2_ref0_3"] = case(75, 40, 7, KS_TEST_REF0=3, KS_TEST_LOOKAHEAD=0, KS265_GOP_LANES=2)
for b in (-1, 0, 3):
    CASES[f"lookahead_cuts_bframes{b}"] = case(60, 128, b, (128, 96), KS_TEST_LOOKAHEAD=8, KS_TEST_CUTS="23,41")
CASES["lookahead_ramp"] = case(100, 128, -1, (128, 96), KS_TEST_LOOKAHEAD=8, KS_TEST_RAMP="32:64:3")
CASES["auto_lookahead_ramp"] = case(100, 128, -1, (128, 96), KS_TEST_RAMP="32:64:3")
CASES["lookahead_ramp_iper44_keyreq"] = case(100, 44, -1, (128, 96), KS_TEST_LOOKAHEAD=8, KS_TEST_KEYREQ=1, KS_TEST_RAMP="32:64:3")
CASES["lookahead_still"] = case(60, 128, -1, (128, 96), KS_TEST_LOOKAHEAD=8, KS_TEST_RAMP="1000:1001:3")
CASES["lanes3_auto_lookahead_ramp"] = case(150, 48, -1, (128, 96), KS_TEST_RAMP="32:64:3", KS265_GOP_LANES=3)
for b in (-1, 3, 2):
    CASES[f"cutree_bframes{b}"] = case(60, 32, b, KS_TEST_RC=3)
CASES["cutree_ramp"] = case(80, 40, -1, (128, 96), KS_TEST_RC=3, KS_TEST_RAMP="32:64:3")
CASES["cutree_keyreq"] = case(60, 0, -1, KS_TEST_RC=3, KS_TEST_KEYREQ=1)
for b in (0, 7):
    CASES[f"rc1_bframes{b}"] = case(60, 32, b, KS_TEST_RC=1, KS_TEST_BR=300, KS_TEST_LOOKAHEAD=0)
for lean in (0, 1, 2, 3):
    CASES[f"lean_b{lean}"] = case(40, 32, 7, KS265_LEAN_B=lean, KS_TEST_LOOKAHEAD=0)
CASES["lean_b3_pyramid4"] = case(30, 32, 3, KS265_LEAN_B=3, KS_TEST_LOOKAHEAD=0)
CASES["zero_latency"] = case(30, 16, -1, KS_TEST_LATENCY="zerolatency")
CASES["low_delay"] = case(30, 16, -1, KS_TEST_LATENCY="lowdelay")


def lookahead_flags(c, records):
    """(cuts, mini4) as display indices"""
    disp = T.display_indices(records)
    keys = [d for d, rec in zip(disp, records) if rec[2] == 19]
    cuts = [d for prev, d in zip(keys, keys[1:]) if not (c["iper"] > 0 and d - prev == c["iper"]) and d not in T.requested_keys(c)]
    mini4 = []
    if c["rules"]["mg_adapt"] and c["rules"]["gop_b"] == 7:
        for start, end in zip(keys, keys[1:] + [c["n"]]):
            anchors = {0} | {rec[0] for d, rec in zip(disp, records) if start <= d < end and rec[2] != 19 and all(p < rec[0] for p in rec[3] + rec[4])}
            mini4 += [start + p + 4 for p in sorted(anchors) if p % 8 == 4 and p - 4 in anchors and p + 4 in anchors]
            c.setdefault("_blocks8", 0)
            c["_blocks8"] += len([p for p in anchors if p % 8 == 0 and p >= 8 and p - 8 in anchors and p - 4 not in anchors])
    return cuts, mini4


def host_sources(arg, d):
    if os.path.isdir(arg):
        return arg, arg
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", arg], text=True).strip()
    for f in subprocess.check_output(["git", "-C", ROOT, "ls-tree", "--name-only", rev, "ks265codec_amd/host/"], text=True).split():
        open(os.path.join(d, os.path.basename(f)), "wb").write(subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:{f}"]))
    return d, rev


with tempfile.TemporaryDirectory() as d:
    host, origin = host_sources(sys.argv[1] if len(sys.argv) > 1 else "HEAD^", d)
    so = build_host_lib("hip_stub.c", host_dir=host)
    doc = {"generated_from": origin, "fields": list(T.FIELDS), "cases": {}}
    for name, c in sorted(CASES.items()):
        c["rules"] = T.lane_rules(c)
        runs = [T.host_records(so, c, os.path.join(d, "o.265")) for _ in range(2)]
        assert runs[0] == runs[1], name
        records, lanes = runs[0]
        assert lanes == int(c["env"].get("KS265_GOP_LANES", 1)), (name, lanes)
        c["cuts"], c["mini4"] = lookahead_flags(c, records)
        blocks8 = c.pop("_blocks8", 0)
        assert not c["cuts"] or "KS_TEST_CUTS" in c["env"], (name, c["cuts"])
        if "KS_TEST_CUTS" in c["env"]:
            assert c["cuts"] == [23, 41], (name, c["cuts"])
        if name.endswith("lookahead_ramp"):                       # at least one block comes out as 4 + 4 and one as 8
            assert c["mini4"] and blocks8, (name, c["mini4"], blocks8)
        c["pictures"] = records
        doc["cases"][name] = c
        print(name, len(records), "pictures", "cuts", c["cuts"], "mini4", c["mini4"], "blocks of 8:", blocks8)
with open(T.GOLDEN, "w") as f:
    f.write("{\n \"generated_from\": %s,\n \"fields\": %s,\n \"cases\": {\n" % (json.dumps(doc["generated_from"]), json.dumps(doc["fields"])))
    for i, (name, c) in enumerate(sorted(doc["cases"].items())):
        pics = c.pop("pictures")
        f.write("  %s: {%s,\n   \"pictures\": [\n" % (json.dumps(name), json.dumps(c, sort_keys=True)[1:-1]))
        f.write(",\n".join("    " + json.dumps(p, separators=(",", ":")) for p in pics))
        f.write("\n   ]}%s\n" % ("," if i + 1 < len(doc["cases"]) else ""))
    f.write(" }\n}\n")
