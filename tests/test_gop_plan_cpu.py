"""CPU: every GOP decision of the encoder host - key pictures, mini-GOP lengths, coding order, slice kinds, both reference lists, reference picture sets, is_ref, the QP ladder -
pinned per picture.  tests/golden/gop_plan.json holds, for every case, what the streams of the host BEFORE the planner existed say about each picture (tests/golden/gop_plan_gen.py
wrote it from that commit's sources; tests/slice_headers.py reads the streams).  A: the host of this tree, driven the same way on the stand-in of the device library, says the
same.  B: the planner alone (ks265codec_amd/host/ks265_gop.h in tests/gop_plan_main.c, under ASan and UBSan), fed each case's rules and an arrival script, plans the same - and
plans the same again with the whole clip visible at once."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from host_harness import HERE, ROOT, build_host_lib, build_host_program

GOLDEN = os.path.join(HERE, "golden", "gop_plan.json")
DOC = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"cases": {}}
CASES = DOC["cases"]
FIELDS = ("poc", "slice_type", "nal_type", "l0", "l1", "rps", "qp")
BASE_QP = 34                                                  # tests/host_driver.py: -qp 34
KEYREQ_AFTER = (17, 18, 40)                                   # tests/host_driver.py, KS_TEST_KEYREQ: the picture behind each of these is asked to be a key picture


def host_records(so: str, case: dict, out: str) -> tuple[list[list], int]:
    """one run of tests/host_driver.py; what the stream says about every picture in coding order (FIELDS), and the lanes that coded it"""
    from slice_headers import pictures
    env = {k: v for k, v in os.environ.items() if not k.startswith(("KS265_", "KS_TEST_"))}
    env.update(KS265_STUB_LIB=so, **{k: str(v) for k, v in case["env"].items()})
    args = [sys.executable, os.path.join(HERE, "host_driver.py"), ROOT, str(case["n"]), str(case["iper"]), str(case["bframes"]), str(case["size"][0]), str(case["size"][1]), out]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-1200:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["vcl"] == case["n"]
    return [[p["poc"], p["slice_type"], p["nal_type"], p["l0"], p["l1"], [list(x) for x in p["rps"]], p["qp"]] for p in pictures(open(out, "rb").read())], res["lanes"]


def lane_rules(case: dict) -> dict:
    """what lane_resolve (ks265_enc.c) makes of the case's inputs, as far as the planner reads it (GopRules); preset medium: -ref 1, -ref0 3"""
    env = case["env"]
    latency = env.get("KS_TEST_LATENCY", "default")
    lookahead = int(env.get("KS_TEST_LOOKAHEAD", -1))
    bframes = case["bframes"]
    gop_b = (7 if latency == "default" else 0) if bframes < 0 else bframes
    hier = gop_b == 7 or bframes == 3
    refs = min(max(int(env.get("KS_TEST_REF", 1)), 1), 4)
    ref0 = int(env.get("KS265_REF0", env.get("KS_TEST_REF0", 3)))
    refs0 = min(max(ref0, 1), 4) if hier else 1
    la_on = (lookahead > 0 or (lookahead < 0 and hier and gop_b == 7)) and case["size"][0] // 2 >= 16 and case["size"][1] // 2 >= 16
    return {"gop_b": gop_b, "hier": int(hier), "refs": 1 if gop_b > 0 else refs, "refs_b": refs if hier else 1, "refs0": refs0,
            "gpb": int(int(env.get("KS265_GPB", 0)) != 0 and gop_b > 0 and refs0 > 1), "fixqp": 0, "lean_b": int(env.get("KS265_LEAN_B", 1)), "mg_adapt": int(hier and la_on)}


def display_indices(records: list[list]) -> list[int]:
    """closed GOPs in display order, POCs relative to the key picture: the display index of every record"""
    out, start, count = [], 0, 0
    for rec in records:
        if rec[2] == 19:
            start += count
            count = 0
        out.append(start + rec[0])
        count += 1
    return out


def requested_keys(case: dict) -> list[int]:
    return [t + 1 for t in KEYREQ_AFTER if t + 1 < case["n"]] if case["env"].get("KS_TEST_KEYREQ") else []


def arrival_scripts(case: dict) -> tuple[list[str], list[tuple[int, int, int]]]:
    """one script per lane (tests/gop_plan_main.c), pictures arriving one at a time, and the chunks (lane, the lane's first index, pictures) in the order the handle hands GOPs out.
    One lane: a requested key picture and a scene cut are key flags on the picture.  GOP lanes (top_encode): a GOP per lane in turn, its first picture a key picture; a GOP that
    a request ends early is told so (gop_end) when its successor arrives - which moves WHEN its last mini-GOP is planned, not what it is: without it the lane's next key picture, or the
    flush, cuts the mini-GOP at the same place"""
    r = case["rules"]
    lanes, n, iper = int(case["env"].get("KS265_GOP_LANES", 1)), case["n"], case["iper"]
    head = "rules " + " ".join(str(r[k]) for k in ("gop_b", "hier", "refs", "refs_b", "refs0", "gpb", "fixqp", "lean_b", "mg_adapt"))
    keys, mini4 = set(requested_keys(case)) | set(case["cuts"]), set(case["mini4"])
    if lanes == 1:
        lines = [head]
        for t in range(n):
            lines += [f"pic {int(t in keys)} {int(t in mini4)} {iper}", f"wake {t + 1} 0 -1"]
        lines.append(f"wake {n} 1 -1")
        return ["\n".join(lines) + "\n"], [(0, 0, n)]
    lines, count, gop_end = [[head] for _ in range(lanes)], [0] * lanes, [-1] * lanes
    chunks, left, cur = [], 0, -1
    for t in range(n):
        first = left <= 0 or t in keys
        if first:
            if chunks and left > 0:                               # the newest GOP ends before its period is over
                gop_end[cur] = count[cur] - 1
                lines[cur].append(f"wake {count[cur]} 0 {gop_end[cur]}")
            cur = (cur + 1) % lanes
            chunks.append([cur, count[cur], 0])
            left = iper
        lines[cur].append(f"pic {int(first)} {int(t in mini4)} {iper}")
        count[cur] += 1
        chunks[-1][2] += 1
        left -= 1
        lines[cur].append(f"wake {count[cur]} 0 {gop_end[cur]}")
    for k in range(lanes):
        lines[k].append(f"wake {count[k]} 1 {gop_end[k]}")
    return ["\n".join(ln) + "\n" for ln in lines], [tuple(c) for c in chunks]


def run_planner(exe: str, script: str) -> list[dict]:
    """tests/gop_plan_main.c plan: the planned pictures, each with the wake-up that planned it"""
    r = subprocess.run([exe, "plan"], input=script, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("arrival: same "), lines[-1]
    return [{k: [int(x) for x in v.split(",") if x] if k in ("l0", "l1", "keep") else v if k == "kind" else int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])} for ln in lines[:-1]]


def expected_tools(rec: list, lean_b: int) -> tuple[int, int]:
    """(lean, key_headers) of a picture as its record in the fixture and KS265_LEAN_B say (not the planner's code): a B picture - one with a reference behind it -
    that nothing predicts from runs lean (2); one others predict from whose nearest references are at most two pictures away runs half lean (1) unless KS265_LEAN_B is 3"""
    poc, _, nal, l0, l1 = rec[:5]
    if not lean_b or not any(p > poc for p in l1):
        return 0, int(nal == 19)
    return (2 if nal == 0 else 1 if lean_b != 3 and poc - l0[0] <= 2 and l1[0] - poc <= 2 else 0), 0


def planned_records(exe: str, case: dict) -> tuple[list[list], list[tuple[int, int]]]:
    """the planner's pictures for the case in the stream's order, mapped to the fixture's fields; QP as the ladder offset on the base QP (None with rate control: the controller's
    offset is a run-time value).  Beside them what no stream shows: (lean, key_headers) of every picture"""
    scripts, chunks = arrival_scripts(case)
    per_lane = [run_planner(exe, script) for script in scripts]
    rc = int(case["env"].get("KS_TEST_RC", 0))
    out, tools = [], []
    for lane, first, count in chunks:
        gop = [p for p in per_lane[lane] if first <= p["disp"] < first + count]
        assert len(gop) == count and gop[0]["kind"] == "I" and gop[0]["disp"] == first, (lane, first, count, len(gop))
        for p in gop:
            rps = []
            if p["kind"] != "I":
                for k in p["keep"]:                               # (fill_job: the keep set without repeats and without the picture itself; used = in one of its lists)
                    if k != p["poc"] and k not in [x[0] for x in rps]:
                        rps.append([k, int(k in p["l0"] or k in p["l1"])])
            out.append([p["poc"], "I" if p["kind"] == "I" else "P" if p["kind"] == "P" and not p["gpb"] else "B", 19 if p["kind"] == "I" else 1 if p["is_ref"] else 0,
                        p["l0"], p["l1"], sorted(rps), None if rc else BASE_QP + p["qp_off"]])
            tools.append((p["lean"], p["key_headers"]))
    return out, tools


def first_difference(got: list[list], want: list[list], skip_qp: bool = False) -> str | None:
    for i, (g, w) in enumerate(zip(got, want)):
        for k, name in enumerate(FIELDS):
            if g[k] != w[k] and not (skip_qp and name == "qp"):
                return f"picture {i} in coding order (POC {w[0]}): {name} is {g[k]}, the fixture says {w[k]}"
    return None if len(got) == len(want) else f"{len(got)} pictures, the fixture has {len(want)}"


@pytest.fixture(scope="module")
def stub_lib():
    return build_host_lib("hip_stub.c")


@pytest.fixture(scope="module")
def planner():
    """tests/gop_plan_main.c: the planner's header and nothing else of the host (the sanitizers' runtimes inside the program)"""
    return build_host_program("gop_plan_main.c")


def test_the_fixture_covers_the_planner():
    assert len(CASES) >= 40 and DOC["generated_from"]
    adaptive = {bool(c["mini4"]) for c in CASES.values() if c["rules"]["mg_adapt"] and c["rules"]["gop_b"] == 7}
    assert adaptive == {True, False}                             # clips with blocks of 8 coded as 4 + 4, and clips where every block stays 8


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_plans_what_it_planned_before(stub_lib, tmp_path, name):
    case = CASES[name]
    got, lanes = host_records(stub_lib, case, str(tmp_path / "o.265"))
    assert lanes == int(case["env"].get("KS265_GOP_LANES", 1))
    diff = first_difference(got, case["pictures"])
    assert diff is None, f"{name}: {diff}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_planner_alone_plans_the_same(planner, name):
    case = CASES[name]
    assert lane_rules(case) == case["rules"]                     # (the generator stored what lane_rules gave: this only says the function has not moved since; the check is below)
    planned, tools = planned_records(planner, case)
    diff = first_difference(planned, case["pictures"], skip_qp=bool(int(case["env"].get("KS_TEST_RC", 0))))
    assert diff is None, f"{name}: {diff}"
    want = [expected_tools(rec, case["rules"]["lean_b"]) for rec in case["pictures"]]
    assert tools == want, f"{name}: (lean, key_headers) of picture {[i for i, (g, w) in enumerate(zip(tools, want)) if g != w][:1]} in coding order"


def test_a_gop_that_is_told_its_end_is_planned_at_once(planner):
    """GOP lanes: a GOP that a key-picture request ends early is told its last picture (gop_end).  What is planned is what the lane's next key picture or the flush would cut as
    well - so no stream shows this branch - but it is planned in the wake-up that brings the news, not when the lane's next GOP arrives"""
    script = "rules 7 1 1 1 3 0 0 1 0\n" + "".join(f"pic {int(t == 0)} 0 32\nwake {t + 1} 0 -1\n" for t in range(12)) + "wake 12 0 11\n"
    pics = run_planner(planner, script)
    assert sorted(p["disp"] for p in pics) == list(range(12))
    assert [p["disp"] for p in pics if p["wake"] == 12] == [11, 9, 10] and max(p["wake"] for p in pics) == 12     # (0 .. 8 were planned as pictures arrived: wake-ups 0 and 8)


def test_more_b_pictures_than_a_mini_gop_can_hold_are_refused(stub_lib, tmp_path):
    """bframes in the configuration struct, past what QY265ConfigParse takes: 16 is the longest mini-GOP the host ever coded (a case of the fixture); 17 and more is QY_NOTSUPPORTED at open"""
    env = dict({k: v for k, v in os.environ.items() if not k.startswith(("KS265_", "KS_TEST_"))}, KS265_STUB_LIB=stub_lib, KS_TEST_LOOKAHEAD="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "host_driver.py"), ROOT, "40", "0", "17", "128", "72"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode != 0 and "AssertionError: 0x80000004" in r.stderr, r.stderr[-800:]


def test_one_walk_for_planner_and_cutree(planner):
    """gop_plan()'s B pictures against gop_walk()'s nodes.  ct_structure() is not run here: it copies gop_walk()'s nodes field by field, and tests/test_calc_frame_cost.py pins what
    the cuTree pass makes of them"""
    r = subprocess.run([planner, "walk"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "walk: ok", r.stdout[-1500:] + r.stderr[-2000:]
    # spans 2, 4, 8 are pyramids, breadth first; 3, 5, 6, 7 are not
    assert "walk: hier 1 span 8 at 8: 4r 2r 6r 1 3 5 7" in r.stdout and "walk: hier 1 span 4 at 0: 2r 1 3" in r.stdout and "walk: hier 1 span 6 at 0: 1 2 3 4 5" in r.stdout and "walk: hier 0 span 8 at 0: 1 2 3 4 5 6 7" in r.stdout and "walk: hier 0 span 17 at 16: 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16" in r.stdout
