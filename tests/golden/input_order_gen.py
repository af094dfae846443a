"""Writes tests/golden/input_order.json (tests/test_input_order_cpu.py, tests/test_lane_put_cpu.py) from the cases below, AT THE HOST OF A NAMED COMMIT (default HEAD): that
commit's ks265codec_amd/host is checked out into a temporary directory and tests/lane_put_main.c is built against it with the tree's stand-in.  Every case runs five times; it
is stored when the five digests, streams and code lists are identical - with the full entry list, else with the first narrower list that is stable (the list is stored with
the case); a case that no list makes stable is reported and not stored.  The failure walks run once.  python tests/golden/input_order_gen.py [commit]"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_input_order_cpu as T  # noqa: E402

ENTRIES = ["ks265_wait_external", "ks265_external_wait_event", "ks265_input_convert", "ks265_input_pad", "ks265_input_scale", "ks265_roi_reduce",
           "ks265_memcpy_h2d_async", "ks265_memcpy_h2d_sync", "ks265_event_record", "ks265_event_wait"]
NARROWER = [ENTRIES, [e for e in ENTRIES if e != "ks265_event_wait"], [e for e in ENTRIES if e not in ("ks265_event_wait", "ks265_event_record")]]
SMALL, RAGGED, BIG, BIG_RAGGED = [128, 72], [202, 134], [1024, 704], [1026, 706]
FAST = {"KS265_STUB_FAST": 1}
# which input slot is free - and with it which event a picture's lines name - is the scheduler's and the writers' timing: every picture costs the stand-in's "device" 30 ms, so
# that no picture of a case has left the lane before the last one is handed in (zero latency: each has left before the next call)
SLOW = {"KS265_STUB_ENCODE_US": 30000}
BRACKET = ["ks265_wait_external", "ks265_external_wait_event"]


def case(size, n, ways, must, args=(), env=None, never=(), same=None):
    c = {"size": size, "n": n, "ways": ways, "must_call": list(must), "args": list(args), "env": dict(SLOW, **(env or {})), "never_calls": list(never)}
    if same:
        c["same_md5_as"] = same
    return c


CASES = {
    "host_packed": case(SMALL, 8, "c", [], never=BRACKET + ["ks265_memcpy_h2d_sync"]),
    "host_strided": case(SMALL, 8, "s", [], never=BRACKET),
    "acquired_used": case(SMALL, 8, "a", [], never=BRACKET),
    "acquired_unused": case(SMALL, 8, "u", [], never=BRACKET),
    "dev_i420": case(SMALL, 8, "d", BRACKET + ["ks265_input_convert", "ks265_event_record"]),
    "dev_rgba": case(SMALL, 8, "r", BRACKET + ["ks265_input_convert"]),
    "dev_i010": case(SMALL, 8, "y", BRACKET + ["ks265_input_convert"]),
    "dev_rgb_f32": case(SMALL, 8, "f", BRACKET + ["ks265_input_convert"]),
    "dev_scaled": case(SMALL, 8, "z", BRACKET + ["ks265_input_scale"], never=["ks265_input_convert"]),
    "roi_host_host_picture": case(SMALL, 8, "hc", ["ks265_memcpy_h2d_async", "ks265_event_record"], args=["roi", 1], never=BRACKET),
    "roi_device_host_picture": case(SMALL, 8, "gc", BRACKET + ["ks265_roi_reduce"], args=["roi", 1]),
    "roi_host_device_picture": case(SMALL, 8, "hd", BRACKET + ["ks265_memcpy_h2d_async", "ks265_input_convert"], args=["roi", 1], never=["ks265_roi_reduce"]),
    "roi_device_device_picture": case(SMALL, 8, "gd", BRACKET + ["ks265_roi_reduce", "ks265_input_convert"], args=["roi", 1]),
    "ragged_host": case(RAGGED, 8, "cs", ["ks265_memcpy_h2d_async", "ks265_input_pad", "ks265_event_record"]),
    "ragged_device_nv12": case(RAGGED, 8, "n", BRACKET + ["ks265_input_pad"], never=["ks265_input_convert"]),
    "registered_sync": case(BIG, 6, "c", ["ks265_memcpy_h2d_sync"], env=FAST, never=["ks265_memcpy_h2d_async"]),
    "registered_sync_three_buffers": case(BIG, 6, "p", ["ks265_memcpy_h2d_sync"], env=FAST, never=["ks265_memcpy_h2d_async"]),
    "registered_async": case(BIG, 6, "cp", ["ks265_memcpy_h2d_async", "ks265_event_record", "ks265_event_wait"], env=dict(FAST, KS265_UPL_ORDER=0), never=["ks265_memcpy_h2d_sync"]),
    "registered_refused": case(BIG, 6, "c", ["ks265_memcpy_h2d_async"], env=dict(FAST, KS265_STUB_NO_REGISTER=1), never=["ks265_memcpy_h2d_sync"]),
    "registered_ragged": case(BIG_RAGGED, 6, "cp", ["ks265_memcpy_h2d_sync", "ks265_input_pad", "ks265_event_record"], env=FAST),
    "zero_latency": case(SMALL, 8, "cd", BRACKET + ["ks265_input_convert"], args=["latency", "zerolatency"]),
    "two_lanes_device": case(SMALL, 10, "d", BRACKET + ["ks265_input_convert"], args=["iper", 4], env={"KS265_GOP_LANES": 2}),
    "lookahead_on": case(SMALL, 10, "cd", BRACKET + ["ks265_input_convert"], env={"KS265_NO_AUTO_LOOKAHEAD": ""}),
    "refused_plane": case(SMALL, 8, "ddXd", BRACKET, same="dev_i420"),
    "refused_over_the_maximum": case(SMALL, 8, "zzYz", BRACKET + ["ks265_input_scale"], same="dev_scaled"),
    "refused_format_ragged": case(RAGGED, 8, "nnZn", BRACKET + ["ks265_input_pad"], same="ragged_device_nv12"),
}
WALKS = {
    "device_picture": {"size": SMALL, "ways": "d", "args": [], "env": {}},          # (one picture per handle: nothing to slow down)
    "device_roi": {"size": SMALL, "ways": "gd", "args": ["roi", 1], "env": {}},
    "registered_async": {"size": BIG, "ways": "c", "args": [], "env": dict(FAST, KS265_UPL_ORDER=0)},
}


def run_walk(exe: str, walk: dict) -> list[int]:
    """the code the picture's call returns when its k-th call to the device library fails, k = 1 .."""
    r = subprocess.run([exe, "walk", str(walk["size"][0]), str(walk["size"][1]), walk["ways"], *[str(a) for a in walk["args"]]], capture_output=True, text=True, timeout=600, env=T.case_env(walk))
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "walk: ok", r.stdout[-1500:] + r.stderr[-3000:]
    codes = [int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("k ")]
    assert len(codes) == int(next(ln for ln in r.stdout.splitlines() if ln.startswith("calls ")).split()[1]) > 0
    return codes


if __name__ == "__main__":
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    commit = subprocess.check_output(["git", "-C", T.ROOT, "rev-parse", rev], text=True).strip()
    doc = {"host_commit": commit, "cases": {}, "walks": {}}
    with tempfile.TemporaryDirectory() as d:
        host = os.path.join(d, "host")
        os.mkdir(host)
        for f in subprocess.check_output(["git", "-C", T.ROOT, "ls-tree", "--name-only", commit, "ks265codec_amd/host/"], text=True).split():
            open(os.path.join(host, os.path.basename(f)), "wb").write(subprocess.check_output(["git", "-C", T.ROOT, "show", f"{commit}:{f}"]))
        exe = T.build_program(host=host)
        for name, c in sorted(CASES.items()):
            for entries in NARROWER:
                c["entries"] = entries
                runs = [T.run_case(exe, c, d) for _ in range(5)]
                if all(r == runs[0] for r in runs[1:]):
                    break
            else:
                print(f"{name}: NOT STORED - the five runs differ with every entry list")
                continue
            missing = [m for m in c["must_call"] if not any(ln.startswith(m + " ") for ln in runs[0]["lines"])]
            if missing:
                print(f"{name}: NOT STORED - never calls {missing}")
                continue
            c.update(lines=len(runs[0]["lines"]), sha256=T.digest(runs[0]["lines"]), md5=runs[0]["md5"], rc=runs[0]["rc"])
            doc["cases"][name] = c
            print(f"{name}: {c['lines']} lines {c['sha256'][:16]} md5 {c['md5'][:8]}" + ("" if entries is ENTRIES else f" (entries narrowed to {len(entries)})"))
        for name, w in sorted(WALKS.items()):
            w["codes"] = run_walk(exe, w)
            doc["walks"][name] = w
            print(f"walk {name}: {w['codes']}")
    json.dump(doc, open(T.GOLDEN, "w"), indent=1, sort_keys=True)
    open(T.GOLDEN, "a").write("\n")
