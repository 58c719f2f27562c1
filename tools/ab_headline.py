#!/usr/bin/env python3
"""A/B of bench.py variants in one session on one box (same clocks): prints one line per variant.
    python tools/ab_headline.py "--col-chunks 1" "--col-chunks 2" "--mode 0" ...
Leading NAME=VALUE words of a variant go into the environment of its run, so two builds of the library can be compared
(SWMI_LIB, sparksmithwaterman_amd/_capi.py); --repeat N runs the whole list N times, interleaved; --raw FILE appends
every run's JSON line to FILE, prefixed with the variant.
    python tools/ab_headline.py --repeat 5 --raw ab_raw.txt "SWMI_LIB=/path/to/parent/libswmi.so" ""
SWMI_TREE=DIR as such a word runs DIR/bench.py instead -- another checkout with its own package and built library: the way to
compare with a parent whose library lacks symbols this tree's binding declares (the binding refuses such a library).
    python tools/ab_headline.py --repeat 5 "SWMI_TREE=/path/to/parent/checkout" "" """
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
repeat, raw = 1, None
while args and args[0] in ("--repeat", "--raw"):
    if args[0] == "--repeat":
        repeat = int(args[1])
    else:
        raw = args[1]
    args = args[2:]
for rep in range(repeat):
    for variant in args or [""]:
        words = variant.split()
        env = dict(os.environ)
        while words and "=" in words[0] and not words[0].startswith("-"):
            k, v = words.pop(0).split("=", 1)
            env[k] = v
        p = subprocess.run([sys.executable, os.path.join(env.pop("SWMI_TREE", ROOT), "bench.py"), "--steps", "50", "--warmup", "5", "--no-cpu-baseline"] + words,
                           capture_output=True, text=True, env=env)
        try:
            line = p.stdout.strip().splitlines()[-1]
            d = json.loads(line)
            if raw:
                with open(raw, "a") as f:
                    f.write("%s\t%s\n" % (variant or "(default)", line))
            rf = d["roofline"]
            print("%-28s GCUPS %8.1f  ms/step %.4f  one in flight %.4f  sweep %.4f  (one in flight %.4f)  traceback %.4f  materialised %.4f" % (
                variant or "(default)", d["value"], d["ms_per_step"], d.get("ms_per_step_one_in_flight", float("nan")), rf["kernel_avg_ms"],
                rf.get("one_in_flight", {}).get("kernel_avg_ms", float("nan")), rf["traceback_avg_ms"], d["ms_per_step_materialised"]), flush=True)
        except Exception as e:      # noqa: BLE001
            print(variant, "FAILED", e, p.stderr[-400:], flush=True)
            sys.exit(1)             # nothing more is started on a GPU that may have faulted
