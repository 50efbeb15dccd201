#!/usr/bin/env python3
"""Re-records tests/golden/reference/ with the oracle binary that
oracle/build_ref.py compiles from the upstream reference.

tests/test_reference_cross.py checks state-file interchange and search
quality against recorded reference results: the XML states the reference
saved and the names (which carry the gate counts) of everything it found.
Those tests therefore need neither the reference nor libxml2. This script
is the recipe that produced the recordings: it runs the commands the tests
were written around and stores what the reference wrote.

    python oracle/build_ref.py && python oracle/record_golden.py

The reference seeds itself from /dev/urandom, so every recording is one
sample of its behaviour; the gate counts in recorded.json are the bar the
head-to-head tests hold this engine to.
"""

import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from build_ref import REF_BINARY, REPO  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "reference")
DES = os.path.join(REPO, "sboxgates_amd", "sboxes", "des_s1.txt")


def run_ref(args, cwd):
    r = subprocess.run([REF_BINARY] + args, cwd=cwd, capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"reference failed on {args}: {r.stderr}")


def names(d, pattern):
    return sorted(os.path.basename(f)
                  for f in glob.glob(os.path.join(d, pattern)))


def main():
    if not os.path.exists(REF_BINARY):
        sys.exit("oracle binary missing: run oracle/build_ref.py first")
    work = tempfile.mkdtemp(prefix="refgolden")
    shutil.rmtree(GOLDEN, ignore_errors=True)
    os.makedirs(GOLDEN)
    recorded = {}

    def subdir(name):
        d = os.path.join(work, name)
        os.makedirs(d)
        return d

    def keep(src_dir, file_names, name):
        dst = os.path.join(GOLDEN, name)
        os.makedirs(dst)
        for f in file_names:
            shutil.copy(os.path.join(src_dir, f), os.path.join(dst, f))

    # Single-output SAT-metric search: every state the reference saved.
    d = subdir("names")
    run_ref(["-i", "1", "-o", "0", "-s", "-n", DES], d)
    keep(d, names(d, "1-*.xml"), "des_s1_o0_sat")

    # Head-to-head quality bar: des_s1 bit 0, gates metric, 3 iterations.
    d = subdir("h2h")
    run_ref(["-i", "3", "-o", "0", DES], d)
    recorded["head_to_head_states"] = names(d, "1-*.xml")

    # Full-graph permuted run (the reference CI's -a 10694 -p 63 config).
    d = subdir("multi")
    run_ref(["-a", "10694", "-i", "1", "-p", "63", DES], d)
    multi = names(d, "4-*.xml")
    recorded["multi_output_states"] = multi
    keep(d, multi[:2], "des_s1_a10694_p63")

    with open(os.path.join(GOLDEN, "recorded.json"), "w") as f:
        json.dump(recorded, f, indent=1)
        f.write("\n")
    shutil.rmtree(work)
    print("recorded", GOLDEN)


if __name__ == "__main__":
    main()
