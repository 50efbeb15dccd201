"""Subprocess worker for the ordered k=7 range-splitting test: a fresh
process, because the engine reads SBOXGATES_HIT_CAP once, when it creates its
GPU side. Runs the windows given on the command line as "begin:end" on the
deep instance of _oracle.py with a gpu="force", ordered=True engine and
prints one JSON line: per window [found, res, evaluated]."""

import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import _oracle as orc  # noqa: E402


def main():
    gpu = orc.rijndael_engine(True, gpu="force", ordered=True)
    assert gpu.gpu_active
    st, target, mask = orc.deep7_setup()
    out = []
    for arg in sys.argv[1:]:
        begin, end = arg.split(":")
        found, res, ev = gpu.scan_pool(7, st, target, mask, int(begin),
                                       int(end), seed=orc.SCAN_SEED)
        out.append([bool(found), list(res), ev])
    stats = gpu.stats()
    assert stats["gpu_scans"] == len(out) and stats["cpu_scans"] == 0, stats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
