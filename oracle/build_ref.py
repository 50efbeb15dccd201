#!/usr/bin/env python3
"""Recipe for the cross-validation oracle: compiles the UPSTREAM reference
(dansarie/sboxgates, a C11+MPI program) as a single-rank binary into
oracle/_ref/sboxgates_ref, using the MPI shim in tests/mpi_stub and the
system's libxml2.

The reference's sources are not part of this repository. They are looked
for in $SBOXGATES_REFERENCE_DIR (default: REF_SRC below, the mount point
the tests have always used). When they, gcc or the libxml2 headers
are missing, nothing is built and the tests that need the oracle skip.
oracle/_ref/ is a build product and stays out of git.

    python oracle/build_ref.py          # also run by __graft_entry__.build()
"""

import glob
import os
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.environ.get("SBOXGATES_REFERENCE_DIR", "/root/reference")
REF_DIR = os.path.join(REPO, "oracle", "_ref")
REF_BINARY = os.path.join(REF_DIR, "sboxgates_ref")
LIBXML2_INC = "/usr/include/libxml2"


def build_reference(ref_src=REF_SRC, out=REF_BINARY):
    """Returns the oracle binary's path, or None (with the reason printed)
    when it cannot be built here."""
    srcs = sorted(glob.glob(os.path.join(ref_src, "*.c")))
    if not srcs:
        print(f"oracle: no reference sources under {ref_src}; not built")
        return None
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.isdir(LIBXML2_INC):
        print("oracle: no gcc/libxml2; not built")
        return None
    stub = os.path.join(REPO, "tests", "mpi_stub")
    deps = srcs + glob.glob(os.path.join(ref_src, "*.h")) + \
        glob.glob(os.path.join(stub, "*"))
    if os.path.exists(out) and all(
            os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # No -march=native: the binary may run on another host than it was
    # built on.
    cmd = [gcc, "-O2", "-std=c11", "-I", stub, "-I", LIBXML2_INC] + srcs + [
        os.path.join(stub, "mpistub.c"), "-lxml2", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(f"oracle: reference build failed: {r.stderr[:2000]}")
        return None
    return out


if __name__ == "__main__":
    sys.exit(0 if build_reference() else 1)
