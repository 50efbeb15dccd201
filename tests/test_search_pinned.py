"""Pins what seeded CPU searches produce, so that a refactor of the host
search that changes which circuit a seed finds, or how many recursion
nodes it takes, is noticed. Expected values live in
golden/search_pins.json; they are this project's own recorded results.

    python tests/test_search_pinned.py --record

rewrites the fixture from the current build. Record only from a commit
whose search behaviour is the intended one, and name it in the header.
"""

import hashlib
import json
import os
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = os.path.join(REPO, "tests", "golden", "search_pins.json")

if __name__ == "__main__":
    sys.path.insert(0, REPO)

from sboxgates_amd import models  # noqa: E402
from sboxgates_amd.ops import make_engine, mask_for_inputs  # noqa: E402

# create_circuit on initial_state() with a full mask: name -> (sbox, bit,
# engine options). A list for sbox is an explicit table.
CIRCUIT_CASES = {
    "gate": (dict(name="des_s1"), 0, dict(seed=42)),
    "gate_nots": (dict(name="des_s1"), 1, dict(seed=5, try_nots=True)),
    "gate_sat": (dict(name="des_s1"), 0,
                 dict(seed=4, metric="sat", try_nots=True)),
    "gate_10694": (dict(name="des_s1"), 0, dict(seed=6, gate_bitfield=10694)),
    "gate_perm": (dict(name="des_s1", permute=63), 0, dict(seed=12)),
    "lut": (dict(name="des_s1"), 0, dict(seed=1, lut_graph=True)),
    "lut_fa": (dict(name="crypto1_fa"), 0, dict(seed=9, lut_graph=True)),
    # The table, seed and options of test_search.test_degenerate_mux_no_abort.
    "degenerate": (dict(table=[4, 6, 4, 0, 0, 2, 4, 2]), 0,
                   dict(seed=2108833752, metric="sat", gate_bitfield=214)),
}

# Drivers on des_s1 with save_states=True: name -> (method, engine options).
DRIVER_CASES = {
    "beam": ("generate_graph", dict(seed=8)),
    "one_out": ("generate_graph_one_output",
                dict(seed=10, oneoutput=2, iterations=3)),
    "one_out_jobs": ("generate_graph_one_output",
                     dict(seed=33, oneoutput=0, iterations=6, jobs=3,
                          lut_graph=True)),
    "beam_jobs": ("generate_graph", dict(seed=44, jobs=3)),
}


def run_circuit(case):
    sbox_spec, bit, opts = CIRCUIT_CASES[case]
    if "table" in sbox_spec:
        sbox, n = models.load_table(sbox_spec["table"])
    else:
        sbox, n = models.load(sbox_spec["name"], sbox_spec.get("permute", 0))
    eng = make_engine(gpu="off", save_states=False, **opts)
    eng.set_sbox(sbox, n)
    st = eng.initial_state()
    out = eng.create_circuit(st, eng.target(bit), mask_for_inputs(n))
    if out >= 0:
        st.set_output(bit, out)
    return {
        "found": out >= 0,
        "xml_sha256": hashlib.sha256(st.to_xml().encode()).hexdigest(),
        "gates": st.num_gates - st.num_inputs,
        "nodes": eng.stats()["nodes"],
    }


def run_driver(case, out_dir):
    method, opts = DRIVER_CASES[case]
    sbox, n = models.load("des_s1")
    eng = make_engine(gpu="off", save_states=True, output_dir=str(out_dir),
                      **opts)
    eng.set_sbox(sbox, n)
    getattr(eng, method)(eng.initial_state())
    return [os.path.basename(f) for f in eng.saved_files()]


def load_pins():
    with open(PINS) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CIRCUIT_CASES))
def test_pinned_create_circuit(case):
    assert run_circuit(case) == load_pins()["create_circuit"][case]


@pytest.mark.parametrize("case", sorted(DRIVER_CASES))
def test_pinned_driver(case, tmp_path):
    assert run_driver(case, tmp_path) == load_pins()["drivers"][case]


def record():
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, check=True,
                            capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "sboxgates_amd"],
                           cwd=REPO, check=True, capture_output=True,
                           text=True).stdout.strip()
    pins = {
        "header": {
            "what": "results of seeded gpu=off searches; see "
                    "tests/test_search_pinned.py for the case table",
            "recorded_from_commit": commit,
            "sources_modified_at_recording": bool(dirty),
        },
        "create_circuit": {c: run_circuit(c) for c in sorted(CIRCUIT_CASES)},
        "drivers": {},
    }
    for c in sorted(DRIVER_CASES):
        with tempfile.TemporaryDirectory() as d:
            pins["drivers"][c] = run_driver(c, d)
    with open(PINS, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", PINS, "from", commit)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_search_pinned.py --record")
    record()
