"""options::ordered on the host side: the option, the CLI flag and the
make_engine argument exist, default to off, and change nothing where no GPU
is in use, because the CPU scans are ordered already. What the option does
to the GPU scans is in test_gpu_ordered.py.
"""

import hashlib
import os
import subprocess

import pytest

import _oracle as orc
import test_search_pinned as pinned
from sboxgates_amd import _core, models
from sboxgates_amd.ops import make_engine, mask_for_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "bin", "sboxgates")
DES = os.path.join(REPO, "sboxgates_amd", "sboxes", "des_s1.txt")


def test_option_defaults_to_off():
    o = _core.Options()
    assert o.ordered is False
    o.ordered = True
    assert o.ordered is True


def run_ordered_circuit(case, gpu):
    """run_circuit of test_search_pinned.py on an `ordered` engine; returns
    (what run_circuit returns, the engine's stats)."""
    sbox_spec, bit, opts = pinned.CIRCUIT_CASES[case]
    if "table" in sbox_spec:
        sbox, n = models.load_table(sbox_spec["table"])
    else:
        sbox, n = models.load(sbox_spec["name"], sbox_spec.get("permute", 0))
    eng = make_engine(gpu=gpu, ordered=True, save_states=False, **opts)
    eng.set_sbox(sbox, n)
    st = eng.initial_state()
    out = eng.create_circuit(st, eng.target(bit), mask_for_inputs(n))
    if out >= 0:
        st.set_output(bit, out)
    stats = eng.stats()
    return {
        "found": out >= 0,
        "xml_sha256": hashlib.sha256(st.to_xml().encode()).hexdigest(),
        "gates": st.num_gates - st.num_inputs,
        "nodes": stats["nodes"],
    }, stats


@pytest.mark.parametrize("case", ["gate", "gate_sat", "lut", "lut_fa"])
def test_ordered_cpu_engine_reproduces_pins(case):
    got, _ = run_ordered_circuit(case, "off")
    want = pinned.load_pins()["create_circuit"][case]
    for key in ("xml_sha256", "gates", "nodes"):
        assert got[key] == want[key], (case, key)


def cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True,
                          text=True, timeout=120)


@pytest.fixture(scope="module")
def cli_built():
    if not os.path.exists(CLI):
        pytest.skip("CLI not built (run make)")


def test_cli_help_lists_ordered(cli_built, tmp_path):
    r = cli(["--help"], tmp_path)
    assert r.returncode == 0
    assert "--ordered" in r.stdout + r.stderr


@pytest.mark.parametrize("mode", [[], ["-l"]], ids=["gates", "lut"])
def test_cli_ordered_cpu_writes_same_files(cli_built, tmp_path, mode):
    names = []
    for flag in ([], ["--ordered"]):
        d = tmp_path / ("ordered" if flag else "plain")
        d.mkdir()
        r = cli(["--cpu", "--seed", "5"] + flag + mode + ["-o", "0", DES], d)
        assert r.returncode == 0, r.stderr
        names.append(sorted(os.listdir(str(d))))
    assert names[0] and names[0] == names[1]


@pytest.mark.parametrize("case", [(5, 12, 12), (7, 11, 24)], ids=orc.case_id)
def test_scan_pool_on_ordered_cpu_engine(case):
    assert case in orc.PER_RANK_CASES
    k = case[0]
    st, target, mask, total = orc.case_setup(case)
    plain = orc.cpu_engine(k)
    ordered = orc.rijndael_engine(True, ordered=True)
    assert not ordered.gpu_active
    for begin, end in ((0, total), (1, total), (total // 3, total),
                       (total // 2, total // 2 + 40), (total - 1, total)):
        want = plain.scan_pool(k, st, target, mask, begin, end,
                               seed=orc.SCAN_SEED)
        got = ordered.scan_pool(k, st, target, mask, begin, end,
                                seed=orc.SCAN_SEED)
        assert tuple(got) == tuple(want), (orc.case_id(case), begin, end)
