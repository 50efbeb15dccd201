"""The distributed 5/7-LUT scan with a forced GPU on every rank (all on
device 0, gloo control plane), against the model of the chunk protocol: the
launches, scenarios and checks of test_dist_scans.py, whose expectations
come from the model and the CPU hit lists and never from a GPU.

With ordered engines every assertion of the CPU file holds, except that a
rank that hit knows its candidate count only within the model's interval.
With the default election the winner's rank reports whichever hit of its
window won, so the combination must be a hit inside the winner's predicted
window; the counts of ranks without a hit stay exact.

The pool-48 launch runs twice: with the default threshold its chunk windows
go to the wide 5-LUT kernel, with set_scan5_wave_min_pool(44) in every worker
to the wave-owned one.

Whole searches: an ordered three-rank search is the same circuit, byte for
byte, under gpu="force" and gpu="off", through torch.distributed and through
the CLI's --gpus thread group.
"""

import glob
import os
import subprocess

import pytest

import test_dist_scans as cpu
from sboxgates_amd import _core

pytestmark = pytest.mark.gpu

POOL48 = cpu.LAUNCHES[-1]
WAVE_MIN_POOL = 44


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not _core.gpu_available():
        pytest.skip("no GPU")


def check_launch(launch, tmp_path, ordered, wave_min_pool=None):
    results = cpu.run_launch(launch, tmp_path, gpu="force", ordered=ordered,
                             wave_min_pool=wave_min_pool)
    mode = "gpu-ordered" if ordered else "gpu-default"
    for idx in range(len(launch.scenarios)):
        cpu.check_scenario(results, launch, idx, mode)


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "default"])
@pytest.mark.parametrize("launch", cpu.LAUNCHES, ids=lambda l: l.name)
def test_scenarios_match_model(launch, ordered, tmp_path):
    if launch is POOL48:
        n = launch.scenarios[0][0]
        # The wide kernel, not the wave-owned one.
        assert n - 3 > _core.SCAN5_WIDE_MIN_ROW
        assert n < _core.scan5_wave_min_pool()
    check_launch(launch, tmp_path, ordered)


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "default"])
def test_pool48_wave_owned_kernel(ordered, tmp_path):
    assert all(s[0] >= WAVE_MIN_POOL for s in POOL48.scenarios)
    check_launch(POOL48, tmp_path, ordered, wave_min_pool=WAVE_MIN_POOL)


def test_ordered_search_gpu_equals_cpu(tmp_path):
    """DES S1 bit 0, LUT mode, seeded, ordered, three ranks, many rounds:
    the gpu="force" search writes the circuit of the gpu="off" search, byte
    for byte, and every scan of every rank ran on the GPU. (Not compared
    with the one-rank search, which is documented to differ.)"""
    dev = cpu.run_search(tmp_path / "gpu", "force")
    host = cpu.run_search(tmp_path / "cpu", "off")
    assert dev[0]["xml"] == host[0]["xml"]
    assert dev[0]["file_name"] == host[0]["file_name"]
    for r in range(cpu.SEARCH_WORLD):
        assert dev[r]["stats"]["cpu_scans"] == 0, (r, dev[r]["stats"])
        assert dev[r]["stats"]["gpu_scans"] > 0, (r, dev[r]["stats"])
        assert dev[r]["stats"]["nodes"] == host[r]["stats"]["nodes"], r
        # The same windows were scanned: one scan per window on either side.
        assert (dev[r]["stats"]["gpu_scans"]
                == host[r]["stats"]["cpu_scans"]), r


CLI = os.path.join(cpu.worker.REPO, "bin", "sboxgates")
DES_S1 = os.path.join(cpu.worker.REPO, "sboxgates_amd", "sboxes", "des_s1.txt")


def test_cli_thread_group_gpu_equals_cpu(tmp_path):
    """--gpus 3 with real GPU engines, one per thread: the same file name
    (the same fingerprint) and the same bytes as the --cpu run."""
    if not os.path.exists(CLI):
        pytest.skip("CLI not built (run make)")
    env = dict(os.environ)
    env["SBOXGATES_CHUNK5"] = str(cpu.SEARCH_CHUNKS[0])
    env["SBOXGATES_CHUNK7"] = str(cpu.SEARCH_CHUNKS[1])
    files = {}
    for side in ("--gpu", "--cpu"):
        cwd = tmp_path / side.strip("-")
        cwd.mkdir()
        r = subprocess.run(
            [CLI, "--gpus", "3", side, "--ordered", "--seed", "4", "-l", "-o",
             "0", DES_S1], cwd=str(cwd), env=env, capture_output=True,
            text=True, timeout=120)
        assert r.returncode == 0, (side, r.stderr)
        produced = sorted(glob.glob(os.path.join(str(cwd), "1-*.xml")))
        assert len(produced) == 1, (side, produced)
        with open(produced[0], "rb") as f:
            files[side] = (os.path.basename(produced[0]), f.read())
    assert files["--gpu"][0] == files["--cpu"][0]
    assert files["--gpu"][1] == files["--cpu"][1]
