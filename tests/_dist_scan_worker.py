"""Subprocess worker of the distributed-scan tests (test_dist_scans.py,
test_gpu_dist_scans.py): one rank of a gloo process group, launched with
torchrun-style environment variables by `launch` below.

argv: result path, then one JSON job:
  {"mode": "scenarios", "gpu": "off" | "force", "ordered": bool,
   "wave_min_pool": int or null, "scenarios": [scenario, ...]}
  {"mode": "search", "gpu": ..., "ordered": ..., "seed": int}

"scenarios": for each scenario of _dist_model, rank 0 calls create_circuit
once on the scenario's state while the other ranks sit in worker_loop() until
rank 0 calls stop_workers(). Every rank records how its stats() moved; rank 0
also the gates the node added and the returned gate's table. The ranks
barrier and go on to the next scenario.

"search": a whole DES S1 bit 0 LUT search; rank 0 records the circuit's XML.

The chunk sizes come from SBOXGATES_CHUNK5 / SBOXGATES_CHUNK7, which the
engine reads once per process: one launch has one pair of chunk sizes.
"""

import json
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.abspath(__file__)

COUNTERS = ("candidates3", "candidates5", "candidates7", "gpu_scans",
            "cpu_scans", "nodes")


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(job, world, tmp_dir, chunk5=None, chunk7=None, timeout=120):
    """Runs `job` on `world` ranks and returns their results by rank. A rank
    that fails or does not end in time fails the caller; nothing is retried."""
    assert 1 < world <= 4
    out = os.path.join(str(tmp_dir), "result")
    port = free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({"RANK": str(rank), "WORLD_SIZE": str(world),
                    "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port)})
        for name, value in (("SBOXGATES_CHUNK5", chunk5),
                            ("SBOXGATES_CHUNK7", chunk7)):
            env.pop(name, None)
            if value is not None:
                env[name] = str(value)
        procs.append(subprocess.Popen(
            [sys.executable, WORKER, out, json.dumps(job)], env=env,
            cwd=str(tmp_dir), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
            text=True))
    results = {}
    try:
        for rank, p in enumerate(procs):
            try:
                stdout, stderr = p.communicate(timeout=timeout)
            except subprocess.TimeoutExpired:
                raise AssertionError(f"rank {rank} did not end in {timeout} s")
            assert p.returncode == 0, f"rank {rank} failed:\n{stderr}\n{stdout}"
            with open(out + f".rank{rank}") as f:
                results[rank] = json.load(f)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return results


def counters(eng):
    stats = eng.stats()
    return {k: int(stats[k]) for k in COUNTERS}


def run_scenarios(eng, rank, job, barrier):
    import _dist_model as model
    out = []
    for scen in job["scenarios"]:
        before = counters(eng)
        rec = {}
        if rank != 0:
            eng.worker_loop()
        else:
            st, target, mask = model.scenario_setup(eng, tuple(scen))
            n = st.num_gates
            try:
                ret = eng.create_circuit(st, target, mask)
            finally:
                eng.stop_workers()
            rec["returned"] = ret
            rec["pool"] = n
            rec["added"] = [
                {key: st.gate(i)[key]
                 for key in ("type_name", "in1", "in2", "in3", "function")}
                for i in range(n, st.num_gates)]
            rec["table"] = st.gate(ret)["table"].hex() if ret >= 0 else None
        after = counters(eng)
        rec["stats"] = {k: after[k] - before[k] for k in COUNTERS}
        out.append(rec)
        barrier()
    return out


def run_search(eng, rank, sbox, n):
    from sboxgates_amd.ops import mask_for_inputs
    from sboxgates_amd.utils import validate_circuit
    if rank != 0:
        eng.worker_loop()
        return {"stats": counters(eng)}
    st = eng.initial_state()
    try:
        ret = eng.create_circuit(st, eng.target(0), mask_for_inputs(n))
    finally:
        eng.stop_workers()
    assert ret >= 0
    st.set_output(0, ret)
    assert validate_circuit(st, sbox, n, bit=0)
    return {"stats": counters(eng), "xml": st.to_xml(),
            "file_name": st.file_name()}


def main():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.dirname(WORKER))
    import torch.distributed as dist

    from sboxgates_amd import _core, models
    from sboxgates_amd.ops import make_engine
    from sboxgates_amd.parallel import init_from_env, make_ctx

    out_path = sys.argv[1]
    job = json.loads(sys.argv[2])

    rank, world, _ = init_from_env(backend="gloo")
    ctx = make_ctx()
    if job.get("wave_min_pool") is not None:
        _core.set_scan5_wave_min_pool(job["wave_min_pool"])
    # All ranks on device 0 when gpu is "force".
    eng = make_engine(lut_graph=True, seed=job.get("seed", 21), gpu=job["gpu"],
                      ordered=job["ordered"], save_states=False, oneoutput=0,
                      ctx=ctx)
    if job["gpu"] == "force":
        assert eng.gpu_active

    if job["mode"] == "scenarios":
        sbox, n = models.load("rijndael")
        eng.set_sbox(sbox, n)
        result = run_scenarios(eng, rank, job, dist.barrier)
    elif job["mode"] == "search":
        sbox, n = models.load("des_s1")
        eng.set_sbox(sbox, n)
        result = run_search(eng, rank, sbox, n)
    else:
        raise SystemExit(f"unknown mode {job['mode']}")

    with open(out_path + f".rank{rank}", "w") as f:
        json.dump(result, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
