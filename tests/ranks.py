"""The one launcher of the suite's multi-rank runs: N processes of one program, started the way
`neutral.hip --gpus N` and torchrun start ranks (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*), on
the CPU (plain-C selftests, the oracle's shard worker) and on the one GPU of the test box
(tests/gpu_ranks_worker.py)."""
import collections
import json
import os
import socket
import subprocess
import sys

import numpy as np

from conftest import ROOT

GPU_WORKER = os.path.join(ROOT, "tests", "gpu_ranks_worker.py")

Rank = collections.namedtuple("Rank", "log stdout")   # log: the last JSON line of stdout, or None


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(argv, nranks, extra_env=None, timeout=600):
    """Starts `argv` nranks times, waits for every rank and asserts that it ended well; -> a Rank
    per rank.  NEUTRAL_COMM_PORT names the rendezvous port outright: the port that was found free
    is the one the ranks meet on (not MASTER_PORT + 1, which nobody checked).  All ranks share
    GPU 0 and stage their exchanges through the host; programs that touch no GPU ignore that part
    of the environment."""
    port = free_port()
    env = dict(os.environ, LOCAL_RANK="0", WORLD_SIZE=str(nranks), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), NEUTRAL_COMM_PORT=str(port), NEUTRAL_COMM_TIMEOUT="120",
               NEUTRAL_HIP_COMM="host", NEUTRAL_HIP_QUIET="1", NEUTRAL_WINDOW_MIN_PARTICLES="32",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(extra_env or {})
    procs = [subprocess.Popen(list(argv), env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(nranks)]
    ranks = []
    try:
        for r, p in enumerate(procs):
            so, se = p.communicate(timeout=timeout)
            assert p.returncode == 0, (r, so[-2000:], se[-3000:])
            lines = [ln for ln in so.splitlines() if ln.startswith("{")]
            ranks.append(Rank(json.loads(lines[-1]) if lines else None, so))
    finally:
        for p in procs:   # (a rank that failed leaves none of the others behind)
            if p.poll() is None:
                p.kill()
                p.communicate()
    return ranks


def launch_gpu_ranks(deck, out, steps, mode, nranks, validate=False, schedule=None, **sim_kw):
    """nranks of tests/gpu_ranks_worker.py on `deck`; mode: "shard" or "domain PXxPY"; sim_kw: the
    Simulation's keyword arguments; schedule (mode "shard"): the census operations between the
    steps, a list of {"after": step, "op": name, its arguments} as the worker's text describes
    them, which it reads from <out>/schedule.json.
    -> (what each rank left in rank<r>.npz, each rank's log)"""
    argv = [sys.executable, GPU_WORKER, deck, str(out), str(steps), mode, json.dumps(sim_kw)]
    if schedule is not None:
        os.makedirs(str(out), exist_ok=True)
        with open(os.path.join(str(out), "schedule.json"), "w") as f:
            json.dump(schedule, f)
        argv += ["--schedule", f.name]
    logs = [r.log for r in launch_ranks(argv + (["--validate"] if validate else []), nranks)]
    return [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(nranks)], logs
