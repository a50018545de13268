"""One rank of a multi-rank run with vacuum sides: tests/gpu_ranks_worker.py as it is -- the same
arguments, the same rank<r>.npz, the same log line -- with the escape stats of every step
(StepResult.escape: summed over the ranks by the library) written to <out>/escape<r>.json as a list
of {"escaped": [4 counts], "weight": [4 sums]}.  Started by tests/test_vacuum.py through
ranks.launch_ranks."""
import json
import os
import sys

import gpu_ranks_worker as worker


def main():
    said = []
    step = worker.iface.Simulation.step

    def step_and_note(self, master_key):
        r = step(self, master_key)
        said.append(dict(escaped=list(r.escape.counts()), weight=list(r.escape.weights())))
        return r
    worker.iface.Simulation.step = step_and_note
    out, rank = sys.argv[2], int(os.environ["RANK"])
    worker.main()
    with open(os.path.join(out, f"escape{rank}.json"), "w") as f:
        json.dump(said, f)


if __name__ == "__main__":
    main()
