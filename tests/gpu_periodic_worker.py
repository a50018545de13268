"""One rank of a multi-rank run with periodic axes: tests/gpu_ranks_worker.py as it is -- the same
arguments, the same rank<r>.npz, the same log line -- on the deck's mesh with the density of
periodic_reference.seam_density (a deck cannot say it), and with the wrap stats of every step
(StepResult.wraps: summed over the ranks by the library) written to <out>/wraps<r>.json as a list of
{"wrapped": [4 counts], "weight": [4 sums]}.  Started by tests/test_periodic.py through
ranks.launch_ranks."""
import json
import os
import sys

import gpu_ranks_worker as worker
import periodic_reference as pr


def main():
    said = []
    step = worker.iface.Simulation.step
    setup_problem = worker.host.setup_problem

    def step_and_note(self, master_key):
        r = step(self, master_key)
        said.append(dict(wrapped=list(r.wraps.counts()), weight=list(r.wraps.weights())))
        return r

    def setup_with_seams(*args, **kw):
        return pr.seam_density(setup_problem(*args, **kw))
    worker.iface.Simulation.step = step_and_note
    worker.host.setup_problem = setup_with_seams
    out, rank = sys.argv[2], int(os.environ["RANK"])
    worker.main()
    with open(os.path.join(out, f"wraps{rank}.json"), "w") as f:
        json.dump(said, f)


if __name__ == "__main__":
    main()
