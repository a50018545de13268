"""One rank of a multi-rank run that keeps the leakage tally: tests/gpu_ranks_worker.py as it is -- the
same arguments, the same rank<r>.npz, the same log line; its Simulation keywords carry
"leakage": [edges or null, ncosines] -- with the rank's tally written to <out>/leakage<r>.npz as
`weight` and `count`, each (4, G + 1, M), read when the worker closes its Simulation.  Started by
tests/test_leakage.py through ranks.launch_ranks."""
import os
import sys

import numpy as np

import gpu_ranks_worker as worker


def main():
    out, rank = sys.argv[2], int(os.environ["RANK"])
    close = worker.iface.Simulation.close

    def read_and_close(self):
        weight, count = self.leakage_host()
        os.makedirs(out, exist_ok=True)
        np.savez(os.path.join(out, f"leakage{rank}.npz"), weight=weight, count=count)
        close(self)
    worker.iface.Simulation.close = read_and_close
    worker.main()


if __name__ == "__main__":
    main()
