"""One rank of a multi-rank run that keeps an escape bank: tests/gpu_ranks_worker.py as it is -- the
same arguments, the same rank<r>.npz, the same log line; its Simulation keywords carry
"escape_bank": capacity -- with, per step, the escape stats (summed over the ranks by the library)
and the rank's own step_claimed / step_recorded written to <out>/bank<r>.json, and the rank's bank
as it stands when the worker closes its Simulation, the raw bytes of `recorded` records, to
<out>/bank<r>.npy.  Started by tests/test_escape_bank.py through ranks.launch_ranks."""
import json
import os
import sys

import numpy as np

import gpu_ranks_worker as worker


def main():
    out, rank = sys.argv[2], int(os.environ["RANK"])
    said = []
    step, close = worker.iface.Simulation.step, worker.iface.Simulation.close

    def step_and_note(self, master_key):
        r = step(self, master_key)
        said.append(dict(escaped=list(r.escape.counts()), step_claimed=r.step_claimed, step_recorded=r.step_recorded))
        return r

    def read_and_close(self):
        os.makedirs(out, exist_ok=True)
        if self.escape_bank is not None:
            np.save(os.path.join(out, f"bank{rank}.npy"), self.escape_bank_host().view(np.uint8))
        close(self)
    worker.iface.Simulation.step = step_and_note
    worker.iface.Simulation.close = read_and_close
    worker.main()
    with open(os.path.join(out, f"bank{rank}.json"), "w") as f:
        json.dump(said, f)


if __name__ == "__main__":
    main()
