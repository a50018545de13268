#!/usr/bin/env python3
"""Writes tests/golden/ref_threefry_vectors.npz: the outputs of the reference's own
Random123 Threefry2x64-20 (oracle/_ref/libref_threefry.so, built by `make -C oracle`
where the reference tree is present) on oracle_binding.threefry_cases(), with the
sha256 of those inputs, so the oracle stays pinned to the reference bit for bit on
machines without the reference tree.

Run: python tests/golden/make_threefry_vectors.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_binding as ob  # noqa: E402


def main():
    if not ob.have_ref_threefry():
        raise SystemExit("oracle/_ref/libref_threefry.so is not built (make -C oracle)")
    cases = ob.threefry_cases()
    out = np.array([ob.ref_threefry(*(int(w) for w in row)) for row in cases], dtype=np.uint64)
    path = os.path.join(HERE, "ref_threefry_vectors.npz")
    np.savez_compressed(path, out=out,
                        inputs_sha256=np.array(hashlib.sha256(cases.tobytes()).hexdigest()))
    print(f"wrote {path}: {len(out)} outputs")


if __name__ == "__main__":
    main()
