#!/bin/bash
# csp at the 8-, 4-, 2- and 1-GPU shares of the bench workload on ONE GPU: the
# single-GPU evidence for strong scaling.
# usage: [OUT=DIR] tools/share_bench.sh <tag> [sizes...]   (lines in DIR/<tag>_<n>.json, DIR default runs/)
set -e
tag=${1:-share}; shift || true
sizes=${@:-12500000 25000000 50000000 100000000}
out=${OUT:-runs}
mkdir -p $out/$(dirname $tag)
for n in $sizes; do
  python bench.py --full --nparticles $n --no-cpu-baseline > $out/${tag}_$n.json 2> $out/${tag}_$n.err
done
python - "$out/$tag" $sizes <<'PY'
import json, sys
prefix = sys.argv[1]
for n in sys.argv[2:]:
    d = json.loads(open(f"{prefix}_{n}.json").read().strip().splitlines()[-1])
    print(n, "default ABI", round(d["ms_per_step"], 3), "ms/step", "%.3e" % d["value"],
          "| lazy export", round(d["lazy_export"]["ms_per_step"], 3), "ms/step",
          "%.3e" % d["lazy_export"]["value"],
          [(k["name"][:14], round(k["ms_per_launch"], 2)) for k in d["kernels"]])
PY
