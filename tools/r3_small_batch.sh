#!/usr/bin/env bash
# per-GPU shard shapes of the strong-scaling run (32 utterances over N GPUs -> 32/N per GPU) and the single-utterance shape, final build
set -u
cd "$(dirname "$0")/.."
for b in 32 16 8 4 1; do
  line=$(timeout -k 10 200 python bench.py --full --batch $b --steps 5 --warmup 2 --no-cpu-baseline --no-extra 2>/dev/null | tail -1)
  python - "$line" <<PY
import json,sys
d=json.loads(sys.argv[1])
k=" ".join(f"{x['kernel']} {x['ms']*1e3:.1f}" for x in d['roofline']['kernels'])
print(f"B=$b: {d['value']:.0f} mel-frames/s, {d['ms_per_step']:.2f} ms per sample(), loop_mfma_frac {d.get('loop_mfma_frac')} | us per launch: {k}")
PY
done
